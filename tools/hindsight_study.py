#!/usr/bin/env python3
"""How far the built-in controllers are from what was achievable: tools/quality_study.py's settings (one episode of
bench.py's workload over --lanes (trace, offset) pairs; weight 1 with the "identity" utility and weight 1 with "log") with
a hindsight beam search of the same pairs (abrsimulator_amd/search.py: HindsightSearch) next to MPC, RATE and the random
policy.  A search runs beam * n_rates lanes per pair, so the pairs go through in chunks of --chunk groups.  Per setting and
width (1, 4, 16, 64): the mean over pairs of the best qoe_q = qoe - weight * quality found, the share of pairs on which the
width matches the widest one, and the action histogram of the winning sequences.  The widths and settings are fixed here,
before any run.  Writes OUT/hindsight_study.json and prints each row.

    python tools/hindsight_study.py OUT [--lanes 65536] [--chunk 8192]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abrsimulator_amd as A  # noqa: E402
import bench  # noqa: E402
import quality_study as Q  # noqa: E402

WIDTHS = (1, 4, 16, 64)
CONTROLLERS = ("mpc", "rate", "random")


def make_env(n, traces, auto_reset):
    mpd = A.MPD(bench.V, bench.L, bench.MAX_BUFFER, bench.START_UP, A.Chunk(bench.LADDER))
    return A.BatchedABREnv(mpd, A.QOEMetric(*bench.WEIGHTS), A.NetworkInfo(bench.INTERVAL, traces), n, device="cuda",
                           auto_reset=auto_reset)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--chunk", type=int, default=8192)
    a = ap.parse_args()
    N, V, M = a.lanes, bench.V, len(bench.LADDER)
    traces = bench.synth_traces()
    tid, off = bench.lane_assignment(0, N, traces)
    tid_t, off_t = torch.from_numpy(tid), torch.from_numpy(off)
    rows = []
    for utility, weight in Q.SETTINGS:
        for kind in CONTROLLERS:                                   # the same figures as quality_study's, on these pairs
            env = make_env(N, traces, True)
            env.reset(tid_t, off_t)
            led, ql = env.set_episode_ledger(1), env.set_quality(weight, utility)
            if kind == "random":
                env.step_random(V, 99)
            else:
                ctl = Q.controller(env, kind)
                env.step_mpc(ctl, V) if isinstance(ctl, A.BatchedMPCController) else env.step_rule(ctl, V)
            rec = ql.records(led)
            rows.append(dict(utility=utility, weight=weight, controller=kind, qoe_q=float(rec["qoe_q"].mean())))
            print(json.dumps(rows[-1]), flush=True)
            del env, led, ql
            torch.cuda.empty_cache()
        best = {}
        for beam in WIDTHS:
            G = min(a.chunk, N)
            env = make_env(G * beam * M, traces, False)
            env.set_quality(weight, utility)
            hs = A.HindsightSearch(env, beam)
            qoe, hist, valid = [], torch.zeros(M, dtype=torch.int64), 0
            for g0 in range(0, N, G):
                t, o = tid_t[g0:g0 + G], off_t[g0:g0 + G]
                if t.numel() < G:                                  # the last chunk: pad with its first pair, drop the padding
                    pad = G - t.numel()
                    t, o = torch.cat([t, t[:1].expand(pad)]), torch.cat([o, o[:1].expand(pad)])
                res = hs.run(t, o)
                n = min(G, N - g0)
                qoe.append(res["qoe"][:n].cpu())
                valid += int(res["valid"][:n].sum())
                hist += torch.bincount(res["actions"][:, :n].reshape(-1).long().cpu(), minlength=M)
            best[beam] = torch.cat(qoe)
            rows.append(dict(utility=utility, weight=weight, controller=f"hindsight, beam {beam}", beam=beam,
                             qoe_q=float(best[beam].mean()), pairs_with_a_result=valid, action_histogram=hist.tolist()))
            print(json.dumps(rows[-1]), flush=True)
            del env, hs
            torch.cuda.empty_cache()
        widest = best[max(WIDTHS)]
        for r in rows:
            if r["utility"] == utility and "beam" in r:
                r["share_equal_to_widest"] = float((best[r["beam"]] == widest).double().mean())
                r["share_worse_than_widest"] = float((best[r["beam"]] > widest).double().mean())
                r["share_better_than_widest"] = float((best[r["beam"]] < widest).double().mean())
    res = dict(device=torch.cuda.get_device_name(0), lanes=N, chunk=a.chunk, video_length=V, ladder=bench.LADDER,
               weights=bench.WEIGHTS, widths=list(WIDTHS), rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "hindsight_study.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
