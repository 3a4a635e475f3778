#!/usr/bin/env python3
"""Where a true-future teacher with a short horizon sits between the best rule and the hindsight bound:
tools/quality_study.py's and tools/hindsight_study.py's settings (one episode of bench.py's workload over --lanes (trace,
offset) pairs; weight 1 with the "identity" utility and weight 1 with "log"), with the lookahead expert
(abrsimulator_amd/expert.py: LookaheadExpert) driving the environment closed loop: at every call site the expert labels
every lane's state and the environment takes the labels.  Horizons 1..5, fixed here before any run.  Per setting and
horizon: the mean over pairs of qoe_q = qoe - weight * quality, the action histogram, and the lanes that met a state with
no label (they take bitrate 0 there).  The rows on record from those two studies are printed beside.  Writes
OUT/lookahead_study.json and prints each row.

    python tools/lookahead_study.py OUT [--lanes 65536]
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

HORIZONS = (1, 2, 3, 4, 5)
# mean qoe_q on the same 65 536 pairs (profiles/quality_study.json, profiles/hindsight_study.json)
ON_RECORD = {"identity": {"mpc": 79.81, "rate": 23.48, "hindsight, beam 64": -15.35},
             "log": {"mpc": 94.21, "rate": 44.12, "hindsight, beam 64": 7.39}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, default=65536)
    a = ap.parse_args()
    N, V, M = a.lanes, bench.V, len(bench.LADDER)
    traces = bench.synth_traces()
    tid, off = bench.lane_assignment(0, N, traces)
    tid_t, off_t = torch.from_numpy(tid), torch.from_numpy(off)
    rows = []
    for utility, weight in Q.SETTINGS:
        for H in HORIZONS:
            mpd = A.MPD(V, bench.L, bench.MAX_BUFFER, bench.START_UP, A.Chunk(bench.LADDER))
            env = A.BatchedABREnv(mpd, A.QOEMetric(*bench.WEIGHTS), A.NetworkInfo(bench.INTERVAL, traces), N, device="cuda",
                                  auto_reset=False)
            env.reset(tid_t, off_t)
            led, ql = env.set_episode_ledger(1), env.set_quality(weight, utility)
            exp = A.LookaheadExpert(A.EnvPlayer(env), H)
            hist, unlabelled = torch.zeros(M, dtype=torch.int64, device="cuda"), 0
            for _ in range(V):
                act = exp.next_bitrate()
                none = act < 0
                unlabelled += int(none.sum())
                act = torch.where(none, torch.zeros_like(act), act)
                hist += torch.bincount(act.long(), minlength=M)
                env.step(act)
            rec = ql.records(led)
            rows.append(dict(utility=utility, weight=weight, controller=f"lookahead, horizon {H}", horizon=H,
                             qoe_q=float(rec["qoe_q"].mean()), qoe=float(rec["qoe"].mean()), episodes=int(rec["qoe_q"].numel()),
                             states_without_a_label=unlabelled, action_histogram=hist.tolist()))
            print(json.dumps(rows[-1]), flush=True)
            del env, led, ql, exp
            torch.cuda.empty_cache()
        for k, v in ON_RECORD[utility].items():
            rows.append(dict(utility=utility, weight=weight, controller=k, qoe_q=v, on_record=True))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), lanes=N, video_length=V, ladder=bench.LADDER, weights=bench.WEIGHTS,
               horizons=list(HORIZONS), rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "lookahead_study.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
