#!/usr/bin/env python3
"""What a lookahead label costs (include/abr_env.h: abr_env_lookahead_select) on bench.py's workload (48-chunk episodes, 6
rates, 1 024 synthetic 1 000-point traces), lanes in mid-episode (seven random decisions in).

lookahead  LookaheadExpert.labels(want_q=True) at --lanes x --horizons: cases alternate after warm-ups, --repeats rounds of
           calls between two HIP events, medians and the spread (max - min over the median).  Tree nodes per call are
           computed here from the shapes: lanes x (M + M^2 + ... + M^h); a node is one lanej_step without the stores.
env        the environment kernel in the same session: fused random rollouts of 48 decisions (auto_reset), env-steps/s =
           lanes x 48 / seconds.  Nodes/s over env-steps/s is how a tree step compares with a stored step.
by_hand    what a user does without the entry, at horizon 3 only (it grows by M^h): state_dict(), then per sequence
           load_state_dict + one step_script launch + observe_f64, and a last load_state_dict.

Writes OUT/lookahead_bench.json and prints it.  --trace-only: a few calls of every lookahead case and no timing, for a
kernel trace (rocprofv3 --kernel-trace --stats, a run of its own).

    python tools/bench_lookahead.py OUT [--lanes 65536 1048576] [--horizons 3 4 5] [--warmup 1] [--repeats 3]
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import abrsimulator_amd as A  # noqa: E402
import bench  # noqa: E402

BY_HAND_HORIZON = 3


def make_env(N, traces, auto_reset):
    mpd = A.MPD(bench.V, bench.L, bench.MAX_BUFFER, bench.START_UP, A.Chunk(bench.LADDER))
    env = A.BatchedABREnv(mpd, A.QOEMetric(*bench.WEIGHTS), A.NetworkInfo(bench.INTERVAL, traces), N, device="cuda",
                          auto_reset=auto_reset)
    tid, off = bench.lane_assignment(0, N, traces)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    return env


def nodes_per_lane(M, h):
    return sum(M ** j for j in range(1, h + 1))


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / 1e3 / calls


def by_hand(env, H):
    M, N = env.n_rates, env.n_lanes
    sd = env.state_dict()
    keep = None
    for seq in itertools.product(range(M), repeat=H):
        env.load_state_dict(sd)
        out = env.step_script(torch.tensor(seq, dtype=torch.int32, device="cuda").reshape(H, 1).repeat(1, N))
        keep = (out["reward"], env.observe_f64()["average_latency"])
    env.load_state_dict(sd)
    return keep


def summary(v):
    sec = float(np.median(v))
    return dict(seconds=sec, runs=v, spread=(max(v) - min(v)) / sec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--horizons", type=int, nargs="+", default=[3, 4, 5])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    traces = bench.synth_traces()
    V, M = bench.V, len(bench.LADDER)
    look, envr, hand = [], [], []
    for N in a.lanes:
        env = make_env(N, traces, False)
        env.step_random(7, 3)                                  # mid-episode state in every lane
        exps = {h: A.LookaheadExpert(A.EnvPlayer(env), h) for h in a.horizons}
        keep = []
        cases = {}
        for h in a.horizons:
            def label(h=h):
                keep[:] = [exps[h].labels(want_q=True)]
            cases[h] = label
        if a.trace_only:
            for fn in cases.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            del env
            torch.cuda.empty_cache()
            continue
        # calls per timing: about 2e9 nodes' worth, at least one, so that a window is never a few microseconds
        calls = {h: int(max(1, min(20, 2e9 // (N * nodes_per_lane(M, h))))) for h in a.horizons}
        runs = {h: [] for h in a.horizons}
        for _ in range(a.repeats):
            for h, fn in cases.items():
                runs[h].append(timed(fn, calls[h], a.warmup))
        for h, v in runs.items():
            nodes = N * nodes_per_lane(M, h)
            r = dict(lanes=N, horizon=h, calls_per_timing=calls[h], nodes_per_call=nodes, leaves_per_lane=M ** h, **summary(v))
            r["nodes_per_s"] = nodes / r["seconds"]
            r["labels_per_s"] = N / r["seconds"]
            look.append(r)
            print(json.dumps(r), flush=True)
        lab = exps[a.horizons[0]].labels()
        labelled = float((lab["action"] >= 0).double().mean())
        # by hand, horizon 3
        v = [timed(lambda: by_hand(env, BY_HAND_HORIZON), 1, 1 if k == 0 else 0) for k in range(a.repeats)]
        r = dict(lanes=N, horizon=BY_HAND_HORIZON, sequences=M ** BY_HAND_HORIZON, launches=3 * M ** BY_HAND_HORIZON, **summary(v))
        same = next((x for x in look if x["lanes"] == N and x["horizon"] == BY_HAND_HORIZON), None)
        if same:
            r["lookahead_speedup"] = r["seconds"] / same["seconds"]
        hand.append(r)
        print(json.dumps(r), flush=True)
        del env, exps
        torch.cuda.empty_cache()
        # the environment kernel, same session
        env = make_env(N, traces, True)
        out = env.bind_out(env._rollout_out(V, want_actions=False))
        v = [timed(lambda: env.step_random(V, 11, out=out), 5, a.warmup) for _ in range(a.repeats)]
        r = dict(lanes=N, fuse=V, impl=env.effective_impl(True), **summary(v))
        r["env_steps_per_s"] = N * V / r["seconds"]
        envr.append(r)
        print(json.dumps(r), flush=True)
        for x in look:
            if x["lanes"] == N:
                x["nodes_per_env_step"] = x["nodes_per_s"] / r["env_steps_per_s"]
                x["share_of_lanes_labelled"] = labelled
        del env, out
        torch.cuda.empty_cache()
    if a.trace_only:
        return
    res = dict(device=torch.cuda.get_device_name(0), video_length=V, n_rates=M, warmup=a.warmup, repeats=a.repeats,
               lookahead=look, env=envr, by_hand=hand)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "lookahead_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
