#!/usr/bin/env python3
"""The size table's throughput cost (include/abr_env.h: abr_env_set_size_table) on bench.py's workload (48-chunk episodes,
6 rates, 1 024 synthetic 1 000-point traces, auto_reset), 48 fused random decisions per launch: no table against the table
S = ladder x chunk_length.  The downloads are identical, so the difference is the lookup and the routing of a sized handle
to the kernels' general instances.  A third case splits the two: no table, but max_ticks = 2^20 + 1, which fails the
host's proof for the unguarded chains and so runs the general instances as well (the tick table it asks for is larger; the
part of it a lane reads is the same).  Each row is R launches between two HIP events after warm-ups; the cases alternate,
--repeats rounds; medians reported.  Writes OUT/chunk_sizes_bench.json and prints it.

    python tools/bench_chunk_sizes.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 5] [--warmup 2] [--repeats 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import abrsimulator_amd as A  # noqa: E402
import bench  # noqa: E402

CASES = ("off", "general_no_table", "cbr_table")


def make_env(N, traces, case):
    mpd = A.MPD(bench.V, bench.L, bench.MAX_BUFFER, bench.START_UP, A.Chunk(bench.LADDER))
    sizes = np.tile(np.asarray(bench.LADDER, np.float64) * bench.L, (bench.V, 1)) if case == "cbr_table" else None
    env = A.BatchedABREnv(mpd, A.QOEMetric(*bench.WEIGHTS), A.NetworkInfo(bench.INTERVAL, traces), N, device="cuda",
                          auto_reset=True, chunk_sizes=sizes, max_ticks=(1 << 20) + 1 if case == "general_no_table" else 0)
    tid, off = bench.lane_assignment(0, N, traces)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    return env


def timed(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(launches):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--fuse", type=int, default=48)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    traces = bench.synth_traces()
    rows = []
    for N in a.lanes:
        envs = {c: make_env(N, traces, c) for c in CASES}
        outs = {c: envs[c].bind_out(envs[c]._rollout_out(a.fuse, want_actions=False)) for c in CASES}
        runs = {c: [] for c in CASES}
        for r in range(a.repeats):
            for c in CASES:
                sec = timed(lambda env=envs[c], c=c: env.step_random(a.fuse, 99, out=outs[c]), a.launches, a.warmup)
                runs[c].append(N * a.fuse * a.launches / sec)
        # the same seed from the same state: the two cases must have written the same rewards
        same = all(bool(torch.equal(outs["off"]["reward"], outs[c]["reward"])) for c in CASES)
        for c in CASES:
            rows.append(dict(lanes=N, case=c, env_steps_per_s=float(np.median(runs[c])), runs=runs[c],
                             impl=envs[c].effective_impl(fused=True), general_instance=envs[c].general_instance(fused=True),
                             same_rewards_as_off=same))
        del envs, outs
        torch.cuda.empty_cache()
    for r in rows:
        base = next(x for x in rows if x["lanes"] == r["lanes"] and x["case"] == "off")
        r["vs_off"] = r["env_steps_per_s"] / base["env_steps_per_s"]
    res = dict(device=torch.cuda.get_device_name(0), fuse=a.fuse, video_length=bench.V, launches=a.launches,
               warmup=a.warmup, repeats=a.repeats, traces=len(traces), rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "chunk_sizes_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
