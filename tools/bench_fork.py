#!/usr/bin/env python3
"""What a lane fork and a hindsight search cost (include/abr_env.h: abr_env_fork, abr_beam_select) on bench.py's workload
(48-chunk episodes, 6 rates, 1 024 synthetic 1 000-point traces).

fork    every lane forked at once under a seeded permutation inside groups of 96 lanes (the shape a beam of 16 produces),
        against workspace.clone() -- until now the only way to copy state -- in the same run: cases alternate after
        warm-ups, --repeats rounds of --launches calls between two HIP events, medians.  Bytes: a fork reads each lane's
        bytes twice and writes them twice (gather into the scratch, scatter out of it); a clone reads and writes the whole
        workspace once.  Shares of peak are against the HBM copy rate named in the result.
search  HindsightSearch.run at beam 16 (96 slots per group) against a loop of video_length single step() calls on the same
        lanes, the floor any per-decision search pays; env-steps/s = lanes x video_length / seconds.

Writes OUT/fork_bench.json and prints it.

    python tools/bench_fork.py OUT [--lanes 65536 1048576] [--launches 10] [--warmup 3] [--repeats 3]
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

HBM_PEAK = 8.0e12          # bytes/s, the HBM3E specification of the MI355X
HBM_COPY = 6.29e12         # bytes/s, the measured float4 copy rate of the same part
BEAM, GROUP = 16, 96


def make_env(N, traces):
    mpd = A.MPD(bench.V, bench.L, bench.MAX_BUFFER, bench.START_UP, A.Chunk(bench.LADDER))
    env = A.BatchedABREnv(mpd, A.QOEMetric(*bench.WEIGHTS), A.NetworkInfo(bench.INTERVAL, traces), N, device="cuda",
                          auto_reset=False)
    tid, off = bench.lane_assignment(0, N, traces)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    return env, tid, off


def lane_bytes(V):
    """Bytes of one lane that a fork moves: the workspace regions and the obs column (no quality model here)."""
    return 8 * 8 + 8 + 15 * 4 + 2 + V + 8 * V + 4 * 8 + 4 + 4 * 8


def group_permutation(N, seed=0):
    rng = np.random.default_rng(seed)
    src = np.arange(N, dtype=np.int32)
    for b in range(0, N, GROUP):
        e = min(N, b + GROUP)
        src[b:e] = b + rng.permutation(e - b)
    return src


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
    return s.elapsed_time(e) / 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true", help="a few launches of every case and no timing: for a kernel trace")
    a = ap.parse_args()
    traces = bench.synth_traces()
    V = bench.V
    fork_rows, search_rows = [], []
    for N in a.lanes:
        env, tid, off = make_env(N, traces)
        env.step_random(7, 3)                                  # mid-episode state in every lane
        src = torch.from_numpy(group_permutation(N)).cuda()
        keep = []

        def do_clone():
            keep[:] = [env.workspace.clone()]
        cases = {"fork": lambda: env.fork(src), "clone": do_clone}
        if a.trace_only:
            for fn in cases.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
        else:
            runs = {k: [] for k in cases}
            for _ in range(a.repeats):
                for k, fn in cases.items():
                    runs[k].append(timed(fn, a.launches, a.warmup))
            moved = {"fork": 4 * lane_bytes(V) * N, "clone": 2 * env.workspace.numel()}
            for k, v in runs.items():
                sec = float(np.median(v))
                fork_rows.append(dict(lanes=N, case=k, seconds=sec, runs=v, bytes_moved=moved[k], bytes_per_s=moved[k] / sec,
                                      share_of_hbm_peak=moved[k] / sec / HBM_PEAK, share_of_hbm_copy_rate=moved[k] / sec / HBM_COPY))
            f, c = (next(r for r in fork_rows if r["lanes"] == N and r["case"] == k) for k in ("fork", "clone"))
            f["vs_clone"] = f["seconds"] / c["seconds"]
            f["lane_bytes"] = lane_bytes(V)
            f["workspace_bytes"] = int(env.workspace.numel())
        # the search: beam 16 on as many whole groups as the lanes hold
        G = N // GROUP
        hs = A.HindsightSearch(env, BEAM)
        g_tid, g_off = torch.from_numpy(tid[:G].copy()), torch.from_numpy(off[:G].copy())
        acts = hs.actions

        def do_search():
            keep[:] = [hs.run(g_tid, g_off)]

        def do_steps():
            env.reset(torch.from_numpy(tid), torch.from_numpy(off))
            for _ in range(V):
                env.step(acts)
        scases = {"search": do_search, "steps": do_steps}
        if a.trace_only:
            for fn in scases.values():
                fn()
            torch.cuda.synchronize()
        else:
            runs = {k: [] for k in scases}
            for _ in range(a.repeats):
                for k, fn in scases.items():
                    runs[k].append(timed(fn, max(1, a.launches // 5), 1))
            for k, v in runs.items():
                sec = float(np.median(v))
                lanes = G * GROUP if k == "search" else N
                search_rows.append(dict(lanes=N, case=k, beam=BEAM, groups=G, lanes_used=lanes, seconds=sec, runs=v,
                                        env_steps_per_s=lanes * V / sec))
            s, b = (next(r for r in search_rows if r["lanes"] == N and r["case"] == k) for k in ("search", "steps"))
            s["vs_steps"] = s["env_steps_per_s"] / b["env_steps_per_s"]
        del env, hs, keep
        torch.cuda.empty_cache()
    if a.trace_only:
        return
    res = dict(device=torch.cuda.get_device_name(0), video_length=V, launches=a.launches, warmup=a.warmup, repeats=a.repeats,
               hbm_peak_bytes_per_s=HBM_PEAK, hbm_peak_source="HBM3E specification, 8.0 TB/s",
               hbm_copy_bytes_per_s=HBM_COPY, hbm_copy_source="measured float4 copy on the same part, 6.29 TB/s",
               fork=fork_rows, search=search_rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "fork_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
