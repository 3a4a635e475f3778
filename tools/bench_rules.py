#!/usr/bin/env python3
"""Throughput of the fused rule rollouts (abr_env_step_rule: BUFFER / RATE / BOLA) next to the built-in random policy on the
SAME kernel (step_random with impl='jump'), same environment, fuse and seed: bench.py's workload (48-chunk episodes under
auto_reset, 1 024 synthetic 1 000-point traces, 6 rates).  Each row: W untimed warm-up launches, then R launches between two
HIP events, the region closed by a synchronise.  Writes OUT/bench_rules.json and prints it.

    python tools/bench_rules.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 20] [--warmup 3]
    python tools/bench_rules.py OUT --only bola --lanes 65536 --launches 3     (a short run, e.g. under rocprofv3)
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

LADDER = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
V, L, MAX_BUFFER, START_UP, INTERVAL, WEIGHTS = 48, 4.0, 20.0, 8.0, 1.0, [4.3, 1.0, 1.0, 0.1]
SEED = 1234
# rows: the built-in random policy on the one-thread-per-lane kernel, then each rule with its defaults and with the second
# parameter set of tests/test_rules_gpu.py.  On this live-stream workload the buffer stays below ~2 chunks, so the default
# BBA-0 (reservoir 5 s) and BOLA (v ~ 2.1) answer rate 0 almost everywhere: short downloads, not a cheaper kernel
SPECS = {"random": None, "buffer": ("buffer", {}), "buffer_r1_k6": ("buffer", dict(reservoir=1.0, cushion=6.0)),
         "rate": ("rate", {}), "bola": ("bola", {}), "bola_v5_gp1": ("bola", dict(gamma_p=1.0, v=5.0))}


def make_env(N, traces, impl):
    mpd = A.MPD(V, L, MAX_BUFFER, START_UP, A.Chunk(LADDER))
    env = A.BatchedABREnv(mpd, A.QOEMetric(*WEIGHTS), A.NetworkInfo(INTERVAL, traces), N, device="cuda",
                          auto_reset=True, impl=impl)
    rng = np.random.default_rng(7)
    tid = torch.from_numpy((np.arange(N) % len(traces)).astype(np.int32))
    off = torch.from_numpy(rng.integers(0, 1000, N).astype(np.int32))
    env.reset(tid, off)
    return env


def timed(launch, warmup, launches):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        launch()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--fuse", type=int, default=48)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=list(SPECS), nargs="+", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    rows = []
    for N in a.lanes:
        kinds = a.only or list(SPECS)
        for kind in kinds:
            env = make_env(N, traces, "jump" if kind == "random" else "auto")
            out = dict(obs=torch.empty(a.fuse, 8, N, device="cuda"), reward=torch.empty(a.fuse, N, device="cuda"),
                       done=torch.empty(a.fuse, N, dtype=torch.uint8, device="cuda"),
                       actions=torch.empty(a.fuse, N, dtype=torch.int32, device="cuda"))
            if kind == "random":
                b = env.bind_out(out)
                launch = (lambda e=env, b=b: e.step_random(a.fuse, SEED, out=b))
                ctl = None
            else:
                p = A.EnvPlayer(env)
                cls, kw = SPECS[kind]
                ctl = {"buffer": A.BufferBasedController, "rate": A.RateBasedController, "bola": A.BolaController}[cls](p, **kw)
                launch = (lambda e=env, c=ctl, o=out: e.step_rule(c, a.fuse, out=o))
            t = timed(launch, a.warmup, a.launches)
            acts = out["actions"].cpu().numpy()
            row = dict(kind=kind, lanes=N, fuse=a.fuse, launches=a.launches, warmup=a.warmup, seconds=t,
                       kernel=("env_jump_kernel<2>" if kind == "random" else "env_jump_kernel<4>"),
                       env_steps_per_s=N * a.fuse * a.launches / t, us_per_launch=1e6 * t / a.launches,
                       action_histogram=np.bincount(acts[acts >= 0], minlength=len(LADDER)).tolist())
            rows.append(row)
            print(json.dumps(row), flush=True)
            del env, out
            torch.cuda.empty_cache()
    for r in rows:
        base = [x for x in rows if x["kind"] == "random" and x["lanes"] == r["lanes"]]
        if base:
            r["vs_random_jump"] = r["env_steps_per_s"] / base[0]["env_steps_per_s"]
    res = dict(device=torch.cuda.get_device_name(0), seed=SEED, workload=dict(video_length=V, chunk_length=L,
               max_buffer=MAX_BUFFER, start_up_length=START_UP, interval=INTERVAL, n_traces=1024, trace_len=1000,
               ladder=LADDER, auto_reset=True), rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_rules.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
