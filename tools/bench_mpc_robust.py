#!/usr/bin/env python3
"""Fused MPC rollouts with the reference's harmonic predictor (abr_env_step_mpc) and with RobustMPC's estimate
(abr_env_step_mpc_robust) on the same environment, fuse and lanes: bench.py's workload (48-chunk episodes under auto_reset,
1 024 synthetic 1 000-point traces, 6 rates, H = 5).  Each throughput row: W untimed warm-up launches, then R launches
between two HIP events, the region closed by a synchronise.  Then one whole episode per lane from the same start under
each controller -- harmonic MPC, RobustMPC and the three bitrate rules with their defaults -- and the mean of
episode_qoe() over the lanes.  Writes OUT/bench_mpc_robust.json and prints it.

    python tools/bench_mpc_robust.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 5] [--warmup 2] [--qoe-lanes 65536]
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
H, WINDOW = 5, 5


def make_env(N, traces, auto_reset):
    mpd = A.MPD(V, L, MAX_BUFFER, START_UP, A.Chunk(LADDER))
    env = A.BatchedABREnv(mpd, A.QOEMetric(*WEIGHTS), A.NetworkInfo(INTERVAL, traces), N, device="cuda",
                          auto_reset=auto_reset)
    rng = np.random.default_rng(7)
    tid = torch.from_numpy((np.arange(N) % len(traces)).astype(np.int32))
    off = torch.from_numpy(rng.integers(0, 1000, N).astype(np.int32))
    env.reset(tid, off)
    return env


def controller(env, kind):
    p = A.EnvPlayer(env)
    if kind == "mpc":
        return A.BatchedMPCController(p, horizon=H, clip_horizon=True)
    if kind == "robust_mpc":
        return A.BatchedMPCController(p, horizon=H, clip_horizon=True, method="robust", window=WINDOW)
    return {"buffer": A.BufferBasedController, "rate": A.RateBasedController, "bola": A.BolaController}[kind](p)


def rollout(env, ctl, n, out=None):
    return env.step_mpc(ctl, n, out=out) if isinstance(ctl, A.BatchedMPCController) else env.step_rule(ctl, n, out=out)


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
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--qoe-lanes", type=int, default=65536)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    rows = []
    for N in a.lanes:
        for kind in ("mpc", "robust_mpc"):
            env = make_env(N, traces, True)
            ctl = controller(env, kind)
            out = dict(obs=torch.empty(a.fuse, 8, N, device="cuda"), reward=torch.empty(a.fuse, N, device="cuda"),
                       done=torch.empty(a.fuse, N, dtype=torch.uint8, device="cuda"),
                       actions=torch.empty(a.fuse, N, dtype=torch.int32, device="cuda"))
            t = timed(lambda: rollout(env, ctl, a.fuse, out), a.warmup, a.launches)
            acts = out["actions"].cpu().numpy()
            row = dict(kind=kind, lanes=N, fuse=a.fuse, launches=a.launches, warmup=a.warmup, seconds=t,
                       env_steps_per_s=N * a.fuse * a.launches / t, us_per_decision=1e6 * t / (a.launches * a.fuse),
                       action_histogram=np.bincount(acts[acts >= 0], minlength=len(LADDER)).tolist())
            rows.append(row)
            print(json.dumps(row), flush=True)
            del env, ctl, out
            torch.cuda.empty_cache()
    for r in rows:
        base = [x for x in rows if x["kind"] == "mpc" and x["lanes"] == r["lanes"]]
        r["vs_mpc"] = r["env_steps_per_s"] / base[0]["env_steps_per_s"]
    qoe = []
    for kind in ("mpc", "robust_mpc", "buffer", "rate", "bola"):
        env = make_env(a.qoe_lanes, traces, False)
        out = rollout(env, controller(env, kind), V)
        q = env.episode_qoe().cpu().numpy()
        acts = out["actions"].cpu().numpy()
        row = dict(kind=kind, lanes=a.qoe_lanes, mean_episode_qoe=float(q.mean()), std_episode_qoe=float(q.std()),
                   action_histogram=np.bincount(acts[acts >= 0], minlength=len(LADDER)).tolist())
        qoe.append(row)
        print(json.dumps(row), flush=True)
        del env, out
        torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), horizon=H, window=WINDOW,
               workload=dict(video_length=V, chunk_length=L, max_buffer=MAX_BUFFER, start_up_length=START_UP,
                             interval=INTERVAL, weights=WEIGHTS, n_traces=1024, trace_len=1000, ladder=LADDER,
                             auto_reset=True), throughput=rows, qoe=qoe)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_mpc_robust.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
