#!/usr/bin/env python3
"""FastMPC (abr_fastmpc_build, abr_env_step_fastmpc) on bench.py's workload (48-chunk episodes under auto_reset, 1 024
synthetic 1 000-point traces, 6 rates, H = 5, W = 5):
  - table build time per grid (16^2 .. 128^2 points) and layout: W untimed builds, then R builds each between two HIP
    events, median and spread;
  - fused rollout env-steps/s of FastMPC next to RATE, harmonic MPC (step_mpc) and RobustMPC (step_mpc_robust) on the same
    environment, fuse and lanes (R launches between two events after W warm-ups, the whole row repeated --repeats times);
  - decision agreement: one whole episode per lane driven by FastMPC; at every call site the share of live lanes whose
    FastMPC action equals abr_mpc_select_robust on a zeroed state (the exact search on the same windowed estimate);
  - mean episode_qoe() of each controller over one whole episode per lane from the same start.
Writes OUT/bench_fastmpc.json and prints it.

    python tools/bench_fastmpc.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 5] [--warmup 2] [--repeats 3]
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
    if kind == "fastmpc":
        return A.FastMPCController(p, horizon=H, window=WINDOW)
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


def build_times(traces, warmup, launches):
    env = make_env(1024, traces, True)
    rows = []
    for n in (16, 32, 64, 128):
        for layout in ("uniform", "per_chunk"):
            ctl = A.FastMPCController(A.EnvPlayer(env), horizon=H, window=WINDOW, layout=layout,
                                      buffer_points=np.linspace(0.0, MAX_BUFFER + L, n),
                                      tput_points=np.geomspace(min(LADDER) / 4, max(LADDER) * 4, n))
            ts = sorted(timed(lambda: ctl.build(force=True), warmup, 1) for _ in range(launches))
            e = ctl.entries()
            row = dict(points=n, layout=layout, entries=int(e.numel()), build_ms_median=1e3 * ts[len(ts) // 2],
                       build_ms_min=1e3 * ts[0], build_ms_max=1e3 * ts[-1], builds=launches)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def agreement(traces, N):
    """FastMPC drives one episode per lane; at every call site its action is compared with the exact search on the same
    windowed harmonic estimate (RobustMPC on a zeroed state, no decision read as bitrate 0)."""
    env = make_env(N, traces, False)
    fm = controller(env, "fastmpc")
    rob = controller(env, "robust_mpc")
    same = live = 0
    per_step = []
    for _ in range(V):
        a = fm.next_bitrate()
        rob.reset_state()
        r = rob.next_bitrate()
        r = torch.where(r < 0, torch.zeros_like(r), r)
        ok = env.done == 0
        s, n = int(((a == r) & ok).sum()), int(ok.sum())
        same, live = same + s, live + n
        per_step.append(s / max(n, 1))
        env.step(a)
    return dict(lanes=N, call_sites=live, agreement=same / live, agreement_min_step=min(per_step),
                agreement_max_step=max(per_step))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--fuse", type=int, default=48)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--qoe-lanes", type=int, default=65536)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    builds = build_times(traces, a.warmup, a.launches)
    rows = []
    for N in a.lanes:
        for kind in ("fastmpc", "rate", "mpc", "robust_mpc"):
            env = make_env(N, traces, True)
            ctl = controller(env, kind)
            out = dict(obs=torch.empty(a.fuse, 8, N, device="cuda"), reward=torch.empty(a.fuse, N, device="cuda"),
                       done=torch.empty(a.fuse, N, dtype=torch.uint8, device="cuda"),
                       actions=torch.empty(a.fuse, N, dtype=torch.int32, device="cuda"))
            rollout(env, ctl, 1, out)                     # FastMPC builds its table here, outside the timed region
            ts = [timed(lambda: rollout(env, ctl, a.fuse, out), a.warmup, a.launches) for _ in range(a.repeats)]
            rates = sorted(N * a.fuse * a.launches / t for t in ts)
            acts = out["actions"].cpu().numpy()
            row = dict(kind=kind, lanes=N, fuse=a.fuse, launches=a.launches, warmup=a.warmup, repeats=a.repeats,
                       env_steps_per_s=rates[len(rates) // 2], env_steps_per_s_all=rates,
                       action_histogram=np.bincount(acts[acts >= 0], minlength=len(LADDER)).tolist())
            rows.append(row)
            print(json.dumps(row), flush=True)
            del env, ctl, out
            torch.cuda.empty_cache()
    for r in rows:
        base = {k: [x for x in rows if x["kind"] == k and x["lanes"] == r["lanes"]][0]["env_steps_per_s"]
                for k in ("mpc", "rate")}
        r["vs_mpc"], r["vs_rate"] = r["env_steps_per_s"] / base["mpc"], r["env_steps_per_s"] / base["rate"]
    agree = agreement(traces, a.qoe_lanes)
    print(json.dumps(agree), flush=True)
    qoe = []
    for kind in ("fastmpc", "mpc", "robust_mpc", "rate", "buffer", "bola"):
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
                             auto_reset=True), build=builds, throughput=rows, agreement=agree, qoe=qoe)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_fastmpc.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
