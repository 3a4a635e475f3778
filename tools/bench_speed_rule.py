#!/usr/bin/env python3
"""What the speed controllers cost, and what they do to QoE.

Throughput: step_random (fused, auto_reset) on bench.py's workload -- 48-chunk episodes, 1 024 synthetic 1 000-point
traces, 6 rates -- with one constant speed 1.0, a 48-row speed schedule (abr_env_set_speed_schedule) and a speed rule
(abr_env_set_speed_rule), at each lane count under impl='auto'; plus step_mpc rows.  Each row: W untimed warm-up launches,
then R launches between two HIP events, the region closed by a synchronise.

QoE study: one episode of --qoe-lanes lanes under MPC and under BBA-0, for the constant speed and a few rules fixed up
front (RULES); mean episode QoE and its four terms (rebuffer, variance, start-up, latency) as run() weighs them.
Writes OUT/bench_speed_rule.json and prints it.

    python tools/bench_speed_rule.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 20] [--warmup 3]
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
LSC = A.LatencySpeedController
# the rule of the throughput rows: catch up above 10 s of latency, slow down under 2 s of buffer
BENCH_RULE = LSC.catch_up(10.0, fast=1.1, low_buffer=2.0, slow=0.9)
# the QoE study's settings, chosen before any run
RULES = {"constant_1.0": None,
         "catch_up_10s_1.1x": LSC.catch_up(10.0, fast=1.1),
         "catch_up_10s_1.1x_slow_below_2s_0.9x": BENCH_RULE,
         "slow_below_2s_0.9x": LSC((), (2.0,), ((0.9, 1.0),))}


def make_env(N, traces, speed_mode, auto_reset=True, impl="auto"):
    mpd = A.MPD(V, L, MAX_BUFFER, START_UP, A.Chunk(LADDER))
    speed = 1.0
    if speed_mode == "schedule":
        speed = torch.from_numpy(np.random.default_rng(3).choice([0.9, 1.0, 1.1], (V, N)))
    env = A.BatchedABREnv(mpd, A.QOEMetric(*WEIGHTS), A.NetworkInfo(INTERVAL, traces), N, device="cuda",
                          auto_reset=auto_reset, impl=impl, speed=speed)
    if speed_mode == "rule":
        env.set_speed_controller(BENCH_RULE)
    elif isinstance(speed_mode, LSC):
        env.set_speed_controller(speed_mode)
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


def qoe_terms(env):
    f = env.observe_f64()
    q = env.episode_qoe().double()
    rb, su, lat = f["rebuffer_time"], f["start_up_time"], f["average_latency"]
    var = (q - WEIGHTS[0] * rb - WEIGHTS[2] * su - WEIGHTS[3] * lat) / WEIGHTS[1]
    m = lambda t: float(t.double().mean())
    return dict(qoe=m(q), rebuffer_time=m(rb), variance=m(var), start_up_time=m(su), average_latency=m(lat),
                mean_speed=None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--qoe-lanes", type=int, default=65536)
    ap.add_argument("--fuse", type=int, default=48)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    rows = []
    for N in a.lanes:
        for kind in ["random", "mpc"] if N == a.lanes[0] else ["random"]:
            for mode in ("constant", "schedule", "rule"):
                env = make_env(N, traces, mode)
                out = dict(obs=torch.empty(a.fuse, 8, N, device="cuda"), reward=torch.empty(a.fuse, N, device="cuda"),
                           done=torch.empty(a.fuse, N, dtype=torch.uint8, device="cuda"),
                           actions=torch.empty(a.fuse, N, dtype=torch.int32, device="cuda"))
                if kind == "random":
                    b = env.bind_out(out)
                    launch = (lambda e=env, b=b: e.step_random(a.fuse, SEED, out=b))
                else:
                    ctl = A.BatchedMPCController(A.EnvPlayer(env), horizon=5, clip_horizon=True)
                    launch = (lambda e=env, c=ctl, o=out: e.step_mpc(c, a.fuse, out=o))
                t = timed(launch, a.warmup, a.launches)
                row = dict(rollout=kind, speed=mode, lanes=N, fuse=a.fuse, launches=a.launches, warmup=a.warmup,
                           seconds=t, impl=env.effective_impl(fused=True),
                           env_steps_per_s=N * a.fuse * a.launches / t, us_per_launch=1e6 * t / a.launches)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del env, out
                torch.cuda.empty_cache()
    for r in rows:
        base = [x for x in rows if x["speed"] == "constant" and x["lanes"] == r["lanes"] and x["rollout"] == r["rollout"]]
        sched = [x for x in rows if x["speed"] == "schedule" and x["lanes"] == r["lanes"] and x["rollout"] == r["rollout"]]
        r["vs_constant"] = r["env_steps_per_s"] / base[0]["env_steps_per_s"]
        r["vs_schedule"] = r["env_steps_per_s"] / sched[0]["env_steps_per_s"]
    study = []
    N = a.qoe_lanes
    for name, rule in RULES.items():
        for abr in ("mpc", "bba0"):
            env = make_env(N, traces, rule if rule is not None else "constant", auto_reset=False)
            if rule is not None:
                env.set_speed_controller(rule, log_rows=V + 4)
                env.reset(env.trace_id, env.start_offset)
            if abr == "mpc":
                env.step_mpc(A.BatchedMPCController(A.EnvPlayer(env), horizon=5, clip_horizon=True), V)
            else:
                env.step_rule(A.BufferBasedController(A.EnvPlayer(env)), V)
            row = dict(setting=name, rule=repr(rule) if rule is not None else "speed 1.0", abr=abr, lanes=N,
                       **qoe_terms(env))
            log = env.speed_log()
            if log is not None:
                row["mean_speed"] = float(log[log > 0].mean())
            study.append(row)
            print(json.dumps(row), flush=True)
            del env
            torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), seed=SEED, workload=dict(video_length=V, chunk_length=L,
               max_buffer=MAX_BUFFER, start_up_length=START_UP, interval=INTERVAL, n_traces=1024, trace_len=1000,
               ladder=LADDER, weights=WEIGHTS, auto_reset=True), bench_rule=repr(BENCH_RULE), rows=rows,
               qoe_study=study)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_speed_rule.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
