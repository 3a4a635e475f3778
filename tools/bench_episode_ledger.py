#!/usr/bin/env python3
"""The episode ledger's throughput cost (include/abr_env.h: abr_episode_ledger): fused rollouts of step_random and
step_policy (W = 8, 64/64 hidden), 48 decisions per launch, under auto_reset with V = 8-chunk episodes so that every lane
ends six episodes per launch, over a corpus of 1 024 synthetic 1 000-point traces, in two cases: no ledger installed, and
a ledger of 8 rows per lane (which wraps: the ring's slots and the totals are rewritten all the time, the steady state of
a long collection).  Each row is R launches between two HIP events after warm-ups; the cases alternate, --repeats rounds;
medians reported.  Writes OUT/episode_ledger_bench.json and prints it.

    python tools/bench_episode_ledger.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 5] [--warmup 2] [--repeats 3]
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
V, L, MAX_BUFFER, START_UP, INTERVAL, WEIGHTS = 8, 4.0, 20.0, 8.0, 1.0, [4.3, 1.0, 1.0, 0.1]
CASES = ("off", "rows8")


def make_env(N, traces, case):
    mpd = A.MPD(V, L, MAX_BUFFER, START_UP, A.Chunk(LADDER))
    env = A.BatchedABREnv(mpd, A.QOEMetric(*WEIGHTS), A.NetworkInfo(INTERVAL, traces), N, device="cuda", auto_reset=True)
    rng = np.random.default_rng(7)
    env.reset(torch.from_numpy((np.arange(N) % len(traces)).astype(np.int32)),
              torch.from_numpy(rng.integers(0, 1000, N).astype(np.int32)))
    if case == "rows8":
        env.set_episode_ledger(8)
    return env


def policy(env):
    torch.manual_seed(0)
    F, mods = 4 + 8 + len(LADDER), []
    for w in (64, 64):
        mods += [torch.nn.Linear(F, w), torch.nn.ReLU()]
        F = w
    net = torch.nn.Sequential(*mods, torch.nn.Linear(F, len(LADDER)))
    return A.PolicyController.from_module(A.EnvPlayer(env), net, window=8, explore=0.0, seed=1)


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
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000) for _ in range(1024)]
    rows = []
    for N in a.lanes:
        envs = {c: make_env(N, traces, c) for c in CASES}
        ctls = {c: policy(envs[c]) for c in CASES}
        outs = {c: envs[c].bind_out(envs[c]._rollout_out(a.fuse, want_actions=False)) for c in CASES}
        pouts = {c: envs[c]._rollout_out(a.fuse, want_obs=True, want_actions=False) for c in CASES}
        for c in CASES:
            pouts[c]["features"] = pouts[c]["scores"] = None
        runs = {(k, c): [] for k in ("random", "policy") for c in CASES}
        for r in range(a.repeats):
            for kind in ("random", "policy"):
                for c in CASES:
                    env = envs[c]
                    fn = ((lambda env=env, c=c: env.step_random(a.fuse, 99, out=outs[c])) if kind == "random"
                          else (lambda env=env, c=c: env.step_policy(ctls[c], a.fuse, out=pouts[c])))
                    sec = timed(fn, a.launches, a.warmup)
                    runs[(kind, c)].append(N * a.fuse * a.launches / sec)
        for (kind, c), v in runs.items():
            led = envs[c].episode_ledger
            rows.append(dict(lanes=N, kind=kind, case=c, env_steps_per_s=float(np.median(v)), runs=v,
                             ledger_bytes=int(led.blob.numel()) if led is not None else 0,
                             episodes_recorded_per_lane=float(led.count().double().mean()) if led is not None else 0.0,
                             impl=envs[c].effective_impl(fused=True) if kind == "random" else "jump"))
        del envs, ctls, outs, pouts
        torch.cuda.empty_cache()
    for r in rows:
        base = next(x for x in rows if x["lanes"] == r["lanes"] and x["kind"] == r["kind"] and x["case"] == "off")
        r["vs_off"] = r["env_steps_per_s"] / base["env_steps_per_s"]
    res = dict(device=torch.cuda.get_device_name(0), fuse=a.fuse, video_length=V, launches=a.launches,
               warmup=a.warmup, repeats=a.repeats, traces=len(traces), trace_points=1000, rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "episode_ledger_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
