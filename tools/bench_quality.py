#!/usr/bin/env python3
"""The quality model's throughput cost (include/abr_env.h: abr_episode_quality) on bench.py's workload (48-chunk episodes,
6 rates, 1 024 synthetic 1 000-point traces, auto_reset), 48 decisions per launch: step_random with the model off, on
(weight 1, the identity utility, 1 row) and on next to an episode ledger (8 rows each); step_policy (W = 8, 64/64 hidden)
with the model off and on.  Each row is R launches between two HIP events after warm-ups; the cases alternate, --repeats
rounds; medians reported.  Writes OUT/quality_bench.json and prints it.

    python tools/bench_quality.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 5] [--warmup 2] [--repeats 3]
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

CASES = {"random": ("off", "quality", "quality+ledger"), "policy": ("off", "quality")}


def make_env(N, traces, case):
    mpd = A.MPD(bench.V, bench.L, bench.MAX_BUFFER, bench.START_UP, A.Chunk(bench.LADDER))
    env = A.BatchedABREnv(mpd, A.QOEMetric(*bench.WEIGHTS), A.NetworkInfo(bench.INTERVAL, traces), N, device="cuda",
                          auto_reset=True)
    tid, off = bench.lane_assignment(0, N, traces)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    if case == "quality+ledger":
        env.set_episode_ledger(8)
    if case != "off":
        env.set_quality(1.0, "identity")
    return env


def policy(env):
    torch.manual_seed(0)
    F, mods = 4 + 8 + len(bench.LADDER), []
    for w in (64, 64):
        mods += [torch.nn.Linear(F, w), torch.nn.ReLU()]
        F = w
    net = torch.nn.Sequential(*mods, torch.nn.Linear(F, len(bench.LADDER)))
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
    traces = bench.synth_traces()
    rows = []
    for N in a.lanes:
        names = sorted({c for v in CASES.values() for c in v})
        envs = {c: make_env(N, traces, c) for c in names}
        ctls = {c: policy(envs[c]) for c in CASES["policy"]}
        outs = {c: envs[c].bind_out(envs[c]._rollout_out(a.fuse, want_actions=False)) for c in CASES["random"]}
        pouts = {c: envs[c]._rollout_out(a.fuse, want_obs=True, want_actions=False) for c in CASES["policy"]}
        for c in pouts:
            pouts[c]["features"] = pouts[c]["scores"] = None
        runs = {(k, c): [] for k, v in CASES.items() for c in v}
        for r in range(a.repeats):
            for kind, cases in CASES.items():
                for c in cases:
                    env = envs[c]
                    fn = ((lambda env=env, c=c: env.step_random(a.fuse, 99, out=outs[c])) if kind == "random"
                          else (lambda env=env, c=c: env.step_policy(ctls[c], a.fuse, out=pouts[c])))
                    sec = timed(fn, a.launches, a.warmup)
                    runs[(kind, c)].append(N * a.fuse * a.launches / sec)
        for (kind, c), v in runs.items():
            ql = envs[c].quality
            rows.append(dict(lanes=N, kind=kind, case=c, env_steps_per_s=float(np.median(v)), runs=v,
                             quality_bytes=int(ql.blob.numel()) if ql is not None else 0,
                             episodes_recorded_per_lane=float(ql.count().double().mean()) if ql is not None else 0.0,
                             impl=envs[c].effective_impl(fused=True) if kind == "random" else "jump"))
        del envs, ctls, outs, pouts
        torch.cuda.empty_cache()
    for r in rows:
        base = next(x for x in rows if x["lanes"] == r["lanes"] and x["kind"] == r["kind"] and x["case"] == "off")
        r["vs_off"] = r["env_steps_per_s"] / base["env_steps_per_s"]
    res = dict(device=torch.cuda.get_device_name(0), fuse=a.fuse, video_length=bench.V, launches=a.launches,
               warmup=a.warmup, repeats=a.repeats, traces=len(traces), rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "quality_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
