#!/usr/bin/env python3
"""The learned policy (abr_env_step_policy) on bench.py's workload (48-chunk episodes under auto_reset, 1 024 synthetic
1 000-point traces, 6 rates):
  - fused rollout env-steps/s of step_policy (W = 8, 64/64 hidden, explore 0 and 0.1; policy_softmax: actions drawn
    from softmax(scores) on the device with the probs written, abr_env_step_policy_sampled) next to step_mpc (harmonic,
    H = 5) and step_rule (RATE), all in one process on the same workload, fuse and lanes; each row is R launches between
    two HIP events after W warm-ups, and the rows alternate, --repeats rounds;
  - per decision: the policy kernel alone (abr_env_policy_select, actions only), its sampled instance alone
    (abr_env_policy_select_sampled, actions and probs) and K1 alone (abr_env_step on fixed actions), each R x fuse
    launches between two events.
Writes OUT/NAME (default policy_bench.json) and prints it.

    python tools/bench_policy.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 5] [--warmup 2] [--repeats 3]
                                     [--name policy_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import abrsimulator_amd as A  # noqa: E402
from abrsimulator_amd import _lib  # noqa: E402

LADDER = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
V, L, MAX_BUFFER, START_UP, INTERVAL, WEIGHTS = 48, 4.0, 20.0, 8.0, 1.0, [4.3, 1.0, 1.0, 0.1]
H, WINDOW, HIDDEN = 5, 8, [64, 64]
KINDS = ("policy", "policy_softmax", "policy_explore", "mpc", "rate")


def make_env(N, traces):
    mpd = A.MPD(V, L, MAX_BUFFER, START_UP, A.Chunk(LADDER))
    env = A.BatchedABREnv(mpd, A.QOEMetric(*WEIGHTS), A.NetworkInfo(INTERVAL, traces), N, device="cuda",
                          auto_reset=True)
    rng = np.random.default_rng(7)
    tid = torch.from_numpy((np.arange(N) % len(traces)).astype(np.int32))
    off = torch.from_numpy(rng.integers(0, 1000, N).astype(np.int32))
    env.reset(tid, off)
    return env


def net():
    torch.manual_seed(0)
    F, mods = 4 + WINDOW + len(LADDER), []
    for w in HIDDEN:
        mods += [torch.nn.Linear(F, w), torch.nn.ReLU()]
        F = w
    return torch.nn.Sequential(*mods, torch.nn.Linear(F, len(LADDER)))


def controller(env, kind):
    p = A.EnvPlayer(env)
    if kind == "mpc":
        return A.BatchedMPCController(p, horizon=H, clip_horizon=True)
    if kind == "rate":
        return A.RateBasedController(p)
    return A.PolicyController.from_module(p, net(), window=WINDOW, explore=0.1 if kind == "policy_explore" else 0.0,
                                          seed=1, sample="softmax" if kind == "policy_softmax" else "argmax")


def rollout(env, ctl, n, out):
    if isinstance(ctl, A.PolicyController):
        return env.step_policy(ctl, n, out=out)
    if isinstance(ctl, A.BatchedMPCController):
        return env.step_mpc(ctl, n, out=out)
    return env.step_rule(ctl, n, out=out)


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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--name", default="policy_bench.json")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    rows, per_decision = [], []
    for N in a.lanes:
        envs = {k: make_env(N, traces) for k in KINDS}
        ctls = {k: controller(envs[k], k) for k in KINDS}
        out = dict(obs=torch.empty(a.fuse, 8, N, device="cuda"), reward=torch.empty(a.fuse, N, device="cuda"),
                   done=torch.empty(a.fuse, N, dtype=torch.uint8, device="cuda"),
                   actions=torch.empty(a.fuse, N, dtype=torch.int32, device="cuda"))
        out_p = dict(out, probs=torch.empty(a.fuse, len(LADDER), N, device="cuda"))   # what a trainer keeps
        ts = {k: [] for k in KINDS}
        for _ in range(a.repeats):                        # alternating: every kind once per round
            for k in KINDS:
                o = out_p if k == "policy_softmax" else out
                ts[k].append(timed(lambda: rollout(envs[k], ctls[k], a.fuse, o), a.warmup, a.launches))
        for k in KINDS:
            rates = sorted(N * a.fuse * a.launches / t for t in ts[k])
            row = dict(kind=k, lanes=N, fuse=a.fuse, launches=a.launches, warmup=a.warmup, repeats=a.repeats,
                       env_steps_per_s=rates[len(rates) // 2], env_steps_per_s_all=rates,
                       us_per_decision=1e6 * sorted(ts[k])[len(ts[k]) // 2] / (a.launches * a.fuse))
            rows.append(row)
            print(json.dumps(row), flush=True)
        # the two kernels of one policy decision, each alone
        env, ctl = envs["policy"], ctls["policy"]
        act = torch.empty(N, dtype=torch.int32, device="cuda")
        pol = ctl.bound(env)

        def select():
            env._call(env.lib.abr_env_policy_select, env._h, C.byref(pol), _lib.ptr(act), None, None)
        probs = torch.empty(len(LADDER), N, device="cuda")
        smp = ctls["policy_softmax"].sampling()

        def select_sampled():
            env._call(env.lib.abr_env_policy_select_sampled, env._h, C.byref(pol), C.byref(smp), _lib.ptr(act), None,
                      None, _lib.ptr(probs))
        fixed = torch.full((N,), 2, dtype=torch.int32, device="cuda")
        n = a.launches * a.fuse
        sel, sam = [], []
        for _ in range(a.repeats):                        # alternating
            sel.append(timed(select, a.warmup, n))
            sam.append(timed(select_sampled, a.warmup, n))
        k1 = [timed(lambda: env.step(fixed), a.warmup, n) for _ in range(a.repeats)]
        pd = dict(lanes=N, policy_kernel_us=1e6 * sorted(sel)[len(sel) // 2] / n,
                  sampled_kernel_us=1e6 * sorted(sam)[len(sam) // 2] / n, k1_us=1e6 * sorted(k1)[len(k1) // 2] / n,
                  policy_kernel_us_all=[1e6 * t / n for t in sel], sampled_kernel_us_all=[1e6 * t / n for t in sam],
                  k1_us_all=[1e6 * t / n for t in k1])
        per_decision.append(pd)
        print(json.dumps(pd), flush=True)
        del envs, ctls, out, env, ctl
        torch.cuda.empty_cache()
    for r in rows:
        base = {k: [x for x in rows if x["kind"] == k and x["lanes"] == r["lanes"]][0]["env_steps_per_s"]
                for k in ("mpc", "rate", "policy")}
        r["vs_mpc"], r["vs_rate"] = r["env_steps_per_s"] / base["mpc"], r["env_steps_per_s"] / base["rate"]
        r["vs_policy"] = r["env_steps_per_s"] / base["policy"]
    res = dict(device=torch.cuda.get_device_name(0), window=WINDOW, hidden=HIDDEN, horizon=H,
               workload=dict(video_length=V, chunk_length=L, max_buffer=MAX_BUFFER, start_up_length=START_UP,
                             interval=INTERVAL, weights=WEIGHTS, n_traces=1024, trace_len=1000, ladder=LADDER,
                             auto_reset=True), throughput=rows, per_decision=per_decision)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
