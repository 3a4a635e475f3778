#!/usr/bin/env python3
"""The learned policy's two engines on bench.py's workload (48-chunk episodes under auto_reset, 1 024 synthetic
1 000-point traces, 6 rates; W = 8, softmax with probs and values): engine "lane" at 64/64 -- the yardstick, the kernel
every earlier measurement of the policy used -- against engine "matrix" at 64/64, 128/128 and 128/128/128.
  - the policy kernel of one decision alone (abr_env_policy_select_ac / abr_env_policy_select_mx; actions, probs and the
    value written), launches x fuse launches between two HIP events after the warm-ups;
  - the fused rollout (env.step_policy, fuse decisions per launch; obs, reward, done, actions, probs, values, last_value).
The kinds alternate inside every round, --repeats rounds, medians.  Writes OUT/NAME and prints it.

    python tools/bench_policy_matrix.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 5] [--warmup 2]
                                            [--repeats 3] [--name policy_matrix_bench.json] [--kernel-only]
                                            [--kinds NAME ...]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abrsimulator_amd as A  # noqa: E402
from abrsimulator_amd import _lib  # noqa: E402
from bench_policy import LADDER, WINDOW, make_env, timed  # noqa: E402

KINDS = (("lane", (64, 64)), ("matrix", (64, 64)), ("matrix", (128, 128)), ("matrix", (128, 128, 128)))


def net(hidden):
    torch.manual_seed(0)
    F, mods = 4 + WINDOW + len(LADDER), []
    for w in hidden:
        mods += [torch.nn.Linear(F, w), torch.nn.ReLU()]
        F = w
    return torch.nn.Sequential(*mods, torch.nn.Linear(F, len(LADDER))), torch.nn.Linear(F, 1)


def name(kind):
    return kind[0] + " " + "/".join(map(str, kind[1]))


def select_call(env, ctl, act, probs, value):
    """One launch of the engine's policy kernel on preallocated outputs (no tensor is made per launch)."""
    pol, smp, val = ctl.bound(env), ctl.sampling(), ctl.value()
    fn = env.lib.abr_env_policy_select_mx if ctl.engine == "matrix" else env.lib.abr_env_policy_select_ac
    args = (env._h, C.byref(pol), C.byref(smp), C.byref(val), _lib.ptr(act), None, None, _lib.ptr(probs), _lib.ptr(value))
    return lambda: env._call(fn, *args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--fuse", type=int, default=48)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--name", default="policy_matrix_bench.json")
    ap.add_argument("--kernel-only", action="store_true", help="the policy kernel alone (a run for a kernel trace)")
    ap.add_argument("--kinds", nargs="+", default=None, help='a subset by name, e.g. "lane 64/64" "matrix 64/64"')
    a = ap.parse_args()
    kinds = [k for k in KINDS if a.kinds is None or name(k) in a.kinds]
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    M, med = len(LADDER), lambda xs: sorted(xs)[len(xs) // 2]
    rows = []
    for N in a.lanes:
        envs = {k: make_env(N, traces) for k in kinds}
        ctls = {}
        for k in kinds:
            actor, critic = net(k[1])
            ctls[k] = A.PolicyController.from_module(A.EnvPlayer(envs[k]), actor, window=WINDOW, seed=1, sample="softmax",
                                                     value_head=critic, engine=k[0])
        out = dict(obs=torch.empty(a.fuse, 8, N, device="cuda"), reward=torch.empty(a.fuse, N, device="cuda"),
                   done=torch.empty(a.fuse, N, dtype=torch.uint8, device="cuda"),
                   actions=torch.empty(a.fuse, N, dtype=torch.int32, device="cuda"),
                   probs=torch.empty(a.fuse, M, N, device="cuda"), values=torch.empty(a.fuse, N, device="cuda"),
                   last_value=torch.empty(N, device="cuda"))
        n = a.launches * a.fuse
        kt, rt = {k: [] for k in kinds}, {k: [] for k in kinds}
        for k in kinds:                                       # every env at a mid-episode state for the kernel timing
            envs[k].step_policy(ctls[k], 7, out=None, want_obs=False, want_actions=False)
        act, probs, value = torch.empty(N, dtype=torch.int32, device="cuda"), out["probs"][0], out["values"][0]
        selects = {k: select_call(envs[k], ctls[k], act, probs, value) for k in kinds}
        for _ in range(a.repeats):                            # alternating: every kind once per round
            for k in kinds:
                kt[k].append(timed(selects[k], a.warmup, n))
        if not a.kernel_only:
            for _ in range(a.repeats):
                for k in kinds:
                    rt[k].append(timed(lambda: envs[k].step_policy(ctls[k], a.fuse, out=out), a.warmup, a.launches))
        for k in kinds:
            row = dict(engine=k[0], hidden=list(k[1]), lanes=N, fuse=a.fuse, launches=a.launches, warmup=a.warmup,
                       repeats=a.repeats, kernel_us=1e6 * med(kt[k]) / n, kernel_us_all=[1e6 * t / n for t in kt[k]])
            if rt[k]:
                rates = sorted(N * a.fuse * a.launches / t for t in rt[k])
                row.update(env_steps_per_s=med(rates), env_steps_per_s_all=rates,
                           rollout_us_per_decision=1e6 * med(rt[k]) / (a.launches * a.fuse))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del envs, ctls, out
        torch.cuda.empty_cache()
    for r in rows:
        base = [x for x in rows if x["engine"] == "lane" and x["lanes"] == r["lanes"]]
        if not base:
            continue
        base = base[0]
        r["kernel_vs_lane"] = base["kernel_us"] / r["kernel_us"]
        if "env_steps_per_s" in r:
            r["rollout_vs_lane"] = r["env_steps_per_s"] / base["env_steps_per_s"]
    res = dict(device=torch.cuda.get_device_name(0), window=WINDOW,
               workload=dict(video_length=48, n_traces=1024, trace_len=1000, ladder=LADDER, auto_reset=True,
                             sample="softmax", outputs="obs, reward, done, actions, probs, values, last_value"),
               kinds=[name(k) for k in kinds], rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
