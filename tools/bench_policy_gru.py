#!/usr/bin/env python3
"""The recurrent policy against the lane engine's MLP on bench.py's workload (48-chunk episodes under auto_reset, 1 024
synthetic 1 000-point traces, 6 rates; W = 8, softmax with probs and values): the MLP at 64/64 -- the yardstick every
earlier measurement of the policy used -- against the GRU cell at H = 32 and H = 64, in the same tree.
  - the policy kernel of one decision alone (abr_env_policy_select_ac / abr_env_policy_select_gru with commit; actions,
    probs and the value written), launches x fuse launches between two HIP events after the warm-ups;
  - the fused rollout (env.step_policy, fuse decisions per launch; obs, reward, done, actions, probs, values, last_value).
The kinds alternate inside every round, --repeats rounds, medians.  fmaf counts per decision are reported next to the
times: the MLP's 64/64 takes F * 64 + 64 * 64 + 64 * (M + 1), the cell 3H (F + H) + H (M + 1) + 2H.
Writes OUT/NAME and prints it.

    python tools/bench_policy_gru.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 5] [--warmup 2] [--repeats 3]
                                         [--name policy_gru_bench.json] [--kernel-only]
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
from bench_policy_matrix import net  # noqa: E402

KINDS = (("mlp", (64, 64)), ("gru", (32,)), ("gru", (64,)))
F, M = 4 + WINDOW + len(LADDER), len(LADDER)


def name(kind):
    return kind[0] + " " + "/".join(map(str, kind[1]))


def fmafs(kind):
    if kind[0] == "mlp":
        w = (F,) + kind[1]
        return sum(a * b for a, b in zip(w[:-1], w[1:])) + w[-1] * (M + 1)
    H = kind[1][0]
    return 3 * H * (F + H) + H * (M + 1) + 2 * H


def controller(kind, env):
    torch.manual_seed(0)
    if kind[0] == "mlp":
        actor, critic = net(kind[1])
        return A.PolicyController.from_module(A.EnvPlayer(env), actor, window=WINDOW, seed=1, sample="softmax",
                                              value_head=critic)
    H = kind[1][0]
    return A.RecurrentPolicyController(A.EnvPlayer(env), torch.nn.GRUCell(F, H), torch.nn.Linear(H, M), window=WINDOW,
                                       seed=1, sample="softmax", value_head=torch.nn.Linear(H, 1))


def select_call(env, ctl, act, probs, value):
    """One launch of the policy kernel on preallocated outputs (no tensor is made per launch)."""
    pol, smp, val = ctl.bound(env), ctl.sampling(), ctl.value()
    if ctl.method == "policy_gru":
        args = (env._h, C.byref(pol), C.byref(smp), C.byref(val), 1, _lib.ptr(act), None, None, _lib.ptr(probs),
                _lib.ptr(value), None)
        return lambda: env._call(env.lib.abr_env_policy_select_gru, *args)
    args = (env._h, C.byref(pol), C.byref(smp), C.byref(val), _lib.ptr(act), None, None, _lib.ptr(probs), _lib.ptr(value))
    return lambda: env._call(env.lib.abr_env_policy_select_ac, *args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--fuse", type=int, default=48)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--name", default="policy_gru_bench.json")
    ap.add_argument("--kernel-only", action="store_true", help="the policy kernel alone (a run for a kernel trace)")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    rows = []
    for N in a.lanes:
        envs = {k: make_env(N, traces) for k in KINDS}
        ctls = {k: controller(k, envs[k]) for k in KINDS}
        out = dict(obs=torch.empty(a.fuse, 8, N, device="cuda"), reward=torch.empty(a.fuse, N, device="cuda"),
                   done=torch.empty(a.fuse, N, dtype=torch.uint8, device="cuda"),
                   actions=torch.empty(a.fuse, N, dtype=torch.int32, device="cuda"),
                   probs=torch.empty(a.fuse, M, N, device="cuda"), values=torch.empty(a.fuse, N, device="cuda"),
                   last_value=torch.empty(N, device="cuda"))
        n = a.launches * a.fuse
        kt, rt = {k: [] for k in KINDS}, {k: [] for k in KINDS}
        for k in KINDS:                                       # every env at a mid-episode state for the kernel timing
            envs[k].step_policy(ctls[k], 7, out=None, want_obs=False, want_actions=False)
        act, probs, value = torch.empty(N, dtype=torch.int32, device="cuda"), out["probs"][0], out["values"][0]
        selects = {k: select_call(envs[k], ctls[k], act, probs, value) for k in KINDS}
        for _ in range(a.repeats):                            # alternating: every kind once per round
            for k in KINDS:
                kt[k].append(timed(selects[k], a.warmup, n))
        if not a.kernel_only:
            for _ in range(a.repeats):
                for k in KINDS:
                    rt[k].append(timed(lambda: envs[k].step_policy(ctls[k], a.fuse, out=out), a.warmup, a.launches))
        for k in KINDS:
            row = dict(kind=k[0], hidden=list(k[1]), lanes=N, fuse=a.fuse, launches=a.launches, warmup=a.warmup,
                       repeats=a.repeats, fmaf_per_decision=fmafs(k), kernel_us=1e6 * med(kt[k]) / n,
                       kernel_us_all=[1e6 * t / n for t in kt[k]])
            if rt[k]:
                rates = sorted(N * a.fuse * a.launches / t for t in rt[k])
                row.update(env_steps_per_s=med(rates), env_steps_per_s_all=rates,
                           rollout_us_per_decision=1e6 * med(rt[k]) / (a.launches * a.fuse))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del envs, ctls, out, selects
        torch.cuda.empty_cache()
    for r in rows:
        base = [x for x in rows if x["kind"] == "mlp" and x["lanes"] == r["lanes"]][0]
        r["fmaf_vs_mlp"] = r["fmaf_per_decision"] / base["fmaf_per_decision"]
        r["kernel_time_vs_mlp"] = r["kernel_us"] / base["kernel_us"]
        r["gfmaf_per_s"] = r["fmaf_per_decision"] * r["lanes"] / r["kernel_us"] * 1e-3
        if "env_steps_per_s" in r:
            r["rollout_vs_mlp"] = r["env_steps_per_s"] / base["env_steps_per_s"]
    res = dict(device=torch.cuda.get_device_name(0), window=WINDOW,
               workload=dict(video_length=48, n_traces=1024, trace_len=1000, ladder=LADDER, auto_reset=True,
                             sample="softmax", outputs="obs, reward, done, actions, probs, values, last_value"),
               kinds=[name(k) for k in KINDS], rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
