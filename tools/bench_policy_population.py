#!/usr/bin/env python3
"""Policy populations on bench.py's workload (48-chunk episodes under auto_reset, 1 024 synthetic 1 000-point traces,
6 rates; W = 8, softmax with probs, fuse decisions per launch) at --lanes lanes, per engine (lane at 64/64, matrix at
128/128):
  (a) "single":   one network over all lanes through the single-network rollout -- the yardstick;
  (b) "pop P":    PolicyPopulation of P = 1, 16, 64, 256 members, group = lanes / P, one launch per decision;
  (c) "separate": what a population cost before -- --separate environments of lanes / --separate lanes, each with its
                  own controller, stepped one after another; the rate is the total env-steps/s of all of them.
The kinds alternate inside every round, --repeats rounds, medians.  Writes OUT/NAME and prints it.

    python tools/bench_policy_population.py OUT [--lanes 65536] [--fuse 48] [--launches 5] [--warmup 2] [--repeats 3]
                                                [--members 1 16 64 256] [--separate 64] [--engines lane matrix]
                                                [--name policy_population_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abrsimulator_amd as A  # noqa: E402
from bench_policy import LADDER, WINDOW, make_env, timed  # noqa: E402
from bench_policy_matrix import net  # noqa: E402

HIDDEN = {"lane": (64, 64), "matrix": (128, 128)}


def members(hidden, P):
    """P perturbations of one network, stacked: [(W [P, out, in], b [P, out]), ...] on the device."""
    actor, _ = net(hidden)
    g = torch.Generator().manual_seed(1)
    out = []
    for m in list(actor)[0::2]:
        Wt, b = m.weight.detach(), m.bias.detach()
        out.append(((Wt[None] + 0.05 * torch.randn(P, *Wt.shape, generator=g)).cuda(),
                    (b[None] + 0.05 * torch.randn(P, *b.shape, generator=g)).cuda()))
    return out


def slabs(fuse, N, M):
    return dict(obs=torch.empty(fuse, 8, N, device="cuda"), reward=torch.empty(fuse, N, device="cuda"),
                done=torch.empty(fuse, N, dtype=torch.uint8, device="cuda"),
                actions=torch.empty(fuse, N, dtype=torch.int32, device="cuda"), probs=torch.empty(fuse, M, N, device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--fuse", type=int, default=48)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--separate", type=int, default=64)
    ap.add_argument("--engines", nargs="+", default=["lane", "matrix"], choices=sorted(HIDDEN))
    ap.add_argument("--name", default="policy_population_bench.json")
    a = ap.parse_args()
    N, M, med = a.lanes, len(LADDER), lambda xs: sorted(xs)[len(xs) // 2]
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    kw = dict(window=WINDOW, seed=1, sample="softmax")
    rows = []
    for engine in a.engines:
        hidden = HIDDEN[engine]
        out, runs = slabs(a.fuse, N, M), {}
        env = make_env(N, traces)
        ctl = A.PolicyController.from_module(A.EnvPlayer(env), net(hidden)[0], engine=engine, **kw)
        runs["single"] = (lambda env=env, ctl=ctl: env.step_policy(ctl, a.fuse, out=out)), [env]
        for P in a.members:
            if N % P or (N // P) % 256:
                raise SystemExit(f"--lanes {N} does not split into {P} groups of a multiple of 256 lanes")
            env = make_env(N, traces)
            pop = A.PolicyPopulation(A.EnvPlayer(env), members(hidden, P), N // P, engine=engine, **kw)
            runs[f"pop {P}"] = (lambda env=env, pop=pop: env.step_policy(pop, a.fuse, out=out)), [env]
        S, n = a.separate, N // a.separate
        small = slabs(a.fuse, n, M)
        envs = [make_env(n, traces) for _ in range(S)]
        stacked = members(hidden, S)
        ctls = [A.PolicyController(A.EnvPlayer(e), [(Wt[m], b[m]) for Wt, b in stacked], engine=engine, **kw)
                for m, e in enumerate(envs)]

        def separate(envs=envs, ctls=ctls, small=small):
            for e, c in zip(envs, ctls):
                e.step_policy(c, a.fuse, out=small)
        runs["separate"] = separate, envs
        times = {k: [] for k in runs}
        for _ in range(a.repeats):                            # alternating: every kind once per round
            for k, (launch, _) in runs.items():
                times[k].append(timed(launch, a.warmup, a.launches))
        for k in runs:
            rates = sorted(N * a.fuse * a.launches / t for t in times[k])
            row = dict(engine=engine, hidden=list(hidden), kind=k, lanes=N, fuse=a.fuse, launches=a.launches,
                       warmup=a.warmup, repeats=a.repeats, env_steps_per_s=med(rates), env_steps_per_s_all=rates,
                       rollout_us_per_decision=1e6 * med(times[k]) / (a.launches * a.fuse))
            if k.startswith("pop"):
                row.update(members=int(k.split()[1]), group=N // int(k.split()[1]))
            if k == "separate":
                row.update(environments=S, lanes_each=n)
            rows.append(row)
            print(json.dumps(row), flush=True)
        base = next(r for r in rows if r["engine"] == engine and r["kind"] == "single")
        for r in rows:
            if r["engine"] == engine:
                r["vs_single"] = r["env_steps_per_s"] / base["env_steps_per_s"]
                r["single_spread"] = base["env_steps_per_s_all"][-1] / base["env_steps_per_s_all"][0]
        for _, es in runs.values():
            for e in es:
                e.close()
        del runs, out, small, envs, ctls
        torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), window=WINDOW,
               workload=dict(video_length=48, n_traces=1024, trace_len=1000, ladder=LADDER, auto_reset=True,
                             sample="softmax", outputs="obs, reward, done, actions, probs"), rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
