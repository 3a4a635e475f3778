#!/usr/bin/env python3
"""Recurrent policy populations on bench.py's workload (48-chunk episodes under auto_reset, 1 024 synthetic 1 000-point
traces, 6 rates; W = 8, softmax with probs, values and the hidden slab, fuse decisions per launch) at --lanes lanes, per
shape (lane engine at H = 32 and 64, matrix engine at H = 128):
  (a) "single":   one GRU over all lanes through the single-network rollout (abr_env_step_policy_gru /
                  abr_env_gru_mx_step) -- the yardstick, whose kernels the population change leaves as they were;
  (b) "pop P":    RecurrentPolicyPopulation of P = 1, 16, 64, 256 members, group = lanes / P, one launch per decision;
  (c) "separate": what a recurrent population cost before -- --separate environments of lanes / --separate lanes, each
                  with its own RecurrentPolicyController, stepped one after another; the rate is the total env-steps/s.
The kinds alternate inside every round, --repeats rounds, medians with min..max.  Each shape is measured by a child
process of its own under `timeout` (a fresh process, so that a shape that fails or hangs ends there and nothing is started
after it).  Writes OUT/NAME and prints it.

    python tools/bench_policy_gru_population.py OUT [--lanes 65536] [--fuse 48] [--launches 5] [--warmup 2] [--repeats 3]
                                                    [--members 1 16 64 256] [--separate 64]
                                                    [--shapes lane:32 lane:64 matrix:128] [--limit 420]
                                                    [--name policy_gru_population_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(a):
    import numpy as np
    import torch

    import abrsimulator_amd as A
    from bench_policy import LADDER, WINDOW, make_env, timed
    engine, H = a.shapes[0].split(":")
    H = int(H)
    F, M, N = 4 + WINDOW + len(LADDER), len(LADDER), a.lanes
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731

    def members(P):
        """P perturbations of one cell, head and value head, stacked on the device."""
        torch.manual_seed(0)
        cell, head, vh = torch.nn.GRUCell(F, H), torch.nn.Linear(H, M), torch.nn.Linear(H, 1)
        g = torch.Generator().manual_seed(1)
        noisy = lambda t: (t.detach()[None] + 0.05 * torch.randn(P, *t.shape, generator=g)).cuda()  # noqa: E731
        six = tuple(noisy(t) for t in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh, head.weight, head.bias))
        return six, (noisy(vh.weight[0]), noisy(vh.bias[0]))

    def slabs(n):
        return dict(obs=torch.empty(a.fuse, 8, n, device="cuda"), reward=torch.empty(a.fuse, n, device="cuda"),
                    done=torch.empty(a.fuse, n, dtype=torch.uint8, device="cuda"),
                    actions=torch.empty(a.fuse, n, dtype=torch.int32, device="cuda"),
                    probs=torch.empty(a.fuse, M, n, device="cuda"), values=torch.empty(a.fuse, n, device="cuda"),
                    last_value=torch.empty(n, device="cuda"), hidden=torch.empty(a.fuse, H, n, device="cuda"))

    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    kw = dict(window=WINDOW, seed=1, sample="softmax", engine=engine)
    out, runs = slabs(N), {}
    env = make_env(N, traces)
    six, (Wv, bv) = members(1)
    ctl = A.RecurrentPolicyController(A.EnvPlayer(env), tuple(t[0] for t in six[:4]), tuple(t[0] for t in six[4:]),
                                      value_head=(Wv[0], bv[0]), **kw)
    runs["single"] = (lambda env=env, ctl=ctl: env.step_policy(ctl, a.fuse, out=out)), [env]
    for P in a.members:
        if N % P or (N // P) % 256:
            raise SystemExit(f"--lanes {N} does not split into {P} groups of a multiple of 256 lanes")
        env = make_env(N, traces)
        six, heads = members(P)
        pop = A.RecurrentPolicyPopulation(A.EnvPlayer(env), six, N // P, value_heads=heads, **kw)
        runs[f"pop {P}"] = (lambda env=env, pop=pop: env.step_policy(pop, a.fuse, out=out)), [env]
    S, n = a.separate, N // a.separate
    small = slabs(n)
    envs = [make_env(n, traces) for _ in range(S)]
    six, (Wv, bv) = members(S)
    ctls = [A.RecurrentPolicyController(A.EnvPlayer(e), tuple(t[m] for t in six[:4]), tuple(t[m] for t in six[4:]),
                                        value_head=(Wv[m], bv[m]), **kw) for m, e in enumerate(envs)]

    def separate():
        for e, c in zip(envs, ctls):
            e.step_policy(c, a.fuse, out=small)
    runs["separate"] = separate, envs
    times = {k: [] for k in runs}
    for _ in range(a.repeats):                                # alternating: every kind once per round
        for k, (launch, _) in runs.items():
            times[k].append(timed(launch, a.warmup, a.launches))
    for k in runs:
        rates = sorted(N * a.fuse * a.launches / t for t in times[k])
        row = dict(engine=engine, hidden=H, blob_bytes=4 * (3 * H * (F + H + 2) + M * (H + 1)), kind=k, lanes=N,
                   fuse=a.fuse, launches=a.launches, warmup=a.warmup, repeats=a.repeats, env_steps_per_s=med(rates),
                   env_steps_per_s_all=rates, rollout_us_per_decision=1e6 * med(times[k]) / (a.launches * a.fuse))
        if k.startswith("pop"):
            row.update(members=int(k.split()[1]), group=N // int(k.split()[1]))
        if k == "separate":
            row.update(environments=S, lanes_each=n)
        print("ROW " + json.dumps(row), flush=True)
    print("DEVICE " + torch.cuda.get_device_name(0), flush=True)


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
    ap.add_argument("--shapes", nargs="+", default=["lane:32", "lane:64", "matrix:128"])
    ap.add_argument("--name", default="policy_gru_population_bench.json")
    ap.add_argument("--limit", type=int, default=420, help="seconds each shape's child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows, device = [], None
    for shape in a.shapes:                                    # one child per shape, each under its own time limit
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), a.out, "--child", "--shapes",
               shape, "--lanes", str(a.lanes), "--fuse", str(a.fuse), "--launches", str(a.launches), "--warmup",
               str(a.warmup), "--repeats", str(a.repeats), "--separate", str(a.separate), "--members"] + \
              [str(P) for P in a.members]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
            elif line.startswith("DEVICE "):
                device = line[7:]
        if r.returncode:
            print(f"the child for {shape} ended with status {r.returncode}: nothing more is started", file=sys.stderr)
            return r.returncode
    for r in rows:
        same = [x for x in rows if (x["engine"], x["hidden"]) == (r["engine"], r["hidden"])]
        base = next(x for x in same if x["kind"] == "single")
        sep = next(x for x in same if x["kind"] == "separate")
        lo, hi = base["env_steps_per_s_all"][0], base["env_steps_per_s_all"][-1]
        r["vs_single"] = r["env_steps_per_s"] / base["env_steps_per_s"]
        r["vs_single_min_max"] = [r["env_steps_per_s_all"][0] / base["env_steps_per_s"],
                                  r["env_steps_per_s_all"][-1] / base["env_steps_per_s"]]
        r["single_spread"] = hi / lo
        r["within_single_spread"] = bool(lo <= r["env_steps_per_s"] <= hi)
        r["vs_separate"] = r["env_steps_per_s"] / sep["env_steps_per_s"]
    res = dict(device=device, window=8,
               workload=dict(video_length=48, n_traces=1024, trace_len=1000, auto_reset=True, sample="softmax",
                             outputs="obs, reward, done, actions, probs, values, last_value, hidden"),
               note="any cause given for a difference is inferred from the code: no hardware counters were collected",
               rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
