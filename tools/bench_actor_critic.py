#!/usr/bin/env python3
"""What an actor-critic trainer pays for values and advantages on bench.py's workload (48-chunk episodes under
auto_reset, 1 024 synthetic 1 000-point traces, 6 rates; W = 8, 64/64 hidden, softmax with probs):
  - fused rollout env-steps/s of step_policy with and without want_values (abr_env_step_policy_ac against
    abr_env_step_policy_sampled), one process, same workload, fuse and lanes; each row is R launches between two HIP
    events after W warm-ups, and the kinds alternate, --repeats rounds, medians;
  - per decision: the sampled policy kernel alone with and without the value head (abr_env_policy_select_ac against
    abr_env_policy_select_sampled, actions, probs and the value written), R x fuse launches between two events;
  - advantage.gae at T = fuse on a rollout's own slabs against the same recurrence written as a torch loop over rows
    (what a trainer writes otherwise), both checked against each other first; algorithmic bytes (13 B read and 8 B
    written per element, last_value aside) over the kernel's time as GB/s.
Writes OUT/NAME (default actor_critic_bench.json) and prints it.

    python tools/bench_actor_critic.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 5] [--warmup 2]
                                           [--repeats 3] [--name actor_critic_bench.json]
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
from bench_policy import HIDDEN, LADDER, WINDOW, make_env, net, timed  # noqa: E402

KINDS = ("sampled", "values")
GAMMA, LAM = 0.99, 0.95


def torch_gae(reward, values, last_value, done, actions, gamma, lam):
    """abr_gae's recurrence as a trainer writes it in torch: one row at a time, newest first."""
    T = reward.shape[0]
    adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    gamma = torch.tensor(gamma, dtype=torch.float32, device=reward.device)
    gl = gamma * torch.tensor(lam, dtype=torch.float32, device=reward.device)
    zero = torch.zeros_like(last_value)
    A_, nv = zero, last_value
    for t in range(T - 1, -1, -1):
        term, dead = done[t] != 0, actions[t] < 0
        q = torch.where(term, zero, gamma * nv)
        delta = (reward[t] + q) - values[t]
        w = torch.where(term, zero, gl * A_)
        A_ = torch.where(dead, zero, delta + w)
        adv[t] = A_
        ret[t] = torch.where(dead, zero, A_ + values[t])
        nv = torch.where(dead, zero, values[t])
    return adv, ret


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--fuse", type=int, default=48)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--name", default="actor_critic_bench.json")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    M, med = len(LADDER), lambda xs: sorted(xs)[len(xs) // 2]
    torch.manual_seed(1)
    critic = torch.nn.Linear(HIDDEN[-1], 1)
    rows, per_decision, gae_rows = [], [], []
    for N in a.lanes:
        envs = {k: make_env(N, traces) for k in KINDS}
        ctls = {k: A.PolicyController.from_module(A.EnvPlayer(envs[k]), net(), window=WINDOW, seed=1, sample="softmax",
                                                  value_head=critic) for k in KINDS}
        out = dict(obs=torch.empty(a.fuse, 8, N, device="cuda"), reward=torch.empty(a.fuse, N, device="cuda"),
                   done=torch.empty(a.fuse, N, dtype=torch.uint8, device="cuda"),
                   actions=torch.empty(a.fuse, N, dtype=torch.int32, device="cuda"),
                   probs=torch.empty(a.fuse, M, N, device="cuda"))
        out_v = dict(out, values=torch.empty(a.fuse, N, device="cuda"), last_value=torch.empty(N, device="cuda"))
        outs = dict(sampled=out, values=out_v)
        ts = {k: [] for k in KINDS}
        for _ in range(a.repeats):                        # alternating: every kind once per round
            for k in KINDS:
                ts[k].append(timed(lambda: envs[k].step_policy(ctls[k], a.fuse, out=outs[k]), a.warmup, a.launches))
        for k in KINDS:
            rates = sorted(N * a.fuse * a.launches / t for t in ts[k])
            row = dict(kind=k, lanes=N, fuse=a.fuse, launches=a.launches, warmup=a.warmup, repeats=a.repeats,
                       env_steps_per_s=med(rates), env_steps_per_s_all=rates,
                       us_per_decision=1e6 * med(ts[k]) / (a.launches * a.fuse))
            rows.append(row)
            print(json.dumps(row), flush=True)
        # the policy kernel of one decision alone, with and without the value head
        env, ctl = envs["values"], ctls["values"]
        act = torch.empty(N, dtype=torch.int32, device="cuda")
        probs, value = torch.empty(M, N, device="cuda"), torch.empty(N, device="cuda")
        pol, smp, val = ctl.bound(env), ctl.sampling(), ctl.value()

        def select_sampled():
            env._call(env.lib.abr_env_policy_select_sampled, env._h, C.byref(pol), C.byref(smp), _lib.ptr(act), None,
                      None, _lib.ptr(probs))

        def select_ac():
            env._call(env.lib.abr_env_policy_select_ac, env._h, C.byref(pol), C.byref(smp), C.byref(val), _lib.ptr(act),
                      None, None, _lib.ptr(probs), _lib.ptr(value))
        n = a.launches * a.fuse
        sam, sav = [], []
        for _ in range(a.repeats):                        # alternating
            sam.append(timed(select_sampled, a.warmup, n))
            sav.append(timed(select_ac, a.warmup, n))
        pd = dict(lanes=N, sampled_kernel_us=1e6 * med(sam) / n, value_kernel_us=1e6 * med(sav) / n,
                  sampled_kernel_us_all=[1e6 * t / n for t in sam], value_kernel_us_all=[1e6 * t / n for t in sav])
        pd["value_over_sampled"] = pd["value_kernel_us"] / pd["sampled_kernel_us"]
        per_decision.append(pd)
        print(json.dumps(pd), flush=True)
        # GAE on the last rollout's slabs: the kernel against the torch loop over rows
        o = out_v
        want = torch_gae(o["reward"], o["values"], o["last_value"], o["done"], o["actions"], GAMMA, LAM)
        got = A.gae(o["reward"], o["values"], o["last_value"], o["done"], o["actions"], GAMMA, LAM)
        same = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
        buf = (torch.empty_like(o["reward"]), torch.empty_like(o["reward"]))
        kt, tt = [], []
        for _ in range(a.repeats):                        # alternating
            kt.append(timed(lambda: A.gae(o["reward"], o["values"], o["last_value"], o["done"], o["actions"], GAMMA, LAM,
                                          out=buf), a.warmup, 20 * a.launches) / (20 * a.launches))
            tt.append(timed(lambda: torch_gae(o["reward"], o["values"], o["last_value"], o["done"], o["actions"], GAMMA,
                                              LAM), a.warmup, a.launches) / a.launches)
        nbytes = 21 * a.fuse * N + 4 * N
        g = dict(lanes=N, T=a.fuse, gae_us=1e6 * med(kt), torch_loop_us=1e6 * med(tt), gae_us_all=[1e6 * t for t in kt],
                 torch_loop_us_all=[1e6 * t for t in tt], torch_over_gae=med(tt) / med(kt), algorithmic_bytes=nbytes,
                 gae_GBps=nbytes / med(kt) / 1e9, equals_torch_loop=same, done_bytes_set=int((o["done"] != 0).sum()))
        gae_rows.append(g)
        print(json.dumps(g), flush=True)
        del envs, ctls, out, out_v, outs, env, ctl, o, buf, want, got
        torch.cuda.empty_cache()
    for r in rows:
        base = [x for x in rows if x["kind"] == "sampled" and x["lanes"] == r["lanes"]][0]["env_steps_per_s"]
        r["vs_sampled"] = r["env_steps_per_s"] / base
    res = dict(device=torch.cuda.get_device_name(0), window=WINDOW, hidden=HIDDEN, gamma=GAMMA, lam=LAM,
               workload=dict(video_length=48, n_traces=1024, trace_len=1000, ladder=LADDER, auto_reset=True,
                             sample="softmax", outputs="obs, reward, done, actions, probs (+ values, last_value)"),
               throughput=rows, per_decision=per_decision, gae=gae_rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
