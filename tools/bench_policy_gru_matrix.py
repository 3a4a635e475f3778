#!/usr/bin/env python3
"""The recurrent policy's two engines on bench.py's workload (48-chunk episodes under auto_reset, 1 024 synthetic
1 000-point traces, 6 rates; W = 8, softmax with probs, values and the hidden slab): the lane GRU at H = 32 and 64 -- the
yardstick, whose code object no change to the matrix engine touches -- against the matrix GRU at H = 32, 64 and 128, and
the matrix MLP at 128/128 for scale, in the same tree.
  - the policy kernel of one decision alone (abr_env_policy_select_gru / abr_env_gru_mx_select with commit, or
    abr_env_policy_select_mx; actions, probs, the value and h_in written), launches x fuse launches between two HIP
    events after the warm-ups;
  - the fused rollout (env.step_policy, fuse decisions per launch; obs, reward, done, actions, probs, values, last_value
    and, for the recurrent kinds, hidden).
The kinds alternate inside every round, --repeats rounds, medians.  Each lane count is measured by a child process of its
own under `timeout` (a fresh process, so that a size that fails or hangs ends there and nothing is started after it).
MFMA floors per wave and decision are reported next to the times: 2 (ceil(H/32) 3 (ceil(F/2) + ceil(H/2)) + ceil(H/2))
instructions of 64 cycles for the cell.  Writes OUT/NAME and prints it.

    python tools/bench_policy_gru_matrix.py OUT [--lanes 65536 1048576] [--fuse 48] [--launches 5] [--warmup 2]
                                                [--repeats 3] [--name policy_gru_matrix_bench.json] [--limit 420]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KINDS = (("gru lane", (32,)), ("gru lane", (64,)), ("gru matrix", (32,)), ("gru matrix", (64,)), ("gru matrix", (128,)),
         ("mlp matrix", (128, 128)))


def name(kind):
    return kind[0] + " " + "/".join(map(str, kind[1]))


def mfma_floor(kind, F):
    """v_mfma_f32_32x32x2_f32 instructions per wave and decision (two column tiles); None for the lane engine."""
    if kind[0] != "gru matrix":
        return None
    H = kind[1][0]
    return 2 * (-(-H // 32) * 3 * (-(-F // 2) + -(-H // 2)) + -(-H // 2))


def child(a):
    import numpy as np
    import torch

    import abrsimulator_amd as A
    from abrsimulator_amd import _lib
    from bench_policy import LADDER, WINDOW, make_env, timed
    from bench_policy_matrix import net
    F, M, N = 4 + WINDOW + len(LADDER), len(LADDER), a.lanes[0]

    def controller(kind, env):
        torch.manual_seed(0)
        if kind[0] == "mlp matrix":
            actor, critic = net(kind[1])
            return A.PolicyController.from_module(A.EnvPlayer(env), actor, window=WINDOW, seed=1, sample="softmax",
                                                  value_head=critic, engine="matrix")
        H = kind[1][0]
        return A.RecurrentPolicyController(A.EnvPlayer(env), torch.nn.GRUCell(F, H), torch.nn.Linear(H, M), window=WINDOW,
                                           seed=1, sample="softmax", value_head=torch.nn.Linear(H, 1),
                                           engine=kind[0].split()[1])

    def select_call(env, ctl, act, probs, value, hidden):
        pol, smp, val = ctl.bound(env), ctl.sampling(), ctl.value()
        if ctl.method == "policy_gru":
            fn = env.lib.abr_env_gru_mx_select if ctl.engine == "matrix" else env.lib.abr_env_policy_select_gru
            args = (env._h, C.byref(pol), C.byref(smp), C.byref(val), 1, _lib.ptr(act), None, None, _lib.ptr(probs),
                    _lib.ptr(value), _lib.ptr(hidden))
            return lambda: env._call(fn, *args)
        args = (env._h, C.byref(pol), C.byref(smp), C.byref(val), _lib.ptr(act), None, None, _lib.ptr(probs), _lib.ptr(value))
        return lambda: env._call(env.lib.abr_env_policy_select_mx, *args)

    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    envs = {k: make_env(N, traces) for k in KINDS}
    ctls = {k: controller(k, envs[k]) for k in KINDS}
    top = max(k[1][0] for k in KINDS if k[0] != "mlp matrix")
    slab = torch.empty(a.fuse * top * N, device="cuda")                   # one hidden slab, viewed at each kind's H
    base = dict(obs=torch.empty(a.fuse, 8, N, device="cuda"), reward=torch.empty(a.fuse, N, device="cuda"),
                done=torch.empty(a.fuse, N, dtype=torch.uint8, device="cuda"),
                actions=torch.empty(a.fuse, N, dtype=torch.int32, device="cuda"),
                probs=torch.empty(a.fuse, M, N, device="cuda"), values=torch.empty(a.fuse, N, device="cuda"),
                last_value=torch.empty(N, device="cuda"))
    outs = {}
    for k in KINDS:
        outs[k] = dict(base)
        if k[0] != "mlp matrix":
            outs[k]["hidden"] = slab[:a.fuse * k[1][0] * N].view(a.fuse, k[1][0], N)
    n = a.launches * a.fuse
    kt, rt = {k: [] for k in KINDS}, {k: [] for k in KINDS}
    for k in KINDS:                                           # every env at a mid-episode state for the kernel timing
        envs[k].step_policy(ctls[k], 7, out=None, want_obs=False, want_actions=False)
    act, probs, value = torch.empty(N, dtype=torch.int32, device="cuda"), base["probs"][0], base["values"][0]
    selects = {k: select_call(envs[k], ctls[k], act, probs, value, slab) for k in KINDS}
    for _ in range(a.repeats):                                # alternating: every kind once per round
        for k in KINDS:
            kt[k].append(timed(selects[k], a.warmup, n))
    for _ in range(a.repeats):
        for k in KINDS:
            rt[k].append(timed(lambda: envs[k].step_policy(ctls[k], a.fuse, out=outs[k]), a.warmup, a.launches))
    for k in KINDS:
        rates = sorted(N * a.fuse * a.launches / t for t in rt[k])
        row = dict(kind=name(k), engine=k[0].split()[1], hidden=list(k[1]), lanes=N, fuse=a.fuse, launches=a.launches,
                   warmup=a.warmup, repeats=a.repeats, mfma_per_wave=mfma_floor(k, F),
                   kernel_us=1e6 * med(kt[k]) / n, kernel_us_all=[1e6 * t / n for t in kt[k]],
                   env_steps_per_s=med(rates), env_steps_per_s_all=rates,
                   rollout_us_per_decision=1e6 * med(rt[k]) / (a.launches * a.fuse))
        print("ROW " + json.dumps(row), flush=True)
    print("DEVICE " + torch.cuda.get_device_name(0), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--fuse", type=int, default=48)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--name", default="policy_gru_matrix_bench.json")
    ap.add_argument("--limit", type=int, default=420, help="seconds each lane count's child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows, device = [], None
    for N in a.lanes:                                         # one child per size, each under its own time limit
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), a.out, "--child", "--lanes",
               str(N), "--fuse", str(a.fuse), "--launches", str(a.launches), "--warmup", str(a.warmup), "--repeats",
               str(a.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
            elif line.startswith("DEVICE "):
                device = line[7:]
        if r.returncode:
            print(f"the child for {N} lanes ended with status {r.returncode}: nothing more is started", file=sys.stderr)
            return r.returncode
    for r in rows:
        same = [x for x in rows if x["lanes"] == r["lanes"]]
        lane = [x for x in same if x["engine"] == "lane" and x["hidden"] == r["hidden"]]
        if r["engine"] == "matrix" and lane:                  # the yardstick: the lane GRU of the same width, same tree
            r["kernel_speedup_vs_lane"] = lane[0]["kernel_us"] / r["kernel_us"]
            r["rollout_speedup_vs_lane"] = r["env_steps_per_s"] / lane[0]["env_steps_per_s"]
        if r["mfma_per_wave"]:
            r["mfma_floor_cycles"] = 64 * r["mfma_per_wave"]
    res = dict(device=device, window=8,
               workload=dict(video_length=48, n_traces=1024, trace_len=1000, auto_reset=True, sample="softmax",
                             outputs="obs, reward, done, actions, probs, values, last_value, hidden"),
               kinds=[name(k) for k in KINDS], rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
