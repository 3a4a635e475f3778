#!/usr/bin/env python3
"""Config-space fuzz of the closed-loop rollouts on the GPU box: each seed is one case of tests/closed_loop_check.py
(random configuration x controller {harmonic MPC, RobustMPC, FastMPC, BBA-0, RATE, BOLA} x speed feature {config speed,
per-lane speeds, schedule, LatencySpeedController} x per-chunk ladder x lane count x accepted impl x auto_reset), run
through the public API (BatchedABREnv, step_mpc / step_rule, set_speed_controller, speed_log) in pieces, then checked
against the C oracle and the controller twins: every action, obs row, reward, done flag, the frame after every piece,
the history, QoE, the speed log and the FastMPC entries the decisions read.
    usage: python tools/gpu_fuzz_closed.py [n_seeds] [lanes (default: the case's own)] [first_seed]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import abrsimulator_amd as A  # noqa: E402
import closed_loop_check as K  # noqa: E402


def _controller(case, env):
    m, p, ctl = case["meta"], case["params"], case["ctl"]
    V, L = m["video_length"], m["chunk_length"]
    if ctl in ("mpc", "robust", "fastmpc"):
        br = K.br_table(case)
        mpd = A.MPD(V, L, m["max_buffer"], m["start_up_length"],
                    [A.Chunk(list(b), list(s)) for b, s in zip(br, p["sizes"])])
        player = A.EnvPlayer(env, mpd=mpd, qoe=A.QOEMetric(*p["qoe"]))
        if ctl == "mpc":
            return A.BatchedMPCController(player, horizon=p["horizon"], clip_horizon=True)
        if ctl == "robust":
            return A.BatchedMPCController(player, horizon=p["horizon"], clip_horizon=True, method="robust",
                                          window=p["window"])
        return A.FastMPCController(player, horizon=p["horizon"], window=p["window"], utility=p["utility"],
                                   clip_horizon=p["clip"], buffer_points=p["buffer_points"],
                                   tput_points=p["tput_points"], layout=p["layout"])
    player = A.EnvPlayer(env)
    if ctl == "buffer":
        return A.BufferBasedController(player, reservoir=p["reservoir"], cushion=p["cushion"])
    if ctl == "rate":
        return A.RateBasedController(player, window=p["window"], safety=p["safety"])
    return A.BolaController(player, gamma_p=p["gp"], v=p["v"])


def run_case(case):
    """Run one case on the device; returns the `out` dict closed_loop_check.check takes."""
    m = case["meta"]
    V, N = m["video_length"], case["n_lanes"]
    chunks = A.Chunk(m["ladder"]) if case["br"] is None else [A.Chunk(list(r)) for r in case["br"]]
    mpd = A.MPD(V, m["chunk_length"], m["max_buffer"], m["start_up_length"], chunks)
    speed = m["speed"]
    if case["feature"] == "lanes":
        speed = torch.from_numpy(np.asarray(case["lane_speeds"], np.float64))
    elif case["feature"] == "schedule":
        speed = torch.from_numpy(np.ascontiguousarray(np.asarray(case["schedule"], np.float64).T))
    env = A.BatchedABREnv(mpd, A.QOEMetric(*m["weights"]), A.NetworkInfo(m["interval"], case["traces"]), N,
                          speed=speed, impl=case["impl"], auto_reset=case["auto_reset"], max_ticks=case["max_ticks"])
    if case["feature"] == "rule":
        env.set_speed_controller(A.LatencySpeedController(*case["rule"]), log_rows=V + 4)
    env.reset(torch.from_numpy(case["tid"]), torch.from_numpy(case["off"]))
    ctl = _controller(case, env)
    mpc = case["ctl"] in ("mpc", "robust")
    parts, frames, t = [], [], 0
    for n in case["pieces"]:
        o = env.step_mpc(ctl, n) if mpc else env.step_rule(ctl, n)
        parts.append({k: v.cpu().numpy() for k, v in o.items()})
        t += n
        frames.append((t, {k: v.cpu().numpy().copy() for k, v in env.observe_f64().items()}))
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("actions", "reward", "done", "obs")}
    out["frames"] = frames
    out["history"] = tuple(x.cpu().numpy().copy() for x in env.history())
    out["qoe"] = env.episode_qoe().cpu().numpy()
    out["speed_log"] = env.speed_log().cpu().numpy().copy() if case["feature"] == "rule" else None
    out["entries"] = ctl.entries().cpu().numpy() if case["ctl"] == "fastmpc" else None
    torch.cuda.synchronize()
    env.close()
    return out


def run_seed(seed, N=None, stats=None):
    """One case against the reference.  Returns (mismatches, lane-steps, cell key, case)."""
    case = K.make_case(seed, N)
    mm = K.check(case, run_case(case), stats)
    return mm, case["n_lanes"] * case["n_steps"], f"{case['ctl']}/{case['feature']}", case


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    N = int(sys.argv[2]) if len(sys.argv) > 2 and int(sys.argv[2]) > 0 else None
    first = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    t0 = time.time()
    bad, lane_steps, cells, impls, stats, cases = 0, 0, {}, {}, {}, []
    for seed in range(first, first + n_seeds):
        mm, ls, key, case = run_seed(seed, N, stats)
        if mm:
            print("MISMATCH", K.describe(case), len(mm), mm[:4], flush=True)
        bad += len(mm)
        lane_steps += ls
        cells[key] = cells.get(key, 0) + 1
        impls[case["impl"]] = impls.get(case["impl"], 0) + 1
        cases.append(case)
    vac = K.assert_non_vacuous(stats, cases)
    print(json.dumps(dict(seeds=n_seeds, first_seed=first, lanes_per_seed=N or "case", lane_steps=lane_steps,
                          mismatches=bad, non_vacuity_problems=vac, cases=cells, impls=impls,
                          clipped_mpc_decisions=stats.get("clipped", 0), seconds=round(time.time() - t0, 1))))
    sys.exit(1 if bad or vac else 0)


if __name__ == "__main__":
    main()
