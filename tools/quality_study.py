#!/usr/bin/env python3
"""What the quality term does to the ranking of the built-in controllers (include/abr_env.h: abr_episode_quality): one
episode of bench.py's workload (48 chunks, 6 rates, 1 024 synthetic traces) over --lanes lanes from the same start, once
per controller -- MPC, RobustMPC, FastMPC (horizon 5, window 5), BBA-0, RATE, BOLA (their defaults) and the random policy
(seed 99) -- and per setting of the model: weight 1 with the "identity" utility and weight 1 with "log".  The controllers
themselves are not told about the model: their objectives are what they were.  Per controller and setting: the mean over
lanes of the ledger's qoe, of the episode's quality sum and of qoe_q = qoe - weight * quality, and the action histogram.
The settings are fixed here, before any run.  Writes OUT/quality_study.json and prints it.

    python tools/quality_study.py OUT [--lanes 65536]
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

H, WINDOW = 5, 5
CONTROLLERS = ("mpc", "robust_mpc", "fastmpc", "bba0", "rate", "bola", "random")
SETTINGS = (("identity", 1.0), ("log", 1.0))


def controller(env, kind):
    p = A.EnvPlayer(env)
    if kind == "mpc":
        return A.BatchedMPCController(p, horizon=H, clip_horizon=True)
    if kind == "robust_mpc":
        return A.BatchedMPCController(p, horizon=H, clip_horizon=True, method="robust", window=WINDOW)
    if kind == "fastmpc":
        return A.FastMPCController(p, horizon=H, window=WINDOW)
    return {"bba0": A.BufferBasedController, "rate": A.RateBasedController, "bola": A.BolaController}[kind](p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, default=65536)
    a = ap.parse_args()
    N, V = a.lanes, bench.V
    traces = bench.synth_traces()
    tid, off = bench.lane_assignment(0, N, traces)
    rows = []
    for utility, weight in SETTINGS:
        for kind in CONTROLLERS:
            mpd = A.MPD(V, bench.L, bench.MAX_BUFFER, bench.START_UP, A.Chunk(bench.LADDER))
            env = A.BatchedABREnv(mpd, A.QOEMetric(*bench.WEIGHTS), A.NetworkInfo(bench.INTERVAL, traces), N,
                                  device="cuda", auto_reset=True)
            env.reset(torch.from_numpy(tid), torch.from_numpy(off))
            led = env.set_episode_ledger(1)
            ql = env.set_quality(weight, utility)
            if kind == "random":
                out = env.step_random(V, 99)
            else:
                ctl = controller(env, kind)
                out = env.step_mpc(ctl, V) if isinstance(ctl, A.BatchedMPCController) else env.step_rule(ctl, V)
            rec = ql.records(led)
            assert rec["lane"].numel() == N, "every lane finishes exactly one episode"
            acts = out["actions"]
            rows.append(dict(utility=utility, weight=weight, controller=kind,
                             qoe=float(rec["qoe"].mean()), quality=float(rec["quality"].mean()),
                             qoe_q=float(rec["qoe_q"].mean()), reward_sum=float(out["reward"].double().sum(0).mean()),
                             rebuffer_time=float(rec["rebuffer_time"].mean()), variance=float(rec["variance"].mean()),
                             timed_out=int((rec["done"] != 1).sum()),
                             action_histogram=torch.bincount(acts[acts >= 0].long(), minlength=len(bench.LADDER)).tolist()))
            print(json.dumps(rows[-1]), flush=True)
            del env, led, ql, out
            torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), lanes=N, video_length=V, horizon=H, window=WINDOW,
               ladder=bench.LADDER, weights=bench.WEIGHTS, rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "quality_study.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
