#!/usr/bin/env python3
"""Where a deployable planner sits: forecast MPC (abrsimulator_amd/planner.py: ForecastMPCController) under
tools/quality_study.py's settings, unchanged -- one episode of bench.py's workload over --lanes (trace, offset) pairs,
weight 1 with the "identity" utility and weight 1 with "log" -- rolled out on the device by BatchedABREnv.step_plan.
Fixed here before any run: horizons 1..5, the robust discount on and off, window 5.  Per setting, horizon and forecast:
the means over pairs of qoe, quality and qoe_q = qoe - weight * quality, and the action histogram (chunk 0 has no
forecast and downloads bitrate 0, as every rollout's "no decision").  The rows on record are printed beside: RATE and MPC
(profiles/quality_study.json), the hindsight bound (profiles/hindsight_study.json) and the lookahead expert at the same
horizons (profiles/lookahead_study.json).  Writes OUT/plan_study.json and prints each row.

    python tools/plan_study.py OUT [--lanes 65536]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abrsimulator_amd as A  # noqa: E402
import bench  # noqa: E402
import lookahead_study as LS  # noqa: E402
import quality_study as Q  # noqa: E402

HORIZONS = (1, 2, 3, 4, 5)
WINDOW = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, default=65536)
    a = ap.parse_args()
    N, V, M = a.lanes, bench.V, len(bench.LADDER)
    traces = bench.synth_traces()
    tid, off = bench.lane_assignment(0, N, traces)
    tid_t, off_t = torch.from_numpy(tid), torch.from_numpy(off)
    with open(os.path.join(ROOT, "profiles", "lookahead_study.json")) as f:
        look = [r for r in json.load(f)["rows"] if "horizon" in r]
    rows = []
    for utility, weight in Q.SETTINGS:
        for robust in (True, False):
            for H in HORIZONS:
                mpd = A.MPD(V, bench.L, bench.MAX_BUFFER, bench.START_UP, A.Chunk(bench.LADDER))
                env = A.BatchedABREnv(mpd, A.QOEMetric(*bench.WEIGHTS), A.NetworkInfo(bench.INTERVAL, traces), N,
                                      device="cuda", auto_reset=False)
                env.reset(tid_t, off_t)
                led, ql = env.set_episode_ledger(1), env.set_quality(weight, utility)
                ctl = A.ForecastMPCController(A.EnvPlayer(env), H, window=WINDOW, robust=robust)
                out = env.step_plan(ctl, V, want_obs=False)
                rec = ql.records(led)
                hist = torch.bincount(out["actions"].reshape(-1).long(), minlength=M)
                name = "forecast MPC, " + ("robust" if robust else "harmonic") + f", horizon {H}"
                rows.append(dict(utility=utility, weight=weight, controller=name, horizon=H, robust=robust, window=WINDOW,
                                 qoe=float(rec["qoe"].mean()), quality=float(rec["quality"].mean()),
                                 qoe_q=float(rec["qoe_q"].mean()), episodes=int(rec["qoe_q"].numel()),
                                 timeouts=int((out["done"][-1] & A._lib.DONE_TIMEOUT != 0).sum()),
                                 action_histogram=hist.tolist()))
                print(json.dumps(rows[-1]), flush=True)
                del env, led, ql, ctl, out
                torch.cuda.empty_cache()
        for k, v in LS.ON_RECORD[utility].items():
            rows.append(dict(utility=utility, weight=weight, controller=k, qoe_q=v, on_record=True))
            print(json.dumps(rows[-1]), flush=True)
        for r in look:
            if r["utility"] == utility:
                rows.append(dict(utility=utility, weight=weight, controller=r["controller"], horizon=r["horizon"],
                                 qoe=r["qoe"], qoe_q=r["qoe_q"], on_record=True))
                print(json.dumps(rows[-1]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), lanes=N, video_length=V, ladder=bench.LADDER, weights=bench.WEIGHTS,
               horizons=list(HORIZONS), window=WINDOW, rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "plan_study.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
