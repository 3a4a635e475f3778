#!/usr/bin/env python3
"""What a forecast-MPC decision costs (include/abr_env.h: abr_env_plan_select, abr_env_step_plan) next to the lookahead
label it shares its walk with, on bench.py's workload (48-chunk episodes, 6 rates, 1 024 synthetic 1 000-point traces),
lanes in mid-episode (seven random decisions in).  tools/bench_lookahead.py's protocol: cases alternate after warm-ups,
--repeats rounds of calls between two HIP events, medians and the spread (max - min over the median).

select     per --lanes x --horizons, on the same states in the same session: LookaheadExpert.labels(want_q=True),
           ForecastMPCController.select(want_q=True) with the built-in robust forecast (forecast kernel + walk), and the
           same with a caller's forecast (the walk alone).  Tree nodes per call are computed from the shapes, lanes x (M +
           M^2 + ... + M^h); the planner's trees are the same size unless a sequence times out earlier.  plan_over_lookahead
           is the ratio of the medians.
rollout    step_plan of 48 decisions from a reset (auto_reset), built-in robust forecast: seconds per rollout, decisions/s.

Writes OUT/plan_bench.json and prints it.

    python tools/bench_plan.py OUT [--lanes 65536 1048576] [--horizons 3 4 5] [--warmup 1] [--repeats 3]
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
from bench_lookahead import make_env, nodes_per_lane, summary, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--horizons", type=int, nargs="+", default=[3, 4, 5])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    traces = bench.synth_traces()
    V, M = bench.V, len(bench.LADDER)
    sel, roll = [], []
    for N in a.lanes:
        env = make_env(N, traces, False)
        env.step_random(7, 3)                                  # mid-episode state in every lane
        keep = []
        F = torch.full((N,), 2.0, dtype=torch.float64, device="cuda")
        cases = {}
        for h in a.horizons:
            exp, ctl = A.LookaheadExpert(A.EnvPlayer(env), h), A.ForecastMPCController(A.EnvPlayer(env), h)
            ctl.select()                                       # the robust state exists and holds this chunk's estimate

            def label(exp=exp):
                keep[:] = [exp.labels(want_q=True)]

            def plan(ctl=ctl):
                keep[:] = [ctl.select(want_q=True)]

            def plan_given(ctl=ctl):
                keep[:] = [ctl.select(want_q=True, forecast=F)]
            cases[(h, "lookahead")], cases[(h, "plan")], cases[(h, "plan_given")] = label, plan, plan_given
        calls = {h: int(max(1, min(20, 2e9 // (N * nodes_per_lane(M, h))))) for h in a.horizons}
        runs = {k: [] for k in cases}
        for _ in range(a.repeats):
            for k, fn in cases.items():
                runs[k].append(timed(fn, calls[k[0]], a.warmup))
        for h in a.horizons:
            nodes = N * nodes_per_lane(M, h)
            r = dict(lanes=N, horizon=h, calls_per_timing=calls[h], nodes_per_call=nodes)
            for what in ("lookahead", "plan", "plan_given"):
                r[what] = summary(runs[(h, what)])
                r[what]["nodes_per_s"] = nodes / r[what]["seconds"]
            r["plan_over_lookahead"] = r["plan"]["seconds"] / r["lookahead"]["seconds"]
            r["plan_given_over_lookahead"] = r["plan_given"]["seconds"] / r["lookahead"]["seconds"]
            sel.append(r)
            print(json.dumps(r), flush=True)
        lab = A.ForecastMPCController(A.EnvPlayer(env), a.horizons[0]).select()
        decided = float((lab["action"] >= 0).double().mean())
        for x in sel:
            if x["lanes"] == N:
                x["share_of_lanes_decided"] = decided
        del env, cases, keep
        torch.cuda.empty_cache()
        # the fused rollout: 48 decisions from a reset
        env = make_env(N, traces, True)
        out = env._rollout_out(V, want_obs=False, want_actions=False)
        for h in a.horizons:
            ctl = A.ForecastMPCController(A.EnvPlayer(env), h)
            v = [timed(lambda: env.step_plan(ctl, V, out=out), 1, a.warmup if k == 0 else 0) for k in range(a.repeats)]
            r = dict(lanes=N, horizon=h, decisions=V, **summary(v))
            r["decisions_per_s"] = N * V / r["seconds"]
            roll.append(r)
            print(json.dumps(r), flush=True)
        del env, out
        torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), video_length=V, n_rates=M, warmup=a.warmup, repeats=a.repeats,
               select=sel, rollout=roll)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "plan_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
