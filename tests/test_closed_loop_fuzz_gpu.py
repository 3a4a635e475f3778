"""The closed-loop rollouts under configuration-space fuzz (tests/closed_loop_check.py, tools/gpu_fuzz_closed.py): the
harmonic MPC, RobustMPC, FastMPC, BBA-0, RATE and BOLA, each under the config speed, per-lane speeds, a speed schedule
and a LatencySpeedController, on every impl that accepts the pair, with and without per-chunk ladders and auto_reset,
launched in pieces that do not divide the video length, at lane counts off the workgroup sizes.  Every action is the
reference controller's answer at the replayed call site, and the replay reproduces every obs row, reward, done flag,
frame, history row, QoE and speed-log entry."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

SLICE = 144          # six times every (controller x speed feature) cell


def test_closed_loop_fuzz_slice():
    import closed_loop_check as K
    import gpu_fuzz_closed
    stats, cells, impls, cases, lane_steps = {}, {}, {}, [], 0
    for seed in range(SLICE):
        mm, ls, key, case = gpu_fuzz_closed.run_seed(seed, None, stats)
        assert not mm, (K.describe(case), len(mm), mm[:6])
        lane_steps += ls
        cells[key] = cells.get(key, 0) + 1
        impls.setdefault(case["ctl"], set()).add(case["impl"])
        cases.append(case)
    print("closed-loop slice:", lane_steps, "lane-steps;", dict(sorted(cells.items())),
          {k: sorted(v) for k, v in impls.items()})
    assert len(cells) == len(K.CELLS) and min(cells.values()) >= SLICE // len(K.CELLS)
    for c in K.CONTROLLERS:
        want = set(K.accepted_impls(c, "config")) | set(K.accepted_impls(c, "rule"))
        assert impls[c] == want, (c, impls[c])
    assert K.assert_non_vacuous(stats, cases) == []


def long_case(n_lanes):
    """RobustMPC under a speed rule on `auto` at the bench ladder, V = 48, launched in five pieces past the end."""
    import closed_loop_check as K
    case = K.make_case(7, n_lanes=n_lanes)                  # a robust / rule cell, reshaped
    assert (case["ctl"], case["feature"]) == ("robust", "rule")
    V, L = 48, 4.0
    ladder = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
    rng = np.random.default_rng(3)
    case["traces"] = [rng.uniform(0.3, 7.0, int(n)).astype(np.float32).astype(np.float64) for n in (800, 1200, 333)]
    case["tid"] = rng.integers(0, 3, n_lanes).astype(np.int32)
    case["off"] = rng.integers(0, 333, n_lanes).astype(np.int32)
    case["meta"].update(ladder=ladder, chunk_length=L, video_length=V, max_buffer=12.0, start_up_length=4.0,
                        interval=1.0)
    case["params"].update(horizon=4, window=5, qoe=[0.3, 1.0, 0.0], sizes=np.tile(np.asarray(ladder) * L, (V, 1)))
    case["rule"] = ((2.0, 6.0), (1.0, 8.0), ((0.9, 1.0, 1.0), (0.9, 1.1, 1.25), (0.75, 1.5, 2.0)))
    case["impl"], case["n_steps"], case["pieces"] = "auto", V + 3, [7, 13, 5, 20, 6]
    case["max_ticks"] = 2_000_000
    return case


def test_closed_loop_long_case_sampled_lanes():
    """16 384 lanes, V = 48: the sampled lanes checked in full (every decision, frame, reward, speed-log entry)."""
    import closed_loop_check as K
    import gpu_fuzz_closed
    case = long_case(16384)
    rng = np.random.default_rng(3)
    B = len(case["meta"]["ladder"])
    out = gpu_fuzz_closed.run_case(case)
    pick = np.sort(rng.choice(case["n_lanes"], 256, replace=False))
    sub = dict(case, n_lanes=len(pick), tid=case["tid"][pick], off=case["off"][pick])
    o = dict(out)
    for k in ("actions", "reward", "done"):
        o[k] = out[k][:, pick]
    o["obs"] = out["obs"][:, :, pick]
    o["frames"] = [(t, {k: v[pick] for k, v in f.items()}) for t, f in out["frames"]]
    o["history"] = tuple(h[:, pick] for h in out["history"])
    o["qoe"] = out["qoe"][pick]
    o["speed_log"] = out["speed_log"][:, pick]
    stats = {}
    mm = K.check(sub, o, stats)
    assert not mm, mm[:6]
    assert len(stats["answers"]["robust"]) >= min(3, B) and stats["clipped"] > 0 and len(stats["speeds"]) >= 2
