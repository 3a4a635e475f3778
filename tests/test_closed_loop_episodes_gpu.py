"""The closed-loop rollouts over sampled, staggered and policy-driven episodes (tests/closed_loop_check.py: the episode
family, tools/gpu_fuzz_closed.py --episodes): the six controllers and the learned policy, each under the config speed,
per-lane speeds, a schedule and a LatencySpeedController, in four episode modes (auto_reset with a sampler; with a sampler
and masked resets; with masked resets and no sampler; auto_reset off with masked resets that revive finished lanes and
restart running ones), on every impl that accepts the pair, at lane_id_base 0, off a multiple of 64 and >= 2^32.  Every
action is the reference controller's answer at the replayed call site of its lane's own episode, and the replay
reproduces every obs row, reward, done flag, and after every operation the frame, episodes() and the speed log; then the
history and the QoE of each lane's last finished episode."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


def test_closed_loop_episode_slice():
    import closed_loop_check as K
    import gpu_fuzz_closed
    stats, cells, impls, cases = {}, {}, {}, []
    for seed in range(K.EP_SLICE):
        mm, _, key, case = gpu_fuzz_closed.run_episode_seed(seed, None, stats)
        assert not mm, (K.describe_ep(case), len(mm), mm[:6])
        cells[key] = cells.get(key, 0) + 1
        impls.setdefault(case["ctl"], set()).add(case["impl"])
        cases.append(case)
    assert len(cells) == K.EP_SLICE
    for c in K.EP_CONTROLLERS:
        want = set(K.accepted_impls_ep(c, "config")) | set(K.accepted_impls_ep(c, "rule"))
        assert impls[c] == want, (c, impls[c])
    assert K.assert_non_vacuous_ep(stats, cases) == []


def long_case(n_lanes, ctl_seed=35):
    """RobustMPC under a speed rule on split3 at the bench ladder, V = 48, with a sampler and masked resets that stagger
    the lanes (seed 35: robust / rule / sampled_staggered, reshaped)."""
    import closed_loop_check as K
    case = K.make_episode_case(ctl_seed, n_lanes=n_lanes)
    assert (case["ctl"], case["feature"], case["mode"]) == ("robust", "rule", "sampled_staggered")
    V, L = 48, 4.0
    ladder = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
    rng = np.random.default_rng(5)
    case["traces"] = [rng.uniform(0.3, 7.0, int(n)).astype(np.float32).astype(np.float64) for n in (800, 1200, 333, 61)]
    case["tid"] = rng.integers(0, 4, n_lanes).astype(np.int32)
    case["off"] = rng.integers(0, 61, n_lanes).astype(np.int32)
    case["meta"].update(ladder=ladder, chunk_length=L, video_length=V, max_buffer=12.0, start_up_length=4.0,
                        interval=1.0)
    case["br"], case["vbr"] = None, False
    case["params"].update(horizon=4, window=5, qoe=[0.3, 1.0, 0.0], sizes=np.tile(np.asarray(ladder) * L, (V, 1)))
    case["rule"] = ((2.0, 6.0), (1.0, 8.0), ((0.9, 1.0, 1.0), (0.9, 1.1, 1.25), (0.75, 1.5, 2.0)))
    case["log_rows"] = V + 4
    case["sampler"] = dict(seed=2 ** 63 + 12345, pool=[0, 2, 3, 2], span=0)
    case["lane_id_base"] = 2 ** 32 + 4097
    case["impl"] = "split3"
    m1 = np.zeros(n_lanes, bool)
    m1[64:128] = True                                            # one whole wave
    m1[200:230] = True                                           # part of one
    m1 |= rng.random(n_lanes) < 0.1
    m2 = rng.random(n_lanes) < 0.3
    case["ops"] = [("reset", None, None, None), ("launch", 17), ("reset", m1, None, None), ("launch", 40),
                   ("launch", 9), ("reset", m2, None, None), ("launch", 50)]
    case["n_steps"] = 17 + 40 + 9 + 50
    case["max_ticks"] = 2_000_000
    return case


def test_closed_loop_episodes_long_case_sampled_lanes():
    """16 384 lanes on split3: 256 sampled lanes checked in full (every decision, frame, episodes(), speed-log row)."""
    import closed_loop_check as K
    import gpu_fuzz_closed
    case = long_case(16384)
    out = gpu_fuzz_closed.run_episode_case(case)
    pick = np.sort(np.random.default_rng(3).choice(case["n_lanes"], 256, replace=False))
    sub, o = K.subset_episode_case(case, out, pick)
    stats = {}
    mm = K.check_episodes(sub, o, stats)
    assert not mm, mm[:6]
    assert len(stats["answers"]["robust"]) >= 3 and stats["clipped"] > 0
    assert stats.get("restarted_history", {}).get("robust") and stats.get("rule_differs")
    assert len({int(x) for x in out["episodes"][-1]["episode"]}) >= 3
