"""The closed-loop checker (tests/closed_loop_check.py) on the reference's own closed loop: it must stay silent there,
name exactly the element of every single-element mutation, and its generator must be deterministic and cover every
(controller x speed feature) cell and every accepted impl in the GPU slice."""
import copy

import numpy as np
import pytest

import closed_loop_check as K

FASTMPC_IDENTITY = 32                                    # a FastMPC case with the identity utility
SEEDS = list(range(0, 144, 3))[:48] + [50, 73]            # every cell, with and without VBR and auto_reset


def _run(seed, n=12):
    case = K.make_case(seed, n_lanes=n)
    ent = K.OracleEntries(case) if case["ctl"] == "fastmpc" else None
    return case, K.oracle_run(case, ent)


@pytest.mark.parametrize("seed", SEEDS)
def test_checker_passes_the_oracle_closed_loop(seed):
    case, out = _run(seed)
    assert K.check(case, out) == [], K.describe(case)


def test_checker_passes_the_composition_under_auto_reset():
    """The harmonic MPC at one speed comes from oracle.env_batch_mpc (the composition), under auto_reset too."""
    seeds = [s for s in range(48, 240, 24) if K.make_case(s)["auto_reset"]]
    assert seeds
    for seed in seeds[:2]:
        case, out = _run(seed)
        assert (case["ctl"], case["feature"]) == ("mpc", "config")
        assert K.check(case, out) == [], K.describe(case)


def _names(mm):
    return {(x["name"], x["step"], x["lane"]) for x in mm}


def _mutated(seed, mutate, run=None):
    case, out = (run or _run)(seed)
    assert K.check(case, out) == []
    out = copy.deepcopy(out)
    want = mutate(case, out)
    mm = K.check(case, out)
    assert want in _names(mm), (want, mm[:6])
    return mm


# single-element mutations of a run: each changes `out` in place and returns the (name, step, lane) the checker must report
# (module level: tests/test_trace_edges_cpu.py applies them to cases on other trace families)

def mutate_action(case, out):
    t, i = 3, 5
    out["actions"][t, i] = (out["actions"][t, i] + 1) % len(case["meta"]["ladder"])
    return ("action", t, i)


def mutate_frame_ulp(case, out):
    t, f = out["frames"][0]
    f["buffer_level"][4] = np.nextafter(f["buffer_level"][4], np.inf)
    return ("frame.buffer_level", t, 4)


def mutate_reward_ulp(case, out):
    out["reward"][2, 7] = np.nextafter(out["reward"][2, 7], np.float32(np.inf))
    return ("reward", 2, 7)


def mutate_speed_log(case, out):
    log = out["speed_log"]
    r = int(np.flatnonzero(log[:, 3])[1])
    log[r, 3] = 2.5 if log[r, 3] != 2.5 else 0.5
    return ("speed_log", r, 3)


def mutate_done_flag(case, out):
    out["done"][1, 2] ^= 1
    return ("done", 1, 2)


def mutate_history(case, out):
    out["history"][1][2, 6] = np.nextafter(out["history"][1][2, 6], 0.0)
    return ("history.bandwidth", 2, 6)


MUTATIONS = dict(action=(12, mutate_action),              # buffer / config
                 frame_ulp=(4, mutate_frame_ulp), reward_ulp=(16, mutate_reward_ulp),
                 speed_log=(19, mutate_speed_log),        # rate / rule
                 done_flag=(20, mutate_done_flag), history=(6, mutate_history))


def test_mutation_action():
    _mutated(*MUTATIONS["action"])


def test_mutation_frame_ulp():
    _mutated(*MUTATIONS["frame_ulp"])


def test_mutation_reward_ulp():
    _mutated(*MUTATIONS["reward_ulp"])


def test_mutation_speed_log():
    _mutated(*MUTATIONS["speed_log"])


def test_mutation_done_flag():
    _mutated(*MUTATIONS["done_flag"])


def test_mutation_history():
    _mutated(*MUTATIONS["history"])


def test_mutation_fastmpc_entry():
    case, out = _run(FASTMPC_IDENTITY)
    assert case["ctl"] == "fastmpc" and case["params"]["utility"] == "identity"
    assert K.check(case, out) == []
    used = sorted(out["entries"].cache)
    out["entries"] = _Dense(out["entries"])
    k = used[len(used) // 2]
    out["entries"].over[k] = (out["entries"][k] + 1) % len(case["meta"]["ladder"])
    mm = K.check(case, out)
    assert any(x["name"] == "entries" and x["value"]["idx"] == k for x in mm), mm[:6]


class _Dense:
    """The oracle's table with some entries overridden (a device table with one wrong entry)."""

    def __init__(self, base):
        self.base, self.shape, self.over = base, base.shape, {}

    def __getitem__(self, idx):
        idx = tuple(int(x) for x in idx)
        return self.over.get(idx, self.base[idx])


def test_generator_is_deterministic():
    for seed in (0, 31, 100):
        a, b = K.make_case(seed), K.make_case(seed)
        for k in a:
            if isinstance(a[k], (list, tuple)) and a[k] and isinstance(a[k][0], np.ndarray):
                assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
            elif isinstance(a[k], np.ndarray):
                assert np.array_equal(a[k], b[k]), k
            elif k != "params":
                assert a[k] == b[k], k
        for k in a["params"]:
            assert np.array_equal(np.asarray(a["params"][k]), np.asarray(b["params"][k])), k


def test_gpu_slice_covers_every_cell_and_impl():
    cases = [K.make_case(s) for s in range(144)]
    cells = {(c["ctl"], c["feature"]) for c in cases}
    assert cells == set(K.CELLS)
    for c in K.CONTROLLERS:
        got = {x["impl"] for x in cases if x["ctl"] == c}
        assert got == set(K.accepted_impls(c, "config")) | set(K.accepted_impls(c, "rule")), c
    for x in cases:
        assert x["impl"] in K.accepted_impls(x["ctl"], x["feature"]), K.describe(x)
        # the tick kernel serves neither speed features nor MPC rollouts; the role-split kernels no rule rollout
        assert not (x["impl"] == "tick" and (x["feature"] != "config" or x["ctl"] in ("mpc", "robust")))
        assert not (x["impl"] in ("split", "split3") and x["ctl"] not in ("mpc", "robust"))
    assert {x["vbr"] for x in cases} == {True, False} and {x["auto_reset"] for x in cases} == {True, False}
    assert any(x["n_lanes"] % 64 for x in cases)
    assert any(x["meta"]["max_buffer"] < 2 * x["meta"]["chunk_length"] for x in cases)
    assert any(x["ctl"] in ("mpc", "robust") and x["meta"]["video_length"] < x["params"]["horizon"] for x in cases)
    for x in cases:
        if x["auto_reset"]:
            V, ends = x["meta"]["video_length"], np.cumsum(x["pieces"])
            assert x["n_steps"] > V and not any(e % V == 0 for e in ends), K.describe(x)
        else:
            assert x["n_steps"] >= x["meta"]["video_length"] + 2


@pytest.mark.parametrize("method,utility", [("expsmoothing", "identity"), ("harmonic", "log"), ("expsmoothing", "log")])
def test_step_mpc_refuses_what_the_fused_rollout_would_ignore(method, utility):
    """abr_env_step_mpc runs the harmonic predictor with the identity utility: a controller asking for another predictor
    or utility used to be run as a harmonic / identity one without a word.  Refused before anything touches a device."""
    import abrsimulator_amd as A

    class Ctl:
        pass
    ctl = Ctl()
    ctl.method, ctl.utility = method, utility
    with pytest.raises(ValueError, match="step_mpc runs"):
        A.BatchedABREnv.step_mpc(object(), ctl, 4)
