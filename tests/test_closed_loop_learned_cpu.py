"""The learned family of the closed-loop checker (tests/closed_loop_check.py: make_learned_case, check_learned) without a
GPU: the checker is silent on the reference's own closed loop (oracle_run_learned) for every (net, speed feature, episode
mode) triple of the GPU slice, at the slice's own lane counts; those 128 reference runs reach everything the slice is for
(assert_non_vacuous_learned); and the checker flags, by name, wrong runs of the kinds the learned-policy kernels, their
host path and the two ledgers could produce.  The wrong runs are the reference closed loop with one rule changed
(LearnedReference / learned_expected / learned_reward_fn: `mut`), not arrays edited at random."""
import numpy as np
import pytest

import closed_loop_check as K
import ledger_twin
import policy_twin as T

STATS, CASES = {}, {}


def _reference_run(seed):
    case = K.make_learned_case(seed)
    out = K.oracle_run_learned(case)
    assert K.check_learned(case, out, STATS) == [], K.describe_learned(case)
    CASES[seed] = case


@pytest.mark.parametrize("seed", range(K.LEARNED_SLICE))
def test_checker_is_silent_on_the_reference_closed_loop(seed):
    _reference_run(seed)


def test_the_reference_slice_is_not_vacuous():
    """Folds the counters of the 128 runs above (a seed that has not run yet, runs here)."""
    for seed in range(K.LEARNED_SLICE):
        if seed not in CASES:
            _reference_run(seed)
    assert K.assert_non_vacuous_learned(STATS, list(CASES.values())) == []


def test_slice_covers_every_triple_impl_and_option():
    cases = [K.make_learned_case(s) for s in range(K.LEARNED_SLICE)]
    assert {(c["net"], c["feature"], c["mode"]) for c in cases} == \
        {(n, f, m) for n, f in K.LEARNED_CELLS for m in K.EP_MODES}
    for net in K.NETS:
        mine = [c for c in cases if c["net"] == net]
        assert {c["impl"] for c in mine} == set(K.accepted_impls_ep("policy", "config")), net
        assert {c["params"]["sample"] for c in mine} == {"argmax", "softmax"}, net
    assert sum(c["params"]["sample"] == "softmax" for c in cases) >= len(cases) // 2
    assert {(c["ledger"] is not None, c["quality"] is not None) for c in cases} == {(a, b) for a in (0, 1) for b in (0, 1)}
    assert all(c["quality"]["rows"] == c["ledger"]["rows"] for c in cases if c["ledger"] and c["quality"])
    assert {c["ledger"]["rows"] for c in cases if c["ledger"]} == {1, 2, 3}
    utils = {c["quality"]["utility"] if isinstance(c["quality"]["utility"], str) else "table" for c in cases if c["quality"]}
    assert utils == {"identity", "log", "log_top", "table"}
    assert {c["params"]["value"] for c in cases} == {True, False}
    for c in cases:
        p, V = c["params"], c["meta"]["video_length"]
        pop = "pop" in c["net"]
        assert c["n_lanes"] in (K.POP_LANES if pop else K.LANES) and V <= 18 and c["n_steps"] < 60
        assert len(p["members"]) == (-(-c["n_lanes"] // K.POP_GROUP) if pop else 1) and p["group"] == K.POP_GROUP
        if c["single"]:
            assert any(op[0] == "launch" and op[1] == 1 for op in c["ops"]), K.describe_learned(c)
        if "hidden" in p:
            assert p["hidden"] in K.GRU_H["gru_mx" if c["net"].endswith("_mx") else "gru"]
        else:
            assert len(p["widths"]) <= (3 if c["net"].endswith("_mx") else 2)
            assert all(1 <= w <= (128 if c["net"].endswith("_mx") else 64) for w in p["widths"])
    assert any(c["single"] for c in cases) and not all(c["single"] for c in cases)
    pops = [c for c in cases if "pop" in c["net"]]
    assert {c["n_lanes"] for c in pops} == set(K.POP_LANES)
    # each member its own weights
    for c in pops:
        first = [mb["layers"][0][0] if "layers" in mb else mb["parts"][0] for mb in c["params"]["members"]]
        assert all(not np.array_equal(first[0], x) for x in first[1:])


def test_make_episode_case_is_unchanged_by_the_hooks():
    """The two existing families draw from their own generators: a learned case of the same seed shares nothing."""
    a, b = K.make_episode_case(24), K.make_learned_case(24)
    assert a["ctl"] == "policy" and a["family"] == "episodes" and b["family"] == "learned"
    assert "net" not in a and "members" not in a["params"]


def test_the_fast_fmaf_is_the_rounding_to_odd():
    """policy_twin.fmaf takes fmaf_odd's path only where one float64 rounding could differ: the same bits everywhere,
    on operands of few bits (exact ties and near ties are frequent), half-way sums, subnormal and overflowing results."""
    rng = np.random.default_rng(3)
    n = 200_000
    for sc in (1.0, 2.0 ** -120, 2.0 ** -140, 2.0 ** 100):
        a = (rng.integers(-2 ** 12, 2 ** 12, n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
        b = (rng.integers(-2 ** 12, 2 ** 12, n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
        with np.errstate(all="ignore"):
            c = ((rng.integers(-2 ** 24, 2 ** 24, n) + 0.0) * 2.0 ** rng.integers(-40, 40, n) * sc).astype(np.float32)
            t = rng.normal(0, 1, n).astype(np.float32)
            mid = (t.astype(np.float64) + np.nextafter(t, np.float32(np.inf)).astype(np.float64)) / 2
            c2 = (mid - a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
        for cc in (c, c2):
            assert np.array_equal(T.fmaf(a, b, cc).view(np.uint32), T.fmaf_odd(a, b, cc).view(np.uint32))
    sp = np.array([0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4e38, -3.4e38, 1.17549435e-38], np.float32)
    A_, B_, C_ = (x.ravel() for x in np.meshgrid(sp, sp, sp))
    assert np.array_equal(T.fmaf(A_, B_, C_).view(np.uint32), T.fmaf_odd(A_, B_, C_).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# wrong runs the checker must flag

def _small(seed):
    return K.make_learned_case(seed, n_lanes=8, group=3)


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _flags(pred, mut, names, seeds=range(K.LEARNED_SLICE), prefix=False):
    """The first small case of `seeds` with pred(case) whose run the perturbation changes: the checker is silent on the
    reference run and reports a mismatch of one of `names` on the perturbed one."""
    for s in seeds:
        case = _small(s)
        if not pred(case):
            continue
        good, bad = K.oracle_run_learned(case), K.oracle_run_learned(case, mut=mut)
        if _same(good, bad):
            continue
        assert K.check_learned(case, good) == [], K.describe_learned(case)
        got = {m["name"] for m in K.check_learned(case, bad)}
        hit = any(g.startswith(n) for g in got for n in names) if prefix else bool(got & set(names))
        assert hit, (K.describe_learned(case), sorted(got))
        return got
    raise AssertionError("the perturbation never changed a run")


gru = lambda c: K.net_is(c, "gru")
pop = lambda c: K.net_is(c, "pop")
drawn = lambda c: c["params"]["sample"] == "softmax" or 0 < c["params"]["thr"] < 1 << 32


def test_flags_a_gru_state_not_restarted_at_a_masked_reset():
    got = _flags(lambda c: gru(c) and c["mode"] != "sampled", dict(gru="no_restart_at_masked_reset"), {"hidden"})
    assert "scores" in got


def test_flags_a_gru_state_restarted_at_a_launch_boundary():
    _flags(gru, dict(gru="restart_at_launch"), {"hidden"})


def test_flags_a_softmax_draw_keyed_by_the_previous_episode_number():
    _flags(lambda c: c["params"]["sample"] == "softmax" and c["sampler"] is not None and c["auto_reset"],
           dict(episode="previous"), {"action"})


def test_flags_a_draw_keyed_by_the_lane_id_modulo_2_32():
    _flags(lambda c: drawn(c) and c["lane_id_base"] >= 2 ** 32, dict(lane="mod_2_32"), {"action"})


def test_flags_a_member_taken_from_the_global_lane_id():
    _flags(lambda c: pop(c) and c["lane_id_base"] > 0, dict(member="global"), {"scores"})


def test_flags_a_member_off_by_one_group_in_the_partial_group():
    _flags(pop, dict(member="partial_off_by_one"), {"scores"})


def test_flags_hidden_holding_the_new_state():
    _flags(gru, dict(hidden_out="hp"), {"hidden"})


def test_flags_last_value_taken_before_the_last_step():
    _flags(lambda c: c["params"]["value"], dict(last_value="before_last_step"), {"last_value"})


def test_flags_a_ledger_record_of_an_abandoned_episode():
    _flags(lambda c: c["ledger"] and c["mode"] != "sampled", dict(ledger="abandoned"), {"ledger.count"})


class _NoWrap(ledger_twin.TwinLedger):
    """A ring whose slot index saturates instead of wrapping."""

    def append(self, lane, *a):
        real = int(self.count[lane])
        self.count[lane] = min(real, self.rows - 1)
        super().append(lane, *a)
        self.count[lane] = real + 1


def test_flags_a_ledger_slot_not_wrapped():
    # a ring of two rows and lanes that finish three episodes: the third record belongs in slot 0
    _flags(lambda c: c["ledger"] and c["ledger"]["rows"] == 2 and c["mode"] == "sampled"
           and c["n_steps"] >= 3 * c["meta"]["video_length"], dict(ledger_cls=_NoWrap), {"ledger.ring."},
           seeds=range(8 * K.LEARNED_SLICE), prefix=True)


def test_flags_the_quality_term_of_the_next_chunk():
    _flags(lambda c: c["quality"], dict(quality="next_chunk"), {"reward"})


def test_flags_the_quality_term_on_a_step_without_a_download():
    _flags(lambda c: c["quality"] and c["mode"] == "masked", dict(quality="on_idle"), {"reward"})


def test_flags_probs_left_on_an_idle_lane():
    _flags(lambda c: c["mode"] == "masked", dict(idle_probs=True), {"probs"})
