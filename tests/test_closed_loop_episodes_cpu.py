"""The episode family of the closed-loop checker (tests/closed_loop_check.py: make_episode_case, check_episodes) without a
GPU: the config family's generator is pinned to what it generated before, the checker is silent on the reference's own
closed loop for every (controller, speed feature, episode mode) triple, it flags wrong runs of the kinds a sampled,
staggered or policy-driven rollout could produce, and the GPU slice covers every triple and every accepted impl."""
import copy
import hashlib

import numpy as np
import pytest

import closed_loop_check as K
from sampler_twin import twin

MAKE_CASE_DIGEST = "4c070420ce4cbb95a55b612493f52a9d475dac0059258534f6e071f0282c3ea3"   # seeds 0..2399


def _feed(h, x):
    if isinstance(x, dict):
        h.update(b"{")
        for k in sorted(x):
            h.update(repr(k).encode())
            _feed(h, x[k])
        h.update(b"}")
    elif isinstance(x, (list, tuple)):
        h.update(b"[" if isinstance(x, list) else b"(")
        for v in x:
            _feed(h, v)
        h.update(b"]")
    elif isinstance(x, np.ndarray):
        h.update(f"nd{x.dtype.str}{x.shape}".encode())
        h.update(np.ascontiguousarray(x).tobytes())
    elif isinstance(x, np.generic):
        _feed(h, np.asarray(x))
    else:
        h.update(f"{type(x).__name__}:{x!r}".encode())


def test_make_case_is_unchanged():
    """profiles/closed_loop_fuzz.json ran seeds 0..2399 of make_case: they must still describe the same cases."""
    h = hashlib.sha256()
    for s in range(2400):
        _feed(h, K.make_case(s))
    assert h.hexdigest() == MAKE_CASE_DIGEST


def _run(seed, n=8, **kw):
    case = K.make_episode_case(seed, n_lanes=n)
    ent = K.OracleEntries(case) if case["ctl"] == "fastmpc" else None
    return case, K.oracle_run_episodes(case, ent, **kw)


@pytest.mark.parametrize("seed", range(K.EP_SLICE))
def test_checker_is_silent_on_the_reference_closed_loop(seed):
    case, out = _run(seed)
    assert K.check_episodes(case, out) == [], K.describe_ep(case)


def test_every_triple_has_a_silent_seed():
    triples = {(c["ctl"], c["feature"], c["mode"]) for c in map(K.make_episode_case, range(K.EP_SLICE))}
    assert triples == {(c, f, m) for c, f in K.EP_CELLS for m in K.EP_MODES}


# ---------------------------------------------------------------------------------------------------------------------
# wrong runs the checker must flag

def _lanes_flagged(mm):
    return {x["lane"] for x in mm}


def _find(pred, seeds):
    for s in seeds:
        c = K.make_episode_case(s, n_lanes=8)
        if pred(c):
            return s
    raise AssertionError("no seed")


def _flag_some_lane(seed, mutant_for_lane, lanes=range(8), run=None, **kw):
    """Build the run with the mutation on one lane at a time until it changes the run; the checker must flag that lane.
    run(seed, **kw) -> (case, out) replaces _run (tests/test_trace_edges_cpu.py: cases on other trace families)."""
    run = run or _run
    case, good = run(seed)
    assert K.check_episodes(case, good) == []
    for x in lanes:
        _, bad = run(seed, **mutant_for_lane(x))
        if any(not np.array_equal(np.asarray(good[k]), np.asarray(bad[k])) for k in ("actions", "reward", "obs")) or \
                any(not np.array_equal(a[k], b[k]) for a, b in zip(good["episodes"], bad["episodes"]) for k in a):
            mm = K.check_episodes(case, bad)
            assert x in _lanes_flagged(mm), (x, mm[:6])
            return mm
    raise AssertionError("the mutation never changed the run")


def next_episodes_pair_mutant(x):
    """Lane x runs its episode 1 on the pair of its episode 2."""
    def pair_fn(case, lanes, eps):
        eps = np.asarray(eps, np.int64) + (np.asarray(lanes) == x) * (np.asarray(eps) == 1)
        return K.sampled_pairs(case, lanes, eps)
    return dict(pair_fn=pair_fn)


def test_flags_a_segment_on_the_next_episodes_pair():
    seed = _find(lambda c: c["mode"] == "sampled" and c["sampler"]["pool"] is None, range(0, 28))
    mm = _flag_some_lane(seed, next_episodes_pair_mutant)
    assert any(m["name"].startswith("episodes.") for m in mm)


def test_flags_pairs_drawn_with_the_local_lane_id():
    seed = _find(lambda c: c["sampler"] is not None and c["sampler"]["pool"] is None and c["lane_id_base"] >= 2 ** 32,
                 range(0, 112))

    def mut(x):
        def pair_fn(case, lanes, eps):
            s = case["sampler"]
            tl = [len(t) for t in case["traces"]]
            return twin(s["seed"], np.asarray(lanes, np.uint64), np.asarray(eps, np.int64), tl, s["pool"], s["span"])
        return dict(pair_fn=pair_fn)
    case, good = _run(seed)
    _, bad = _run(seed, **mut(0))
    mm = K.check_episodes(case, bad)
    assert any(m["name"].startswith("episodes.") for m in mm), mm[:4]


class _StaleRobust(K.Reference):
    """RobustMPC whose state is not emptied at chunk 0 of a lane's later segments (a masked reset or a re-arm)."""

    def __init__(self, case, entries=None):
        super().__init__(case, entries)
        self.starts = {}

    def new_episode(self, i):
        super().new_episode(i)
        self.starts[i] = self.starts.get(i, -1) + 1

    def answer(self, i, c, prev, buf, h):
        if c == 0 and self.starts[i] > 0:
            snap = K._robust_snapshot(self, i)
            a = super().answer(i, c, prev, buf, h)
            K._robust_restore(self, i, snap)
            return a
        return super().answer(i, c, prev, buf, h)


def test_robust_state_not_emptied_at_a_restart_changes_nothing():
    """RobustMPC's chunk test (an error sample is taken only when the last estimate was made at chunk c - 1, the window
    kept only when it was made at chunk c) drops a stale state by itself: a segment's first estimate with a history is
    at chunk 1, and no estimate ever leaves the state at chunk 1 or at chunk 2 with errors in its window.  So a lane whose
    state survives a restart -- cut after one, two or three decisions -- plays exactly the run of one whose state was
    emptied, and there is nothing for the checker to flag; this pins that reasoning on every lane."""
    answers = set()
    for seed in range(4, 4 * 28 * 4, 28):                        # robust / config
        case = K.make_episode_case(seed, n_lanes=8)
        V = case["meta"]["video_length"]
        every = np.ones(8, bool)
        case["ops"] = [case["ops"][0]]
        for n in (3, 1, 2, 3, 2, 4):
            case["ops"] += [("launch", n), ("reset", every, case["tid"], case["off"])]
        case["ops"].append(("launch", V + 2))
        case["n_steps"] = 15 + V + 2
        good = K.oracle_run_episodes(case)
        assert K.check_episodes(case, good) == []
        bad = K.oracle_run_episodes(case, ref_factory=_StaleRobust)
        assert np.array_equal(good["actions"], bad["actions"]), seed
        answers |= set(np.unique(good["actions"][good["actions"] >= 0]).tolist())
    assert len(answers) >= 3


def _wave_max_episode(segs, batch):
    """Each call site's episode number replaced by the largest episode number in its lane's wave at that decision."""
    V = max(s.n for x in segs for s in x) or 1
    out = []
    for sg in batch:
        w = sg.lane // 64
        row = []
        for s in range(V):
            t = sg.t0 + s
            row.append(max(max((x.episode for x in segs[j] if x.t0 <= t), default=0)
                           for j in range(w * 64, min(len(segs), w * 64 + 64))))
        out.append(row)
    return np.asarray(out)


def test_flags_policy_exploration_keyed_by_the_waves_largest_episode():
    """Lanes of one wave at different episode numbers: a draw keyed by the wave's largest one is flagged."""
    for s in range(24, 28 * 40, 28):                             # policy / config
        case = K.make_episode_case(s, n_lanes=8)
        if not 0 < case["params"]["thr"] < 1 << 32:
            continue
        V = case["meta"]["video_length"]
        some, one = np.isin(np.arange(8), [0, 2, 5]), np.arange(8) == 1
        case["ops"] = [case["ops"][0], ("launch", 3), ("reset", some, case["tid"], case["off"]), ("launch", V),
                       ("reset", one, case["tid"], case["off"]), ("launch", V)]
        case["n_steps"] = 3 + 2 * V
        good = K.oracle_run_episodes(case)
        assert K.check_episodes(case, good) == []
        bad = K.oracle_run_episodes(case, policy_episode_fn=lambda segs, b: _wave_max_episode(segs, b)[:, :V])
        if not np.array_equal(good["actions"], bad["actions"]):
            mm = K.check_episodes(case, bad)
            assert any(m["name"] == "action" for m in mm), mm[:4]
            return
    raise AssertionError("the mutation never changed an action")


def test_flags_a_speed_log_row_left_from_the_previous_episode():
    seed = _find(lambda c: c["feature"] == "rule" and c["auto_reset"] and c["log_rows"] > c["meta"]["video_length"],
                 range(3, 112, 4))
    case, out = _run(seed)
    assert K.check_episodes(case, out) == []
    flags_a_stale_speed_log_row(case, out)


def flags_a_stale_speed_log_row(case, out):
    """The first speed-log row an operation rewrote, put back to what the previous episode left: flagged by name."""
    logs = out["speed_logs"]
    for oi in range(1, len(logs)):
        diff = np.argwhere(logs[oi] != logs[oi - 1])
        if len(diff):
            r, i = diff[0]
            bad = copy.deepcopy(out)
            bad["speed_logs"][oi][r, i] = logs[oi - 1][r, i]
            mm = K.check_episodes(case, bad)
            assert ("speed_log", oi * 10_000 + r, i) in {(m["name"], m["step"], m["lane"]) for m in mm}, mm[:4]
            return
    raise AssertionError("no row was rewritten")


# ---------------------------------------------------------------------------------------------------------------------
# the GPU slice

def test_gpu_slice_covers_every_triple_and_impl():
    cases = [K.make_episode_case(s) for s in range(K.EP_SLICE)]
    triples = {(c, f, m) for c, f in K.EP_CELLS for m in K.EP_MODES}
    assert {(c["ctl"], c["feature"], c["mode"]) for c in cases} == triples
    for ctl in K.EP_CONTROLLERS:
        got = {x["impl"] for x in cases if x["ctl"] == ctl}
        assert got == set(K.accepted_impls_ep(ctl, "config")) | set(K.accepted_impls_ep(ctl, "rule")), ctl
    for x in cases:
        assert x["impl"] in K.accepted_impls_ep(x["ctl"], x["feature"]), K.describe_ep(x)
        assert not (x["impl"] == "tick" and (x["feature"] != "config" or x["ctl"] in ("mpc", "robust", "policy")))
        assert x["auto_reset"] == (x["mode"] != "masked")
        assert (x["sampler"] is not None) >= (x["mode"] in ("sampled", "sampled_staggered"))
        masks = [op[1] for op in x["ops"][1:] if op[0] == "reset"]
        assert bool(masks) == (x["mode"] != "sampled")
    masks = [(x, op[1]) for x in cases for op in x["ops"][1:] if op[0] == "reset"]
    whole = lambda m: any(m[w:w + 64].all() and len(m[w:w + 64]) == 64 for w in range(0, len(m), 64))
    partial = lambda m: any(0 < m[w:w + 64].sum() < len(m[w:w + 64]) for w in range(0, len(m), 64))
    assert any(whole(m) for _, m in masks) and any(partial(m) for _, m in masks)
    # masked resets that revive finished lanes and restart running ones (auto_reset off)
    revived = restarted = 0
    for x in cases:
        if x["mode"] == "masked":
            segs, after = K.episode_plan(x)
            for oi, op in enumerate(x["ops"][1:], 1):
                if op[0] == "reset":
                    fin = after[oi - 1][1]
                    revived += int((op[1] & fin).sum())
                    restarted += int((op[1] & ~fin).sum())
    assert revived and restarted
    bases = [x["lane_id_base"] for x in cases]
    assert 0 in bases and any(b % 64 and b < 2 ** 32 for b in bases) and any(b >= 2 ** 32 for b in bases)
    smp = [x["sampler"] for x in cases if x["sampler"]]
    assert {None, 1} <= {None if s["pool"] is None else min(len(s["pool"]), 2) for s in smp} and \
        any(s["pool"] and len(s["pool"]) >= 2 for s in smp)
    spans = {s["span"] for s in smp}
    longest = lambda x: max(len(t) for t in x["traces"])
    assert 0 in spans and 1 in spans and any(1 < s["span"] < 40 for s in smp)
    assert any(x["sampler"] and x["sampler"]["span"] > longest(x) for x in cases)
    pol = [x["params"] for x in cases if x["ctl"] == "policy"]
    assert {p["thr"] == 0 for p in pol} == {True, False} and any(p["thr"] == 1 << 32 for p in pol)
    assert {len(p["layers"]) for p in pol} == {1, 2, 3}
    assert any(x["n_lanes"] % 64 for x in cases)


class _LateRule:
    """The tick loop with the speed rule answered one tick late: a chunk's first playing tick keeps the previous speed,
    the rule is read at its second tick (speed_twin.RuleTickEnv otherwise)."""

    @staticmethod
    def env(case, trace, offset):
        from speed_twin import RuleTickEnv

        class Late(RuleTickEnv):
            pending = False

            @property
            def speed(self):
                if self.play_len == 0:
                    self.pending = True
                    return self._sp
                if self.pending:
                    self.pending = False
                    self._sp = float(K.rule_np(*self.rule, self.t - self.play_time, self.buf))
                    self.log.append(self._sp)
                return self._sp

            @speed.setter
            def speed(self, _):
                pass
        m = case["meta"]
        return Late(m["ladder"], m["chunk_length"], m["video_length"], m["max_buffer"], m["start_up_length"],
                    m["interval"], m["weights"], list(trace), int(offset), rule=K.rule_arrays(case))

    @classmethod
    def run_batch(cls, case, segs_k, acts):
        from oracle import oracle as O
        V, rows = case["meta"]["video_length"], case["log_rows"]
        K_ = len(segs_k)
        steps, bw, fin = np.zeros((K_, V), O.STEP_DTYPE), np.zeros((K_, V)), np.zeros(K_, O.FINAL_DTYPE)
        log, calls = np.zeros((K_, rows)), np.zeros(K_, np.int32)
        for j, sg in enumerate(segs_k):
            env = cls.env(case, case["traces"][sg.trace], sg.offset)
            env.reset()
            for s in range(V):
                r = steps[j, s]
                for k, a in (("global_time", "t"), ("rebuffer_time", "rebuf"), ("start_up_time", "startup"),
                             ("play_time", "play_time"), ("average_latency", "avg_lat"), ("buffer_level", "buf"),
                             ("play_length", "play_len"), ("chunk_id", "chunk"), ("play_id", "play_id")):
                    r[k] = getattr(env, a)
                r["last_bitrate"] = env.hist_rates[-1] if env.hist_rates else -1
                r["last_bandwidth"] = env.hist_bw[-1] if env.hist_bw else 0.0
                env.step(int(acts[j, s]))
            for k, a in (("global_time", "t"), ("rebuffer_time", "rebuf"), ("start_up_time", "startup"),
                         ("play_time", "play_time"), ("average_latency", "avg_lat"), ("buffer_level", "buf"),
                         ("chunk_id", "chunk"), ("play_id", "play_id"), ("ticks", "ticks")):
                fin[j][k] = getattr(env, a)
            fin[j]["qoe"] = env.qoe()
            bw[j] = env.hist_bw
            n = min(len(env.log), rows)
            log[j, :n], calls[j] = env.log[:n], len(env.log)
        return steps, bw, fin, log, calls


def test_flags_the_rule_answered_one_tick_late_in_the_replay():
    """The checker's replay with the rule read one tick late disagrees with the reference's (the device's) run."""
    for seed in range(3, 112, 28):                               # mpc / rule, every mode
        case, out = _run(seed, n=6)
        if case["vbr"]:
            continue
        assert K.check_episodes(case, out) == []
        mm = K.check_episodes(case, out, run_batch=_LateRule.run_batch)
        names = {m["name"] for m in mm}
        assert names & {"frame.play_time", "obs.play_time"} and "qoe" in names, names
        return
    raise AssertionError("no case with one ladder")
