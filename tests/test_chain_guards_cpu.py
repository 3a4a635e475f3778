"""The proven form of chain_segment (csrc/abr_exact_jump.h: GUARDS_PROVEN -- no budget clamp, no `n > 0` selects, no
`normal` test per segment) and its callers' side (csrc/abr_lane_jump.h: chains_proven, TablesT<false>::kGuards), on the CPU.

Part one: chains.  proven == checked == the naive one-addition-per-tick loop, bits of the value, the count and the hit flag,
and the same number of segments in both forms, over the generators of tests/test_chain_settle_cpu.py (their budgets cut to
the proven form's domain 1..2^20) and over the edges of that domain.

Part two: the lane functions.  The oracle-replay configurations of tests/test_lane_jump_cpu.py run on the no-speeds tables
(proven chains) next to the general tables (checked chains) and against the oracle; a hook on every call of the proven form
counts the calls that break a precondition: none may.

Part three: the routing predicate.  A configuration whose trace interval is shorter than a tick, or whose tick bound is
above 2^20, fails the proof, runs the general tables and still equals the oracle.

The chain cases also run through a stand-alone build of the harness with AddressSanitizer and UndefinedBehaviorSanitizer
(no sanitizer runs on code loaded into Python)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import native_harness
from test_chain_settle_cpu import _block, _cases
from test_lane_jump_cpu import CASES, _case, _check, _random_config

GE, LE, LT = 0, 1, 2
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 20


@pytest.fixture(scope="module")
def H():
    lib = native_harness("chain_guards_harness")
    lib.guards_check.restype = C.c_int64
    lib.cg_create.restype = C.c_void_p
    lib.cg_batch.restype = C.c_int64
    assert lib.guards_jump_cap() == CAP
    return lib


def _in_domain(block):
    """A block of test_chain_settle_cpu with its budgets cut to 1..2^20: the proven form's callers never hand it another."""
    kind, bias, x0, c, thr, n = block
    return kind, bias, x0, c, thr, np.clip(n, 1, CAP).astype(np.int32)


def _precondition_edges():
    out = []
    q = 2.0 ** -22
    # budgets of 1 and of exactly 2^20, with the stop within two steps of the budget's end and far beyond it
    for n in (1, 2, CAP - 1, CAP):
        for M in (n - 2, n - 1, n, n + 1, 4 * CAP):
            M = max(M, 1)
            if 1.0 + M * q < 2.0:
                out.append(_block(GE, 0, [1.0], q, 1.0 + M * q, n))
            if 1.75 - M * q > 1.0:
                out.append(_block(LE, 0, [1.75], -q, 1.75 - M * q, n))
                out.append(_block(LT, 0, [1.75], -q, 1.75 - M * q, n))
    out.append(_block(GE, 0, [0.0, 1.0, 3.0], [0.01, 0.01, 0.0125], 1e9, CAP))
    out.append(_block(LE, 0, [20.0, 1e6], [-0.01, -0.0125], 0.0, CAP))
    # c == 0 (an outage: nothing moves, a whole budget per segment), from zero, subnormal, tiny and ordinary values
    x = [0.0, 5e-324, 1e-310, 2.0 ** -1000, 2.0 ** -968, 1.0, 3.7, 1e300]
    for n in (1, 7, 100, CAP):
        out.append(_block(GE, 0, x, 0.0, 1e301, n))
        out.append(_block(LE, 0, x, -0.0, -1.0, n))
        out.append(_block(LT, 0, x, -0.0, -1.0, n))
    # x0 == 0 and thresholds already behind x
    out.append(_block(GE, 0, [0.0, 0.0, 0.0], [0.01, 0.048, 1e-3], [4.3, 17.2, 1.2], 3000))
    out.append(_block(GE, 0, [5.0, 5.0, 1e10], [0.01, 0.5, 3.0], [1.0, 5.0, -4.0], 100))
    out.append(_block(LE, 0, [1.0, 5.0, 0.0, -3.0], -0.01, [5.0, 5.0, 0.0, 1.0], 100))
    out.append(_block(LT, 0, [1.0, 5.0, 0.0, -3.0], -0.01, [5.0, 5.0000001, 0.0, 1.0], 100))
    # subnormal constants, and constants just either side of where `expo(|c|) < e` alone would let a tiny value jump
    cs = [5e-324, 1e-310, 2.0 ** -1022, 2.0 ** -1000, 2.0 ** -970, 2.0 ** -969, 2.0 ** -968, 2.0 ** -960]
    for x0 in (0.0, 1e-310, 2.0 ** -1010, 2.0 ** -969, 2.0 ** -968, 2.0 ** -967, 2.0 ** -950, 1.0):
        out.append(_block(GE, 0, np.full(len(cs), x0), cs, 17.2, 2000))
        out.append(_block(GE, 0, np.full(len(cs), x0), cs, np.array(cs) * 777.5 + x0, 2000))
        out.append(_block(LE, 0, np.full(len(cs), x0), -np.array(cs), 0.0, 2000))
        out.append(_block(LT, 0, np.full(len(cs), x0), -np.array(cs), x0 / 2, 2000))
    # 1e298 per tick against a finite target (the chunk is down on its first tick), and values of 2^1023 and more, where
    # the checked form does not jump and the proven one may
    out.append(_block(GE, 0, [0.0, 0.3, 17.0], 1e298, [17.2, 1.2, 17.2], [1, 50, 4000]))
    out.append(_block(GE, 0, [1e308, 2.0 ** 1023, 1.2e308], [1e300, 2.0 ** 970, 1e292], [1.7e308, 1.5e308, 1.79e308], 5000))
    out.append(_block(LE, 0, [1.7e308, 2.0 ** 1023 * 1.5], [-1e300, -2.0 ** 970], [1e308, 0.0], 5000))
    out.append(_block(LT, 0, [1.7e308, 2.0 ** 1023 * 1.5], [-1e300, -2.0 ** 970], [1e308, 2.0 ** 1023], 5000))
    return out


@pytest.fixture(scope="module")
def cases():
    T = {name: [_in_domain(b) for b in blocks] for name, blocks in _cases(CAP).items()}
    T["precondition"] = _precondition_edges()
    return T


def run_block(H, block):
    """One block through the harness, asserted; returns (segments of the checked form, of the proven form, hits)."""
    kind, bias, x0, c, thr, n = block
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    st = np.zeros(4, np.int64)
    bad = H.guards_check(C.c_int32(kind), C.c_int32(bias), P(x0, C.c_double), P(c, C.c_double), P(thr, C.c_double),
                         P(n, C.c_int32), C.c_int64(len(x0)), P(st, C.c_int64))
    why = {1: "proven != naive loop", 2: "checked != naive loop", 3: "the two forms take different trips",
           4: "a call outside the proven form's preconditions"}
    assert bad == -1, (f"kind {kind} bias {bias} case {bad}: {why.get(int(st[3]), st[3])}: x0={x0[bad]!r} c={c[bad]!r} "
                       f"thr={thr[bad]!r} n={n[bad]}" if bad >= 0 else f"harness says {bad}")
    return int(st[0]), int(st[1]), int(st[2])


def _total(H, blocks):
    r = np.array([run_block(H, b) for b in blocks])
    return r.sum(axis=0)


@pytest.mark.parametrize("name", ["random", "ties", "pow2", "edges", "general", "budgets", "bias"])
def test_proven_checked_and_naive_agree(H, cases, name):
    """Simulator shapes, ties, exact thresholds r == 0 and r == dm, landings on powers of two, subnormals and 1e300,
    spoiled estimates: the same value, count and hit flag three ways, the same trips two ways."""
    seg_c, seg_p, hits = _total(H, cases[name])
    assert seg_c == seg_p > 0 and hits > 0


def test_edges_of_the_precondition(H, cases):
    seg_c, seg_p, hits = _total(H, cases["precondition"])
    assert 0 < seg_p <= seg_c and hits > 0


def test_a_zero_constant_takes_one_segment_per_budget(H):
    """An outage must stay one trip per interval, not one per tick: from a value in the normal range a zero constant jumps
    the whole budget in both forms (from zero or a subnormal value neither form jumps: a segment per tick)."""
    for kind, c, thr in ((GE, 0.0, 1e301), (LE, -0.0, -1.0), (LT, -0.0, -1.0)):
        x0 = np.array([1.5, 3.7, 1.5 * 2.0 ** -960, 1e300])      # (not on a binade's bottom: going down nothing jumps from there)
        seg_c, seg_p, hits = run_block(H, _block(kind, 0, x0, c, thr, CAP))
        assert (seg_c, seg_p, hits) == (len(x0), len(x0), 0)
    seg_c, seg_p, _ = run_block(H, _block(GE, 0, [0.0, 1e-310], 0.0, 1e9, 100))
    assert seg_c == seg_p == 200


def test_the_harness_refuses_cases_outside_the_domain(H):
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    st = np.zeros(4, np.int64)
    one = np.ones(1)
    for n, x in ((0, 1.0), (CAP + 1, 1.0), (5, np.inf), (5, np.nan)):
        assert H.guards_check(C.c_int32(GE), C.c_int32(0), P(np.array([x]), C.c_double), P(one, C.c_double), P(one, C.c_double),
                              P(np.array([n], np.int32), C.c_int32), C.c_int64(1), P(st, C.c_int64)) == -3


# ---------------------------------------------------------------------------------------------------------------------
# the lane functions

def run_lanes(H, meta, traces, trace_id, offset, actions, max_ticks=0):
    """Episodes on the tables the host would pick for this configuration; returns (rec, bw, fin, n_play, proven?, stats)."""
    from oracle.oracle import pack_traces
    ladder = np.asarray(meta["ladder"], np.float64)
    V = meta["video_length"]
    if not max_ticks:
        max_ticks = int(32 * V * np.ceil(meta["chunk_length"] / 0.01))
    h = H.cg_create(C.c_double(meta["interval"]), C.c_double(meta["chunk_length"]), C.c_double(meta.get("speed", 1.0)),
                    C.c_int32(V), C.c_double(meta["max_buffer"]), C.c_double(meta["start_up_length"]), C.c_int32(max_ticks),
                    ladder.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(len(ladder)))
    flat, off, lens = pack_traces(traces)
    trace_id = np.ascontiguousarray(trace_id, np.int32); offset = np.ascontiguousarray(offset, np.int32)
    actions = np.ascontiguousarray(actions, np.int32)
    N = actions.shape[0]
    rec = np.zeros((N, V, 8)); bw = np.zeros((N, V)); fin = np.zeros((N, 6)); fin_i = np.zeros((N, 2), np.int32)
    st = np.zeros(4, np.int64)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    proven = bool(H.cg_proven(C.c_void_p(h)))
    rc = H.cg_batch(C.c_void_p(h), P(flat, C.c_double), P(off, C.c_int64), P(lens, C.c_int32), P(trace_id, C.c_int32),
                    P(offset, C.c_int32), P(actions, C.c_int32), C.c_int32(N), P(rec, C.c_double), P(bw, C.c_double),
                    P(fin, C.c_double), P(fin_i, C.c_int32), P(st, C.c_int64))
    H.cg_destroy(C.c_void_p(h))
    assert rc == 0, rc
    return rec, bw, fin, fin_i[:, 0], proven, [int(v) for v in st]


def _oracle_cfg(oracle, meta):
    return oracle.env_cfg(meta["ladder"], meta["chunk_length"], meta["video_length"], meta["max_buffer"],
                          meta["start_up_length"], meta["interval"], meta["weights"], meta["speed"])


@pytest.mark.parametrize("case", CASES)
def test_seeded_configurations_keep_the_preconditions(H, oracle, case):
    meta, traces, trace_id, offset, actions = _case(**dict(case, N=min(case["N"], 600)))
    steps, bwo, fino, _ = oracle.env_batch(_oracle_cfg(oracle, meta), traces, trace_id, offset, actions)
    rec, bw, fin, _, proven, st = run_lanes(H, meta, traces, trace_id, offset, actions)
    _check(rec, bw, fin, steps, bwo, fino)
    assert proven and st[0] > 1000 and st[1] == 0, st           # the proven form really ran, never outside its domain
    assert st[2] == st[3]                                       # ... and took the checked form's trips


@pytest.mark.parametrize("seed", range(20))
def test_random_configurations_keep_the_preconditions(H, oracle, seed):
    rng = np.random.default_rng(1000 + seed)
    meta, (lo, hi) = _random_config(rng)
    n_traces, N = 6, 200
    lens = rng.integers(40, 3000, n_traces)
    traces = [rng.uniform(lo, hi, l).astype(np.float32).astype(np.float64) for l in lens]
    trace_id = rng.integers(0, n_traces, N).astype(np.int32)
    offset = np.array([rng.integers(0, lens[t]) for t in trace_id], np.int32)
    actions = rng.integers(0, len(meta["ladder"]), (N, meta["video_length"])).astype(np.int32)
    steps, bwo, fino, _ = oracle.env_batch(_oracle_cfg(oracle, meta), traces, trace_id, offset, actions, max_ticks=4_000_000)
    mt = int(fino["ticks"].max()) + 1000
    rec, bw, fin, _, proven, st = run_lanes(H, meta, traces, trace_id, offset, actions, max_ticks=mt)
    _check(rec, bw, fin, steps, bwo, fino)
    assert proven == (mt <= CAP)
    if proven:
        assert st[0] > 0 and st[1] == 0 and st[2] == st[3], st


@pytest.mark.parametrize("family", ["outage", "tiny", "burst", "short", "extreme"])
def test_trace_families_keep_the_preconditions(H, oracle, family):
    """Zeros, samples that add less than an ulp, samples that finish a chunk on its first tick, subnormals and 1e300, traces
    of one to seven samples: through the proven chains, against the oracle."""
    import trace_families as F
    rng = np.random.default_rng([5, F.OPEN_LOOP_FAMILIES.index(family)])
    meta = dict(ladder=[0.3, 1.2, 4.3], chunk_length=2.0, video_length=5, max_buffer=6.0, start_up_length=2.0, interval=0.5,
                weights=[4.3, 1, 1, 0.1], speed=1.0)
    traces = F.make_pool(family, rng, rng.integers(8, 200, 5))
    N = 130
    tl = np.array([len(t) for t in traces])
    trace_id = rng.integers(0, 5, N).astype(np.int32)
    offset = (rng.integers(0, 1 << 20, N) % tl[trace_id]).astype(np.int32)
    actions = rng.integers(0, 3, (N, 5)).astype(np.int32)
    steps, bwo, fino, _ = oracle.env_batch(_oracle_cfg(oracle, meta), traces, trace_id, offset, actions, max_ticks=4_000_000)
    mt = int(fino["ticks"].max()) + 1000
    assert mt <= CAP
    rec, bw, fin, _, proven, st = run_lanes(H, meta, traces, trace_id, offset, actions, max_ticks=mt)
    _check(rec, bw, fin, steps, bwo, fino)
    assert proven and st[0] > 0 and st[1] == 0 and st[2] == st[3], st


# ---------------------------------------------------------------------------------------------------------------------
# the routing predicate

ROUTED = [
    ("interval below one tick", dict(interval=0.004), 0),
    ("interval of 0.013 s: spans of one and two ticks", dict(interval=0.013), 0),
    ("intervals of 2^20 ticks and more", dict(interval=10486.0, bw=(3.0, 6.0)), 1_200_000),
    ("max_ticks one above 2^20", dict(), CAP + 1),
]


@pytest.mark.parametrize("what,over,max_ticks", ROUTED, ids=[r[0] for r in ROUTED])
def test_a_handle_that_fails_the_proof_runs_the_general_tables(H, oracle, what, over, max_ticks):
    meta, traces, trace_id, offset, actions = _case(seed=61, N=150, V=6, n_traces=4, **over)
    steps, bwo, fino, _ = oracle.env_batch(_oracle_cfg(oracle, meta), traces, trace_id, offset, actions)
    rec, bw, fin, _, proven, st = run_lanes(H, meta, traces, trace_id, offset, actions, max_ticks=max_ticks)
    expect = what.startswith("interval of 0.013")               # every span is at least one tick: the proof holds
    assert proven == expect, what
    assert (st[0] > 0) == expect and st[1] == 0                 # the proven form ran only where the proof holds
    _check(rec, bw, fin, steps, bwo, fino)


def test_the_proof_on_its_own(H):
    ladder = np.array([0.3, 4.3])

    def proven(interval=1.0, L=4.0, speed=1.0, max_buffer=20.0, mt=100_000, ladder=ladder):
        h = H.cg_create(C.c_double(interval), C.c_double(L), C.c_double(speed), C.c_int32(4), C.c_double(max_buffer),
                        C.c_double(4.0), C.c_int32(mt), ladder.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(len(ladder)))
        r = bool(H.cg_proven(C.c_void_p(h)))
        H.cg_destroy(C.c_void_p(h))
        return r

    assert proven() and proven(mt=CAP) and proven(interval=0.02) and proven(interval=0.05)
    assert not proven(mt=CAP + 1)
    assert not proven(interval=0.0099) and not proven(interval=0.001)
    assert not proven(max_buffer=np.inf) and not proven(max_buffer=1e300)
    assert not proven(speed=1e295) and not proven(speed=np.nan)
    assert not proven(ladder=np.array([0.3, 1e300])) and not proven(ladder=np.array([np.inf, 1.0]))


def test_sanitized_program(cases, tmp_path):
    """The chain cases, and a built-in replay of episodes on traces with zeros, subnormals and 1e300, through a stand-alone
    build of the harness with AddressSanitizer and UndefinedBehaviorSanitizer.  The runtimes are linked statically."""
    src = os.path.join(_ROOT, "tests", "native", "chain_guards_harness.cpp")
    exe, data = str(tmp_path / "chain_guards_san"), str(tmp_path / "cases.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-DCHAIN_GUARDS_MAIN", "-I", os.path.join(_ROOT, "abrsimulator_amd", "csrc"),
                           src, "-o", exe])
    blocks = [b for name in sorted(cases) for b in cases[name]]
    with open(data, "wb") as f:
        np.array([len(blocks)], np.int64).tofile(f)
        for kind, bias, x0, c, thr, n in blocks:
            np.array([kind, bias, 0, 0], np.int32).tofile(f)
            np.array([len(x0)], np.int64).tofile(f)
            for a in (x0, c, thr, n):
                a.tofile(f)
    r = subprocess.run([exe, data], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout.split()
    assert out[:2] == ["ok", str(sum(len(b[2]) for b in blocks))] and int(out[2]) > 1000, r.stdout[-3000:]
