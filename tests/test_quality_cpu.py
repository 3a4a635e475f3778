"""The quality model without a GPU (include/abr_env.h: abr_episode_quality): the struct against the C compiler's view; the
layout arithmetic of the library (abr_env_quality_bytes), of the kernels' header compiled for the host and of the Python
wrapper against an independent numpy twin; the kernels' per-step and per-episode rules (csrc/abr_lane_jump.h:
quality_step, quality_close, quality_reset) against the twin byte for byte; the built-in utility tables against math.log
bit for bit; EpisodeQuality's views and reductions on a CPU blob written by the twin; the refusals that need no device."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import c_abi_output, native_harness
from ledger_twin import TwinLedger
from quality_twin import TwinQuality, layout

P_ = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
W = (4.3, 1.0, 1.0, 0.1)
LADDER = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]


@pytest.fixture(scope="module")
def QH():
    return native_harness("quality_harness")


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


SIZES = [(n, r) for n in (1, 2, 31, 32, 33, 63, 64, 65, 200, 256, 257, 65536, 1048576) for r in (1, 2, 3, 8, 17)]


def test_struct_layout_matches_header(L, QH):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(abr_episode_quality), offsetof(abr_episode_quality, wq),
         offsetof(abr_episode_quality, u_dev), offsetof(abr_episode_quality, base_dev), offsetof(abr_episode_quality, rows),
         offsetof(abr_episode_quality, reserved_), ABR_ABI_VERSION);
  return 0;
}'''
    got = list(map(int, c_abi_output(prog)[0].split()))
    S = L.EpisodeQuality
    assert got[:6] == [C.sizeof(S), S.wq.offset, S.u_dev.offset, S.base_dev.offset, S.rows.offset, S.reserved_.offset]
    assert got[:6] == [32, 0, 8, 16, 24, 28]
    assert got[6] == 4 == L.ABI_VERSION                       # additive: the ABI version stays
    assert QH.qh_quality_size() == 32


def test_symbols_exported(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "abr_env.h")).read()
    for sym in ("abr_env_quality_bytes", "abr_env_set_episode_quality", "abr_env_episode_quality"):
        assert hasattr(lib, sym) and sym in {n for n, _, _ in L.SYMBOLS}
        assert sym + "(" in header
    import abrsimulator_amd as A
    assert A.EpisodeQuality is __import__("abrsimulator_amd.quality", fromlist=["x"]).EpisodeQuality


def test_quality_bytes_equals_the_twin_and_needs_no_gpu(L, QH):
    from abrsimulator_amd.quality import quality_layout
    lib = L.lib()
    for n, r in SIZES:
        want = layout(n, r)
        b = C.c_size_t()
        assert lib.abr_env_quality_bytes(n, r, C.byref(b)) == 0
        assert b.value == want[5], (n, r)
        out = np.zeros(6, np.uint64)
        QH.qh_layout(C.c_int64(n), C.c_int32(r), P_(out, C.c_uint64))
        assert out.tolist() == list(want), (n, r)
        lo = quality_layout(n, r)
        assert [lo[k] for k in ("count", "q_run", "q_last", "total_q", "rec_q", "bytes")] == list(want), (n, r)
        assert all(o % 256 == 0 for o in want)
    n, r = 65, 3                                              # the regions do not overlap and hold what the contract says
    o = layout(n, r)
    assert o[1] >= 4 * n and all(o[k + 1] - o[k] >= 8 * n for k in (1, 2, 3)) and o[5] - o[4] >= 8 * n * r
    b = C.c_size_t(7)
    assert lib.abr_env_quality_bytes(64, 0, C.byref(b)) == -1 and b"rows" in lib.abr_last_error()
    assert lib.abr_env_quality_bytes(0, 1, C.byref(b)) == -1 and b"n_lanes" in lib.abr_last_error()
    assert lib.abr_env_quality_bytes(64, 1, None) == -1
    assert b.value == 7                                       # nothing written on a refusal


def test_refusals_that_need_no_device(L):
    lib = L.lib()
    buf = (C.c_uint8 * 1024)()
    base = (C.addressof(buf) + 255) // 256 * 256
    tab = (C.c_double * 8)()
    u = C.addressof(tab)
    Q = L.EpisodeQuality
    ok = dict(wq=1.0, u_dev=u, base_dev=base, rows=2, reserved_=0)
    for change, word in ((dict(wq=float("nan")), b"finite"), (dict(wq=float("inf")), b"finite"),
                         (dict(wq=float("-inf")), b"finite"), (dict(u_dev=None), b"u_dev is NULL"),
                         (dict(u_dev=u + 4), b"8-byte"), (dict(base_dev=None), b"base_dev is NULL"),
                         (dict(base_dev=base + 8), b"256-byte"), (dict(rows=0), b"rows"), (dict(rows=-3), b"rows")):
        s = Q(**{**ok, **change})
        # the struct is checked before the handle: a refusal stores nothing
        assert lib.abr_env_set_episode_quality(None, C.byref(s)) == -1 and word in lib.abr_last_error(), change
    assert lib.abr_env_set_episode_quality(None, C.byref(Q(**ok))) == -1 and b"env is NULL" in lib.abr_last_error()
    assert lib.abr_env_set_episode_quality(None, None) == -1 and b"env is NULL" in lib.abr_last_error()
    assert lib.abr_env_episode_quality(None, None, None) == -1


# ---- the host build of the kernels' helpers against the twin, byte for byte ----
def events(rng, n, rows, V, M, per_lane):
    """Seeded events in launch order: every lane plays per_lane episodes of V steps, interleaved across lanes.  A step is
    a completed download (kind 0) or, now and then, one without (kind 1: the chunk is tried again); an episode ends with
    a re-arm (3) or -- the lane's last -- without one (2); now and then a lane is reset in mid-episode (4) and starts its
    episode again.  Returns the arrays quality_harness.cpp: qh_run takes."""
    kind, lane, chunk, action, rew = [], [], [], [], []
    state = [[0, 0] for _ in range(n)]                        # [episodes closed, chunk]
    alive = [i for i in range(n)]
    while alive:
        i = alive[int(rng.integers(0, len(alive)))]
        ep, c = state[i]
        x = rng.random()
        if x < 0.08:
            k = 1                                             # a step without a completed download
        elif x < 0.12 and c > 0:
            k = 4                                             # a reset in mid-episode
        else:
            k = 0
        kind.append(k); lane.append(i); chunk.append(c); action.append(int(rng.integers(0, M)))
        rew.append(float(rng.choice([0.0, -0.0, 0.45, 4.3 * 0.37, 17.2, 1e-9, 1e9])))
        if k == 0:
            c += 1
        elif k == 4:
            c = 0
        if c >= V:
            ep += 1
            last = ep >= per_lane
            kind.append(2 if last else 3); lane.append(i); chunk.append(0); action.append(0); rew.append(0.0)
            c = 0
            if last:
                alive.remove(i)
        state[i] = [ep, c]
    return (np.array(kind, np.int32), np.array(lane, np.int64), np.array(chunk, np.int32), np.array(action, np.int32),
            np.array(rew, np.float64))


def run_native(QH, n, rows, M, wq, u, ev):
    kind, lane, chunk, action, rew = ev
    blob = np.zeros(layout(n, rows)[5], np.uint8)
    out = rew.copy()
    QH.qh_run(blob.ctypes.data_as(C.c_void_p), C.c_int64(n), C.c_int32(rows), C.c_int32(M), C.c_double(wq),
              P_(u, C.c_double), C.c_int64(kind.size), P_(kind, C.c_int32), P_(lane, C.c_int64), P_(chunk, C.c_int32),
              P_(action, C.c_int32), out.ctypes.data_as(C.POINTER(C.c_double)))
    return blob, out


def run_twin(n, rows, wq, u, ev):
    kind, lane, chunk, action, rew = ev
    t = TwinQuality(n, rows, wq, u)
    out = rew.copy()
    for e in range(kind.size):
        k, i = int(kind[e]), int(lane[e])
        if k == 0:
            out[e] = t.step(i, int(chunk[e]), int(action[e]), rew[e])
        elif k in (2, 3):
            t.close(i, k == 3)
        elif k == 4:
            m = np.zeros(n, bool)
            m[i] = True
            t.reset(m)
    return t, out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("rows", [1, 2, 8])
def test_native_rules_equal_the_twin_byte_for_byte(QH, n, rows):
    V, M = 5, 3
    rng = np.random.default_rng(1000 * n + rows)
    u = rng.uniform(-2.0, 5.0, (V, M))
    u[rng.integers(0, V), rng.integers(0, M)] = 1e-12           # a small entry next to big sums
    for per_lane in sorted({max(1, rows - 1), rows, rows + 1, 2 * rows + 1}):     # fewer, as many, more episodes than rows
        ev = events(rng, n, rows, V, M, per_lane)
        if n >= 63:                                           # non-vacuity: every kind of step and both kinds of end occur
            assert {0, 1, 2, 4}.issubset(set(ev[0].tolist())) and (per_lane == 1 or 3 in ev[0])
        wq = float(rng.choice([1.0, 0.37, -2.5]))
        blob, rew = run_native(QH, n, rows, M, wq, u, ev)
        t, want = run_twin(n, rows, wq, u, ev)
        assert blob.tobytes() == t.blob.tobytes(), (n, rows, per_lane)
        assert rew.tobytes() == want.tobytes(), (n, rows, per_lane)
        assert (t.count == per_lane).all()
        # a step without a completed download reports the reward it had, and the last episode left its sum in q_run
        assert np.array_equal(rew[ev[0] == 1], ev[4][ev[0] == 1])
        assert np.array_equal(t.q_run, t.q_last)


def test_a_reset_in_mid_episode_zeroes_the_running_sum_only(QH):
    u = np.array([[1.0, 2.0], [4.0, 8.0]])
    kind = np.array([0, 0, 3, 0, 4, 0, 0, 2], np.int32)
    lane = np.zeros(8, np.int64)
    chunk = np.array([0, 1, 0, 0, 0, 0, 1, 0], np.int32)
    action = np.array([1, 1, 0, 1, 0, 0, 0, 0], np.int32)
    ev = (kind, lane, chunk, action, np.full(8, 10.0))
    blob, rew = run_native(QH, 1, 2, 2, 0.5, u, ev)
    t = TwinQuality(1, 2, 0.5, u)
    t.blob[:] = blob
    # episode 0: 2 + 8; then 2 abandoned by the reset; episode 1: 1 + 4
    assert t.count[0] == 2 and t.rec_q[:, 0].tolist() == [10.0, 5.0] and t.total_q[0] == 15.0 and t.q_last[0] == 5.0
    assert t.q_run[0] == 5.0                                  # no re-arm at the end: the sum stays until a reset
    assert rew.tolist() == [9.0, 6.0, 10.0, 9.0, 10.0, 9.5, 8.0, 10.0]


def test_sums_are_added_in_order_and_the_reward_is_one_multiply_one_subtract(QH):
    """1e16 + 1 + 1 in order is 1e16 (each 1 is absorbed); rew - wq * q rounds the product before the subtraction."""
    u = np.array([[1e16, 1.0, 1.0 + 2.0 ** -30]])
    kind = np.array([0, 0, 0, 2, 0], np.int32)
    ev = (kind, np.zeros(5, np.int64), np.zeros(5, np.int32), np.array([0, 1, 1, 0, 2], np.int32),
          np.array([0.0, 0.0, 0.0, 0.0, 1.0 + 2.0 ** -29]))
    wq = 1.0 + 2.0 ** -30
    blob, rew = run_native(QH, 1, 1, 3, wq, u, ev)
    t = TwinQuality(1, 1, wq, u)
    t.blob[:] = blob
    assert t.q_last[0] == 1e16 and (1.0 + 1.0) + 1e16 != 1e16
    prod = np.float64(wq) * np.float64(u[0, 2])               # (1 + 2^-30)^2 = 1 + 2^-29 + 2^-60 rounds to 1 + 2^-29
    assert prod == 1.0 + 2.0 ** -29 and rew[4] == 0.0         # a fused multiply-subtract would leave -2^-60


# ---- the built-in tables ----
def test_utility_tables_equal_math_log_bit_for_bit():
    from abrsimulator_amd.quality import utility_table
    V = 5
    rng = np.random.default_rng(3)
    per_chunk = np.sort(rng.uniform(0.2, 9.0, (V, 6)), axis=1)
    for br in (np.array(LADDER), per_chunk):
        tab = np.broadcast_to(br, (V, 6)) if br.ndim == 1 else br
        ident = utility_table("identity", br, V)
        assert ident.dtype == np.float64 and ident.shape == (V, 6) and ident.tobytes() == np.ascontiguousarray(tab).tobytes()
        for name, ref in (("log", 0), ("log_top", -1)):
            got = utility_table(name, br, V)
            assert got.dtype == np.float64 and got.shape == (V, 6) and got.flags.c_contiguous
            for c in range(V):
                for m in range(6):
                    want = math.log(float(tab[c, m]) / float(tab[c, ref]))
                    assert got[c, m] == want and math.copysign(1, got[c, m]) == math.copysign(1, want), (name, c, m)
        assert (utility_table("log", br, V)[:, 0] == 0).all() and (utility_table("log", br, V)[:, 1:] > 0).all()
        assert (utility_table("log_top", br, V)[:, -1] == 0).all() and (utility_table("log_top", br, V)[:, :-1] < 0).all()
    own = rng.normal(size=(V, 6))
    assert utility_table(own, LADDER, V).tobytes() == own.tobytes()
    with pytest.raises(ValueError):
        utility_table("sqrt", LADDER, V)
    with pytest.raises(ValueError):
        utility_table(own[:, :5], LADDER, V)
    with pytest.raises(ValueError):
        utility_table("log", per_chunk[:4], V)


# ---- EpisodeQuality on CPU tensors ----
def joined(n, rows, lanes, rng, wq=0.7, rows_led=None):
    """A ledger blob and a quality blob written by their twins from the same episode ends."""
    from abrsimulator_amd.ledger import EpisodeLedger
    from abrsimulator_amd.quality import EpisodeQuality
    u = np.array([[1.0]])
    tq, tl = TwinQuality(n, rows, wq, u), TwinLedger(n, rows_led or rows)
    ep = {}
    ev = []
    for i in lanes:
        f = (rng.uniform(0, 30), rng.uniform(0, 5), rng.uniform(0, 40), float(rng.choice([0.0, 0.45, 13.25])))
        q = float(rng.uniform(0, 40)) * (1e-9 if rng.random() < 0.1 else 1.0)
        ep[i] = ep.get(i, -1) + 1
        w = (ep[i], int(rng.integers(0, 7)), int(rng.integers(0, 300)), 5, 1)
        tl.append(int(i), W, *f, w)
        tq.q_run[i] = q
        tq.close(int(i), True)
        qoe = ((W[0] * f[0] + W[1] * f[3]) + W[2] * f[1]) + W[3] * f[2]
        ev.append((int(i), w[0], w[1], qoe, q))
    led = EpisodeLedger(n, rows_led or rows, "cpu")
    led.blob.copy_(torch.from_numpy(tl.blob))
    ql = EpisodeQuality(n, rows, wq, u, "cpu")
    ql.blob.copy_(torch.from_numpy(tq.blob))
    return ql, led, tq, ev


def test_views_and_joined_records_after_a_wrap():
    n, rows = 65, 3
    rng = np.random.default_rng(5)
    # lane 0: no record; lane 1: one; lane 2: exactly rows; lane 3: rows + 2 (wrapped); the rest random
    lanes = rng.permutation(np.concatenate([[1], [2] * rows, [3] * (rows + 2), rng.integers(4, n, 300)]))
    ql, led, tq, ev = joined(n, rows, lanes, rng)
    assert np.array_equal(ql.count().numpy(), tq.count) and ql.count().dtype == torch.int32
    assert np.array_equal(ql.last().numpy(), tq.q_last) and np.array_equal(ql.totals().numpy(), tq.total_q)
    assert np.array_equal(ql.running().numpy(), tq.q_run)
    assert ql.ring().shape == (rows, n) and np.array_equal(ql.ring().numpy(), tq.rec_q)
    assert ql.count().data_ptr() == ql.blob.data_ptr()        # the views alias the blob
    want = []
    for i in range(n):
        want += [e for e in ev if e[0] == i][-rows:]
    rec = ql.records(led)
    assert list(rec)[-2:] == ["quality", "qoe_q"] and list(rec)[:-2] == list(led.records())
    assert rec["lane"].numel() == len(want) == int(np.minimum(tq.count, rows).sum())
    assert rec["lane"].tolist() == [e[0] for e in want] and rec["episode"].tolist() == [e[1] for e in want]
    assert rec["trace_id"].tolist() == [e[2] for e in want]
    assert rec["qoe"].tolist() == [e[3] for e in want] and rec["quality"].tolist() == [e[4] for e in want]
    assert rec["qoe_q"].tolist() == [e[3] - 0.7 * e[4] for e in want]
    alone = ql.records()
    assert list(alone) == ["lane", "quality"] and torch.equal(alone["quality"], rec["quality"])
    assert torch.equal(alone["lane"], rec["lane"])
    lanes_seen = rec["lane"].numpy()
    assert 0 not in lanes_seen and (lanes_seen == 1).sum() == 1 and (lanes_seen == 3).sum() == rows
    # clear() empties it; state_dict round trip; another shape, weight or table is refused
    from abrsimulator_amd.quality import EpisodeQuality
    sd = ql.state_dict()
    ql.clear()
    assert not ql.blob.any() and ql.records()["lane"].numel() == 0
    ql.load_state_dict(sd)
    assert ql.blob.numpy().tobytes() == tq.blob.tobytes()
    for other in (EpisodeQuality(n, rows + 1, 0.7, [[1.0]]), EpisodeQuality(n, rows, 0.8, [[1.0]]),
                  EpisodeQuality(n, rows, 0.7, [[2.0]])):
        with pytest.raises(ValueError):
            other.load_state_dict(sd)
    for bad in (lambda: EpisodeQuality(0, 1, 1.0, [[1.0]]), lambda: EpisodeQuality(4, 0, 1.0, [[1.0]]),
                lambda: EpisodeQuality(4, 1, float("nan"), [[1.0]]), lambda: EpisodeQuality(4, 1, 1.0, [1.0])):
        with pytest.raises(ValueError):
            bad()


def test_rows_or_count_mismatch_is_an_error():
    rng = np.random.default_rng(6)
    lanes = rng.integers(0, 8, 40)
    ql, led, _, _ = joined(8, 3, lanes, rng, rows_led=4)
    with pytest.raises(ValueError, match="rows"):
        ql.records(led)
    with pytest.raises(ValueError, match="rows"):
        ql.per_member(4, 2, led)
    ql, led, _, _ = joined(8, 3, lanes, rng)
    ql.records(led)
    led.count()[2] += 1
    for call in (lambda: ql.records(led), lambda: ql.per_trace(7, led), lambda: ql.per_member(4, 2, led)):
        with pytest.raises(ValueError, match="counts"):
            call()


def sum_bound(x):
    """The error of a float64 sum of x's terms in any order (ledger.py: per_trace), plus the two roundings of a mean's
    division and of the multiplication that undoes it."""
    u, m = 2.0 ** -53, len(x)
    return m * u * math.fsum(np.abs(x)) / (1 - m * u) + 2 * u * abs(math.fsum(x))


def test_per_trace_and_per_member_against_numpy():
    n, rows, n_traces, wq = 200, 8, 9, 0.7
    rng = np.random.default_rng(11)
    lanes = rng.integers(0, n, 1500)
    ql, led, tq, ev = joined(n, rows, lanes, rng, wq)
    rec = {k: v.numpy() for k, v in ql.records(led).items()}
    pt = ql.per_trace(n_traces, led)
    assert pt["count"].tolist() == [int((rec["trace_id"] == k).sum()) for k in range(n_traces)]
    base = led.per_trace(n_traces)
    for k in base:
        assert torch.equal(torch.nan_to_num(pt[k].double(), nan=-1.0), torch.nan_to_num(base[k].double(), nan=-1.0)), k
    for k in ("quality", "qoe_q"):
        assert math.isnan(float(pt[k][7])) and math.isnan(float(pt[k][8]))
        for tr in range(7):
            x = rec[k][rec["trace_id"] == tr]
            assert abs(float(pt[k][tr]) * x.size - math.fsum(x)) <= sum_bound(x), (k, tr)
    # per_member: from the totals, so every episode counts, also the ones the ring has dropped
    group, P = 64, 4                                          # 200 lanes: three full groups and a partial one
    pm = ql.per_member(group, P, led)
    basem = led.per_member(group, P)
    for k in basem:
        assert torch.equal(pm[k], basem[k]), k
    ev = np.array([(e[0], e[3], e[4]) for e in ev])
    assert (tq.count > rows).any()
    for m in range(P):
        sel = (ev[:, 0] // group) == m
        q, qoe = ev[sel, 2], ev[sel, 1]
        cnt = int(sel.sum())
        assert int(pm["count"][m]) == cnt
        assert abs(float(pm["quality"][m]) * cnt - math.fsum(q)) <= sum_bound(q), m
        # qoe_q = mean qoe - wq * mean quality: each mean within its bound, then one multiply and one subtract
        got, want = float(pm["qoe_q"][m]), (math.fsum(qoe) - wq * math.fsum(q)) / cnt
        tol = (sum_bound(qoe) + wq * sum_bound(q)) / cnt + 4 * 2.0 ** -53 * (abs(math.fsum(qoe)) + wq * abs(math.fsum(q))) / cnt
        assert abs(got - want) <= tol, (m, got, want, tol)
    with pytest.raises(ValueError):
        ql.per_member(64, 3, led)
