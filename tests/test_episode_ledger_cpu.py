"""The episode ledger without a GPU: the layout arithmetic of the library (abr_env_ledger_bytes), of the kernels' header
compiled for the host and of the Python wrapper against an independent numpy twin of include/abr_env.h's contract; the
kernels' append (csrc/abr_lane_jump.h: ledger_append) against the twin byte for byte; EpisodeLedger's views and
reductions on a CPU blob written by the twin; the struct against the header; the refusals that need no device."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import c_abi_output, native_harness
from ledger_twin import FLOATS, INTS, TwinLedger, layout

P_ = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
W = (4.3, 1.0, 1.0, 0.1)


@pytest.fixture(scope="module")
def LH():
    return native_harness("ledger_harness")


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


SIZES = [(n, r) for n in (1, 2, 63, 64, 65, 100, 200, 255, 256, 257, 1000, 65536, 1048576) for r in (1, 2, 3, 8, 17)]


def test_ledger_bytes_equals_the_twin_and_needs_no_gpu(L, LH):
    from abrsimulator_amd.ledger import ledger_layout
    lib = L.lib()
    for n, r in SIZES:
        want = layout(n, r)
        b = C.c_size_t()
        assert lib.abr_env_ledger_bytes(n, r, C.byref(b)) == 0
        assert b.value == want[4], (n, r)
        out = np.zeros(5, np.uint64)
        LH.lh_layout(C.c_int64(n), C.c_int32(r), P_(out, C.c_uint64))
        assert out.tolist() == list(want), (n, r)
        lo = ledger_layout(n, r)
        assert [lo[k] for k in ("count", "total", "rec_f64", "rec_i32", "bytes")] == list(want), (n, r)
        assert all(o % 256 == 0 for o in want)
    # the regions do not overlap and hold what the contract says
    n, r = 65, 3
    o = layout(n, r)
    assert o[1] >= 4 * n and o[2] - o[1] >= 40 * n and o[3] - o[2] >= 40 * n * r and o[4] - o[3] >= 20 * n * r


def test_struct_layout_matches_header(L, LH):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %d\n", sizeof(abr_episode_ledger), offsetof(abr_episode_ledger, base_dev),
         offsetof(abr_episode_ledger, rows), offsetof(abr_episode_ledger, reserved_), ABR_ABI_VERSION);
  return 0;
}'''
    got = list(map(int, c_abi_output(prog)[0].split()))
    S = L.EpisodeLedger
    assert got[:4] == [C.sizeof(S), S.base_dev.offset, S.rows.offset, S.reserved_.offset] == [16, 0, 8, 12]
    assert got[4] == 4 == L.ABI_VERSION
    assert LH.lh_ledger_size() == 16


def test_symbols_exported(L):
    lib = L.lib()
    for sym in ("abr_env_ledger_bytes", "abr_env_set_episode_ledger"):
        assert hasattr(lib, sym) and sym in {n for n, _, _ in L.SYMBOLS}
        assert sym + "(" in open(os.path.join(ROOT, "include", "abr_env.h")).read()
    import abrsimulator_amd as A
    assert A.EpisodeLedger is __import__("abrsimulator_amd.ledger", fromlist=["x"]).EpisodeLedger


def episode_ends(rng, n_lanes, n_events, lanes=None):
    """Seeded episode ends in launch order: (lane, four float terms, five int fields) per event."""
    lane = rng.integers(0, n_lanes, n_events) if lanes is None else np.asarray(lanes)
    f = np.stack([rng.uniform(0, 30, lane.size), rng.uniform(0, 5, lane.size), rng.uniform(0, 40, lane.size),
                  rng.choice([0.0, 0.45, 1.55, 13.25], lane.size)], 1)
    f[rng.random(lane.size) < 0.1] *= 1e-9                      # small magnitudes next to big totals
    w = np.stack([np.zeros(lane.size, np.int64), rng.integers(0, 7, lane.size), rng.integers(0, 300, lane.size),
                  rng.integers(0, 9, lane.size), rng.choice([1, 2], lane.size)], 1).astype(np.int32)
    seen = {}
    for e, i in enumerate(lane.tolist()):                       # episode numbers grow per lane, with gaps
        seen[i] = seen.get(i, int(rng.integers(0, 3))) + int(rng.integers(1, 3))
        w[e, 0] = seen[i]
    return lane.astype(np.int64), np.ascontiguousarray(f), np.ascontiguousarray(w)


def native_blob(LH, n, rows, lane, f, w, weights=W):
    blob = np.zeros(layout(n, rows)[4], np.uint8)
    LH.lh_append(blob.ctypes.data_as(C.c_void_p), C.c_int64(n), C.c_int32(rows), P_(np.asarray(weights, np.float64), C.c_double),
                 C.c_int64(lane.size), P_(lane, C.c_int64), P_(f, C.c_double), P_(w, C.c_int32))
    return blob


def twin_blob(n, rows, lane, f, w, weights=W):
    t = TwinLedger(n, rows)
    for e in range(lane.size):
        t.append(int(lane[e]), weights, *f[e], w[e])
    return t


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("rows", [1, 2, 8])
def test_native_append_equals_the_twin_byte_for_byte(LH, n, rows):
    rng = np.random.default_rng(1000 * n + rows)
    for per_lane in (max(1, rows - 1), rows, rows + 1, 3 * rows + 2):     # fewer, as many, more episodes than rows
        # every lane gets exactly per_lane ends, interleaved across lanes; then a ragged tail
        lanes = np.concatenate([rng.permutation(np.repeat(np.arange(n), per_lane)), rng.integers(0, n, n // 2)])
        lane, f, w = episode_ends(rng, n, 0, lanes)
        got, want = native_blob(LH, n, rows, lane, f, w), twin_blob(n, rows, lane, f, w)
        assert got.tobytes() == want.blob.tobytes(), (n, rows, per_lane)
        assert want.count.sum() == lane.size and want.count.min() >= per_lane
    # lanes that never end an episode keep all-zero rows
    if n >= 63:
        lane, f, w = episode_ends(rng, n, 0, np.repeat(np.arange(0, n, 2), 3))
        got, want = native_blob(LH, n, rows, lane, f, w), twin_blob(n, rows, lane, f, w)
        assert got.tobytes() == want.blob.tobytes()
        assert (want.count[1::2] == 0).all() and (want.rf[:, :, 1::2] == 0).all()


def test_totals_are_added_in_episode_order(LH):
    """1e16 + 1 + 1 in order is 1e16 (each 1 is absorbed); any other order of the three gives another float64."""
    lane = np.zeros(3, np.int64)
    f = np.array([[1e16, 0, 0, 0], [1.0, 0, 0, 0], [1.0, 0, 0, 0]])
    w = np.zeros((3, 5), np.int32)
    t = TwinLedger(1, 2)
    blob = native_blob(LH, 1, 2, lane, f, w)
    t.blob[:] = blob
    assert t.total[0, 0] == 1e16 and (1.0 + 1.0) + 1e16 != 1e16
    assert t.count[0] == 3 and t.rf[0, 0, 0] == 1.0 and t.rf[1, 0, 0] == 1.0       # slots 0, 1, 0: the ring wrapped


def cpu_ledger(n, rows, lane, f, w):
    from abrsimulator_amd.ledger import EpisodeLedger
    t = twin_blob(n, rows, lane, f, w)
    led = EpisodeLedger(n, rows, "cpu")
    led.blob.copy_(torch.from_numpy(t.blob))
    return led, t


def test_views_and_records_on_a_twin_blob():
    n, rows = 65, 3
    rng = np.random.default_rng(5)
    # lane 0: no record; lane 1: one; lane 2: exactly rows; lane 3: rows + 2 (wrapped); the rest random
    lanes = np.concatenate([[1], [2] * rows, [3] * (rows + 2), rng.integers(4, n, 300)])
    lane, f, w = episode_ends(rng, n, 0, rng.permutation(lanes))
    led, t = cpu_ledger(n, rows, lane, f, w)
    assert np.array_equal(led.count().numpy(), t.count)
    for q, k in enumerate(FLOATS):
        assert np.array_equal(led.totals()[k].numpy(), t.total[q])
        assert led.ring()[k].shape == (rows, n) and np.array_equal(led.ring()[k].numpy(), t.rf[:, q])
    for q, k in enumerate(INTS):
        assert led.ring()[k].dtype == torch.int32 and np.array_equal(led.ring()[k].numpy(), t.ri[:, q])
    # the views alias the blob
    led.count()[5] += 0
    assert led.count().data_ptr() == led.blob.data_ptr()
    # expected records: per lane, the last min(count, rows) events in order
    want = []
    qoe = lambda x: ((W[0] * x[0] + W[1] * x[3]) + W[2] * x[1]) + W[3] * x[2]
    for i in range(n):
        ev = [e for e in range(lane.size) if lane[e] == i][-rows:]
        want += [(i, *w[e], *f[e], qoe(f[e])) for e in ev]
    rec = led.records()
    assert list(rec) == ["lane"] + list(INTS) + list(FLOATS)
    assert rec["lane"].numel() == len(want) == int(np.minimum(t.count, rows).sum())
    got = list(zip(*[rec[k].tolist() for k in rec]))
    assert got == [tuple(float(x) if isinstance(x, (float, np.floating)) else int(x) for x in r) for r in want]
    lanes_seen = rec["lane"].numpy()
    assert 0 not in lanes_seen and (lanes_seen == 1).sum() == 1 and (lanes_seen == 3).sum() == rows
    assert (np.diff(lanes_seen) >= 0).all()
    ep3 = rec["episode"].numpy()[lanes_seen == 3]
    assert (np.diff(ep3) > 0).all() and ep3[-1] == max(w[e, 0] for e in range(lane.size) if lane[e] == 3)
    # clear() empties it; state_dict round trip
    sd = led.state_dict()
    led.clear()
    assert not led.blob.any() and led.records()["lane"].numel() == 0
    led.load_state_dict(sd)
    assert led.blob.numpy().tobytes() == t.blob.tobytes()
    from abrsimulator_amd.ledger import EpisodeLedger
    with pytest.raises(ValueError):
        EpisodeLedger(n, rows + 1).load_state_dict(sd)
    with pytest.raises(ValueError):
        EpisodeLedger(0, 1)
    with pytest.raises(ValueError):
        EpisodeLedger(4, 0)


def test_per_trace_counts_are_exact_and_means_within_the_summation_bound():
    n, rows, n_traces = 200, 8, 9                                   # traces 7 and 8 never occur (ids are drawn below 7)
    rng = np.random.default_rng(11)
    lane, f, w = episode_ends(rng, n, 1500)
    led, t = cpu_ledger(n, rows, lane, f, w)
    rec = {k: v.numpy() for k, v in led.records().items()}
    pt = led.per_trace(n_traces)
    assert pt["count"].dtype == torch.int64 and pt["count"].shape == (n_traces,)
    assert pt["count"].tolist() == [int((rec["trace_id"] == k).sum()) for k in range(n_traces)]
    assert pt["count"][8] == 0 and pt["count"][:7].min() > 0 and pt["count"].sum() == rec["lane"].size
    u = 2.0 ** -53
    for k in FLOATS:
        assert math.isnan(float(pt[k][7])) and math.isnan(float(pt[k][8]))
        for tr in range(7):
            x = rec[k][rec["trace_id"] == tr]
            m = x.size
            # a float64 sum of m terms in ANY order (Higham, Accuracy and Stability, eq. 4.4 with gamma_(m-1) <= gamma_m);
            # the mean's division and the multiplication that undoes it here round once each: 2u relative on top
            bound = m * u * math.fsum(np.abs(x)) / (1 - m * u)
            exact = math.fsum(x)
            got_sum = float(pt[k][tr]) * m
            assert abs(got_sum - exact) <= bound + 2 * u * abs(exact), (k, tr)


def test_refusals_that_need_no_device(L):
    lib = L.lib()
    b = C.c_size_t(7)
    assert lib.abr_env_ledger_bytes(64, 0, C.byref(b)) == -1 and b"rows" in lib.abr_last_error()
    assert lib.abr_env_ledger_bytes(0, 1, C.byref(b)) == -1 and b"n_lanes" in lib.abr_last_error()
    assert lib.abr_env_ledger_bytes(64, 1, None) == -1
    assert b.value == 7                                                            # nothing written on a refusal
    buf = (C.c_uint8 * 1024)()
    base = (C.addressof(buf) + 255) // 256 * 256
    # the struct is checked before the handle
    s = L.EpisodeLedger(base_dev=base, rows=0, reserved_=0)
    assert lib.abr_env_set_episode_ledger(None, C.byref(s)) == -1 and b"rows" in lib.abr_last_error()
    s = L.EpisodeLedger(base_dev=None, rows=2, reserved_=0)
    assert lib.abr_env_set_episode_ledger(None, C.byref(s)) == -1 and b"NULL" in lib.abr_last_error()
    s = L.EpisodeLedger(base_dev=base + 8, rows=2, reserved_=0)
    assert lib.abr_env_set_episode_ledger(None, C.byref(s)) == -1 and b"aligned" in lib.abr_last_error()
    s = L.EpisodeLedger(base_dev=base, rows=2, reserved_=0)
    assert lib.abr_env_set_episode_ledger(None, C.byref(s)) == -1 and b"env is NULL" in lib.abr_last_error()
    assert lib.abr_env_set_episode_ledger(None, None) == -1 and b"env is NULL" in lib.abr_last_error()
