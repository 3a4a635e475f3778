"""The lookahead expert without a GPU (include/abr_env.h: abr_env_lookahead_select): the depth-first walk the kernel compiles
(csrc/abr_lane_jump.h: look_subtree, look_pick) built for the host next to a brute-force loop over flat indices, bit for bit
on action, key and every q; the walk against the C oracle, which is the reference -- every sequence's reward sum with ==,
its latency to the project's 1e-9 contract, and the walk's action by the oracle's own keys; the struct, the symbol, the
refusals that need no device and the launch-splitting arithmetic."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers import c_abi_output, native_harness
import trace_families as TF

P_ = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t)) if a is not None else None
W = (4.3, 1.0, 1.0, 0.1)                                        # wr, wv, ws, wl
LADDER16 = [0.3, 0.5, 0.75, 1.0, 1.2, 1.5, 1.85, 2.3, 2.85, 3.5, 4.3, 5.2, 6.0, 7.0, 8.0, 9.5]
MAX_LEAVES = 65536


def ladder(M):
    return [LADDER16[(16 * k) // M] for k in range(M)]


@pytest.fixture(scope="module")
def LH():
    h = native_harness("lookahead_harness")
    h.la_create.restype = C.c_void_p
    for f in (h.la_leaves, h.la_nodes, h.la_lanes_per_launch, h.la_default_nodes, h.la_max_leaves):
        f.restype = C.c_int64
    return h


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


class Ctx:
    def __init__(self, LH, M, V, max_ticks, chunk_length=4.0, max_buffer=20.0, start_up=8.0, interval=1.0, lad=None):
        self.LH, self.M, self.V = LH, M, V
        self.ladder = lad or ladder(M)
        self.h = C.c_void_p(LH.la_create(C.c_double(interval), C.c_double(chunk_length), C.c_double(1.0), C.c_int32(V),
                                         C.c_double(max_buffer), C.c_double(start_up), C.c_int32(max_ticks),
                                         P_(np.array(self.ladder, np.float64), C.c_double), C.c_int32(M),
                                         P_(np.array(W, np.float64), C.c_double)))
        self._u = None

    def quality(self, wq, u):
        self._u = None if u is None else np.ascontiguousarray(u, np.float64)
        self.LH.la_set_quality(self.h, C.c_double(wq), P_(self._u, C.c_double))

    def run(self, mode, horizon, traces, tid, off, prefix, leaves=False):
        from oracle.oracle import pack_traces
        flat, toff, tlen = pack_traces(traces)
        prefix = np.ascontiguousarray(prefix, np.int32)
        n, n_prefix = prefix.shape
        act, key, q, done = np.zeros(n, np.int32), np.zeros(n), np.zeros((self.M, n)), np.zeros(n, np.uint8)
        S = self.M ** horizon
        lR = np.full((n, S), np.nan) if leaves else None
        ll = np.full((n, S), np.nan) if leaves else None
        lo = np.zeros((n, S), np.uint8) if leaves else None
        rc = self.LH.la_run(self.h, C.c_int32(mode), C.c_int32(horizon), P_(flat, C.c_double), P_(toff, C.c_int64),
                            P_(tlen, C.c_int32), P_(np.asarray(tid, np.int32), C.c_int32), P_(np.asarray(off, np.int32), C.c_int32),
                            P_(prefix, C.c_int32), C.c_int32(n_prefix), C.c_int32(n), P_(act, C.c_int32), P_(key, C.c_double),
                            P_(q, C.c_double), P_(done, C.c_uint8), P_(lR, C.c_double), P_(ll, C.c_double), P_(lo, C.c_uint8))
        assert rc == 0
        return dict(action=act, key=key, q=q, done=done, leaf_R=lR, leaf_lat=ll, leaf_ok=lo)

    def close(self):
        self.LH.la_destroy(self.h)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same(a, b, what):
    assert np.array_equal(a["action"], b["action"]), what
    assert np.array_equal(a["done"], b["done"]), what
    # NaN is one pattern here (both sides write the same quiet NaN); -0.0 and +0.0 are told apart
    assert np.array_equal(bits(a["key"]), bits(b["key"])), what
    assert np.array_equal(bits(a["q"]), bits(b["q"])), what


# ---- the walk against brute force ----
V_DEEP = 11                                                     # after two downloads nine decisions are left: h = 8 is whole


@pytest.mark.parametrize("M", [1, 2, 3, 6, 16])
def test_walk_equals_brute_force(LH, M):
    seen = dict(ties=0, answers=0, shrunk=0, runs=0)
    ctx = Ctx(LH, M, V_DEEP, max_ticks=120_000)
    try:
        for fi, family in enumerate(TF.FAMILIES):
            rng = np.random.default_rng([M, fi, 77])
            traces = TF.make_pool(family, rng, [int(rng.integers(20, 120)) for _ in range(4)])
            for H in range(1, 9):
                leaves = M ** H
                if leaves > MAX_LEAVES:
                    continue
                n = int(max(1, min(8, 20_000 // leaves)))
                for c in (0, 1, 2, V_DEEP - 1):
                    tid = rng.integers(0, len(traces), n).astype(np.int32)
                    off = rng.integers(0, 200, n).astype(np.int32)
                    prefix = rng.integers(0, M, (n, c)).astype(np.int32).reshape(n, c)
                    w = ctx.run(0, H, traces, tid, off, prefix)
                    b = ctx.run(1, H, traces, tid, off, prefix)
                    same(w, b, (family, M, H, c))
                    seen["runs"] += 1
                    seen["answers"] += int((w["action"] >= 0).sum())
                    seen["shrunk"] += int(c == V_DEEP - 1 and H > 1)
                    q = w["q"][:, np.isfinite(w["q"]).all(0)]
                    seen["ties"] += int(((q == q.min(0, keepdims=True)).sum(0) > 1).any()) if M > 1 and q.size else 0
    finally:
        ctx.close()
    assert seen["answers"] > 0 and seen["shrunk"] > 0
    if M > 1:
        assert seen["ties"] > 0                                 # burst: every rate finishes on one tick


def test_walk_equals_brute_force_with_a_quality_model(LH):
    M, H = 3, 3
    ctx = Ctx(LH, M, 6, max_ticks=60_000)
    try:
        rng = np.random.default_rng(5)
        traces = TF.make_pool("outage", rng, [60, 90, 120])
        u = np.tile(np.log(np.array(ctx.ladder) / ctx.ladder[0]), (6, 1)) * rng.uniform(0.5, 1.5, (6, 1))
        n = 32
        tid, off = rng.integers(0, 3, n), rng.integers(0, 60, n)
        prefix = rng.integers(0, M, (n, 2))
        plain = ctx.run(0, H, traces, tid, off, prefix)
        ctx.quality(3.0, u)
        w, b = ctx.run(0, H, traces, tid, off, prefix), ctx.run(1, H, traces, tid, off, prefix)
        same(w, b, "quality")
        assert not np.array_equal(bits(w["key"]), bits(plain["key"]))       # the keys carry the term
        ctx.quality(0.0, None)
        same(ctx.run(0, H, traces, tid, off, prefix), plain, "model removed")
    finally:
        ctx.close()


def test_timeouts_drop_sequences(LH):
    """A dead trace next to a live one; then a max_ticks that times out the high rates only, then every rate."""
    M, H, V = 3, 3, 6
    lad = [0.3, 1.2, 2.85]
    zero, live = np.zeros(40), np.full(40, 1.0)
    prefix = np.zeros((2, 0), np.int32)
    for max_ticks, kind in ((100_000, "dead"), (2_000, "some"), (1_000, "all")):
        ctx = Ctx(LH, M, V, max_ticks=max_ticks, lad=lad)
        try:
            tr = [zero, live if kind != "all" else np.full(40, 0.1)]
            w = ctx.run(0, H, tr, [0, 1], [0, 0], prefix)
            b = ctx.run(1, H, tr, [0, 1], [0, 0], prefix, leaves=True)
            same(w, b, kind)
            # the dead trace: the lane stands at its first call site and no download ever completes
            assert w["done"][0] == 0 and w["action"][0] == -1 and np.isnan(w["key"][0]) and np.isnan(w["q"][:, 0]).all()
            assert b["leaf_ok"][0].sum() == 0
            ok = int(b["leaf_ok"][1].sum())
            if kind == "dead":
                assert ok == M ** H and w["action"][1] >= 0
            elif kind == "some":
                assert 0 < ok < M ** H and w["action"][1] >= 0 and np.isfinite(w["key"][1])
                # three top-rate chunks are 34 s of download at 1.0, three bottom-rate ones 3.6 s; max_ticks is 20 s
                assert b["leaf_ok"][1][M ** H - 1] == 0 and b["leaf_ok"][1][0] == 1
            else:
                assert ok == 0 and w["action"][1] == -1 and np.isnan(w["key"][1])
        finally:
            ctx.close()


# ---- the walk against the C oracle ----
@pytest.mark.parametrize("family", TF.FAMILIES)
def test_walk_against_the_oracle(LH, oracle, family):
    from oracle.oracle import step_rewards
    M, H, V, N = 3, 3, 6, 64
    lad = [0.3, 1.2, 2.85]
    rng = np.random.default_rng([TF.FAMILIES.index(family), 99])
    traces = TF.make_pool(family, rng, [int(rng.integers(30, 200)) for _ in range(8)])
    cfg = oracle.env_cfg(lad, 4.0, V, 20.0, 8.0, 1.0, W, 1.0)
    tid = rng.integers(0, len(traces), N).astype(np.int32)
    off = rng.integers(0, 200, N).astype(np.int32)
    max_ticks = 400_000
    ctx = Ctx(LH, M, V, max_ticks=max_ticks, lad=lad)
    try:
        for c in (0, 2, 4, 5):
            h = min(H, V - c)
            prefix = rng.integers(0, M, (N, c)).astype(np.int32).reshape(N, c)
            seqs = np.array(list(itertools.product(range(M), repeat=h)), np.int32)          # flat index order
            S = len(seqs)
            acts = np.zeros((N, S, V), np.int32)
            acts[:, :, :c] = prefix[:, None, :]
            acts[:, :, c:c + h] = seqs[None]
            flat = acts.reshape(N * S, V)
            steps, _, fin, _ = oracle.env_batch(cfg, traces, np.repeat(tid, S), np.repeat(off, S), flat, threads=8)
            assert int(fin["ticks"].max()) < max_ticks - 1000                               # no time-out on either side
            r32 = step_rewards(steps["rebuffer_time"], steps["start_up_time"], fin["rebuffer_time"], fin["start_up_time"],
                               flat, W, ladder=lad)
            R = np.zeros(N * S)
            for j in range(c, c + h):
                R = R + r32[:, j].astype(np.float64)
            lat = steps["average_latency"][:, c + h] if c + h < V else fin["average_latency"]
            R, lat = R.reshape(N, S), np.asarray(lat, np.float64).reshape(N, S)
            b = ctx.run(1, H, traces, tid, off, prefix, leaves=True)
            w = ctx.run(0, H, traces, tid, off, prefix)
            same(w, b, (family, c))
            assert (b["leaf_ok"][:, :S] == 1).all() and (w["done"] == 0).all()
            assert np.array_equal(b["leaf_R"][:, :S], R), (family, c)                        # every sequence's R part: ==
            got_lat = b["leaf_lat"][:, :S]
            assert (np.abs(got_lat - lat) <= 1e-9 * np.abs(lat)).all(), (family, c)
            key = R + W[3] * lat                                                             # the oracle's own keys
            q = key.reshape(N, M, S // M).min(2)
            tol = 2 * W[3] * 1e-9 * np.abs(lat).max(1)
            pick = q[np.arange(N), w["action"]]
            assert (pick - q.min(1) <= tol).all(), (family, c)
            assert (np.abs(w["key"] - q.min(1)) <= tol).all(), (family, c)
    finally:
        ctx.close()


# ---- the struct, the symbol, the refusals, the splitting ----
def test_struct_matches_the_header(L):
    prog = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "abr_env.h"
    int main(void) {
        printf("%zu %zu %zu %zu %d %d\n", sizeof(abr_lookahead_config), offsetof(abr_lookahead_config, horizon),
               offsetof(abr_lookahead_config, reserved_), offsetof(abr_lookahead_config, max_nodes_per_launch),
               ABR_ABI_VERSION, ABR_MAX_HORIZON);
        return 0;
    }"""
    got = list(map(int, c_abi_output(prog)[0].split()))
    S = L.LookaheadConfig
    assert got[:4] == [C.sizeof(S), S.horizon.offset, S.reserved_.offset, S.max_nodes_per_launch.offset] == [16, 0, 4, 8]
    assert got[4] == 4 == L.ABI_VERSION and got[5] == 8          # additive: the ABI version stays


def test_symbol_declared_exported_and_bound(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "abr_env.h")).read()
    sym = "abr_env_lookahead_select"
    assert hasattr(lib, sym) and sym in {n for n, _, _ in L.SYMBOLS} and sym + "(" in header
    assert lib.abr_abi_version() == 4
    import abrsimulator_amd as A
    assert A.LookaheadExpert is __import__("abrsimulator_amd.expert", fromlist=["x"]).LookaheadExpert
    with pytest.raises(ValueError):
        A.LookaheadExpert(None, horizon=0)
    with pytest.raises(ValueError):
        A.LookaheadExpert(None, horizon=9)
    with pytest.raises(ValueError):
        A.LookaheadExpert(None, horizon=3, max_nodes_per_launch=-1)


def test_refusals_that_need_no_device(L):
    """The documented order: cfg, action_out_dev, horizon, reserved_, max_nodes_per_launch, then the handle."""
    lib = L.lib()
    one = C.c_void_p(256)
    E = lambda: lib.abr_last_error()
    call = lambda cfg, act: lib.abr_env_lookahead_select(None, cfg, act, None, None, None)
    cfg = lambda h=3, r=0, n=0: C.byref(L.LookaheadConfig(h, r, n))
    assert call(None, None) == -1 and b"cfg is NULL" in E()
    assert call(cfg(0, 1, -1), None) == -1 and b"action_out_dev" in E()
    for h in (0, -1, 9):
        assert call(cfg(h, 1, -1), one) == -1 and b"horizon" in E()
    assert call(cfg(3, 1, -1), one) == -1 and b"reserved_" in E()
    assert call(cfg(3, 0, -1), one) == -1 and b"max_nodes_per_launch" in E()
    for h in (1, 8):
        assert call(cfg(h, 0, 0), one) == -1 and b"env is NULL" in E()
    assert call(cfg(3, 0, 2 ** 40), one) == -1 and b"env is NULL" in E()


def test_launch_splitting_arithmetic(LH):
    assert LH.la_default_nodes() == 2 ** 31 and LH.la_max_leaves() == MAX_LEAVES
    for M, h in itertools.product(range(1, 17), range(1, 9)):
        assert LH.la_leaves(M, h) == M ** h
        nodes = sum(M ** j for j in range(1, h + 1))
        assert LH.la_nodes(M, h) == nodes
        for cap in (0, 1, nodes - 1, nodes * 64, nodes * 64 + 1, nodes * 127, nodes * 128, nodes * 200 // 3, 2 ** 31, 2 ** 40):
            lanes = LH.la_lanes_per_launch(C.c_int64(cap), M, h)
            eff = cap if cap > 0 else 2 ** 31
            assert lanes % 64 == 0 and lanes >= 64
            assert lanes == max(64, eff // nodes // 64 * 64)
            assert lanes == 64 or lanes * nodes <= eff           # no launch above the bound, unless one wave already is
            assert (lanes + 64) * nodes > eff                    # and no smaller than it has to be
    # 200 lanes in three launches: 64 lanes each at 3 rates, horizon 3
    assert LH.la_lanes_per_launch(C.c_int64(39 * 64), 3, 3) == 64
    # the flagship shape at the default: 6 rates, horizon 5
    assert LH.la_lanes_per_launch(C.c_int64(0), 6, 5) == 2 ** 31 // 9330 // 64 * 64 == 230144
