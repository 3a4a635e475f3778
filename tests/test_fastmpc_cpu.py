"""FastMPC without a GPU: the device source of the lookup (csrc/abr_lane_jump.h: fastmpc_lookup) compiled for the host
against the numpy twin on seeded cases with their knife edges, the ABI struct, the size queries, every validation refusal
and the controller's arguments."""
import ctypes as C
import re

import numpy as np
import pytest

from fastmpc_twin import lookup
from helpers import c_abi_output, native_harness

HMAX = 40


@pytest.fixture(scope="module")
def FH():
    return native_harness("fastmpc_harness")


def _blob(entries, be, te):
    """The device blob's bytes: entries padded to 8, then be, then te."""
    e = entries.ravel()
    pad = (-e.size) % 8
    return np.concatenate([e, np.zeros(pad, np.uint8), np.asarray(be, np.float64).view(np.uint8),
                           np.asarray(te, np.float64).view(np.uint8)])


def _grid(rng, n, lo, hi, geometric):
    if n == 1:
        return np.array([rng.uniform(lo, hi)]), np.zeros(0)
    p = np.geomspace(lo, hi, n) if geometric else np.linspace(lo, hi, n)
    e = np.sqrt(p[:-1] * p[1:]) if geometric else (p[:-1] + p[1:]) / 2.0
    return p, e


def _run(FH, blob, W, M, V, H, uniform, nb, nq, c, pv, B, h):
    n = len(c)
    out = np.zeros(n, np.int32)
    P_ = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
    c, pv, B, h = (np.ascontiguousarray(x) for x in (c, pv, B, h))
    FH.fh_lookup(C.c_int64(n), P_(blob, C.c_uint8), C.c_int32(W), C.c_int32(M), C.c_int32(V), C.c_int32(H),
                 C.c_int32(uniform), C.c_int32(nb), C.c_int32(nq), P_(c, C.c_int32), P_(pv, C.c_int32),
                 P_(B, C.c_double), P_(h, C.c_double), C.c_int32(HMAX), out.ctypes.data_as(C.POINTER(C.c_int32)))
    return out


def _cases(rng, n, W, M, V, be, te, tp):
    """n seeded lanes, many of them on the contract's knife edges."""
    c = rng.integers(0, min(V, HMAX + 1), n).astype(np.int32)
    k = rng.random(n)
    c[k < 0.05] = 0
    c[(k >= 0.05) & (k < 0.12)] = rng.integers(0, W + 1, ((k >= 0.05) & (k < 0.12)).sum()).clip(0, V - 1)
    c[(k >= 0.12) & (k < 0.15)] = V - 1 if V - 1 <= HMAX else HMAX
    pv = rng.integers(-M, M, n).astype(np.int32)
    pv[rng.random(n) < 0.1] = -1
    bad = rng.random(n) < 0.01
    pv[bad] = rng.choice([-M - 1, M, 99], bad.sum())
    B = rng.uniform(-1.0, 30.0, n)
    x = rng.random(n)
    if be.size:
        on = x < 0.2
        B[on] = rng.choice(be, on.sum())                                    # exactly on an edge
        B[(x >= 0.2) & (x < 0.25)] = np.nextafter(rng.choice(be, ((x >= 0.2) & (x < 0.25)).sum()), -np.inf)
    B[(x >= 0.25) & (x < 0.27)] = np.inf
    h = rng.uniform(0.05, 12.0, (n, HMAX))
    y = rng.random(n)
    for i in np.flatnonzero(y < 0.35):
        j = slice(max(c[i] - W, 0), max(c[i], 1))
        z = rng.integers(0, 7)
        if z == 0 and te.size:
            h[i, j] = rng.choice(te)                                        # P exactly on an edge (n copies)
        elif z == 1:
            h[i, j] = rng.choice(tp)                                        # P on a point
        elif z == 2:
            h[i, j] = np.nan                                                # P NaN
        elif z == 3:
            h[i, j] = 1e-310                                                # 1/h = inf: P = 0
        elif z == 4:
            h[i, j] = np.inf                                                # 1/inf = 0: P = inf
        elif z == 5:
            h[i, j] = 1e-300                                                # tiny
        else:
            h[i, j] = 1.5e308                                               # huge
    return c, pv, B, h


CONFIGS = [  # (M, V, H, uniform, Nb, Nq, W)
    (6, 48, 5, True, 64, 64, 5), (6, 48, 5, False, 64, 64, 5), (4, 20, 3, True, 16, 40, 1), (3, 9, 2, False, 1, 7, 3),
    (2, 12, 4, True, 9, 1, 16), (5, 6, 5, False, 1, 1, 2), (8, 30, 6, True, 256, 3, 8), (6, 48, 5, False, 5, 256, 5),
    (7, 40, 2, False, 33, 17, 12), (16, 10, 8, False, 2, 2, 4), (1, 5, 2, True, 3, 3, 5), (6, 41, 5, True, 64, 64, 7),
]


def test_host_build_matches_twin(FH):
    rng = np.random.default_rng(777)
    total = 0
    for (M, V, H, uniform, nb, nq, W) in CONFIGS:
        rows = H if uniform else V
        entries = rng.integers(0, M, (rows, M, nb, nq)).astype(np.uint8)
        bp, be = _grid(rng, nb, 0.0, 24.0, False)
        tp, te = _grid(rng, nq, 0.1, 20.0, True)
        blob = _blob(entries, be, te)
        n = 10000
        c, pv, B, h = _cases(rng, n, W, M, V, be, te, tp)
        got = _run(FH, blob, W, M, V, H, int(uniform), nb, nq, c, pv, B, h)
        want = np.array([lookup(entries, be, te, W, V, H, uniform, c[i], pv[i], B[i], h[i]) for i in range(n)])
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (M, V, H, uniform, nb, nq, W, bad[:5], got[bad[:5]], want[bad[:5]])
        assert (got == -1).sum() > 0 and (c == 0).sum() > 0
        total += n
    assert total >= 100000


def test_knife_edges(FH):
    """Hand-made lanes: B and P exactly on an edge read the upper cell, NaN reads cell 0, +inf the last cell, c = 0 is 0."""
    M, V, H, W = 3, 10, 2, 2
    bp, be = np.array([0.0, 2.0, 4.0]), np.array([1.0, 3.0])
    tp, te = np.array([1.0, 4.0]), np.array([2.0])
    entries = np.arange(H * M * 3 * 2, dtype=np.uint8).reshape(H, M, 3, 2) % 251
    blob = _blob(entries, be, te)

    def one(c, pv, B, hist):
        h = np.zeros((1, HMAX))
        h[0, :len(hist)] = hist
        return _run(FH, blob, W, M, V, H, 1, 3, 2, np.array([c], np.int32), np.array([pv], np.int32),
                    np.array([B]), h)[0]
    row = lambda c: min(V - c, H) - 1
    assert one(0, 1, 1.0, []) == 0                                          # no history: 0, as RATE
    assert one(3, 1, 1.0, [9, 2.0, 2.0]) == entries[row(3), 1, 1, 1]         # both exactly on an edge: upper cells
    assert one(3, 1, np.nextafter(1.0, 0), [9, 2.0, 2.0]) == entries[row(3), 1, 0, 1]
    assert one(3, -1, 1.0, [9, np.nan, 2.0]) == entries[row(3), M - 1, 1, 0]  # P NaN: cell 0; prev -1: M - 1
    assert one(3, 0, np.inf, [9, np.inf, np.inf]) == entries[row(3), 0, 2, 1]  # B, P = inf: last cells
    assert one(9, 2, np.nan, [1.0] * 9) == entries[row(9), 2, 0, 0]           # the last chunk reads row 0
    assert one(1, 0, 3.5, [5.0]) == entries[row(1), 0, 2, 1]                 # c < W: n = c
    assert one(10, 0, 1.0, [1.0] * 10) == -1 and one(2, 3, 1.0, [1.0] * 2) == -1 and one(2, -4, 1.0, [1.0] * 2) == -1


def test_struct_layout_matches_header():
    from abrsimulator_amd import _lib
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(abr_fastmpc), offsetof(abr_fastmpc, window),
         offsetof(abr_fastmpc, utility), offsetof(abr_fastmpc, n_rows), offsetof(abr_fastmpc, n_buffer),
         offsetof(abr_fastmpc, n_tput), offsetof(abr_fastmpc, buffer_points), offsetof(abr_fastmpc, buffer_edges),
         offsetof(abr_fastmpc, tput_points), offsetof(abr_fastmpc, tput_edges), offsetof(abr_fastmpc, reserved_));
  printf("%d\n", ABR_FASTMPC_MAX_POINTS);
  return 0;
}'''
    out = c_abi_output(prog)
    F = _lib.FastMpc
    assert list(map(int, out[0].split())) == [C.sizeof(F), F.window.offset, F.utility.offset, F.n_rows.offset,
                                              F.n_buffer.offset, F.n_tput.offset, F.buffer_points.offset,
                                              F.buffer_edges.offset, F.tput_points.offset, F.tput_edges.offset,
                                              F.reserved_.offset]
    assert int(out[1]) == _lib.FASTMPC_MAX_POINTS


ADDR = 1 << 20          # an aligned address no call below ever dereferences: each one is refused first
_KEEP = []


def _cfg(**kw):
    from abrsimulator_amd import _lib
    c = _lib.MpcConfig()
    c.n_rates, c.horizon, c.video_length, c.clip_horizon = 6, 5, 48, 1
    c.chunk_length, c.max_buffer, c.variance_weight, c.rebuffer_weight = 4.0, 20.0, 1.0, 4.3
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _arr(x):
    a = np.ascontiguousarray(x, np.float64)
    _KEEP.append(a)
    return a.ctypes.data


def _fm(bp=None, be=None, tp=None, te=None, **kw):
    from abrsimulator_amd import _lib
    bp = np.linspace(0.0, 24.0, 8) if bp is None else np.asarray(bp, np.float64)
    be = (bp[:-1] + bp[1:]) / 2 if be is None else np.asarray(be, np.float64)
    tp = np.geomspace(0.1, 20.0, 6) if tp is None else np.asarray(tp, np.float64)
    te = np.sqrt(tp[:-1] * tp[1:]) if te is None else np.asarray(te, np.float64)
    f = _lib.FastMpc()
    f.window, f.utility, f.n_rows, f.n_buffer, f.n_tput = 5, 0, 5, bp.size, tp.size
    f.buffer_points, f.buffer_edges, f.tput_points, f.tput_edges = _arr(bp), _arr(be), _arr(tp), _arr(te)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _bytes(lib, cfg, fm):
    b = C.c_size_t()
    rc = lib.abr_fastmpc_table_bytes(None if cfg is None else C.byref(cfg), None if fm is None else C.byref(fm),
                                     C.byref(b))
    return rc, b.value


def test_size_queries():
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    for (M, V, H, rows, nb, nq) in ((6, 48, 5, 5, 64, 64), (6, 48, 5, 48, 8, 6), (3, 9, 2, 9, 1, 1), (5, 7, 3, 3, 3, 1)):
        cfg = _cfg(n_rates=M, video_length=V, horizon=H)
        fm = _fm(bp=np.arange(nb, dtype=float), tp=np.arange(1, nq + 1, dtype=float), n_rows=rows)
        rc, b = _bytes(lib, cfg, fm)
        n = rows * M * nb * nq
        assert rc == 0 and b == (n + 7) // 8 * 8 + 8 * (nb - 1 + nq - 1), lib.abr_last_error()
        s = C.c_size_t()
        assert lib.abr_fastmpc_build_scratch_bytes(C.byref(cfg), C.byref(fm), C.byref(s)) == 0
        S = min(n, 131072)
        assert s.value == 8 * (nb + nq) + S * (8 * (H + 1) + 20)
    # the scratch is bounded however large the table
    cfg = _cfg(video_length=2000)
    fm = _fm(bp=np.arange(256.0), tp=np.arange(1.0, 257.0), n_rows=2000)
    s = C.c_size_t()
    assert lib.abr_fastmpc_build_scratch_bytes(C.byref(cfg), C.byref(fm), C.byref(s)) == 0
    assert s.value == 8 * 512 + 131072 * (8 * 6 + 20)
    assert lib.abr_fastmpc_table_bytes(C.byref(_cfg()), C.byref(_fm()), None) == -1


# (fields of abr_fastmpc / grids, words the message must contain)
BAD_FM = [
    (dict(window=0), "window"), (dict(window=17), "window"), (dict(utility=2), "utility"), (dict(utility=-1), "utility"),
    (dict(n_rows=6), "n_rows"), (dict(n_rows=0), "n_rows"),
    (dict(n_buffer=0), "points"), (dict(n_tput=257), "points"),
    (dict(bp=[0.0, 2.0, 1.0, 3.0]), "ascending"), (dict(bp=[0.0, 1.0, 1.0, 3.0]), "ascending"),
    (dict(tp=[1.0, np.nan, 3.0]), "finite"), (dict(bp=[0.0, np.inf]), "finite"),
    (dict(bp=[-1.0, 2.0]), ">= 0"), (dict(tp=[0.0, 2.0]), "> 0"), (dict(tp=[-1.0, 2.0], te=[1.0]), "> 0"),
    (dict(bp=[0.0, 2.0, 4.0], be=[1.0, 5.0]), "cell"), (dict(bp=[0.0, 2.0, 4.0], be=[2.5, 3.0]), "cell"),
    (dict(bp=[0.0, 2.0, 4.0], be=[1.0, 2.0]), "cell"),                    # a point on its upper edge: outside
    (dict(tp=[1.0, 2.0], te=[np.nan]), "finite"), (dict(bp=[0.0, 2.0, 4.0], be=[3.0, 1.0]), "ascending"),
    (dict(buffer_points=None), "NULL"), (dict(tput_edges=None), "NULL"),
]


def _fm_bad(bad):
    grid = {k: bad[k] for k in ("bp", "be", "tp", "te") if k in bad}
    f = _fm(**grid)
    for k, v in bad.items():
        if k not in grid:
            setattr(f, k, v)
    return f


@pytest.mark.parametrize("bad,word", BAD_FM, ids=[str(b) for b, _ in BAD_FM])
def test_grid_and_option_refusals(bad, word):
    """The size query and the build refuse with ABR_E_INVALID and a message naming what is wrong; nothing is launched."""
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    fm = _fm_bad(bad)
    rc, _ = _bytes(lib, _cfg(), fm)
    assert rc == -1 and word in lib.abr_last_error().decode(), lib.abr_last_error()
    p = C.c_void_p(ADDR)
    assert lib.abr_fastmpc_build(C.byref(_cfg()), C.byref(fm), p, p, p, 1 << 40, p, 1 << 40, None) == -1
    assert word in lib.abr_last_error().decode(), lib.abr_last_error()


def test_point_count_limit():
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    assert _bytes(lib, _cfg(), _fm(bp=np.arange(256.0)))[0] == 0
    rc, _ = _bytes(lib, _cfg(), _fm(bp=np.arange(257.0)))
    assert rc == -1 and "257" in lib.abr_last_error().decode()
    # a grid of one point needs no edges
    assert _bytes(lib, _cfg(), _fm(bp=[3.0], tp=[2.0], buffer_edges=None, tput_edges=None))[0] == 0


def test_layout_refusals():
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    assert _bytes(lib, _cfg(horizon=5, video_length=5), _fm(n_rows=5))[0] == 0      # V == H: the per-chunk layout
    rc, _ = _bytes(lib, _cfg(horizon=6, video_length=4), _fm(n_rows=6))
    assert rc == -1 and "uniform" in lib.abr_last_error().decode()
    assert _bytes(lib, _cfg(horizon=1), _fm())[0] == -1 and "horizon" in lib.abr_last_error().decode()
    assert _bytes(lib, None, _fm())[0] == -1
    assert _bytes(lib, _cfg(), None)[0] == -1 and "fastmpc" in lib.abr_last_error().decode()


def test_build_refusals_blob_and_scratch():
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    cfg, fm = _cfg(), _fm()
    _, tb = _bytes(lib, cfg, fm)
    s = C.c_size_t()
    lib.abr_fastmpc_build_scratch_bytes(C.byref(cfg), C.byref(fm), C.byref(s))
    sb = s.value
    p = C.c_void_p(ADDR)

    def build(table=ADDR, tbytes=tb, scratch=ADDR, sbytes=sb, br=ADDR):
        return lib.abr_fastmpc_build(C.byref(cfg), C.byref(fm), C.c_void_p(br), p, C.c_void_p(table), tbytes,
                                     C.c_void_p(scratch), sbytes, None)
    for kw, word in ((dict(table=0), "table"), (dict(table=ADDR + 4), "aligned"), (dict(tbytes=tb - 1), "table"),
                     (dict(scratch=0), "scratch"), (dict(scratch=ADDR + 2), "aligned"), (dict(sbytes=sb - 1), "scratch"),
                     (dict(br=0), "NULL")):
        assert build(**kw) == -1, kw
        assert word in lib.abr_last_error().decode(), (kw, lib.abr_last_error())


def test_select_refusals():
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    cfg, fm = _cfg(), _fm()
    _, tb = _bytes(lib, cfg, fm)
    p = C.c_void_p(ADDR)

    def sel(fm=fm, table=ADDR, tbytes=tb, hist=ADDR, stride=100, n=100, ptr=ADDR):
        q = C.c_void_p(ptr)
        return lib.abr_fastmpc_select(C.byref(cfg), C.byref(fm), C.c_void_p(table), tbytes, q, q, q, C.c_void_p(hist),
                                      stride, None, 0, q, n, None)
    for kw, word in ((dict(table=0), "table"), (dict(table=ADDR + 1), "aligned"), (dict(tbytes=tb - 1), "table"),
                     (dict(hist=0), "history"), (dict(stride=0), "history"), (dict(n=0), "n_lanes"),
                     (dict(ptr=0), "NULL"), (dict(fm=_fm(window=0)), "window")):
        assert sel(**kw) == -1, kw
        assert word in lib.abr_last_error().decode(), (kw, lib.abr_last_error())
    # the lookup reads the grid from the blob: the host grid pointers are not needed
    f2 = _fm(buffer_points=None, buffer_edges=None, tput_points=None, tput_edges=None)
    assert lib.abr_env_step_fastmpc(None, C.byref(cfg), C.byref(f2), p, 4, None, None, None, None, None) == -1
    assert "env is NULL" in lib.abr_last_error().decode()


@pytest.mark.parametrize("bad,word", [(dict(window=17), "window"), (dict(utility=3), "utility"), (dict(n_rows=7), "n_rows"),
                                      (dict(n_tput=0), "points")])
def test_env_refusals_before_the_handle(bad, word):
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(ADDR)
    fm = _fm(**bad)
    assert lib.abr_env_step_fastmpc(None, C.byref(_cfg()), C.byref(fm), p, 4, None, None, None, None, None) == -1
    msg = lib.abr_last_error().decode()
    assert word in msg and "env" not in msg, msg
    assert lib.abr_env_fastmpc_select(None, C.byref(_cfg()), C.byref(fm), p, p, None) == -1
    msg = lib.abr_last_error().decode()
    assert word in msg and "env" not in msg, msg
    assert lib.abr_env_step_fastmpc(None, C.byref(_cfg()), C.byref(_fm()), p, 0, None, None, None, None, None) == -1
    assert "n_steps" in lib.abr_last_error().decode()
    assert lib.abr_env_step_fastmpc(None, C.byref(_cfg()), C.byref(_fm()), None, 4, None, None, None, None, None) == -1
    assert "table" in lib.abr_last_error().decode()


class _Player:
    def __init__(self, mpd, qoe):
        self.mpd, self.qoe = mpd, qoe

    def get_mpd(self):
        return self.mpd

    def get_qoe_metric(self):
        return self.qoe


def test_controller_defaults_and_arguments():
    import abrsimulator_amd as A
    ladder = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
    p = _Player(A.MPD(48, 4.0, 20.0, 0.0, A.Chunk(ladder)), A.QOEMetric(4.3, 1, 0))
    ctl = A.FastMPCController(p, device="cpu")
    assert (ctl.horizon, ctl.window, ctl.utility, ctl.clip_horizon) == (5, 5, "identity", True)
    assert ctl.buffer_points.size == 64 and ctl.buffer_points[0] == 0.0 and ctl.buffer_points[-1] == 24.0
    assert np.array_equal(ctl.buffer_edges, (ctl.buffer_points[:-1] + ctl.buffer_points[1:]) / 2)
    assert ctl.tput_points.size == 64 and np.isclose(ctl.tput_points[0], 0.075) and np.isclose(ctl.tput_points[-1], 17.2)
    assert np.array_equal(ctl.tput_edges, np.sqrt(ctl.tput_points[:-1] * ctl.tput_points[1:]))
    assert ctl.uniform and ctl.n_rows == 5
    from abrsimulator_amd import _lib
    rc, b = _bytes(_lib.lib(), ctl.config(), ctl.options())
    assert rc == 0 and b == 5 * 6 * 64 * 64 + 8 * 126
    # per-chunk ladders (or sizes) select the per-chunk layout
    vbr = A.MPD(10, 4.0, 20.0, 0.0, [A.Chunk(ladder, [x * 4.0 * (1 + 0.01 * i) for x in ladder]) for i in range(10)])
    assert A.FastMPCController(_Player(vbr, A.QOEMetric(4.3, 1, 0)), device="cpu").n_rows == 10
    assert A.FastMPCController(p, layout="per_chunk", device="cpu").n_rows == 48
    with pytest.raises(ValueError):
        A.FastMPCController(_Player(vbr, A.QOEMetric(4.3, 1, 0)), layout="uniform", device="cpu").n_rows
    for w in (0, 17, 2.5, True):
        with pytest.raises(ValueError):
            A.FastMPCController(p, window=w, device="cpu")
    with pytest.raises(ValueError):
        A.FastMPCController(p, utility="sqrt", device="cpu")
    with pytest.raises(ValueError):
        A.FastMPCController(p, buffer_points=np.arange(300.0), device="cpu")


def test_lookup_kernels_compiled_without_scratch():
    """make asm: the standalone lookup and the grid kernel exist with a 0 B private segment and no calls."""
    from test_rules_cpu import _product_asm
    text = _product_asm()
    found = [(name, desc) for name, desc in
             re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
             if "fastmpc_" in name]
    assert len(found) == 4, [n for n, _ in found]
    for name, desc in found:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1)) == 0, name
        body = re.search(r"^" + re.escape(name) + r":(.*?)^\.Lfunc_end\d+:", text, re.S | re.M).group(1)
        assert "s_swappc" not in body and "s_setpc" not in body, name
