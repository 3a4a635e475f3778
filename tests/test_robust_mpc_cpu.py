"""RobustMPC without a GPU: the device source of its estimate (csrc/abr_lane_jump.h: robust_estimate) compiled for the
host against the numpy twin on seeded cases with their edges, the ABI struct, every validation refusal, the controller's
arguments, and the compiled predictor kernel."""
import ctypes as C
import re

import numpy as np
import pytest

from helpers import c_abi_output, native_harness
from robust_twin import empty_state, estimate_scalar, estimate_vec, state_bytes, state_from_bytes, state_nbytes

HMAX = 40


@pytest.fixture(scope="module")
def H():
    return native_harness("robust_harness")


def _cases(rng, n):
    """n seeded (window, chunk, history, state) cases, most of them on one of the contract's edges."""
    W = rng.integers(1, 17, n).astype(np.int32)
    W[rng.random(n) < 0.3] = 5
    c = rng.integers(0, HMAX + 1, n).astype(np.int32)
    e = rng.random(n)
    c = np.where(e < 0.08, 0, c)
    c = np.where((e >= 0.08) & (e < 0.16), 1, c)
    c = np.where((e >= 0.16) & (e < 0.26), np.minimum(W, HMAX), c)
    c = np.where((e >= 0.26) & (e < 0.36), np.minimum(W + 1, HMAX), c).astype(np.int32)
    h = rng.uniform(0.05, 10.0, (n, HMAX))
    # c* relative to c: none, c - 1 (push), c (keep), gaps, rewinds, garbage
    rel = rng.random(n)
    cs1 = np.where(rel < 0.15, 0, np.where(rel < 0.55, c, np.where(rel < 0.7, c + 1, np.where(
        rel < 0.8, np.maximum(c - 2, 0), np.where(rel < 0.9, c + 4, rng.integers(-3, 3, n)))))).astype(np.int32)
    cnt = (rng.random(n) * (W + 1)).astype(np.int32)
    full = rng.random(n) < 0.3
    cnt[full] = W[full]
    bad = rng.random(n) < 0.02
    cnt[bad] = rng.choice([-1, 17, 99], bad.sum())
    ps = rng.uniform(0.05, 10.0, n)
    err = rng.uniform(0.0, 2.0, (n, 16))
    # ties in E: the maximum twice (and an all-equal row)
    tie = rng.random(n) < 0.1
    for i in np.flatnonzero(tie):
        k = max(int(min(cnt[i], W[i])), 2)
        a, b = rng.choice(k, 2, replace=False)
        err[i, b] = err[i, a] = err[i, :k].max() + 0.5
    eq = rng.random(n) < 0.03
    err[eq] = 0.75
    # huge and tiny throughputs: 1 / h overflows or underflows, hm overflows or underflows, P underflows
    x = rng.random(n)
    for i in np.flatnonzero(x < 0.12):
        k = rng.integers(0, 8)
        j = slice(max(c[i] - W[i], 0), c[i]) if c[i] else slice(0, 1)
        if k == 0:
            h[i, j] = 1e-310                                   # subnormal: 1/h = inf, S = inf, hm = 0
        elif k == 1:
            h[i, j] = 1.7e308                                  # hm near DBL_MAX
        elif k == 2:
            h[i, j] = 1e300
            err[i] = 1e300                                     # P = hm / 1e300
        elif k == 3:
            h[i, j] = 1e-300
            err[i] = 1e300                                     # P underflows to 0: no decision, estimate recorded
        elif k == 4:
            h[i, j] = 0.0                                      # 1/0 = inf
        elif k == 5:
            h[i, j] = np.inf                                   # 1/inf = 0: S = 0, hm = inf
        elif k == 6:
            ps[i] = 1e308
            h[i, max(c[i] - 1, 0)] = 1e-308                    # a pushed error of inf: P = 0
        else:
            h[i, max(c[i] - 1, 0)] = np.inf                    # a pushed error of NaN
    return dict(W=W, c=c, h=h, cs1=cs1, cnt=cnt, ps=ps, err=err)


def _run(H, k):
    n = len(k["W"])
    cs1, cnt, ps, err = k["cs1"].copy(), k["cnt"].copy(), k["ps"].copy(), np.ascontiguousarray(k["err"]).copy()
    P = np.zeros(n)
    P_ = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    W, c, h = (np.ascontiguousarray(k[x]) for x in ("W", "c", "h"))
    H.rh_robust(C.c_int64(n), P_(W, C.c_int32), P_(c, C.c_int32), P_(h, C.c_double), C.c_int32(HMAX),
                P_(cs1, C.c_int32), P_(cnt, C.c_int32), P_(ps, C.c_double), P_(err, C.c_double), P_(P, C.c_double))
    return P, cs1, cnt, ps, err


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_host_build_matches_twin(H):
    rng = np.random.default_rng(4242)
    n = 120000
    k = _cases(rng, n)
    P, cs1, cnt, ps, err = _run(H, k)
    # the scalar twin on every case, state as a one-lane slice of the 16-row layout
    wP = np.zeros(n)
    st = dict(cs1=k["cs1"].copy(), cnt=k["cnt"].copy(), ps=k["ps"].copy(), err=k["err"].T.copy())
    for i in range(n):
        wP[i] = estimate_scalar(k["W"][i], k["c"][i], k["h"][i], st, i)
    assert np.array_equal(_bits(P), _bits(wP)), np.flatnonzero(_bits(P) != _bits(wP))[:5]
    assert np.array_equal(cs1, st["cs1"]) and np.array_equal(cnt, st["cnt"])
    assert np.array_equal(_bits(ps), _bits(st["ps"]))
    assert np.array_equal(_bits(err), _bits(st["err"].T))
    # the vectorised twin, one window at a time (lanes over cases)
    for w in (1, 5, 16):
        sel = np.flatnonzero(k["W"] == w)
        sv = dict(cs1=k["cs1"][sel].copy(), cnt=k["cnt"][sel].copy(), ps=k["ps"][sel].copy(),
                  err=k["err"][sel, :w].T.copy())
        vP = estimate_vec(w, k["c"][sel], k["h"][sel].T, sv)
        assert np.array_equal(_bits(vP), _bits(P[sel])), w
        assert np.array_equal(sv["cs1"], cs1[sel]) and np.array_equal(sv["cnt"], cnt[sel]), w
        assert np.array_equal(_bits(sv["ps"]), _bits(ps[sel])), w
        assert np.array_equal(_bits(sv["err"]), _bits(err[sel, :w].T)), w
    # every branch was taken
    assert (P > 0).sum() > n // 3                                         # decisions
    assert ((P == 0) & (cs1 == 0)).sum() > 1000                           # no decision, state emptied
    assert ((P == 0) & (cs1 > 0)).sum() > 100                             # no decision, estimate recorded (P not > 0)
    assert (cnt == k["W"]).sum() > 1000 and ((cnt > 0) & (cnt < k["W"])).sum() > 1000
    assert np.isnan(err).any() and np.isinf(err).any()


def test_contract_examples(H):
    """The contract's steps on hand-made lanes: push, keep, clear, the window, the discount."""
    def one(W, c, h, cs1=0, cnt=0, ps=0.0, errs=()):
        hh = np.zeros((1, HMAX))
        hh[0, :len(h)] = h
        e = np.zeros((1, 16))
        e[0, :len(errs)] = errs
        k = dict(W=np.array([W], np.int32), c=np.array([c], np.int32), h=hh, cs1=np.array([cs1], np.int32),
                 cnt=np.array([cnt], np.int32), ps=np.array([ps]), err=e)
        P, a, b, p, er = _run(H, k)
        return P[0], a[0], b[0], p[0], er[0]
    assert one(5, 0, [], cs1=3, cnt=2, ps=1.5)[:4] == (0.0, 0, 0, 0.0)        # c = 0: no decision, state emptied
    P, cs1, cnt, ps, _ = one(5, 2, [2.0, 4.0])                               # no state: hm of both, no discount
    assert (P, cs1, cnt, ps) == (2.0 / (1.0 / 2.0 + 1.0 / 4.0), 3, 0, P)
    P, cs1, cnt, ps, er = one(2, 3, [1.0, 2.0, 4.0], cs1=3, ps=3.0)         # c* = c - 1: push |3 - 4| / 4
    hm = 2.0 / (1.0 / 2.0 + 1.0 / 4.0)
    assert (cs1, cnt, er[0], ps) == (4, 1, 0.25, hm) and P == hm / 1.25
    P2, cs1b, cnt2, _, _ = one(2, 3, [1.0, 2.0, 4.0], cs1=4, cnt=1, ps=hm, errs=[0.25])   # c* = c: unchanged
    assert (P2, cs1b, cnt2) == (P, 4, 1)
    P3, _, cnt3, _, _ = one(2, 3, [1.0, 2.0, 4.0], cs1=2, cnt=1, ps=hm, errs=[0.25])      # a gap: errors cleared
    assert cnt3 == 0 and P3 == hm
    _, _, cnt4, _, er4 = one(3, 4, [1.0] * 4, cs1=4, cnt=3, ps=2.0, errs=[0.1, 0.2, 0.3])  # full: oldest drops out
    assert cnt4 == 3 and list(er4[:3]) == [0.2, 0.3, 1.0]


def test_state_bytes_round_trip():
    rng = np.random.default_rng(3)
    st = empty_state(7, 5)
    st["cs1"][:] = rng.integers(0, 9, 7)
    st["cnt"][:] = rng.integers(0, 6, 7)
    st["ps"][:] = rng.random(7)
    st["err"][:] = rng.random((5, 7))
    b = state_bytes(st)
    assert b.size == state_nbytes(7, 5) == 7 * 8 * (2 + 5)
    back = state_from_bytes(b, 7, 5)
    assert all(np.array_equal(back[k], st[k]) for k in st)
    assert not state_bytes(empty_state(7, 5)).any()                      # all-zero bytes are the empty state


def test_robust_struct_layout_matches_header():
    from abrsimulator_amd import _lib
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(abr_mpc_robust), offsetof(abr_mpc_robust, window),
         offsetof(abr_mpc_robust, utility), offsetof(abr_mpc_robust, state_dev), offsetof(abr_mpc_robust, state_bytes),
         offsetof(abr_mpc_robust, hist_dev), offsetof(abr_mpc_robust, hist_stride), offsetof(abr_mpc_robust, scratch_dev),
         offsetof(abr_mpc_robust, scratch_bytes), offsetof(abr_mpc_robust, mask_is_done),
         offsetof(abr_mpc_robust, reserved_));
  printf("%d\n", ABR_ROBUST_MAX_WINDOW);
  return 0;
}'''
    out = c_abi_output(prog)
    R = _lib.MpcRobust
    assert list(map(int, out[0].split())) == [C.sizeof(R), R.window.offset, R.utility.offset, R.state_dev.offset,
                                              R.state_bytes.offset, R.hist_dev.offset, R.hist_stride.offset,
                                              R.scratch_dev.offset, R.scratch_bytes.offset, R.mask_is_done.offset,
                                              R.reserved_.offset]
    assert int(out[1]) == _lib.ROBUST_MAX_WINDOW


N_LANES = 100
ADDR = 1 << 20          # an aligned address no call below ever dereferences: each one is refused first


def _cfg(**kw):
    from abrsimulator_amd import _lib
    c = _lib.MpcConfig()
    c.n_rates, c.horizon, c.video_length, c.clip_horizon = 6, 5, 48, 1
    c.chunk_length, c.max_buffer, c.variance_weight, c.rebuffer_weight = 4.0, 20.0, 1.0, 4.3
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _rob(**kw):
    from abrsimulator_amd import _lib
    r = _lib.MpcRobust()
    r.window, r.utility = 5, 0
    r.state_dev, r.state_bytes = ADDR, state_nbytes(N_LANES, 5)
    r.hist_dev, r.hist_stride = ADDR, N_LANES
    r.scratch_dev, r.scratch_bytes = ADDR, N_LANES * (5 * 8 + 8)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


# (robust fields, words the message must contain)
BAD_ROBUST = [(dict(window=0), "window"), (dict(window=17), "window"), (dict(window=-1), "window"),
              (dict(utility=2), "utility"), (dict(utility=-1), "utility"), (dict(state_dev=None), "state"),
              (dict(state_dev=ADDR + 4), "aligned")]
# refusals only the standalone select makes (it needs the history and the scratch)
BAD_SELECT = [(dict(hist_dev=None), "history"), (dict(hist_stride=0), "history"),
              (dict(state_bytes=state_nbytes(N_LANES, 5) - 1), "state"),
              (dict(window=6), "state"),                                  # the state was sized for window 5
              (dict(scratch_dev=None), "scratch"), (dict(scratch_bytes=N_LANES * 48 - 1), "scratch"),
              (dict(scratch_dev=ADDR + 4), "scratch")]


def _select(lib, cfg, rob, n=N_LANES, ptr=ADDR):
    p = C.c_void_p(ptr)
    return lib.abr_mpc_select_robust(None if cfg is None else C.byref(cfg), None if rob is None else C.byref(rob),
                                     p, p, p, p, p, None, p, None, None, n, None)


@pytest.mark.parametrize("bad,word", BAD_ROBUST + BAD_SELECT, ids=[str(b) for b, _ in BAD_ROBUST + BAD_SELECT])
def test_select_validation(bad, word):
    """Every refusal answers ABR_E_INVALID with a message that names what is wrong; nothing is launched."""
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    assert _select(lib, _cfg(), _rob(**bad)) == -1
    assert word in lib.abr_last_error().decode(), lib.abr_last_error()


def test_select_validation_of_config_lanes_and_pointers():
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    assert _select(lib, None, _rob()) == -1
    assert _select(lib, _cfg(horizon=1), _rob()) == -1 and "horizon" in lib.abr_last_error().decode()
    assert _select(lib, _cfg(), None) == -1 and "robust" in lib.abr_last_error().decode()
    assert _select(lib, _cfg(), _rob(), n=0) == -1 and "n_lanes" in lib.abr_last_error().decode()
    # too many lanes for the state (and the scratch)
    assert _select(lib, _cfg(), _rob(), n=N_LANES + 1) == -1 and "state" in lib.abr_last_error().decode()
    assert _select(lib, _cfg(), _rob(state_bytes=1 << 40), n=N_LANES + 1) == -1
    assert "scratch" in lib.abr_last_error().decode()
    assert _select(lib, _cfg(), _rob(), ptr=0) == -1 and "NULL" in lib.abr_last_error().decode()


@pytest.mark.parametrize("bad,word", BAD_ROBUST, ids=[str(b) for b, _ in BAD_ROBUST])
def test_env_step_validation_before_the_handle(bad, word):
    """The fused rollout refuses bad options with a NULL handle and a message about them, not about the handle."""
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(ADDR)
    assert lib.abr_env_step_mpc_robust(None, C.byref(_cfg()), C.byref(_rob(**bad)), p, p, 4, None, None, None, None,
                                       None) == -1
    msg = lib.abr_last_error().decode()
    assert word in msg and "env" not in msg, msg


def test_env_step_validation_n_steps_config_and_handle():
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(ADDR)

    def step(cfg, rob, n):
        return lib.abr_env_step_mpc_robust(None, None if cfg is None else C.byref(cfg),
                                           None if rob is None else C.byref(rob), p, p, n, None, None, None, None, None)
    assert step(_cfg(), _rob(), 0) == -1 and "n_steps" in lib.abr_last_error().decode()
    assert step(_cfg(n_rates=0), _rob(), 4) == -1 and "n_rates" in lib.abr_last_error().decode()
    assert step(None, _rob(), 4) == -1
    assert step(_cfg(), None, 4) == -1 and "robust" in lib.abr_last_error().decode()
    # hist, scratch and mask_is_done are not the rollout's business: a valid config gets as far as the handle
    assert step(_cfg(), _rob(hist_dev=None, hist_stride=0, scratch_dev=None), 4) == -1
    assert "env is NULL" in lib.abr_last_error().decode()


def test_state_bytes_query():
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    b = C.c_size_t()
    for w, n in ((1, 1), (5, 65536), (16, 3)):
        assert lib.abr_mpc_robust_state_bytes(w, n, C.byref(b)) == 0 and b.value == state_nbytes(n, w)
    for w, n in ((0, 4), (17, 4), (5, 0)):
        assert lib.abr_mpc_robust_state_bytes(w, n, C.byref(b)) == -1
    assert lib.abr_mpc_robust_state_bytes(5, 4, None) == -1


class _Stub:
    pass


def test_controller_arguments():
    import abrsimulator_amd as A
    ctl = A.BatchedMPCController(method="robust")
    assert (ctl.method, ctl.window) == ("robust", 5)
    assert A.BatchedMPCController(method="robust", window=16).window == 16
    for w in (0, 17, 2.5, True, -1):
        with pytest.raises(ValueError):
            A.BatchedMPCController(method="robust", window=w)
    with pytest.raises(ValueError):
        A.BatchedMPCController(method="robustmpc")
    sd = ctl.state_dict()
    assert sd["window"] == 5 and sd["state"] is None
    with pytest.raises(ValueError):
        A.BatchedMPCController(method="robust", window=4).load_state_dict(sd)


def test_predictor_kernel_is_compiled_without_scratch():
    """make asm: mpc_robust_predict_kernel exists with a 0 B private segment and no calls."""
    from test_rules_cpu import _product_asm
    text = _product_asm()
    found = [(name, desc) for name, desc in
             re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
             if "mpc_robust_predict_kernel" in name]
    assert len(found) == 1, [n for n, _ in found]
    name, desc = found[0]
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1)) == 0
    body = re.search(r"^" + re.escape(name) + r":(.*?)^\.Lfunc_end\d+:", text, re.S | re.M).group(1)
    assert "s_swappc" not in body and "s_setpc" not in body
