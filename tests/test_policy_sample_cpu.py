"""The learned policy's sampled decision without a GPU: the device source (csrc/abr_lane_jump.h: exp_c,
policy_softmax_sample, policy_decide) compiled for the host against the numpy twin (tests/policy_sample_twin.py) bit for
bit, on seeded cases and the contract's knife edges; exp_c's accuracy; the abr_policy_sampling struct, every refusal
before the handle; the controller's sample and temperature settings."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import c_abi_output, native_harness
import policy_sample_twin as S
import policy_twin as T

P_ = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
f32 = np.float32
TINY = np.finfo(np.float32).tiny


@pytest.fixture(scope="module")
def PS():
    return native_harness("policy_sample_harness")


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


def bits_equal(u, v):
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    return np.array_equal(u.view(np.uint32), v.view(np.uint32))


def host_exp(PS, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    PS.ps_exp(C.c_int64(x.size), P_(x, C.c_float), P_(out, C.c_float))
    return out


def host_sample(PS, s, g, iT, w2):
    """s [N, M] row-major (lane-major for the harness); returns pick [N], probs [N, M], e [N, M]."""
    s = np.ascontiguousarray(s, np.float32)
    N, M = s.shape
    g = np.ascontiguousarray(g, np.int32)
    iT = np.ascontiguousarray(np.broadcast_to(np.asarray(iT, np.float32), (N,)))
    w2 = np.ascontiguousarray(w2, np.uint32)
    pick = np.empty(N, np.int32)
    probs = np.empty((N, M), np.float32)
    e = np.empty((N, M), np.float32)
    PS.ps_sample(C.c_int64(N), M, P_(s, C.c_float), P_(g, C.c_int32), P_(iT, C.c_float), P_(w2, C.c_uint32),
                 P_(pick, C.c_int32), P_(probs, C.c_float), P_(e, C.c_float))
    return pick, probs, e


def check_sample(PS, s, iT, w2):
    """host build == twin on scores s [N, M]; returns the twin's (pick, probs)."""
    g = T.argmax_first(np.asarray(s, np.float32).T)
    pick, probs, e = host_sample(PS, s, g, iT, w2)
    tp, tprobs, te, _ = S.softmax_sample(np.asarray(s, np.float32).T, g, iT, np.asarray(w2, np.uint64))
    assert np.array_equal(pick, tp)
    assert bits_equal(probs, tprobs.T)
    fin = np.isfinite(np.asarray(s, np.float32)[np.arange(len(g)), g])
    assert bits_equal(e[fin], te.T[fin])                                 # the buffer holds e_m unless the fallback ran
    return tp, tprobs.T


# ---------------------------------------------------------------------------------------------------------------------
# exp_c

def _rint_ties():
    """float32 x in [-80, 0] whose rounded product x * LOG2E is exactly a half-integer (rintf's ties)."""
    out = []
    for h in np.arange(-115.5, 0.0, 1.0):
        x0 = f32(h / float(S.LOG2E))
        for x in (x0, np.nextafter(x0, f32(-np.inf)), np.nextafter(x0, f32(np.inf))):
            if x >= f32(-80) and float(f32(x * S.LOG2E)) == h:
                out.append(x)
    return np.array(out, np.float32)


def test_exp_c_host_equals_twin(PS):
    rng = np.random.default_rng(41)
    edges = np.array([-80.0, np.nextafter(f32(-80), f32(-np.inf)), np.nextafter(f32(-80), f32(0)), -0.0, 0.0,
                      -np.inf, np.nan, -1e-45, -TINY, -1e30, -88.0, -103.0], np.float32)
    ties = _rint_ties()
    assert len(ties) >= 50
    x = np.concatenate([edges, ties, -rng.uniform(0, 81, 60000).astype(np.float32),
                        -np.exp(rng.uniform(-100, 5, 40000)).astype(np.float32),
                        -rng.integers(0, 2 ** 31, 5000).astype(np.uint32).view(np.float32)[:5000]])
    x = x[~(x > 0)]
    got, want = host_exp(PS, x), S.exp_c(x)
    assert bits_equal(got, want)
    assert x.size >= 100_000
    assert got[3] == 1.0 and got[4] == 1.0 and got[0] > 0 and got[1] == 0 and got[5] == 0 and got[6] == 0
    assert not np.signbit(got[1]) and not np.signbit(got[6])             # +0


def test_exp_c_accuracy_on_a_dense_grid(PS):
    x = np.unique(np.concatenate([np.linspace(-80, 0, 4_000_001).astype(np.float32),
                                  -np.arange(1 << 20, dtype=np.float32) * f32(2.0 ** -21)]))
    e = host_exp(PS, x).astype(np.float64)
    rel = np.abs(e / np.exp(x.astype(np.float64)) - 1.0)
    assert rel.max() <= 2.0 ** -23, rel.max()                            # the bound include/abr_env.h states
    assert host_exp(PS, np.array([0.0, -0.0], np.float32)).tolist() == [1.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------------
# the draw

def test_sample_host_equals_twin_on_seeded_cases(PS):
    rng = np.random.default_rng(42)
    n = 0
    for M in range(1, 17):
        N = 7000
        scale = np.exp(rng.uniform(-6, 6, (N, 1)))
        s = (rng.normal(0, 1, (N, M)) * scale).astype(np.float32)
        ties = rng.random(N) < 0.1                                        # repeated top scores
        s[ties] = np.round(s[ties])
        iT = np.exp(rng.uniform(-4, 4, N)).astype(np.float32)
        w2 = rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
        pick, probs = check_sample(PS, s, iT, w2)
        assert ((pick >= 0) & (pick < M)).all()
        n += N
    assert n >= 100_000


def test_sample_edges(PS):
    # t == cum_m exactly: two equal scores, q = 1/2, t = 1 = cum_0: action 0 must not be taken
    pick, probs = check_sample(PS, np.zeros((1, 2), np.float32), 1.0, [1 << 31])
    assert pick.tolist() == [1] and probs.tolist() == [[0.5, 0.5]]
    # t == cum_m at every M with equal scores: w2 = (m * 2^24 / M) << 8 where exact
    for M in (2, 4, 8, 16):
        w2 = [(m * (1 << 24) // M) << 8 for m in range(M)]
        pick, _ = check_sample(PS, np.zeros((M, M), np.float32), 1.0, w2)
        assert pick.tolist() == list(range(M))
    # w2 < 256: q = 0, t = 0: the first action with e_m > 0;  w2 = 2^32 - 1: the last one
    s = np.array([[-200.0, 0.0, -1.0, -300.0]], np.float32)
    assert check_sample(PS, s, 1.0, [255])[0].tolist() == [1]
    assert check_sample(PS, s, 1.0, [0])[0].tolist() == [1]
    assert check_sample(PS, s, 1.0, [2 ** 32 - 1])[0].tolist() == [2]
    # M = 1 and M = 16
    assert check_sample(PS, np.array([[3.5]], np.float32), 1.0, [2 ** 32 - 1])[0].tolist() == [0]
    rng = np.random.default_rng(5)
    check_sample(PS, rng.normal(0, 1, (500, 16)).astype(np.float32), 1.0, rng.integers(0, 2 ** 32, 500))
    # NaN at index 0 (fallback, one-hot at 0) and elsewhere (e_m = 0, never drawn); +-inf
    nan, inf = np.nan, np.inf
    cases = np.array([[nan, 1.0, 2.0], [1.0, nan, 1.0], [nan, nan, nan], [inf, 1.0, 2.0], [1.0, inf, inf],
                      [-inf, -inf, -inf], [-inf, 0.0, -inf], [1.0, -inf, 1.0], [3e38, -3e38, 0.0]], np.float32)
    for w in (0, 1 << 31, 2 ** 32 - 1):
        pick, probs = check_sample(PS, cases, 1.0, np.full(len(cases), w))
        assert pick[0] == 0 and probs[0].tolist() == [1.0, 0.0, 0.0]
        assert pick[1] != 1 and probs[1][1] == 0.0
        assert pick[3] == 0 and pick[4] == 1 and pick[5] == 0 and probs[5].tolist() == [1.0, 0.0, 0.0]
        assert pick[6] == 1 and pick[7] != 1 and pick[8] == 0
    # inv_temperature: the smallest normal (uniform up to rounding), 1 and 2^100 (the argmax unless scores tie)
    rng = np.random.default_rng(6)
    s = rng.normal(0, 1, (4000, 6)).astype(np.float32)
    w2 = rng.integers(0, 2 ** 32, 4000)
    for iT in (TINY, 1.0, 2.0 ** 100):
        pick, probs = check_sample(PS, s, f32(iT), w2)
        if iT == 2.0 ** 100:
            assert np.array_equal(pick, T.argmax_first(s.T))
        if iT == TINY:
            assert (probs == f32(1) / f32(6)).all()
    check_sample(PS, np.zeros((3, 5), np.float32), f32(2.0 ** 100), [0, 1 << 31, 2 ** 32 - 1])


def _layers(rng, F, widths, M):
    out, fan = [], F
    for w in widths + [M]:
        out.append((rng.normal(0, 1.5 / np.sqrt(fan), (w, fan)).astype(np.float32), rng.normal(0, 0.2, w).astype(np.float32)))
        fan = w
    return out


def test_decide_host_equals_twin(PS):
    rng = np.random.default_rng(43)
    for W, widths, M, thr, iT in ((8, [64, 64], 6, 0, 1.0), (3, [7], 16, 1 << 30, 3.3), (0, [], 1, 0, 1.0),
                                  (16, [5, 9], 4, 1 << 32, 0.5), (2, [12], 6, 123456789, 2.0 ** 10)):
        F, N = 4 + W + M, 3000
        layers = _layers(rng, F, widths, M)
        x = rng.normal(0, 1, (N, F)).astype(np.float32)
        lane = rng.integers(0, 2 ** 40, N, dtype=np.uint64)
        c = rng.integers(0, 50, N).astype(np.int32)
        ep = rng.integers(0, 5, N).astype(np.int32)
        blob = np.concatenate([np.concatenate([Wl.ravel(), b]) for Wl, b in layers]).astype(np.float32)
        seed = int(rng.integers(1 << 62))
        for mode in (S.ARGMAX, S.SOFTMAX):
            s_out, p_out, act = np.empty((N, M), np.float32), np.empty((N, M), np.float32), np.empty(N, np.int32)
            w = widths + [0, 0]
            PS.ps_decide(C.c_int64(N), W, len(widths), w[0], w[1], M, P_(blob, C.c_float), C.c_uint64(seed),
                         C.c_uint64(thr), mode, C.c_float(iT), P_(x, C.c_float), P_(lane, C.c_uint64), P_(c, C.c_int32),
                         P_(ep, C.c_int32), P_(s_out, C.c_float), P_(p_out, C.c_float), P_(act, C.c_int32))
            a, s, coin, probs = S.decide_sampled(layers, x.T, seed, thr, lane, c.astype(np.uint64),
                                                 ep.astype(np.uint64), M, f32(iT), mode)
            assert bits_equal(s_out, s.T)
            assert bits_equal(p_out, probs.T), (W, widths, mode)
            assert np.array_equal(act, a), (W, widths, mode)
            if mode == S.ARGMAX:
                a0, _, _ = T.decide(layers, x.T, seed, thr, lane, c.astype(np.uint64), ep.astype(np.uint64), M)
                assert np.array_equal(act, a0)                          # exactly abr_env_policy_select's action


def test_behaviour_probs_sum_to_one():
    rng = np.random.default_rng(1)
    p = rng.dirichlet(np.ones(6), 50).T
    for thr in (0, 1 << 31, 1 << 32):
        b = S.behaviour_probs(p, 6, thr)
        assert np.allclose(b.sum(0), 1.0, atol=1e-12)
    rho = S.behaviour_probs(np.zeros((5, 1)), 5, 1 << 32)[:, 0]
    w0 = np.arange(0, 2 ** 32, 2 ** 12, dtype=np.uint64)                # a uniform grid of words 0: the same shares
    hist = np.bincount(((w0 * np.uint64(5)) >> np.uint64(32)).astype(np.int64), minlength=5) / len(w0)
    assert np.allclose(rho, hist, atol=2.0 ** -19)


# ---------------------------------------------------------------------------------------------------------------------
# the ABI: struct layout and refusals (all before the handle)

def test_sampling_struct_layout_matches_header(L):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(abr_policy_sampling), offsetof(abr_policy_sampling, mode),
         offsetof(abr_policy_sampling, inv_temperature), offsetof(abr_policy_sampling, reserved_));
  printf("%d %d %zu\n", ABR_POLICY_ARGMAX, ABR_POLICY_SOFTMAX, sizeof(abr_policy));
  return 0;
}'''
    out = c_abi_output(prog)
    P = L.PolicySampling
    got = list(map(int, out[0].split()))
    assert got == [C.sizeof(P), P.mode.offset, P.inv_temperature.offset, P.reserved_.offset]
    assert got[0] == 32
    assert list(map(int, out[1].split())) == [L.POLICY_ARGMAX, L.POLICY_SOFTMAX, 72]


def _pol(L, **kw):
    p = L.Policy()
    p.window, p.n_hidden = 8, 2
    p.width[0], p.width[1] = 64, 64
    p.weights_dev, p.weights_bytes, p.seed = 4096, 100, 1
    for k, v in kw.items():
        if k == "width":
            p.width[0], p.width[1] = v
        elif k == "reserved":
            p.reserved_[v] = 1
        else:
            setattr(p, k, v)
    return p


def _smp(L, mode=1, iT=1.0, reserved=None):
    s = L.PolicySampling()
    s.mode, s.inv_temperature = mode, iT
    if reserved is not None:
        s.reserved_[reserved] = 7
    return s


POLICY_REFUSALS = [dict(window=-1), dict(window=17), dict(n_hidden=3), dict(width=(0, 64)), dict(n_hidden=1, width=(64, 64)),
                   dict(reserved=0), dict(reserved=3), dict(weights_dev=None), dict(weights_dev=4098),
                   dict(norm_dev=4100), dict(explore_threshold=2 ** 32 + 1)]
SAMPLING_REFUSALS = [dict(mode=-1), dict(mode=2), dict(iT=0.0), dict(iT=-0.0), dict(iT=-1.0), dict(iT=math.inf),
                     dict(iT=-math.inf), dict(iT=math.nan), dict(reserved=0), dict(reserved=5)]


def _select(lib, p, s, act=C.c_void_p(8192)):
    return lib.abr_env_policy_select_sampled(None, p, s, act, None, None, None, None)


def _roll(lib, p, s, n=4):
    return lib.abr_env_step_policy_sampled(None, p, s, n, None, None, None, None, None, None, None, None)


def test_every_refusal_before_the_handle(L):
    lib = L.lib()
    ok_p, ok_s = _pol(L), _smp(L)
    for kw in POLICY_REFUSALS:
        p = _pol(L, **kw)
        for fn in (_select, _roll):
            assert fn(lib, C.byref(p), C.byref(ok_s)) == -1, kw
            assert b"policy" in lib.abr_last_error() or b"explore" in lib.abr_last_error(), kw
    for kw in SAMPLING_REFUSALS:
        s = _smp(L, **kw)
        for fn in (_select, _roll):
            assert fn(lib, C.byref(ok_p), C.byref(s)) == -1, kw
            assert b"sampling" in lib.abr_last_error(), kw
    for fn in (_select, _roll):
        assert fn(lib, None, C.byref(ok_s)) == -1
        assert fn(lib, C.byref(ok_p), None) == -1 and b"sampling is NULL" in lib.abr_last_error()
    for n in (0, -1):
        assert _roll(lib, C.byref(ok_p), C.byref(ok_s), n) == -1 and b"n_steps" in lib.abr_last_error()
    # valid structs reach the handle, both modes, the whole inv_temperature range
    for mode in (0, 1):
        for iT in (float(TINY), 1.0, 2.0 ** 100, float(np.finfo(np.float32).max)):
            s = _smp(L, mode, iT)
            assert _roll(lib, C.byref(ok_p), C.byref(s), 1) == -1 and b"env is NULL" in lib.abr_last_error()
            assert _select(lib, C.byref(ok_p), C.byref(s)) == -1 and b"NULL argument" in lib.abr_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the controller's settings

class _Player:
    env = None

    def get_mpd(self):
        from abrsimulator_amd.datamodel import MPD, Chunk
        return MPD(10, 4.0, 20.0, 4.0, Chunk([0.3, 0.75, 1.2, 1.85, 2.85, 4.3]))


def test_controller_sample_and_temperature(L):
    pytest.importorskip("torch")
    from abrsimulator_amd.policy import PolicyController
    layers = _layers(np.random.default_rng(0), 4 + 2 + 6, [4], 6)
    ctl = PolicyController(_Player(), layers, window=2, device="cpu")
    assert ctl.sample == "argmax" and ctl.temperature == 1.0 and ctl.inv_temperature == f32(1.0)
    assert not ctl.uses_sampled_entries(False) and ctl.uses_sampled_entries(True)
    smp = ctl.sampling()
    assert (smp.mode, smp.inv_temperature, list(smp.reserved_)) == (L.POLICY_ARGMAX, 1.0, [0] * 6)
    ctl.sample, ctl.temperature = "softmax", 0.3
    assert ctl.uses_sampled_entries(False)
    smp = ctl.sampling()
    assert smp.mode == L.POLICY_SOFTMAX and f32(smp.inv_temperature) == f32(1.0 / 0.3)
    assert ctl.inv_temperature == f32(1.0 / 0.3)                        # rounded once, from float64
    ctl2 = PolicyController(_Player(), layers, window=2, device="cpu", sample="softmax", temperature=2.5)
    assert ctl2.sampling().mode == 1 and ctl2.sampling().inv_temperature == 0.4000000059604645
    for bad in (0.0, -1.0, math.inf, math.nan, 1e-300, 1e300, True, "x"):
        with pytest.raises(ValueError):
            ctl.temperature = bad
        with pytest.raises(ValueError):
            PolicyController(_Player(), layers, window=2, device="cpu", temperature=bad)
    assert ctl.temperature == 0.3                                        # a refused value changes nothing
    for bad in ("greedy", "Softmax", None, 1):
        with pytest.raises(ValueError):
            ctl.sample = bad
        with pytest.raises(ValueError):
            PolicyController(_Player(), layers, window=2, device="cpu", sample=bad)
    assert ctl.sample == "softmax"
