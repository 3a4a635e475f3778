"""The learned policy without a GPU: the device source (csrc/abr_lane_jump.h: policy_features, policy_forward,
policy_explore) compiled for the host against the numpy twin, bit for bit, on seeded cases with their knife edges; the
twin's fmaf against exact rational arithmetic; the ABI struct, the size queries and every validation refusal; the
controller's packing of an nn.Sequential and its refusals."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from helpers import c_abi_output, native_harness
import policy_twin as T

HMAX = 40
P_ = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))


@pytest.fixture(scope="module")
def PH():
    return native_harness("policy_harness")


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


# ---------------------------------------------------------------------------------------------------------------------
# fmaf: the twin against exact arithmetic

def _f32_exact(q):
    """Round a Fraction to float32, to nearest even, with subnormals and overflow."""
    if q == 0:
        return np.float32(0.0)
    sgn, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    ulp = Fraction(2) ** max(e - 23, -149)
    m = q / ulp
    r = m.numerator // m.denominator
    rem = m - r
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and r % 2 == 1):
        r += 1
    v = r * ulp
    if v >= Fraction(2) ** 128:
        return np.float32(sgn * np.inf)
    return np.float32(sgn * float(v))


def double_rounding_cases(rng, n):
    """c a float32 with a random mantissa, a = 1 +- 2^-k, b = (1 -+ 2^-k) * ulp(c) / 2, k in 15..23: a*b + c sits next to
    a float32 rounding boundary, where float32(float64(a*b + c)) rounds twice."""
    k = rng.integers(15, 24, n)
    sgn = rng.choice([-1.0, 1.0], n)
    c = (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-20, 20, n) * rng.choice([-1, 1], n)).astype(np.float32)
    ulp = np.spacing(np.abs(c)).astype(np.float64)                          # float32's ulp
    a = (1.0 + sgn * 2.0 ** -k).astype(np.float32)
    b = ((1.0 - sgn * 2.0 ** -k) * ulp / 2.0 * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return a, b, c.astype(np.float32)


def test_twin_fmaf_is_exact_on_double_rounding_cases():
    rng = np.random.default_rng(1)
    a, b, c = double_rounding_cases(rng, 20000)
    got = T.fmaf(a, b, c)
    want = np.array([_f32_exact(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)],
                    np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    naive = (a.astype(np.float64) * b + c).astype(np.float32)
    assert (naive.view(np.uint32) != want.view(np.uint32)).sum() > 1000       # the generator does hit double rounding


def test_twin_fmaf_random_and_special_sample():
    rng = np.random.default_rng(2)
    n = 4000
    bits = rng.integers(0, 2 ** 32, (3, n), dtype=np.uint64).astype(np.uint32)
    a, b, c = (bits[i].view(np.float32) for i in range(3))
    sub = rng.random(n) < 0.2
    a[sub] = np.float32(1e-40) * rng.uniform(-1, 1, sub.sum()).astype(np.float32)      # subnormals
    got = T.fmaf(a, b, c)
    for i in range(n):
        x, y, z = float(a[i]), float(b[i]), float(c[i])
        if not all(np.isfinite([x, y, z])):
            continue
        w = _f32_exact(Fraction(x) * Fraction(y) + Fraction(z))
        if w == 0 and got[i] == 0:
            continue                                    # the sign of an exact zero follows IEEE (checked on the host build)
        assert got[i].view(np.uint32) == w.view(np.uint32), (i, x, y, z, got[i], w)


# ---------------------------------------------------------------------------------------------------------------------
# the host build of the device source against the twin

def same_bits(x, y):
    """Bitwise equal float32 arrays, any NaN equal to any NaN (the contract does not fix a NaN's sign or payload)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return x.shape == y.shape and bool(((x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))).all())


def _layers(rng, F, widths, M, special=False):
    out, fan = [], F
    for w in widths + [M]:
        W = rng.normal(0, 1.0 / np.sqrt(fan), (w, fan)).astype(np.float32)
        b = rng.normal(0, 0.1, w).astype(np.float32)
        if special:                                     # -0, subnormals, and a few infinities / NaNs per layer
            for arr in (W.reshape(-1), b):
                k = rng.random(arr.size)
                arr[k < 0.02] = np.float32(-0.0)
                arr[(k >= 0.02) & (k < 0.04)] = np.float32(1e-41)
                r = 0.3 / arr.size
                arr[(k >= 0.04) & (k < 0.04 + r)] = np.float32(np.inf)
                arr[(k >= 0.05) & (k < 0.05 + r)] = np.float32(-np.inf)
                arr[(k >= 0.06) & (k < 0.06 + r)] = np.float32(np.nan)
        out.append((W, b))
        fan = w
    return out


def _run(PH, layers, W, M, V, norm, seed, thr, c, a, B, G, P, h, br, lane, ep):
    n = len(c)
    widths = [Wl.shape[0] for Wl, _ in layers[:-1]]
    F = 4 + W + M
    blob = np.concatenate([np.concatenate([Wl.ravel(), bl]) for Wl, bl in layers]).astype(np.float32)
    x, s = np.zeros((n, F), np.float32), np.zeros((n, M), np.float32)
    g, act = np.zeros(n, np.int32), np.zeros(n, np.int32)
    w0 = widths[0] if len(widths) > 0 else 0
    w1 = widths[1] if len(widths) > 1 else 0
    PH.ph_run(C.c_int64(n), C.c_int32(W), C.c_int32(len(widths)), C.c_int32(w0), C.c_int32(w1), C.c_int32(M),
              C.c_int32(V), P_(blob, C.c_float), None if norm is None else P_(norm, C.c_double), C.c_uint64(seed),
              C.c_uint64(thr), P_(c, C.c_int32), P_(a, C.c_int32), P_(B, C.c_double), P_(G, C.c_double),
              P_(P, C.c_double), P_(h, C.c_double), C.c_int32(HMAX), P_(br, C.c_double), P_(lane, C.c_uint64),
              P_(ep, C.c_int32), P_(x, C.c_float), P_(s, C.c_float), P_(g, C.c_int32), P_(act, C.c_int32))
    return x, s, g, act


def _lane_inputs(rng, n, W, M, V):
    c = rng.integers(0, V, n).astype(np.int32)
    few = rng.random(n) < 0.2
    c[few] = rng.integers(0, min(W + 1, V), few.sum())                     # c < W: zero-filled history rows
    a = rng.integers(-1, M, n).astype(np.int32)
    a[rng.random(n) < 0.2] = -1
    B = rng.uniform(0.0, 30.0, n)
    G = rng.uniform(0.0, 500.0, n)
    P = G - rng.uniform(0.0, 40.0, n)
    h = rng.uniform(0.05, 12.0, (n, HMAX))
    k = rng.random((n, HMAX))
    h[k < 0.01] = np.inf
    h[(k >= 0.01) & (k < 0.02)] = np.nan
    h[(k >= 0.02) & (k < 0.03)] = 1e-310
    h[(k >= 0.03) & (k < 0.04)] = -0.0
    e = rng.random(n)
    B[e < 0.01] = np.nan
    B[(e >= 0.01) & (e < 0.02)] = 1e-44                                  # float32 subnormal after the cast
    B[(e >= 0.02) & (e < 0.03)] = -0.0
    G[(e >= 0.03) & (e < 0.04)] = np.inf
    return c, a, B, G, P, h


CONFIGS = [  # (W, widths, M, V, thr, norm, special weights)
    (8, [64, 64], 16, 40, 0, "rand", False), (8, [64, 64], 6, 24, 2 ** 31, None, True), (0, [], 6, 10, 0, "rand", True),
    (16, [64], 16, 30, 1, "rand", False), (1, [1], 3, 5, 2 ** 32, None, False), (16, [1, 64], 4, 40, 0, None, True),
    (5, [33], 1, 12, 2 ** 31, "rand", True), (3, [64, 1], 8, 20, 123456789, "rand", False),
    (0, [7, 2], 2, 3, 0, None, False), (12, [], 16, 40, 2 ** 30, "rand", False), (16, [64, 64], 16, 40, 2 ** 32 - 1, None, True),
]


def test_host_build_matches_twin(PH):
    rng = np.random.default_rng(4242)
    total = explored = finite = 0
    for (W, widths, M, V, thr, norm, special) in CONFIGS:
        n = 10000
        F = 4 + W + M
        layers = _layers(rng, F, widths, M, special)
        nrm = None
        if norm == "rand":
            nrm = np.stack([rng.normal(0, 1, F), rng.uniform(0.01, 2.0, F)])
        br = np.sort(rng.uniform(0.2, 8.0, (V, M)), axis=1)                   # a per-chunk ladder
        c, a, B, G, P, h = _lane_inputs(rng, n, W, M, V)
        lane = rng.integers(0, 2 ** 40, n).astype(np.uint64)
        ep = rng.integers(0, 5, n).astype(np.int32)
        seed = int(rng.integers(0, 2 ** 63))
        x, s, g, act = _run(PH, layers, W, M, V, nrm, seed, thr, c, a, B, G, P, h, br, lane, ep)
        wx = T.features(W, M, V, c, a, B, G, P, h.T, lambda r: br[r], nrm)
        assert same_bits(x, wx.T), (W, widths, M)
        want_a, ws, coin = T.decide(layers, wx, seed, thr, lane, c, ep, M)
        assert same_bits(s, ws.T), (W, widths, M)
        finite += int(np.isfinite(s).all(axis=1).sum())
        assert np.array_equal(g, T.argmax_first(ws)), (W, widths, M)
        assert np.array_equal(act, want_a), (W, widths, M)
        if thr == 0:
            assert not coin.any() and np.array_equal(act, g)
        if thr == 2 ** 32:
            assert coin.all()
        if thr == 1:
            assert coin.sum() <= 1
        explored += int(coin.sum())
        total += n
    assert total >= 100000 and explored > 10000 and finite > total // 2


def _forward(PH, layers, W, M, x):
    n = x.shape[0]
    widths = [Wl.shape[0] for Wl, _ in layers[:-1]]
    blob = np.concatenate([np.concatenate([Wl.ravel(), bl]) for Wl, bl in layers]).astype(np.float32)
    s, g = np.zeros((n, M), np.float32), np.zeros(n, np.int32)
    PH.ph_forward(C.c_int64(n), C.c_int32(W), C.c_int32(len(widths)), C.c_int32(widths[0] if widths else 0),
                  C.c_int32(widths[1] if len(widths) > 1 else 0), C.c_int32(M), P_(blob, C.c_float),
                  P_(np.ascontiguousarray(x, np.float32), C.c_float), P_(s, C.c_float), P_(g, C.c_int32))
    return s, g


def test_double_rounding_through_the_forward_pass(PH):
    """score = fmaf(a, b, fmaf(1, c, 0)) then terms 0 * 0: x = [c, b, 0, 0, 0], W = [1, a, 0, 0, 0], bias 0; grouped by a
    (the generator draws few distinct a)."""
    rng = np.random.default_rng(5)
    n = 20000
    a, b, c = double_rounding_cases(rng, n)
    M, W = 1, 0
    F = 4 + W + M
    x = np.zeros((n, F), np.float32)
    x[:, 0], x[:, 1] = c, b
    got = np.empty(n, np.float32)
    for av in np.unique(a):
        idx = np.flatnonzero(a == av)
        Wm = np.zeros((1, F), np.float32)
        Wm[0, 0], Wm[0, 1] = 1.0, av
        s, _ = _forward(PH, [(Wm, np.zeros(1, np.float32))], W, M, x[idx])
        got[idx] = s[:, 0]
    want = T.fmaf(a, b, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got.view(np.uint32) != (a.astype(np.float64) * b + c).astype(np.float32).view(np.uint32)).sum() > 1000


def test_ties_nan_and_relu(PH):
    M, W = 4, 0
    F = 4 + W + M
    x = np.zeros((6, F), np.float32)
    x[:, 0] = [1, 2, 3, -1, 0, 5]
    # output j = bias_j only: ties -> first, NaN never wins, NaN at 0 answers 0
    for bias, want in (([1, 3, 3, 2], 1), ([np.nan, 5, 9, 1], 0), ([np.nan] * 4, 0), ([0, np.nan, 2, 2], 2),
                       ([-0.0, 0.0, 0.0, 0.0], 0), ([-np.inf, -np.inf, -1e30, -np.inf], 2)):
        Wm = np.zeros((M, F), np.float32)
        s, g = _forward(PH, [(Wm, np.array(bias, np.float32))], W, M, x)
        assert (g == want).all(), (bias, g)
        assert np.array_equal(T.argmax_first(s.T), g)
    # ReLU: NaN, -0 and negatives -> +0 (the second layer sees exactly +0: 1 * +0 + -0 = +0)
    Wm0 = np.zeros((3, F), np.float32)
    b0 = np.array([np.nan, -0.0, -5.0], np.float32)
    Wo = np.ones((M, 3), np.float32)
    bo = np.full(M, -0.0, np.float32)
    s, g = _forward(PH, [(Wm0, b0), (Wo, bo)], W, M, x)
    assert (s.view(np.uint32) == 0).all()


def test_twin_matches_torch_modules_within_rounding():
    torch = pytest.importorskip("torch")
    from abrsimulator_amd.policy import PolicyController, pack_layers
    torch.manual_seed(0)
    for hidden in ([], [64], [64, 64], [5, 1]):
        F, M = 4 + 8 + 6, 6
        mods, fan = [], F
        for w in hidden:
            mods += [torch.nn.Linear(fan, w), torch.nn.ReLU()]
            fan = w
        mods.append(torch.nn.Linear(fan, M))
        net = torch.nn.Sequential(*mods)
        layers = PolicyController.module_layers(net)
        blob = pack_layers(layers)
        # the packing order: per layer weight (row-major [out][in]) then bias
        o = 0
        for lin in mods[0::2]:
            w = lin.weight.detach().numpy().ravel()
            assert np.array_equal(blob[o:o + w.size], w)
            o += w.size
            assert np.array_equal(blob[o:o + lin.out_features], lin.bias.detach().numpy())
            o += lin.out_features
        assert o == blob.size
        x = np.random.default_rng(1).normal(0, 1, (F, 500)).astype(np.float32)
        lay = [(W.detach().numpy(), b.detach().numpy()) for W, b in layers]
        tw = T.forward(lay, x)
        with torch.no_grad():
            ref = net(torch.from_numpy(x.T)).numpy().T
        assert np.allclose(tw, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def test_from_module_refusals():
    torch = pytest.importorskip("torch")
    from abrsimulator_amd.datamodel import MPD, Chunk
    from abrsimulator_amd.policy import PolicyController
    nn = torch.nn

    class Player:
        env = None

        def get_mpd(self):
            return MPD(10, 4.0, 20.0, 4.0, Chunk([0.3, 0.75, 1.2, 1.85, 2.85, 4.3]))
    F, M = 4 + 8 + 6, 6
    bad = [nn.Linear(F, M),                                                        # not a Sequential
           nn.Sequential(nn.Linear(F, 8), nn.Tanh(), nn.Linear(8, M)),             # another activation
           nn.Sequential(nn.Linear(F, 8), nn.ReLU()),                              # ends in ReLU
           nn.Sequential(nn.Linear(F, 8, bias=False), nn.ReLU(), nn.Linear(8, M)),
           nn.Sequential(nn.Linear(F, 8), nn.ReLU(), nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 8), nn.ReLU(),
                         nn.Linear(8, M)),                                         # three hidden layers
           nn.Sequential(nn.Linear(F, 8), nn.ReLU(), nn.Linear(8, M + 1)),         # output width != M
           nn.Sequential(nn.Linear(F + 1, 8), nn.ReLU(), nn.Linear(8, M)),         # input width != F
           nn.Sequential(nn.Linear(F, 65), nn.ReLU(), nn.Linear(65, M)),           # hidden width > 64
           nn.Sequential()]
    for m in bad:
        with pytest.raises(ValueError):
            PolicyController.from_module(Player(), m, window=8)
    for w in (-1, 17, 2.5, True):
        with pytest.raises(ValueError):
            PolicyController.from_module(Player(), nn.Sequential(nn.Linear(F, M)), window=w)


# ---------------------------------------------------------------------------------------------------------------------
# the ABI: struct layout, size queries, refusals (all before any HIP call)

def test_policy_struct_layout_matches_header(L):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(abr_policy), offsetof(abr_policy, window),
         offsetof(abr_policy, n_hidden), offsetof(abr_policy, width), offsetof(abr_policy, weights_dev),
         offsetof(abr_policy, weights_bytes), offsetof(abr_policy, norm_dev), offsetof(abr_policy, seed),
         offsetof(abr_policy, explore_threshold), offsetof(abr_policy, reserved_));
  printf("%d %d %d\n", ABR_POLICY_MAX_WINDOW, ABR_POLICY_MAX_HIDDEN, ABR_POLICY_MAX_WIDTH);
  return 0;
}'''
    out = c_abi_output(prog)
    P = L.Policy
    got = list(map(int, out[0].split()))
    assert got == [C.sizeof(P), P.window.offset, P.n_hidden.offset, P.width.offset, P.weights_dev.offset,
                   P.weights_bytes.offset, P.norm_dev.offset, P.seed.offset, P.explore_threshold.offset,
                   P.reserved_.offset]
    assert got[0] == 72
    assert list(map(int, out[1].split())) == [L.POLICY_MAX_WINDOW, L.POLICY_MAX_HIDDEN, L.POLICY_MAX_WIDTH]


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


def test_size_queries(L):
    lib = L.lib()
    d = C.c_int32()
    assert lib.abr_policy_feature_dim(8, 6, C.byref(d)) == 0 and d.value == 18
    assert lib.abr_policy_feature_dim(16, 16, C.byref(d)) == 0 and d.value == 36
    for w, m in ((-1, 6), (17, 6), (0, 0), (0, 17)):
        assert lib.abr_policy_feature_dim(w, m, C.byref(d)) == -1
    assert lib.abr_policy_feature_dim(0, 1, None) == -1
    b = C.c_size_t()
    assert lib.abr_policy_weights_bytes(C.byref(_pol(L, window=16)), 16, C.byref(b)) == 0
    assert b.value == 4 * 7568                                                  # the largest blob: 30 272 B
    assert lib.abr_policy_weights_bytes(C.byref(_pol(L, n_hidden=0, width=(0, 0), window=0)), 1, C.byref(b)) == 0
    assert b.value == 4 * (5 * 1 + 1)
    assert lib.abr_policy_weights_bytes(C.byref(_pol(L, n_hidden=1, width=(3, 0), window=2)), 4, C.byref(b)) == 0
    assert b.value == 4 * (3 * 10 + 3 + 4 * 3 + 4)
    # the size query does not look at the pointers
    assert lib.abr_policy_weights_bytes(C.byref(_pol(L, weights_dev=None)), 6, C.byref(b)) == 0
    for m in (0, 17):
        assert lib.abr_policy_weights_bytes(C.byref(_pol(L)), m, C.byref(b)) == -1


STRUCT_REFUSALS = [dict(window=-1), dict(window=17), dict(n_hidden=-1), dict(n_hidden=3), dict(width=(0, 64)),
                   dict(width=(64, 65)), dict(n_hidden=1, width=(64, 64)), dict(n_hidden=0, width=(8, 0)),
                   dict(reserved=0), dict(reserved=3), dict(weights_dev=None), dict(weights_dev=4098),
                   dict(norm_dev=4100), dict(explore_threshold=2 ** 32 + 1), dict(explore_threshold=2 ** 64 - 1)]


def test_every_refusal_before_the_handle(L):
    lib = L.lib()
    act = C.c_void_p(8192)
    for kw in STRUCT_REFUSALS:
        p = _pol(L, **kw)
        assert lib.abr_env_policy_select(None, C.byref(p), act, None, None, None) == -1, kw
        assert b"policy" in lib.abr_last_error() or b"explore" in lib.abr_last_error(), kw
        assert lib.abr_env_step_policy(None, C.byref(p), 4, None, None, None, None, None, None, None) == -1, kw
        assert b"policy" in lib.abr_last_error() or b"explore" in lib.abr_last_error(), kw
    assert lib.abr_env_policy_select(None, None, act, None, None, None) == -1
    assert lib.abr_env_step_policy(None, None, 4, None, None, None, None, None, None, None) == -1
    ok = _pol(L)
    for n in (0, -1):
        assert lib.abr_env_step_policy(None, C.byref(ok), n, None, None, None, None, None, None, None) == -1
        assert b"n_steps" in lib.abr_last_error()
    # a valid struct reaches the handle
    assert lib.abr_env_step_policy(None, C.byref(ok), 1, None, None, None, None, None, None, None) == -1
    assert b"env is NULL" in lib.abr_last_error()
    assert lib.abr_env_policy_select(None, C.byref(ok), act, None, None, None) == -1
    assert b"NULL argument" in lib.abr_last_error()
    for thr in (0, 1, 2 ** 31, 2 ** 32):                                    # the whole threshold range is accepted
        p = _pol(L, explore_threshold=thr)
        assert lib.abr_env_step_policy(None, C.byref(p), 1, None, None, None, None, None, None, None) == -1
        assert b"env is NULL" in lib.abr_last_error()


def test_explore_threshold_mapping():
    pytest.importorskip("torch")
    from abrsimulator_amd.policy import PolicyController
    c = PolicyController.__new__(PolicyController)
    for eps, thr in ((0.0, 0), (1.0, 2 ** 32), (0.5, 2 ** 31), (0.1, int(np.floor(0.1 * 2 ** 32))), (2 ** -32, 1)):
        c.explore = eps
        assert c.explore_threshold == thr
    for eps in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            c.explore = eps
