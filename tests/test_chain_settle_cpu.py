"""The settlement of chain_segment (csrc/abr_exact_jump.h) on the CPU, in both of its forms (by the exact remainder of the
guess: every caller's default; by three candidates: kept for one family of kernels): chain<GE/LE/LT> against the naive
one-addition-per-tick loop, bit for bit, and -- segment by segment -- that an unspoiled estimate yields the LONGEST legal
jump (counted with naive additions), so that a cheaper settlement cannot quietly buy its instructions back with more trips.

The cases live in one table that two builds of tests/native/chain_settle_harness.cpp read: the shared native-harness
library, and a stand-alone program compiled with -fsanitize=address,undefined (no sanitizer runs on code loaded into
Python)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import native_harness

GE, LE, LT = 0, 1, 2
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    lib = native_harness("chain_settle_harness")
    lib.settle_check.restype = C.c_int64
    return lib


def _block(kind, bias, x0, c, thr, n):
    x0 = np.ascontiguousarray(x0, np.float64)
    f = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), x0.shape))
    return kind, bias, x0, f(c), f(thr), np.ascontiguousarray(np.broadcast_to(np.asarray(n), x0.shape).astype(np.int32))


def _edges(cap):
    """The settlement's own edges, built in the binade [1, 2) (u = 2^-52) with constants on u's grid, so that dm == |c|
    and every product below is exact: the stop sits exactly M steps away (r == 0 for a guess of M, r == dm for M - 1) or
    one ulp either side of that, and the budget puts room = n - 1 within one of M - 1, M and M + 1."""
    rng = np.random.default_rng(41)
    out = []
    u = 2.0 ** -52
    K = 4000
    c = rng.integers(1, 1 << 30, K) * u * rng.choice([1.0, 2.0 ** 8, 2.0 ** 16], K)
    M = rng.integers(1, 2000, K)
    dn = rng.integers(-2, 4, K)
    for du in (0, 1, -1):
        # going up from x0 to thr = x0 + M*c (+- one ulp), staying below 2
        x0 = 1.0 + rng.integers(0, 1 << 40, K) * u
        thr = x0 + M * c + du * u
        ok = thr < 2.0
        out.append(_block(GE, 0, x0[ok], c[ok], thr[ok], np.maximum(M + dn, 0)[ok]))
        # going down from x1 to thr = x1 - M*c (+- one ulp), staying above 1: LE is strict, LT may land on thr (r == dm)
        x1 = 2.0 - rng.integers(1, 1 << 40, K) * u
        thr = x1 - M * c + du * u
        ok = thr > 1.0
        for kind in (LE, LT):
            out.append(_block(kind, 0, x1[ok], -c[ok], thr[ok], np.maximum(M + dn, 0)[ok]))
        # ... and down to the binade's bottom itself: thr == 2^e makes LT strict, M*c reaches 1.0 exactly
        x2 = 1.0 + M * c
        ok = x2 < 2.0
        for kind in (LE, LT):
            out.append(_block(kind, 0, x2[ok], -c[ok], 1.0 + du * u, np.maximum(M + dn, 0)[ok]))
    # a quotient within one of room and of room + 1 at the segment cap: 2^20 +- 2 steps fit the binade and the stop
    for M in (cap - 2, cap - 1, cap, cap + 1, cap + 2):
        for n in (cap - 1, cap, cap + 1, cap + 2):
            out.append(_block(GE, 0, [1.0], 2.0 ** -22, 1.0 + M * 2.0 ** -22, n))
            out.append(_block(LE, 0, [1.75], -2.0 ** -22, 1.75 - M * 2.0 ** -22, n))
            out.append(_block(LT, 0, [1.75], -2.0 ** -22, 1.75 - M * 2.0 ** -22, n))
    return out


def _cases(cap):
    rng = np.random.default_rng(40)
    T = {}
    # ---- random chains: the download accumulation, drains to zero, drains to a threshold ----
    N = 60_000
    c = rng.uniform(0.05, 12.0, N).astype(np.float32).astype(np.float64) * 0.01
    x0 = np.where(rng.random(N) < 0.4, 0.0, rng.uniform(0, 20, N))
    thr = rng.choice([0.3, 0.75, 1.2, 1.85, 2.85, 4.3, 1.0, 2.5, 5.0, 8.0], N) * rng.choice([1.0, 2.0, 3.0, 4.0], N)
    xb = np.where(rng.random(N) < 0.5, rng.integers(1, 7, N) * 4.0, rng.uniform(0.001, 30, N))
    sd = rng.choice([0.01, 0.0125, 0.005, 0.02, 0.0075], N)
    t2 = rng.choice([20.0, 3.0, 5.0, 9.0, 6.0, 4.0, 16.0], N)          # powers of two among them
    xt = t2 + rng.uniform(0, 5, N)
    nr, nd = rng.integers(1, 3000, N), rng.integers(1, 4000, N)
    T["random"] = [_block(GE, 0, x0, c, thr, nr), _block(LE, 0, xb, -sd, 0.0, nd), _block(LE, 0, xb, -sd, 16 * sd, nd),
                   _block(LT, 0, xt, -sd, t2, nd)]
    T["bias"] = [_block(k, b, *a) for b in (4, -4) for k, a in ((GE, (x0, c, thr, nr)), (LE, (xb, -sd, 0.0, nd)),
                                                              (LT, (xt, -sd, t2, nd)))]
    # ---- ties (c = q*u + u/2 in the binade of x0) and thresholds on / one ulp around reachable values ----
    N = 30_000
    base = np.ldexp(1.0, rng.integers(-8, 6, N))
    u = base * 2.0 ** -52
    km = rng.integers(0, 1 << 20, N)
    ct = rng.integers(1, 1 << 44, N).astype(np.float64) * u + u / 2
    xu, xd = base * (1.0 + km * 2.0 ** -52), base * (2.0 - km * 2.0 ** -52)
    n = rng.integers(1, 500, N)
    tu = xu + ct * rng.integers(1, 600, N)
    td = np.maximum(xd - ct * rng.integers(1, 600, N), 0.0)
    T["ties"] = []
    for w in (0.0, np.inf, -np.inf):
        nudge = (lambda t: t) if w == 0.0 else (lambda t: np.nextafter(t, w))
        T["ties"] += [_block(GE, 0, xu, ct, nudge(tu), n), _block(LE, 0, xd, -ct, nudge(td), n),
                      _block(LT, 0, xd, -ct, nudge(td), n)]
    # ---- landings exactly on 2^e, from above and from below ----
    xs, cs, ns, xs2 = [], [], [], []
    for e in range(-6, 7):
        y = 2.0 ** e
        for cc in list(rng.uniform(0.001, 0.12, 25) * y) + [0.01, 0.0125, 0.005]:
            if not cc < y / 8:
                continue
            x1 = y * 1.5 - cc
            d = x1 - (x1 - cc)                    # the steady decrement of the binade [y, 2y)
            z1 = y * 0.75 + cc
            d2 = (z1 + cc) - z1                   # the steady increment of the binade [y/2, y)
            for j in (1, 2, 3, 7, 20):
                if y + j * d < 2 * y:
                    xs.append(y + j * d); cs.append(cc); ns.append(j + 50); xs2.append(y - j * d2)
    xs, cs, xs2 = np.array(xs), np.array(cs), np.array(xs2)
    T["pow2"] = [_block(LE, 0, xs, -cs, 0.0, ns), _block(LT, 0, xs, -cs, xs / 3, ns), _block(GE, 0, xs2, cs, 1e9, ns),
                 _block(LE, 0, [2.0299999999999994], -0.01, 0.0, 72)]
    # ---- subnormal neighbourhoods and 1e300 ----
    N = 6_000
    n = rng.integers(1, 2000, N)
    xs_, cs_ = rng.uniform(0, 1e-300, N), rng.uniform(1e-310, 1e-302, N)
    xh_, ch_ = rng.uniform(1e299, 1e300, N), rng.uniform(1e290, 1e297, N)
    T["general"] = [_block(GE, 0, xs_, cs_, rng.uniform(0, 1e-299, N), n), _block(LE, 0, xs_, -cs_, 0.0, n),
                    _block(LT, 0, xs_, -cs_, 1e-305, n), _block(GE, 0, xh_, ch_, 1.5e300, n),
                    _block(LE, 0, xh_, -ch_, 1e299, n), _block(LT, 0, xh_, -ch_, 1e299, n),
                    _block(GE, 0, [0.0, 1.0, 1e300], [0.01, 1e300, 1.0], 1e308, 50)]
    # ---- budgets of 0, 1 and one more than a segment takes ----
    T["budgets"] = []
    for nn in (0, 1, cap + 1):
        T["budgets"] += [_block(GE, 0, [0.0, 1.0, 1.0, 3.0, 1.5], [0.01, 2.0 ** -30, 2.0 ** -29 + 2.0 ** -52, 2.0 ** -27, 0.3],
                                [4.3, 10.0, 1.2, 3.9, 1.6], nn),
                         _block(LE, 0, [2.0 - 2.0 ** -52, 1.75, 20.0, 0.16], [-2.0 ** -30, -2.0 ** -29, -0.01, -0.01],
                                [0.0, 1.1, 0.16, 0.16], nn),
                         _block(LT, 0, [2.0 - 2.0 ** -52, 1.75, 24.0, 20.0], [-2.0 ** -30, -2.0 ** -29, -0.01, -0.01],
                                [1.5, 1.25, 20.0, 20.0], nn)]
    T["edges"] = _edges(cap)
    return T


@pytest.fixture(scope="module")
def cases(H):
    return _cases(H.settle_jump_cap())


REMAINDER, CANDIDATES = 0, 1            # abr_exact_jump.h: SettleKind
FORMS = pytest.mark.parametrize("form", [REMAINDER, CANDIDATES], ids=["remainder", "candidates"])


def run_block(H, block, form=REMAINDER):
    """One block through the harness, asserted: (value, additions, hit flag per case -- the naive loop's, since the harness
    compares -- and its stats: segments run, -, estimates repaired)."""
    kind, bias, x0, c, thr, n = block
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    N = len(x0)
    xo = np.zeros(N); ao = np.zeros(N, np.int32); ho = np.zeros(N, np.uint8); st = np.zeros(3, np.int64)
    bad = H.settle_check(C.c_int32(kind), C.c_int32(bias), C.c_int32(form), P(x0, C.c_double), P(c, C.c_double),
                         P(thr, C.c_double), P(n, C.c_int32), C.c_int64(N), P(xo, C.c_double), P(ao, C.c_int32),
                         P(ho, C.c_uint8), P(st, C.c_int64))
    why = {1: "chain != naive loop", 2: "a jump is not the longest legal one"}
    assert bad == -1, (f"kind {kind} bias {bias} form {form} case {bad}: {why.get(int(st[1]), st[1])}: x0={x0[bad]!r} "
                       f"c={c[bad]!r} thr={thr[bad]!r} n={n[bad]}")
    return xo, ao, ho, st


def _check(H, blocks, form):
    """Every block through the harness; returns (segments run, estimates repaired, hit flags of all blocks)."""
    seg = rep = 0
    hits = []
    for block in blocks:
        _, _, ho, st = run_block(H, block, form)
        seg += int(st[0]); rep += int(st[2])
        hits.append(ho)
    return seg, rep, np.concatenate(hits)


@FORMS
def test_random_chains(H, cases, form):
    seg, rep, hit = _check(H, cases["random"], form)
    assert rep == 0 and hit.mean() > 0.2 and seg > 4 * len(hit)          # the jumps really ran, none needed a repair


@FORMS
def test_ties_and_exact_thresholds(H, cases, form):
    assert _check(H, cases["ties"], form)[1] == 0


@FORMS
def test_landings_on_a_power_of_two(H, cases, form):
    assert _check(H, cases["pow2"], form)[1] == 0


@FORMS
def test_settlement_edges(H, cases, form):
    """r == 0, r == dm (non-strict LT), stops one ulp either side of a reachable value, and quotients within one of
    room and room + 1 -- at small budgets and at the segment cap."""
    seg, rep, hit = _check(H, cases["edges"], form)
    assert rep == 0 and hit.any() and not hit.all()


@FORMS
def test_budgets_of_zero_one_and_past_the_cap(H, cases, form):
    assert _check(H, cases["budgets"], form)[1] == 0


@FORMS
def test_subnormal_and_huge_inputs(H, cases, form):
    """Below the normal range chain_segment does not jump (every segment is one real addition: the harness counts a longest
    jump of 0 there); at 1e300 it jumps as anywhere else."""
    seg, rep, hit = _check(H, cases["general"], form)
    assert rep == 0 and hit.any()


@FORMS
def test_spoiled_estimates(H, cases, form):
    """+4 must take the repair path, -4 the short-jump path; both are still the naive loop bit for bit."""
    plus = [b for b in cases["bias"] if b[1] == 4]
    minus = [b for b in cases["bias"] if b[1] == -4]
    assert _check(H, plus, form)[1] > 1000
    assert _check(H, minus, form)[1] == 0


def test_sanitized_program_on_the_same_cases(cases, tmp_path):
    """The same table through a stand-alone build of the harness with AddressSanitizer and UndefinedBehaviorSanitizer.  The
    runtimes are linked statically: the program carries them itself."""
    src = os.path.join(_ROOT, "tests", "native", "chain_settle_harness.cpp")
    exe, data = str(tmp_path / "chain_settle_san"), str(tmp_path / "cases.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-DCHAIN_SETTLE_MAIN", "-I", os.path.join(_ROOT, "abrsimulator_amd", "csrc"),
                           src, "-o", exe])
    blocks = [(form, b) for form in (REMAINDER, CANDIDATES) for name in sorted(cases) for b in cases[name]]
    with open(data, "wb") as f:
        np.array([len(blocks)], np.int64).tofile(f)
        for form, (kind, bias, x0, c, thr, n) in blocks:
            np.array([kind, bias, form, 0], np.int32).tofile(f)
            np.array([len(x0)], np.int64).tofile(f)
            for a in (x0, c, thr, n):
                a.tofile(f)
    r = subprocess.run([exe, data], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.split()[:2] == ["ok", str(sum(len(b[2]) for _, b in blocks))], r.stdout[-3000:]
