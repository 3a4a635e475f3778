"""Every compiled instance of the MPC search kernel (mpc_select_kernel<H, BC, WVM>, tests/mpc_matrix.py) against the C
oracle, bit for bit: J, the flat arg-min, the action and the D9 history, through the predictor pre-kernel and through
the single kernel.  Then the shapes at the edges of the launch geometry and of int32, lanes whose objective is not
finite, and writes past n_lanes."""
import ctypes as C
import math
import threading

import numpy as np
import pytest
import torch

from conftest import load_golden
from mpc_matrix import MPC_CASES, case_id, lanes_per_block, mpc_instance

pytestmark = pytest.mark.gpu

V, L, MB, WR = 24, 4.0, 20.0, 4.3
ABR_E_UNSUPPORTED = -4


class _Info:
    pass


class _Player:
    def __init__(self, mpd, qoe, ci):
        self.mpd, self.qoe, self.ci = mpd, qoe, ci

    def get_mpd(self):
        return self.mpd

    def get_qoe_metric(self):
        return self.qoe

    def get_next_chunk_info(self):
        return self.ci


def _run(br, sz, H, wv, wr, chunk, prev, buf, hn, hs, mask=None, use_scratch=True, L_=L, mb=MB):
    """One next_bitrate() of BatchedMPCController with clip_horizon: (action, flat, J, hist_n, hist_s) as numpy."""
    import abrsimulator_amd as A
    mpd = A.MPD(len(br), L_, mb, 0.0, [A.Chunk(list(b), list(s)) for b, s in zip(br, sz)])
    ci = _Info()
    ci.chunk_number = torch.as_tensor(np.asarray(chunk, np.int32)).cuda()
    ci.previous_bitrate = torch.as_tensor(np.asarray(prev, np.int32)).cuda()
    ci.buffer_level = torch.as_tensor(np.asarray(buf, np.float64)).cuda()
    ci.hist_n = torch.as_tensor(np.array(hn, np.float64)).cuda()
    ci.hist_sum_inv = torch.as_tensor(np.array(hs, np.float64)).cuda()
    if mask is not None:
        ci.mask = torch.as_tensor(np.asarray(mask, np.uint8)).cuda()
    ctl = A.BatchedMPCController(_Player(mpd, A.QOEMetric(wr, wv, 0.0), ci), horizon=H, clip_horizon=True)
    ctl.use_scratch = use_scratch
    a = ctl.next_bitrate(want_details=True)
    torch.cuda.synchronize()
    return (a.cpu().numpy(), ctl.last_flat.cpu().numpy(), ctl.last_J.cpu().numpy(), ci.hist_n.cpu().numpy(),
            ci.hist_sum_inv.cpu().numpy())


def _expected(oracle, B, H, wv, wr, br, sz, chunk, prev, buf, hn, hs, L_=L, mb=MB):
    """Per lane from the oracle: (action, flat, J, hist_n, hist_s).  H_eff = min(H, V - chunk); a zero prediction is a
    lane the reference raises on: no decision, history untouched (include/abr_env.h: abr_mpc_select)."""
    N = len(chunk)
    act, flat, J = np.zeros(N, np.int32), np.zeros(N, np.int64), np.zeros(N)
    hn_o, hs_o = np.array(hn, np.float64), np.array(hs, np.float64)
    for i in range(N):
        pred, n2, s2 = oracle.mpc_predict_ns(H, hn[i], hs[i])
        if (pred == 0.0).any():
            act[i], flat[i], J[i] = -1, -1, np.nan
            continue
        hn_o[i], hs_o[i] = n2, s2
        he = min(H, len(br) - int(chunk[i]))
        cfg = oracle.mpc_cfg(B, he, len(br), L_, mb, wv, wr, 0.0)
        f, jm, _ = oracle.mpc_brute(cfg, br, sz, chunk[i], prev[i], buf[i], pred[:he], want_J=False)
        act[i], flat[i], J[i] = f // B ** (he - 1), f, jm
    return act, flat, J, hn_o, hs_o


def _inputs(B, H, seed, ties, n_lanes=None):
    """Lanes for one launch: N = k * lanes_per_block + 1 (a partial last workgroup); lanes 0 .. H-2 end the video
    within the horizon (clipped H_eff = 1 .. H-1), lane H-1 has an empty buffer, one lane's history is a single tiny
    value (every J = +inf, or at H >= 4 a prediction that underflows to 0: no decision), previous_bitrate spans
    [-B, B), and about a fifth of the other lanes are masked (never the last)."""
    rng = np.random.default_rng(seed)
    lpb = lanes_per_block(B, H)
    N = n_lanes or max(2, math.ceil((H + 6) / lpb)) * lpb + 1
    if ties:
        lad = np.arange(1, B + 1, dtype=np.float64) * 0.5
        lad[B - max(2, (B + 1) // 2):] = lad[-1]          # the upper rates are one rate: exact ties
        br = np.tile(lad, (V, 1))
        sz = br * L
        buf = np.where(rng.random(N) < 0.25, 0.0, rng.integers(0, 9, N) * 2.5)
        hn = np.full(N, 4.0)
        hs = hn / np.where(rng.random(N) < 0.5, 64.0, 0.25)
    else:
        lad = np.sort(rng.uniform(0.2, 6.0, B))
        br = lad[None, :] * rng.uniform(0.8, 1.2, (V, B))
        sz = br * L * rng.uniform(0.7, 1.3, (V, B))
        buf = np.where(rng.random(N) < 0.25, 0.0, rng.uniform(0, MB, N))
        hn = rng.integers(1, 30, N).astype(np.float64)
        hs = hn / rng.uniform(0.3, 5.0, N)
    chunk = rng.integers(0, V - H + 1, N).astype(np.int32)
    prev = rng.integers(-B, B, N).astype(np.int32)
    mask = (rng.random(N) > 0.2).astype(np.uint8)
    if N > 1:
        for j in range(min(H - 1, N - 1)):
            chunk[j] = V - 1 - j                          # H_eff = j + 1
            mask[j] = 1
        if H - 1 < N:
            buf[H - 1] = 0.0
        tiny = H if H < N - 1 else N - 2
        hn[tiny], hs[tiny], mask[tiny] = 1.0, 1.0 / 2.0e-308, 1
    mask[N - 1] = 1
    return br, sz, chunk, prev, buf, hn, hs, mask


def _check(oracle, B, H, wv, seed, ties=False, n_lanes=None):
    br, sz, chunk, prev, buf, hn, hs, mask = _inputs(B, H, seed, ties, n_lanes)
    m = mask.astype(bool)
    act, flat, J, hn_o, hs_o = _expected(oracle, B, H, wv, WR, br, sz, chunk[m], prev[m], buf[m], hn[m], hs[m])
    for scratch in (True, False):
        a, f, j, hn_g, hs_g = _run(br, sz, H, wv, WR, chunk, prev, buf, hn, hs, mask, use_scratch=scratch)
        assert np.array_equal(j[m], J, equal_nan=True), scratch
        assert np.array_equal(f[m].astype(np.int64), flat), scratch
        assert np.array_equal(a[m], act), scratch
        assert np.array_equal(hn_g[m], hn_o) and np.array_equal(hs_g[m], hs_o), scratch
        assert np.array_equal(hn_g[~m], hn[~m]) and np.array_equal(hs_g[~m], hs[~m]), scratch     # masked: untouched
    return br, sz, chunk[m], prev[m], buf[m], hn[m], hs[m], flat


@pytest.mark.parametrize("case", MPC_CASES, ids=[case_id(c) for c in MPC_CASES])
def test_instance_matches_oracle_seeded(oracle, case):
    B, H, wv = case
    br, sz, chunk, prev, buf, _, _, flat = _check(oracle, B, H, wv, seed=1000 * B + 10 * H + int(wv * 4))
    he = np.minimum(H, V - chunk)
    assert set(he.tolist()) >= set(range(1, H + 1))                 # every clipped horizon and the full one
    assert (buf == 0.0).any() and (prev < 0).any() and (flat == -1).sum() <= 1


@pytest.mark.parametrize("case", MPC_CASES, ids=[case_id(c) for c in MPC_CASES])
def test_instance_ties_resolve_to_the_first_combination(oracle, case):
    """The coinciding-rates ladder of test_mpc_gpu.py: many combinations tie bit for bit at the optimum, so a resolve
    (mpc_resolve_group) that forms a leaf in another operation order than the search would pick another one."""
    B, H, wv = case
    br, sz, chunk, prev, buf, hn, hs, flat = _check(oracle, B, H, wv, seed=7 + 1000 * B + 10 * H, ties=True)
    ties = 0
    cfg = oracle.mpc_cfg(B, H, V, L, MB, wv, WR, 0.0)
    full = np.flatnonzero((chunk + H <= V) & (flat >= 0))
    for i in full:
        pred, _, _ = oracle.mpc_predict_ns(H, hn[i], hs[i])
        _, jmin, J = oracle.mpc_brute(cfg, br, sz, chunk[i], prev[i], buf[i], pred)
        ties += int(np.isfinite(jmin) and (J == jmin).sum() > 1)
    assert len(full) and ties > 0


@pytest.mark.parametrize("H", range(2, 9))
def test_one_rate(oracle, H):
    """n_rates = 1: T = 1 thread per lane (D = 2 with B = 1 from horizon 3), 16 lanes per workgroup, one combination."""
    _check(oracle, 1, H, 1.0, seed=500 + H)


@pytest.mark.parametrize("H", [2, 3])
def test_sixteen_rates(oracle, H):
    """n_rates = 16: at H = 3 one lane fills the 256-thread workgroup and phase 5 runs with LPB * B = 16 threads."""
    _check(oracle, 16, H, 1.0, seed=600 + H)
    _check(oracle, 16, H, 1.0, seed=610 + H, ties=True)


def test_sixteen_rates_horizon_7(oracle):
    """16^7 = 268 435 456 combinations on two lanes (T = 256, one lane per workgroup), both paths, against the oracle
    (the two brute forces run in parallel threads)."""
    B, H = 16, 7
    rng = np.random.default_rng(716)
    lad = np.sort(rng.uniform(0.2, 6.0, B))
    br = lad[None, :] * rng.uniform(0.8, 1.2, (V, B))
    sz = br * L * rng.uniform(0.7, 1.3, (V, B))
    chunk = np.array([3, V - H], np.int32)
    prev = np.array([-1, 5], np.int32)
    buf = np.array([0.0, 12.5])
    hn = np.array([5.0, 12.0])
    hs = hn / np.array([1.3, 3.7])
    res = [None, None]

    def one(i):
        res[i] = _expected(oracle, B, H, 1.0, WR, br, sz, chunk[i:i + 1], prev[i:i + 1], buf[i:i + 1], hn[i:i + 1],
                           hs[i:i + 1])
    th = [threading.Thread(target=one, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    exp = [np.concatenate([r[k] for r in res]) for k in range(5)]
    for scratch in (True, False):
        a, f, j, hn_g, hs_g = _run(br, sz, H, 1.0, WR, chunk, prev, buf, hn, hs, use_scratch=scratch)
        assert np.array_equal(j, exp[2]) and np.array_equal(f.astype(np.int64), exp[1]) and np.array_equal(a, exp[0])
        assert np.array_equal(hn_g, exp[3]) and np.array_equal(hs_g, exp[4])


def _top_wins_tables(B):
    """A ladder 10, 20, .. 10 B with plenty of throughput (10^4): a step up the ladder gains 10 in quality, changes
    the variance term by at most 10 * wv (wv < 1) and the rebuffer term by far less than 1, so the top rate everywhere
    is the unique optimum whatever the previous bitrate."""
    br = np.tile(np.arange(1, B + 1, dtype=np.float64) * 10.0, (V, 1))
    return br, br * L


def test_largest_accepted_grid_14_to_the_8(oracle):
    """14^8 = 1 475 789 056 combinations, the largest grid validate_mpc accepts: flat indices run up to 14^8 - 1, close
    to INT32_MAX, through `flat * B + r` and `bf * B * B`.  Where the top rate wins everywhere the answer is the last
    combination; its J is the oracle's objective() of that combination (the tables' claim is checked by brute force
    at horizon 4)."""
    B, H, wv = 14, 8, 0.5
    br, sz = _top_wins_tables(B)
    chunk = np.array([2, 9], np.int32)
    prev = np.array([B - 1, 0], np.int32)
    buf = np.array([7.5, 0.0])
    hn = np.array([3.0, 3.0])
    hs = hn / 1.0e4
    small = oracle.mpc_cfg(B, 4, V, L, MB, wv, WR, 0.0)
    for i in range(2):
        pred, _, _ = oracle.mpc_predict_ns(4, hn[i], hs[i])
        assert oracle.mpc_brute(small, br, sz, chunk[i], prev[i], buf[i], pred, want_J=False)[0] == B ** 4 - 1
    cfg = oracle.mpc_cfg(B, H, V, L, MB, wv, WR, 0.0)
    top = np.full(H, B - 1, np.int32)
    J = []
    for i in range(2):
        pred, _, _ = oracle.mpc_predict_ns(H, hn[i], hs[i])
        J.append(oracle.lib().oracle_mpc_objective(
            C.byref(cfg), oracle._p(np.ascontiguousarray(br), C.c_double), oracle._p(np.ascontiguousarray(sz), C.c_double),
            C.c_int(int(chunk[i])), C.c_int(int(prev[i])), C.c_double(float(buf[i])), oracle._p(pred, C.c_double),
            oracle._p(top, C.c_int32)))
    last = B ** H - 1
    assert last == 1475789055 and last < 2 ** 31 - 1
    for scratch in (True, False):
        a, f, j, hn_g, _ = _run(br, sz, H, wv, WR, chunk, prev, buf, hn, hs, use_scratch=scratch)
        assert f.dtype == np.int32 and f.tolist() == [last, last], (scratch, f)
        assert a.tolist() == [B - 1, B - 1] and j.tolist() == J
        assert hn_g.tolist() == [3.0 + H] * 2


def _abi_buffers(N, extra, sentinel_i=-777, sentinel_f=-7.25):
    d = "cuda"
    return dict(action=torch.full((N + extra,), sentinel_i, dtype=torch.int32, device=d),
                flat=torch.full((N + extra,), sentinel_i, dtype=torch.int32, device=d),
                J=torch.full((N + extra,), sentinel_f, dtype=torch.float64, device=d))


def _abi_select(cfg, opt, t, br, sz, out, N):
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    args = [_lib.ptr(t["chunk"]), _lib.ptr(t["prev"]), _lib.ptr(t["buf"]), _lib.ptr(t["hn"]), _lib.ptr(t["hs"]),
            _lib.ptr(br), _lib.ptr(sz), None, _lib.ptr(out["action"]), _lib.ptr(out["flat"]), _lib.ptr(out["J"]),
            N, _lib.current_stream(torch.device("cuda"))]
    if opt is None:
        return lib.abr_mpc_select(C.byref(cfg), *args)
    return lib.abr_mpc_select_opt(C.byref(cfg), C.byref(opt), *args)


def test_grid_over_2e9_is_refused_before_any_launch():
    """15^8 = 2 562 890 625 > 2e9: ABR_E_UNSUPPORTED, and nothing is written (no kernel ran)."""
    from abrsimulator_amd import _lib
    B, H, N = 15, 8, 4
    cfg = _lib.MpcConfig()
    cfg.n_rates, cfg.horizon, cfg.video_length, cfg.clip_horizon = B, H, V, 1
    cfg.chunk_length, cfg.max_buffer, cfg.variance_weight, cfg.rebuffer_weight = L, MB, 1.0, WR
    br = torch.ones((V, B), dtype=torch.float64, device="cuda")
    t = dict(chunk=torch.zeros(N, dtype=torch.int32, device="cuda"), prev=torch.zeros(N, dtype=torch.int32, device="cuda"),
             buf=torch.zeros(N, dtype=torch.float64, device="cuda"), hn=torch.full((N,), 3.0, dtype=torch.float64,
                                                                                      device="cuda"),
             hs=torch.full((N,), 1.5, dtype=torch.float64, device="cuda"))
    out = _abi_buffers(N, 0)
    assert _abi_select(cfg, None, t, br, br, out, N) == ABR_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out["action"] == -777).all() and (out["flat"] == -777).all() and (out["J"] == -7.25).all()
    assert (t["hn"] == 3.0).all() and (t["hs"] == 1.5).all()


@pytest.mark.parametrize("B,H,wv", [(6, 5, 1.0), (4, 3, 0.0), (16, 3, 1.0), (1, 4, 1.0), (3, 2, 0.5), (9, 7, 1.0)])
def test_one_lane(oracle, B, H, wv):
    _check(oracle, B, H, wv, seed=900 + B * 10 + H, n_lanes=1)


@pytest.mark.parametrize("B,H,wv", [(6, 5, 1.0), (4, 3, 0.0), (16, 3, 1.0), (1, 4, 1.0), (3, 2, 0.5), (2, 8, 1.0),
                                    (7, 6, 0.5)])
@pytest.mark.parametrize("pre_kernel", [False, True])
def test_nothing_written_past_n_lanes(oracle, B, H, wv, pre_kernel):
    """The C ABI with every per-lane buffer 64 lanes longer than n_lanes and filled with sentinels (N = k * lanes per
    workgroup + 1, so the last workgroup is partial): lanes below N match the oracle, every sentinel past N is intact."""
    from abrsimulator_amd import _lib
    X = 64
    br_, sz_, chunk, prev, buf, hn, hs, _ = _inputs(B, H, 1200 + B * 10 + H, ties=False)
    N = len(chunk)
    cfg = _lib.MpcConfig()
    cfg.n_rates, cfg.horizon, cfg.video_length, cfg.clip_horizon = B, H, V, 1
    cfg.chunk_length, cfg.max_buffer, cfg.variance_weight, cfg.rebuffer_weight = L, MB, wv, WR

    def pad(a, fill):
        return torch.from_numpy(np.concatenate([a, np.full(X, fill, a.dtype)])).cuda()
    t = dict(chunk=pad(chunk, 0), prev=pad(prev, 0), buf=pad(buf, 1.0), hn=pad(hn, -3.5), hs=pad(hs, -9.25))
    out = _abi_buffers(N, X)
    br = torch.from_numpy(br_).cuda()
    sz = torch.from_numpy(sz_).cuda()
    opt, scratch = None, None
    if pre_kernel:
        opt = _lib.MpcOptions()
        need = C.c_size_t()
        _lib.check(_lib.lib().abr_mpc_scratch_bytes(C.byref(cfg), N, C.byref(need)))
        scratch = torch.full((need.value + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        opt.scratch_dev, opt.scratch_bytes = scratch.data_ptr(), need.value
    _lib.check(_abi_select(cfg, opt, t, br, sz, out, N))
    torch.cuda.synchronize()
    act, flat, J, hn_o, hs_o = _expected(oracle, B, H, wv, WR, br_, sz_, chunk, prev, buf, hn, hs)
    assert np.array_equal(out["J"].cpu().numpy()[:N], J, equal_nan=True)
    assert np.array_equal(out["flat"].cpu().numpy()[:N].astype(np.int64), flat)
    assert np.array_equal(out["action"].cpu().numpy()[:N], act)
    assert np.array_equal(t["hn"].cpu().numpy()[:N], hn_o) and np.array_equal(t["hs"].cpu().numpy()[:N], hs_o)
    assert (out["action"][N:] == -777).all() and (out["flat"][N:] == -777).all() and (out["J"][N:] == -7.25).all()
    assert (t["hn"][N:] == -3.5).all() and (t["hs"][N:] == -9.25).all()
    if pre_kernel:
        assert (scratch[need.value:] == 0xA5).all()


def test_nonfinite_objectives_match_the_reference():
    """tests/golden/mpc_nonfinite (the reference itself): an all-+inf grid gives combination 0, a grid holding NaN
    gives its first NaN (wr = 0: 0 * inf), an all-NaN grid combination 0, and a lane the reference raises on (a zero
    prediction) no decision with its history untouched.  Lanes of one (H, wr, wv) are one launch; both paths."""
    m, g = load_golden("mpc_nonfinite")
    B = m["n_rates"]
    groups = sorted({(int(h), float(r), float(v)) for h, r, v in zip(g["H"], g["wr"], g["wv"])})
    assert {mpc_instance(B, h, v) for h, _, v in groups} == {(3, 6, 1), (4, 6, 0), (4, 6, 1)}
    for H, wr, wv in groups:
        idx = np.flatnonzero((g["H"] == H) & (g["wr"] == wr) & (g["wv"] == wv))
        for scratch in (True, False):
            a, f, j, hn, hs = _run(g["br"], g["sz"], H, wv, wr, g["chunk"][idx], g["prev"][idx], g["buf"][idx],
                                   g["hist_n"][idx].astype(np.float64), g["hist_s"][idx], use_scratch=scratch,
                                   L_=m["chunk_length"], mb=m["max_buffer"])
            assert np.array_equal(a, g["action"][idx]), (H, wr, wv, scratch, a, g["action"][idx])
            assert np.array_equal(f, g["flat"][idx]), (H, wr, wv, scratch, f, g["flat"][idx])
            assert np.array_equal(j, g["Jmin"][idx], equal_nan=True), (H, wr, wv, scratch)
            assert np.array_equal(hn, g["hist_n_after"][idx].astype(np.float64)), (H, wr, wv, scratch)
            assert np.array_equal(hs, g["hist_s_after"][idx]), (H, wr, wv, scratch)
