"""The lane fork and the beam selection without a GPU (include/abr_env.h: abr_env_fork, abr_beam_select): the kernels' row
table, index guard and per-thread move (csrc/abr_lane_jump.h: fork_table_init, fork_pair_ok, fork_move) compiled for the
host and run thread by thread as the two launches would, against the numpy twin byte for byte -- out-of-range and -1
indices are tested HERE and nowhere on a device; the select arithmetic against the twin; the scratch arithmetic; the
refusals that need no device; the search loop's twin against an exhaustive enumeration on the oracle."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers import native_harness
import fork_twin as T

P_ = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
SIZES = [(n, v) for n in (1, 63, 64, 65, 200) for v in (1, 5, 48)]


@pytest.fixture(scope="module")
def FH():
    h = native_harness("fork_harness")
    h.fh_table.restype = C.c_uint64
    h.fh_fork.restype = C.c_uint64
    return h


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


def table(FH, V, N, count):
    elem, rows, scr, ch = np.zeros(10, np.int32), np.zeros(10, np.int32), np.zeros(10, np.int64), C.c_int32()
    b = FH.fh_table(C.c_int32(V), C.c_int64(N), C.c_int64(count), P_(elem, C.c_int32), P_(rows, C.c_int32), P_(scr, C.c_int64),
                    C.byref(ch))
    return elem, rows, scr, ch.value, b


def world(V, N, seed, f64_off=512):
    """A random byte image: the workspace's per-lane regions behind f64_off, then a q_run column and an obs block, each
    at a 256-byte boundary, then a tail; and the ten region offsets in fork order."""
    offs = T.workspace_offsets(V, N, f64_off)
    last = offs["mpc_action"]
    q_off = T.align(last[0] + 4 * N) + 256
    obs_off = T.align(q_off + 8 * N) + 256
    total = T.align(obs_off + 4 * T.OBS_DIM * N) + 256
    ws = np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)
    off10 = np.array([offs[k][0] for k, _, _ in T.workspace_regions(V)] + [q_off, obs_off], np.int64)
    return ws, off10, q_off, obs_off


def twin_world(ws, V, N, q_off, obs_off, src, dst, f64_off=512, with_q=True, with_obs=True):
    out = T.fork_workspace(ws, V, N, f64_off, src, dst)
    if with_q:
        out[q_off:q_off + 8 * N] = T.fork_columns(ws[q_off:q_off + 8 * N].view(np.float64).view(np.uint64)[None], src, dst).view(np.uint8).reshape(-1)
    if with_obs:
        o = ws[obs_off:obs_off + 4 * T.OBS_DIM * N].view(np.uint32).reshape(T.OBS_DIM, N)
        out[obs_off:obs_off + 4 * T.OBS_DIM * N] = T.fork_columns(o, src, dst).view(np.uint8).reshape(-1)
    return out


def run_native(FH, ws, off10, V, N, src, dst):
    got = ws.copy()
    src = np.ascontiguousarray(src, np.int32)
    count = len(src)
    need = T.scratch_layout(V, count)[1]
    guard = 64
    scratch = np.full(need + guard, 0xA5, np.uint8)
    d = P_(np.ascontiguousarray(dst, np.int32), C.c_int32) if dst is not None else None
    used = FH.fh_fork(P_(got, C.c_uint8), P_(off10, C.c_int64), C.c_int32(V), C.c_int64(N), P_(src, C.c_int32), d,
                      C.c_int64(count), P_(scratch, C.c_uint8))
    assert used == need
    assert (scratch[need:] == 0xA5).all()                       # nothing written past the scratch the arithmetic promises
    return got


def mappings(rng, N):
    """Seeded (src, dst) mappings: identity-dst with skips and repeats, a permutation made of cycles, explicit dst with
    out-of-range and -1 indices on both sides, a source used many times, a lane copied onto itself."""
    out = []
    src = rng.integers(0, N, N).astype(np.int32)
    src[rng.random(N) < 0.3] = -1
    out.append((src, None))
    perm = rng.permutation(N).astype(np.int32)                   # every cycle of a random permutation, 1-cycles included
    out.append((perm, None))
    out.append((np.roll(np.arange(N, dtype=np.int32), 1), None))  # ONE cycle through every lane
    k = max(1, N // 2)
    dst = rng.permutation(N)[:k].astype(np.int32)
    src = np.full(k, rng.integers(0, N), np.int32)               # one source, many destinations
    out.append((src, dst))
    src = rng.integers(-3, N + 3, k).astype(np.int32)            # out of range on the source side
    dst = rng.permutation(N)[:k].astype(np.int32)
    bad = rng.random(k) < 0.3
    dst[bad] = rng.choice(np.array([-1, -7, N, N + 1, 2 ** 31 - 1, -2 ** 31], np.int64), int(bad.sum())).astype(np.int32)
    out.append((src, dst))
    out.append((np.array([N - 1, 0, -1, N, 0], np.int32), np.array([N - 1, 0, 0, 0, -1], np.int32)))   # self-copies, skips
    out.append((np.zeros(0, np.int32), None))
    out.append((np.arange(N + 300, dtype=np.int32) % N, np.concatenate([np.arange(N), np.full(300, -1)]).astype(np.int32)))  # count > N
    return out


def test_row_table_and_scratch_arithmetic(FH):
    assert FH.fh_regions() == 10 and FH.fh_rows_per_thread() >= 1
    rpt = FH.fh_rows_per_thread()
    for (N, V), count in itertools.product(SIZES, (0, 1, 63, 64, 65, 200, 1000, 2 ** 20)):
        elem, rows, scr, chunks, b = table(FH, V, N, count)
        want = T.workspace_regions(V) + [("q_run", 8, 1), ("obs", 4, 8)]
        assert elem.tolist() == [e for _, e, _ in want] and rows.tolist() == [r for _, _, r in want]
        offs, total = T.scratch_layout(V, count)
        assert scr.tolist() == offs and b == total, (N, V, count)
        assert all(o % 256 == 0 for o in offs) and total % 256 == 0
        assert chunks == sum((r + rpt - 1) // rpt for r in rows)
        assert total >= count * (8 * 8 + 8 + 15 * 4 + 2 + V + 8 * V + 32 + 4 + 8 + 32)
    assert table(FH, 65535, 7, 5)[3] <= 65535                    # the longest video still fits a launch's y extent


def test_index_guard(FH):
    for N in (1, 64, 200):
        for s, d in itertools.product((-2 ** 31, -2, -1, 0, 1, N - 1, N, N + 1, 2 ** 31 - 1), repeat=2):
            want = 0 <= s < N and 0 <= d < N
            assert bool(FH.fh_pair_ok(C.c_int64(s), C.c_int64(d), C.c_int64(N))) == want, (N, s, d)


@pytest.mark.parametrize("N,V", SIZES)
def test_fork_equals_the_twin_byte_for_byte(FH, N, V):
    rng = np.random.default_rng(1000 * N + V)
    ws, off10, q_off, obs_off = world(V, N, seed=N * 7 + V)
    for k, (src, dst) in enumerate(mappings(rng, N)):
        got = run_native(FH, ws, off10, V, N, src, dst)
        want = twin_world(ws, V, N, q_off, obs_off, src, dst)
        assert np.array_equal(got, want), (N, V, k, np.nonzero(got != want)[0][:8])
    # absent optional regions (no quality model, no obs): their bytes stay, the rest moves
    src, dst = mappings(rng, N)[1]
    off = off10.copy()
    off[8] = off[9] = -1
    got = run_native(FH, ws, off, V, N, src, dst)
    assert np.array_equal(got, twin_world(ws, V, N, q_off, obs_off, src, dst, with_q=False, with_obs=False))


def test_fork_touches_only_the_destination_columns(FH):
    N, V = 65, 5
    ws, off10, q_off, obs_off = world(V, N, seed=3)
    src, dst = np.array([4, 4, 9, -1, 70], np.int32), np.array([0, 64, 4, 5, 6], np.int32)
    got = run_native(FH, ws, off10, V, N, src, dst)
    changed = np.nonzero(got != ws)[0]
    allowed = T.lane_byte_mask(len(ws), V, N, 512, [0, 64, 4])
    allowed[q_off:q_off + 8 * N].reshape(N, 8)[[0, 64, 4]] = True
    allowed[obs_off:obs_off + 32 * N].reshape(8, N, 4)[:, [0, 64, 4]] = True
    assert allowed[changed].all() and len(changed) > 0
    # lane 4 received OLD lane 9 while lanes 0 and 64 received OLD lane 4: the gather ran before any scatter
    i32 = T.workspace_offsets(V, N, 512)["i32"][0]
    old, new = ws[i32:i32 + 60 * N].view(np.int32).reshape(15, N), got[i32:i32 + 60 * N].view(np.int32).reshape(15, N)
    assert np.array_equal(new[:, 0], old[:, 4]) and np.array_equal(new[:, 64], old[:, 4]) and np.array_equal(new[:, 4], old[:, 9])


def run_select(FH, G, beam, M, wl, R, rew, lat, done, valid, key=None):
    n = G * beam * M
    src, Ro, vo = np.full(n, -9, np.int32), np.full(n, np.nan), np.full(n, 9, np.uint8)
    FH.fh_select(C.c_int32(G), C.c_int32(beam), C.c_int32(M), C.c_double(wl), P_(R, C.c_double), P_(rew, C.c_float),
                 P_(lat, C.c_double) if lat is not None else None, P_(done, C.c_uint8), P_(valid, C.c_uint8),
                 P_(key, C.c_double) if key is not None else None, P_(src, C.c_int32), P_(Ro, C.c_double), P_(vo, C.c_uint8))
    return src, Ro, vo


def check_select(FH, G, beam, M, wl, R, rew, lat, done, valid, key=None):
    got = run_select(FH, G, beam, M, wl, R, rew, lat, done, valid, key)
    want = T.select(beam * M, M, wl, R, rew, lat, done, valid, key)
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint8) if g.dtype == np.float64 else g, w.view(np.uint8) if w.dtype == np.float64 else w)
    return got


@pytest.mark.parametrize("beam,M", [(1, 1), (1, 3), (2, 3), (4, 3), (9, 6), (81, 3), (64, 16)])
def test_select_equals_the_twin(FH, beam, M):
    rng = np.random.default_rng(beam * 100 + M)
    G, S = 5, beam * M
    n = G * S
    R = rng.choice([0.0, 1.5, 2.25, 40.0, -0.0], n) + rng.integers(0, 3, n)          # many exact ties
    rew = rng.choice(np.array([0.0, -0.0, 0.5, 4.3, 1e-3], np.float32), n)
    lat = rng.choice([3.0, 4.0, 4.01, 550.0], n)
    done = rng.choice(np.array([0, 0, 0, 1, 2, 4, 8, 3], np.uint8), n)
    valid = (rng.random(n) < 0.8).astype(np.uint8)
    valid[S:2 * S] = 0                                           # an all-invalid group
    valid[2 * S:3 * S] = 0
    valid[2 * S + S - 1] = 1; done[2 * S + S - 1] = 1            # one candidate, in the last slot, fewer than beam when beam > 1
    src, Ro, vo = check_select(FH, G, beam, M, 0.1, R, rew, lat, done, valid)
    assert (src[S:2 * S] == -1).all() and not vo[S:2 * S].any() and (Ro[S:2 * S] == 0).all()
    assert (src[2 * S:2 * S + M] == 3 * S - 1).all() and (src[2 * S + M:3 * S] == -1).all()
    key = rng.choice([np.nan, 1.0, 2.0, -0.0, 0.0, np.inf, -np.inf], n)
    check_select(FH, G, beam, M, 0.1, R, rew, None, done, valid, key)


def test_select_ties_zeros_and_nans(FH):
    M, beam = 3, 2
    S = beam * M
    one, z = np.ones(S, np.uint8), np.zeros(S, np.uint8)
    R, rew = np.zeros(S), np.zeros(S, np.float32)
    # every key equal: the slots decide, in order
    src, Ro, vo = check_select(FH, 1, beam, M, 0.1, R, rew, np.full(S, 5.0), z, one)
    assert src.tolist() == [0, 0, 0, 1, 1, 1] and vo.all()
    # -0.0 in a later slot does not beat +0.0 in an earlier one; NaN keys drop out
    key = np.array([np.nan, 0.0, -0.0, np.nan, 1.0, -0.0])
    src, _, vo = check_select(FH, 1, beam, M, 0.1, R, rew, None, z, one, key)
    assert src.tolist() == [1, 1, 1, 2, 2, 2]
    # a NaN reward makes the key NaN
    rew2 = rew.copy(); rew2[0] = np.nan
    src, _, _ = check_select(FH, 1, beam, M, 0.1, R, rew2, np.arange(S, dtype=np.float64), z, one)
    assert src.tolist() == [1, 1, 1, 2, 2, 2]
    # done bits: an ended episode stays, a time-out, a bad action and a bad argument drop out
    done = np.array([2, 4, 8, 1, 3, 0], np.uint8)
    src, _, vo = check_select(FH, 1, beam, M, 0.1, R, rew, np.arange(S, dtype=np.float64), done, one)
    assert src.tolist() == [3, 3, 3, 5, 5, 5]
    # R_new is the float64 sum of the float64 R and the float32 reward, the key adds wl * lat unfused
    R3 = np.array([0.1, 0.1, 0.1, 0.1, 0.1, 0.1]); r3 = np.full(S, np.float32(0.2)); l3 = np.array([3.0, 2.0, 1.0, 0.5, 7.0, 9.0])
    _, Ro, _ = check_select(FH, 1, beam, M, 0.1, R3, r3, l3, z, one)
    assert Ro[0] == np.float64(0.1) + np.float64(np.float32(0.2))
    # one valid candidate and a beam of two: the second survivor's slots are empty
    v1 = z.copy(); v1[4] = 1
    src, Ro, vo = check_select(FH, 1, beam, M, 0.1, R, rew, l3, z, v1)
    assert src.tolist() == [4, 4, 4, -1, -1, -1] and vo.tolist() == [1, 1, 1, 0, 0, 0]


def test_symbols_bound_and_documented(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "abr_env.h")).read()
    for sym in ("abr_env_fork_scratch_bytes", "abr_env_fork", "abr_beam_select"):
        assert hasattr(lib, sym) and sym in {n for n, _, _ in L.SYMBOLS} and sym + "(" in header
    assert lib.abr_abi_version() == 4                            # additive
    import abrsimulator_amd as A
    assert A.HindsightSearch is __import__("abrsimulator_amd.search", fromlist=["x"]).HindsightSearch
    assert callable(A.BatchedABREnv.fork)


def test_refusals_that_need_no_device(L):
    lib = L.lib()
    one, n = C.c_void_p(256), C.c_size_t(7)
    E = lambda: lib.abr_last_error()
    assert lib.abr_env_fork_scratch_bytes(None, 4, None) == -1 and b"bytes_out" in E()
    assert lib.abr_env_fork_scratch_bytes(None, -1, C.byref(n)) == -1 and b"count" in E()
    assert lib.abr_env_fork_scratch_bytes(None, 2 ** 31, C.byref(n)) == -1 and b"count" in E()
    assert lib.abr_env_fork_scratch_bytes(None, 4, C.byref(n)) == -1 and b"env is NULL" in E()
    assert n.value == 7
    # the arguments before the handle
    assert lib.abr_env_fork(None, None, None, 4, one, 1 << 20, None, None) == -1 and b"src_dev" in E()
    assert lib.abr_env_fork(None, one, None, -1, one, 1 << 20, None, None) == -1 and b"count" in E()
    assert lib.abr_env_fork(None, one, None, 4, None, 1 << 20, None, None) == -1 and b"scratch_dev" in E()
    assert lib.abr_env_fork(None, one, None, 4, C.c_void_p(264), 1 << 20, None, None) == -1 and b"256-byte" in E()
    assert lib.abr_env_fork(None, one, None, 4, one, 1 << 20, None, None) == -1 and b"env is NULL" in E()
    sel = lambda *a: lib.abr_beam_select(*a)
    ok = [one] * 5 + [None] + [one] * 3 + [None]
    assert sel(-1, 2, 3, 0.1, *ok) == -1 and b"n_groups" in E()
    assert sel(1, 0, 3, 0.1, *ok) == -1 and b"beam" in E()
    assert sel(1, 2, 0, 0.1, *ok) == -1 and sel(1, 2, 17, 0.1, *ok) == -1 and b"n_rates" in E()
    assert sel(1, 342, 3, 0.1, *ok) == -4 and b"1024" in E()
    assert sel(1, 65, 16, 0.1, *ok) == -4
    for k in (0, 1, 3, 4, 6, 7, 8):
        a = list(ok); a[k] = None
        assert sel(1, 2, 3, 0.1, *a) == -1 and b"NULL" in E(), k
    a = list(ok); a[2] = None
    assert sel(1, 2, 3, 0.1, *a) == -1 and b"lat_dev" in E()
    assert sel(0, 2, 3, 0.1, *ok) == 0                           # no group: nothing is launched


# ---- the search loop's twin on the oracle: exhaustive width finds the optimum, the widths are monotone ----
LADDER, V, CL, MB, SU, W, WQ = [0.3, 1.2, 2.85], 5, 4.0, 20.0, 4.0, [4.3, 1.0, 1.0, 0.1], 3.0


def test_search_twin_on_the_oracle(oracle):
    from oracle.oracle import step_rewards
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.5, 6.0, int(rng.integers(30, 200))) for _ in range(8)]
    G, M = 6, len(LADDER)
    cfg = oracle.env_cfg(LADDER, CL, V, MB, SU, 1.0, W, 1.0)
    u = np.log(np.array(LADDER) / LADDER[0])
    seqs = np.array(list(itertools.product(range(M), repeat=V)), np.int32)
    index = {tuple(s): k for k, s in enumerate(seqs.tolist())}
    per_group = []
    for g in range(G):
        tid, off = np.full(len(seqs), g % 8, np.int32), np.full(len(seqs), (g * 7) % 13, np.int32)
        steps, _, fin, _ = oracle.env_batch(cfg, traces, tid, off, seqs)
        r = step_rewards(steps["rebuffer_time"], steps["start_up_time"], fin["rebuffer_time"], fin["start_up_time"], seqs, W,
                         ladder=LADDER, dtype=np.float64)
        r = (r - WQ * u[seqs]).astype(np.float32)
        lat = np.concatenate([steps["average_latency"][:, 1:], fin["average_latency"][:, None]], 1)
        per_group.append((r, lat, fin["qoe"] - WQ * u[seqs].sum(1)))

    def evaluate(g, prefixes):
        r, lat, qoe = per_group[g]
        t = len(prefixes[0]) - 1
        k = np.array([index[tuple(p) + (0,) * (V - len(p))] for p in prefixes])     # a step depends on its prefix only
        return r[k, t], lat[k, t], np.full(len(k), 1 if t == V - 1 else 0, np.uint8), qoe[k]

    best = {}
    for beam in (1, 2, 4, 81):
        q, a, _ = T.search(evaluate, G, beam, M, V, W[3])
        best[beam] = q
        for g in range(G):
            assert q[g] == per_group[g][2][index[tuple(a[:, g].tolist())]]            # the actions are the episode scored
    opt = np.array([per_group[g][2].min() for g in range(G)])
    assert np.array_equal(best[81], opt)
    assert (best[1] >= best[2]).all() and (best[2] >= best[4]).all() and (best[4] >= best[81]).all()
    assert (best[1] > best[81]).any()
