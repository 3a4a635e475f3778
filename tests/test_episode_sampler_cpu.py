"""The episode sampler without a GPU: the device draw (csrc/abr_lane_jump.h: episode_assign) compiled for the host against
an independent numpy twin of the contract in include/abr_env.h, on seeded cases and their edges; the package's host mirror
(abrsimulator_amd/episodes.py) against the same twin; the exported symbols, the ctypes mirror of abr_episode_sampler against
the header, and the refusals that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers import c_abi_output, native_harness
import policy_twin as T
from sampler_twin import twin

P_ = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
M32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def EH():
    return native_harness("episode_harness")


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


def device_draw(EH, seed, lanes, eps, trace_len, pool=None, span=0):
    lanes = np.ascontiguousarray(lanes, np.uint64)
    eps = np.ascontiguousarray(np.asarray(eps, np.int64) & M32, np.uint32)
    tl = np.ascontiguousarray(trace_len, np.int32)
    n = lanes.size
    t, off = np.zeros(n, np.int32), np.zeros(n, np.int32)
    pl = np.ascontiguousarray(pool, np.int32) if pool is not None else None
    EH.eh_draw(C.c_int64(n), C.c_uint64(seed), P_(pl, C.c_int32) if pl is not None else None,
               C.c_int32(len(pool) if pool is not None else 0), C.c_int32(span), C.c_int32(tl.size), P_(tl, C.c_int32),
               P_(lanes, C.c_uint64), P_(eps, C.c_uint32), P_(t, C.c_int32), P_(off, C.c_int32))
    return t, off


def cases():
    """(seed, lanes, episodes, trace_len, pool, span) covering the edges the contract names, then seeded bulk."""
    rng = np.random.default_rng(20261016)
    big = np.array([2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 40 + 3, 2 ** 63 + 11, 2 ** 64 - 1], np.uint64)
    yield 1, np.arange(2000, dtype=np.uint64), np.zeros(2000, np.int64), [17], None, 0            # n_traces = 1
    yield 2, np.arange(2000, dtype=np.uint64), np.arange(2000) % 5, [3, 900, 40], [1], 0          # a pool of one
    yield 3, np.arange(2000, dtype=np.uint64), np.arange(2000), [50, 60, 70], None, 1             # span 1: offset 0
    yield 4, np.arange(2000, dtype=np.uint64), np.arange(2000), [5, 6, 7, 800], None, 10 ** 6     # span above every length
    yield 5, np.repeat(big, 300), np.tile(np.arange(300), big.size), [9, 11, 13], None, 0       # lane ids >= 2^32
    yield 6, np.arange(1000, dtype=np.uint64), np.full(1000, 2 ** 31 - 1), [1, 2, 3], [2, 0, 2], 2  # episode 2^31-1
    yield 2 ** 64 - 1, np.arange(1000, dtype=np.uint64), np.arange(1000), [1, 1, 1], None, 0     # length-1 traces
    for k in range(18):
        nt = int(rng.integers(1, 400))
        tl = rng.integers(1, 5000, nt)
        pool = rng.integers(0, nt, int(rng.integers(1, 64))).tolist() if k % 3 == 0 else None
        span = int(rng.choice([0, 1, 2, 37, 4096, 10 ** 5]))
        lanes = rng.integers(0, 2 ** 63, 5000, dtype=np.uint64) if k % 2 else np.arange(5000, dtype=np.uint64)
        eps = rng.integers(0, 2 ** 31, 5000)
        yield int(rng.integers(0, 2 ** 63)), lanes, eps, tl, pool, span


def test_device_draw_equals_the_twin(EH):
    total = 0
    for seed, lanes, eps, tl, pool, span in cases():
        got = device_draw(EH, seed, lanes, eps, tl, pool, span)
        want = twin(seed, lanes, eps, tl, pool, span)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (seed, span)
        tl_ = np.asarray(tl)
        assert (got[1] >= 0).all() and (got[1] < tl_[got[0]]).all()
        if span > 0:
            assert (got[1] < span).all()
        if pool is not None:
            assert np.isin(got[0], pool).all()
        total += len(lanes)
    assert total >= 100_000


def test_edges_hold_what_they_promise(EH):
    t, off = device_draw(EH, 3, np.arange(5000, dtype=np.uint64), np.arange(5000), [50, 60, 70], None, 1)
    assert (off == 0).all() and set(t.tolist()) == {0, 1, 2}
    t, off = device_draw(EH, 1, np.arange(500, dtype=np.uint64), np.zeros(500), [17])
    assert (t == 0).all() and len(set(off.tolist())) > 10
    # the draw never shares the random policy's counters: step 0xFFFFFFFF vs chunk ids, same seed and lane
    w = T.philox4(5, np.arange(10, dtype=np.uint64), 0xFFFFFFFF, np.zeros(10, np.uint64))[0]
    v = T.philox4(5, np.arange(10, dtype=np.uint64), 0, np.zeros(10, np.uint64))[0]
    assert not np.array_equal(w, v)


def test_host_mirror_equals_the_twin():
    from abrsimulator_amd.episodes import EpisodeSampler
    for seed, lanes, eps, tl, pool, span in cases():
        got = EpisodeSampler(seed, pool, span).draw(lanes, eps, tl)
        want = twin(seed, lanes, eps, tl, pool, span)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (seed, span)
    # broadcasting: one lane, many episodes
    t, off = EpisodeSampler(9).draw(np.uint64(2 ** 33), np.arange(7), [4, 5, 6])
    assert t.shape == (7,) and np.array_equal(t, twin(9, np.full(7, 2 ** 33, np.uint64), np.arange(7), [4, 5, 6])[0])


def test_host_mirror_refuses_bad_pools_and_spans():
    from abrsimulator_amd.episodes import EpisodeSampler
    with pytest.raises(ValueError):
        EpisodeSampler(1, offset_span=-1)
    with pytest.raises(ValueError):
        EpisodeSampler(1, pool=[])
    with pytest.raises(ValueError):
        EpisodeSampler(1, pool=[0, -1])
    with pytest.raises(ValueError):
        EpisodeSampler(1, pool=[0.5])
    with pytest.raises(ValueError):
        EpisodeSampler(1, pool=[0, 3]).draw([0], [0], [10, 10, 10])
    with pytest.raises(ValueError):
        EpisodeSampler(1, pool=[3]).check(3)
    EpisodeSampler(1, pool=[2]).check(3)


def test_symbols_exported(L):
    lib = L.lib()
    for sym in ("abr_env_set_episode_sampler", "abr_env_get_episode"):
        assert hasattr(lib, sym)
        assert sym in {n for n, _, _ in L.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "abr_env.h")).read()
    assert "abr_env_set_episode_sampler(" in hdr and "abr_env_get_episode(" in hdr


def test_sampler_struct_layout_matches_header(L, EH):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(abr_episode_sampler), offsetof(abr_episode_sampler, seed),
         offsetof(abr_episode_sampler, pool), offsetof(abr_episode_sampler, n_pool),
         offsetof(abr_episode_sampler, offset_span));
  return 0;
}'''
    got = list(map(int, c_abi_output(prog)[0].split()))
    S = L.EpisodeSampler
    assert got == [C.sizeof(S), S.seed.offset, S.pool.offset, S.n_pool.offset, S.offset_span.offset] == [24, 0, 8, 16, 20]
    assert EH.eh_sampler_size() == 24


def test_set_episode_sampler_refuses_before_the_handle(L):
    """The struct is checked before the handle: these refusals need neither a device nor an environment."""
    lib = L.lib()
    pool = (C.c_int32 * 2)(0, 1)
    s = L.EpisodeSampler(seed=1, pool=C.cast(pool, C.c_void_p), n_pool=0, offset_span=0)
    assert lib.abr_env_set_episode_sampler(None, C.byref(s)) == -1
    assert b"n_pool" in lib.abr_last_error()
    s = L.EpisodeSampler(seed=1, pool=None, n_pool=0, offset_span=-3)
    assert lib.abr_env_set_episode_sampler(None, C.byref(s)) == -1
    assert b"offset_span" in lib.abr_last_error()
    s = L.EpisodeSampler(seed=1, pool=None, n_pool=0, offset_span=0)
    assert lib.abr_env_set_episode_sampler(None, C.byref(s)) == -1      # a valid struct: then the NULL handle
    assert b"env is NULL" in lib.abr_last_error()
    assert lib.abr_env_get_episode(None, None, None, None, None) == -1
