"""The trace generator without a GPU (include/abr_env.h: abr_trace_synth): the kernels' own header built for the host
(tests/native/trace_synth_harness.cpp) -- as a sequential chain and as an emulation of the kernel's tiled wave scan --
against the independent numpy twin (tests/trace_synth_twin.py), bit for bit; the edge models; the algebra of the packed
state maps; the package's host mirror; the struct layout, the refusals and the probability -> threshold conversion."""
import ctypes as C

import numpy as np
import pytest

import trace_synth_twin as twin
from helpers import c_abi_output, native_harness

ONE = 1 << 32
LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 200, 1000]
BIG = (1 << 32) + 5


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(scope="module")
def H():
    h = native_harness("trace_synth_harness")
    h.th_map.restype = h.th_compose.restype = h.th_apply.restype = h.th_initial.restype = h.th_identity.restype = C.c_uint32
    h.th_map.argtypes = h.th_initial.argtypes = [C.c_void_p, C.c_uint32]
    h.th_compose.argtypes = h.th_apply.argtypes = [C.c_uint32, C.c_uint32]
    h.th_value.restype, h.th_value.argtypes = C.c_double, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    for f in (h.th_chain, h.th_scan):
        f.restype, f.argtypes = None, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p]
    return h


def struct_of(L, m, poison=True):
    """The ctypes abr_trace_model of a twin dict.  Entries the contract says are never read ([K, 8) of every array, the
    last entry of a cumulative row) are filled with values that would change the result if they were."""
    st, K = L.TraceModel(), m["K"]
    if poison:
        for s in range(8):
            st.level[s], st.spread[s], st.outage_thr[s], st.init_cum[s] = 1e300, 0.5, ONE // 2, 7
            for j in range(8):
                st.cum[s][j] = 3
    st.n_states, st.reserved_ = K, 0
    for s in range(K):
        st.level[s], st.spread[s] = m["level"][s], m["spread"][s]
        st.outage_thr[s], st.init_cum[s] = m["outage_thr"][s], m["init_cum"][s]
        for j in range(K):
            st.cum[s][j] = m["cum"][s][j]
        if poison:
            st.cum[s][K - 1], st.init_cum[K - 1] = 0, 0          # the last cumulative value is implicitly 2^32
    return st


def random_model(K, rng, outage=True):
    row = lambda: sorted(int(x) for x in rng.integers(0, ONE + 1, K))
    return twin.model_dict(rng.uniform(0.1, 6.0, K), rng.uniform(0.0, 1.0, K),
                           [int(x) for x in rng.integers(0, ONE // 4, K)] if outage else [0] * K, row(), [row() for _ in range(K)])


def harness_rows(H, L, m, seed, gen, g, n):
    st = struct_of(L, m)
    out = {}
    for name, fn in (("chain", H.th_chain), ("scan", H.th_scan)):
        x, s = np.full(n, -1.0), np.full(n, -1, np.int32)
        fn(C.byref(st), seed, gen, g, n, x.ctypes.data, s.ctypes.data)
        out[name] = (x, s)
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def check_valid(rows):
    from abrsimulator_amd import pack_traces
    for r in rows:
        assert np.isfinite(r).all() and (r >= 0).all()
        assert not np.signbit(r).any()
    flat, off, lens = pack_traces(rows, "cpu")
    assert flat.numel() == sum(len(r) for r in rows)


def test_harness_chain_and_emulated_scan_equal_the_twin(H, L):
    rng = np.random.default_rng(20)
    seeds = [0, 2 ** 64 - 1] + [int(x) for x in rng.integers(0, 2 ** 63, 2)]
    total, rows = 0, []
    for K in (1, 2, 3, 8):
        m = random_model(K, rng)
        for seed in seeds:
            for gen in (0, 1, 2 ** 32 - 1):
                ids = [int(rng.integers(0, 1000)), BIG + int(rng.integers(0, 2 ** 40))]
                for k, n in enumerate(LENGTHS * 2):
                    g = ids[k // len(LENGTHS)] + k
                    want, states = twin.trace(m, seed, gen, g, n)
                    got = harness_rows(H, L, m, seed, gen, g, n)
                    for name, (x, s) in got.items():
                        assert same_bits(x, want), (name, K, seed, gen, g, n)
                        assert np.array_equal(s, states), (name, K, seed, gen, g, n)
                    assert states.max() < K
                    total += n
                    if seed == 0:
                        rows.append(want)
    assert total >= 100_000
    check_valid(rows)


def edge(H, L, m, n=300, seed=11, gen=3, g=BIG):
    want, states = twin.trace(m, seed, gen, g, n)
    for name, (x, s) in harness_rows(H, L, m, seed, gen, g, n).items():
        assert same_bits(x, want) and np.array_equal(s, states), name
    check_valid([want])
    return want, states


def test_edge_models(H, L):
    lv = [0.5, 1.5, 3.0, 6.0]
    to = lambda j, K=4: [0] * j + [ONE] * (K - j)                                        # the cumulative row of "always j"
    # identity: every trace stays in its initial state
    m = twin.model_dict(lv, 0.2, [0] * 4, [ONE // 4, ONE // 2, 3 * (ONE // 4), ONE], [to(s) for s in range(4)])
    seen = set()
    for g in range(12):
        _, st = edge(H, L, m, g=g)
        assert (st == st[0]).all()
        seen.add(int(st[0]))
    assert len(seen) > 1
    # a cyclic permutation
    m = twin.model_dict(lv, 0.2, [0] * 4, to(0), [to((s + 1) % 4) for s in range(4)])
    _, st = edge(H, L, m)
    assert np.array_equal(st, (np.arange(300) + 1) % 4)
    # an absorbing state: 3 is left never, reached with probability 1/8 per sample from anywhere else
    leak = [7 * (ONE // 8)] * 3 + [ONE]
    m = twin.model_dict(lv, 0.2, [0] * 4, to(0), [[ONE // 2] + leak[1:], leak, leak, to(3)])
    _, st = edge(H, L, m, n=1000)
    first = int(np.argmax(st == 3))
    assert (st == 3).any() and (st[first:] == 3).all() and (st[:first] != 2).all()
    # spread 0: the samples are the levels; spread 1: the minimum stays >= 0
    m = random_model(4, np.random.default_rng(1), outage=False)
    m["spread"] = [0.0] * 4
    x, st = edge(H, L, m, n=1000)
    assert same_bits(x, np.asarray(m["level"])[st])
    m["spread"] = [1.0] * 4
    x, _ = edge(H, L, m, n=1000)
    assert x.min() >= 0.0 and x.max() <= 2 * max(m["level"])
    # outage_thr 2^32 on one state: its samples are +0.0, no sign bit; outage_thr 0: never an outage
    m = random_model(3, np.random.default_rng(2), outage=False)
    m["outage_thr"] = [0, ONE, 0]
    x, st = edge(H, L, m, n=1000)
    assert (st == 1).any() and (x[st == 1].view(np.uint64) == 0).all() and (x[st != 1] > 0).all()
    # a threshold row of all 0 (every w0 goes to the last state) and a row of all 2^32 (to state 0)
    m = twin.model_dict(lv, 0.2, [0] * 4, [0] * 4, [[0] * 4, [ONE] * 4, [ONE] * 4, [ONE] * 4])
    _, st = edge(H, L, m, n=200)
    assert np.array_equal(st, np.where(np.arange(200) % 2 == 0, 0, 3))              # s_-1 = 3 -> 0 -> 3 -> ...


def test_packed_maps_compose_associatively_and_agree_with_apply(H, L):
    rng = np.random.default_rng(5)
    ident = H.th_identity()
    assert ident == twin.IDENTITY and [H.th_apply(ident, s) for s in range(8)] == list(range(8))
    maps = [int(sum(int(x) << (3 * s) for s, x in enumerate(rng.integers(0, 8, 8)))) for _ in range(60)]
    for a, b, c in zip(maps[0::3], maps[1::3], maps[2::3]):
        ab, bc = H.th_compose(a, b), H.th_compose(b, c)
        assert H.th_compose(ab, c) == H.th_compose(a, bc)
        assert H.th_compose(a, ident) == a and H.th_compose(ident, a) == a
        for s in range(8):
            assert H.th_apply(ab, s) == H.th_apply(a, H.th_apply(b, s))            # a after b
    # trace_map is the map of the sample: state s goes where the twin's pick sends it; states >= K stay
    for K in (1, 3, 8):
        m = random_model(K, rng)
        st = struct_of(L, m)
        for w0 in [0, 1, ONE - 1, ONE // 2] + [int(x) for x in rng.integers(0, ONE, 40)]:
            F = H.th_map(C.byref(st), w0)
            assert [H.th_apply(F, s) for s in range(8)] == [twin.pick(m["cum"][s], K, w0) if s < K else s for s in range(8)]
            assert H.th_initial(C.byref(st), w0) == twin.pick(m["init_cum"], K, w0)
    # trace_value at the extremes of the noise word
    m = twin.model_dict([2.0, 4.0], [1.0, 0.5], [0, ONE // 2], [0, ONE], [[0, ONE]] * 2)
    st = struct_of(L, m)
    assert H.th_value(C.byref(st), 0, 0, 0) == 0.0 and H.th_value(C.byref(st), 0, 0xFFFFFFFF, 0) == 2.0 * (1.0 + (1.0 - 2.0 ** -23))
    assert H.th_value(C.byref(st), 1, 0x80000000, ONE // 2) == 4.0 and H.th_value(C.byref(st), 1, 0x80000000, ONE // 2 - 1) == 0.0


def test_mirror_equals_the_twin(L):
    import abrsimulator_amd as A
    models = [A.TraceModel([0.4, 1.2, 2.5, 5.0], spread=0.3, stay=0.8, outage=0.05),
              A.TraceModel([3.0]), A.TraceModel(np.linspace(0.2, 6, 8), spread=np.linspace(0, 1, 8), stay=0.5,
                                                outage=[0, 0.1, 0, 0.5, 0, 1.0, 0, 0], initial=[0.5, 0.5, 0, 0, 0, 0, 0, 0]),
              A.TraceModel([1.0, 2.0, 4.0], transition=[[0.1] * 2 + [0.8], [0.3, 0.3, 0.4], [1, 0, 0]])]
    ids = np.array([0, 1, 7, BIG, BIG + 1, 2 ** 40], np.uint64)
    for model in models:
        m = twin.from_package(model)
        for seed, gen in ((0, 0), (2 ** 64 - 1, 2 ** 32 - 1), (1234567, 1)):
            got = model.draw(seed, gen, ids, 200)
            assert got.shape == (len(ids), 200) and got.dtype == np.float64
            for r, g in enumerate(ids):
                assert same_bits(got[r], twin.trace(m, seed, gen, int(g), 200)[0]), (seed, gen, g)
            check_valid(list(got))
    model = models[0]
    whole = model.draw(9, 4, np.arange(20), 150)
    assert same_bits(model.draw(9, 4, 6 + np.arange(5), 150), whole[6:11])             # trace_id_base = 6
    assert same_bits(model.draw(9, 4, np.arange(20), 70), whole[:, :70])                # a shorter trace is a prefix
    assert not np.array_equal(model.draw(9, 5, np.arange(20), 150), whole)             # another generation
    assert not np.array_equal(model.draw(10, 4, np.arange(20), 150), whole)            # another seed


def test_struct_layout_matches_the_header(H, L):
    out = c_abi_output(r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(abr_trace_model), offsetof(abr_trace_model, n_states),
         offsetof(abr_trace_model, reserved_), offsetof(abr_trace_model, level), offsetof(abr_trace_model, spread),
         offsetof(abr_trace_model, outage_thr), offsetof(abr_trace_model, init_cum), offsetof(abr_trace_model, cum),
         ABR_TRACE_MAX_STATES);
  return 0;
}''')
    T = L.TraceModel
    assert list(map(int, out[0].split())) == [C.sizeof(T), T.n_states.offset, T.reserved_.offset, T.level.offset,
                                              T.spread.offset, T.outage_thr.offset, T.init_cum.offset, T.cum.offset,
                                              L.TRACE_MAX_STATES]
    assert C.sizeof(T) == 776 == H.th_model_size()


def test_model_refusals():
    import abrsimulator_amd as A
    ok = dict(levels=[1.0, 2.0, 3.0])
    A.TraceModel(**ok)
    bad = [dict(levels=[]), dict(levels=[1.0] * 9), dict(levels=[1.0, float("nan")]), dict(levels=[1.0, float("inf")]),
           dict(levels=[1.0, -0.5]), dict(levels=[0.0, 0.0]), dict(levels=[1.0, 0.0], outage=[1.0, 0.0]),
           dict(ok, spread=float("nan")), dict(ok, spread=-0.1), dict(ok, spread=1.5), dict(ok, spread=[0.1, 0.2]),
           dict(ok, outage=-0.1), dict(ok, outage=1.1), dict(ok, outage=float("nan")), dict(ok, stay=1.5), dict(ok, stay=-0.1),
           dict(ok, transition=[[1, 0], [0, 1]]), dict(ok, transition=[[0.5, 0.5, 0.1]] * 3),
           dict(ok, transition=[[1.5, -0.5, 0.0]] * 3), dict(ok, transition=[[float("nan"), 0.5, 0.5]] * 3),
           dict(ok, initial=[0.5, 0.5]), dict(ok, initial=[0.5, 0.6, 0.0]), dict(ok, initial=[-1.0, 1.0, 1.0])]
    for kw in bad:
        with pytest.raises(ValueError):
            A.TraceModel(**kw)
    ft = A.TraceModel.from_thresholds
    row = [0, ONE // 2, ONE]
    ft([1, 2, 3], 0.1, [0] * 3, row, [row] * 3)
    for args in (([1, 2, 3], 0.1, [0] * 3, [5, 4, ONE], [row] * 3),                   # a cumulative row that decreases
                 ([1, 2, 3], 0.1, [0] * 3, row, [row, [ONE, 0, ONE], row]),
                 ([1, 2, 3], 0.1, [0, ONE + 1, 0], row, [row] * 3),                  # a threshold above 2^32
                 ([1, 2, 3], 0.1, [0] * 3, row, [row, row, [0, ONE + 1, ONE]]),
                 ([1, 2, 3], 0.1, [0] * 3, row, [row] * 2),                           # a missing row
                 ([1, 0, 0], 0.1, [ONE, 0, 0], row, [row] * 3)):                      # no state that can be positive
        with pytest.raises(ValueError):
            ft(*args)
    # the last entry of a cumulative row is never read, here as in the C entry: anything there is accepted and stored as 2^32
    m = ft([1, 2, 3], 0.1, [0] * 3, [5, 9, 0], [[0, 7, 3], row, [1, 1, ONE + 99]])
    assert m.thresholds["initial"].tolist() == [5, 9, ONE] and m.thresholds["transition"].tolist() == [[0, 7, ONE], row, [1, 1, ONE]]


def test_c_entry_refusals(L):
    lib = L.lib()
    one = C.c_void_p(256)
    good = twin.model_dict([1.0, 2.0, 3.0], 0.25, [0, 5, ONE], [7, 9, ONE], [[0, ONE // 2, ONE]] * 3)

    def call(st, traces=one, off=one, lens=one, n=4, base=0):
        return lib.abr_trace_synth(C.byref(st) if st is not None else None, 1, 0, base, traces, off, lens, n, None)

    def model(**kw):
        st = struct_of(L, good, poison=False)
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def arr(field, idx, v, **kw):
        st = model(**kw)
        a = getattr(st, field)
        if isinstance(idx, tuple):
            a[idx[0]][idx[1]] = v
        else:
            a[idx] = v
        return st

    assert call(None) == -1 and b"NULL" in lib.abr_last_error()
    bad = [model(n_states=0), model(n_states=9), model(n_states=-1), model(reserved_=1),
           arr("level", 1, float("nan")), arr("level", 2, float("inf")), arr("level", 0, -1.0),
           arr("spread", 1, float("nan")), arr("spread", 0, -0.01), arr("spread", 2, 1.01),
           arr("outage_thr", 1, ONE + 1), arr("init_cum", 0, ONE + 1), arr("cum", (1, 1), ONE + 1),
           arr("init_cum", 0, 10), arr("cum", (2, 0), ONE)]
    for st in bad:
        # a bad struct is refused before the pointers are looked at
        assert lib.abr_trace_synth(C.byref(st), 1, 0, 0, None, None, None, 0, None) == -1
        assert b"trace model" in lib.abr_last_error(), lib.abr_last_error()
    dead = model()                                                  # the only positive levels are always in outage
    dead.level[0], dead.level[1], dead.outage_thr[2] = 0.0, 0.0, ONE
    assert call(dead) == -1 and b"positive" in lib.abr_last_error()
    st = model()
    for kw in (dict(traces=None), dict(off=None), dict(lens=None), dict(traces=C.c_void_p(260)), dict(off=C.c_void_p(257)),
               dict(lens=C.c_void_p(258)), dict(n=0), dict(n=-3), dict(base=-1)):
        assert call(st, **kw) == -1, kw
        assert b"trace synth" in lib.abr_last_error()
    # entries past K are never read: garbage there is not refused (the launch itself needs a device, so stop at a pointer)
    assert call(struct_of(L, good, poison=True), traces=None) == -1 and b"trace synth" in lib.abr_last_error()


def test_threshold_conversion():
    import abrsimulator_amd as A
    from abrsimulator_amd.tracesynth import threshold
    assert threshold(0.0) == 0 and threshold(1.0) == ONE and threshold(0.5) == ONE // 2
    assert threshold(2.0 ** -33) == 0                                   # 0.5 rounds to even
    assert threshold(3 * 2.0 ** -33) == 2 and threshold(2.0 ** -32) == 1 and threshold(1.0 - 2.0 ** -34) == ONE
    m = A.TraceModel([1.0, 2.0], outage=[2.0 ** -33, 0.5], transition=[[1.0, 0.0], [0.0, 1.0]], initial=[0.5, 0.5])
    th = m.thresholds
    assert th["outage"].tolist() == [0, ONE // 2] and th["initial"].tolist() == [ONE // 2, ONE]
    assert th["transition"].tolist() == [[ONE, ONE], [0, ONE]]
    # rows that sum to 1 only after rounding: their float64 cumulative sums end at 0.9999999999999999, the model is
    # accepted, and the last threshold is 2^32; the expected integers are written out
    for p, want in (([0.7, 0.2, 0.1], [3006477107, 3865470566, 4294967296]),
                    ([1 / 6] * 6, [715827883, 1431655765, 2147483648, 2863311531, 3579139413, 4294967296])):
        K = len(p)
        assert float(np.cumsum(np.asarray(p, np.float64))[-1]) == 0.9999999999999999 != 1.0
        m = A.TraceModel(np.arange(1, K + 1), transition=[p] * K, initial=p)
        assert m.thresholds["initial"].tolist() == want and m.thresholds["initial"][-1] == ONE
        assert all(m.thresholds["transition"][s].tolist() == want for s in range(K))
        st = m.struct()
        assert st.n_states == K and st.reserved_ == 0 and [int(st.cum[2][j]) for j in range(K)] == want
        assert [int(st.init_cum[j]) for j in range(K)] == want and [st.level[s] for s in range(K)] == list(range(1, K + 1))
    eighths = A.TraceModel([1.0] * 8, transition=[[0.125] * 8] * 8)
    assert eighths.thresholds["transition"][0].tolist() == [536870912, 1073741824, 1610612736, 2147483648, 2684354560,
                                                            3221225472, 3758096384, 4294967296]
    # a row whose sum is off by more than rounding is refused (test_model_refusals); one that is a few ulps off is not
    A.TraceModel([1.0, 2.0, 3.0], initial=[0.1, 0.2, 0.7000000000000001])


def test_env_case_cannot_time_out(oracle):
    """The corpus tests/test_trace_synth_gpu.py regenerates its small environment from: on the oracle alone, every trace
    of generations 1 and 2, from offsets across the trace, finishes an episode of the HIGHEST bitrate throughout -- the
    most bits any controller can ask for -- well inside the library's default tick bound, so no lane of those tests can
    end in ABR_DONE_TIMEOUT whatever it decides."""
    import abrsimulator_amd as A
    m = twin.from_package(A.TraceModel(**twin.ENV_MODEL))
    cfg = oracle.env_cfg(twin.ENV_LADDER, twin.ENV_L, twin.ENV_V, twin.ENV_MB, twin.ENV_SU, 1.0, twin.ENV_W, 1.0)
    for gen in (1, 2):
        traces = twin.corpus(m, twin.ENV_SEED, gen, twin.ENV_LENGTHS)
        tid = np.repeat(np.arange(len(traces)), 8).astype(np.int32)
        off = np.concatenate([np.linspace(0, n - 1, 8).astype(np.int32) for n in twin.ENV_LENGTHS])
        a = np.full((len(tid), twin.ENV_V), len(twin.ENV_LADDER) - 1, np.int32)
        _, _, fin, _ = oracle.env_batch(cfg, traces, tid, off, a)
        assert fin["chunk_id"].min() == twin.ENV_V and fin["ticks"].max() < twin.ENV_MAX_TICKS // 2, fin["ticks"].max()
