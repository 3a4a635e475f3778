"""Forecast MPC without a GPU (include/abr_env.h: abr_plan_config, abr_env_plan_select, abr_env_step_plan): the lookahead's
walk with the root's cursor on a one-sample forecast (csrc/abr_lane_jump.h: plan_cursor, plan_usable around look_subtree)
built for the host next to a brute-force loop over flat indices that steps lanej_step on an explicit constant trace, bit
for bit on action, key and every q; the same walk against the existing lookahead walk on corpora whose traces are
constant; the built-in forecast (plan_forecast) against the numpy twin of RobustMPC's estimate, P and state bytes; the
struct, the symbols, the refusals that need no device and the Python ValueErrors."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers import c_abi_output, native_harness
import robust_twin as RT
import trace_families as TF

P_ = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t)) if a is not None else None
W = (4.3, 1.0, 1.0, 0.1)                                        # wr, wv, ws, wl
LADDER16 = [0.3, 0.5, 0.75, 1.0, 1.2, 1.5, 1.85, 2.3, 2.85, 3.5, 4.3, 5.2, 6.0, 7.0, 8.0, 9.5]
MAX_LEAVES = 65536
CONST_LEN = 7                                                   # the brute force's explicit constant trace


def ladder(M):
    return [LADDER16[(16 * k) // M] for k in range(M)]


@pytest.fixture(scope="module")
def PH():
    h = native_harness("plan_harness")
    h.la_create.restype = C.c_void_p
    return h


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


class Ctx:
    def __init__(self, PH, M, V, max_ticks, lad=None):
        self.PH, self.M, self.V = PH, M, V
        self.ladder = lad or ladder(M)
        self.h = C.c_void_p(PH.la_create(C.c_double(1.0), C.c_double(4.0), C.c_double(1.0), C.c_int32(V), C.c_double(20.0),
                                         C.c_double(8.0), C.c_int32(max_ticks), P_(np.array(self.ladder, np.float64), C.c_double),
                                         C.c_int32(M), P_(np.array(W, np.float64), C.c_double)))
        self._u = None

    def quality(self, wq, u):
        self._u = None if u is None else np.ascontiguousarray(u, np.float64)
        self.PH.la_set_quality(self.h, C.c_double(wq), P_(self._u, C.c_double))

    def _args(self, traces, tid, off, prefix):
        from oracle.oracle import pack_traces
        flat, toff, tlen = pack_traces(traces)
        prefix = np.ascontiguousarray(prefix, np.int32)
        n, n_prefix = prefix.shape
        out = dict(action=np.zeros(n, np.int32), key=np.zeros(n), q=np.zeros((self.M, n)), done=np.zeros(n, np.uint8))
        head = (P_(flat, C.c_double), P_(toff, C.c_int64), P_(tlen, C.c_int32), P_(np.asarray(tid, np.int32), C.c_int32),
                P_(np.asarray(off, np.int32), C.c_int32), P_(prefix, C.c_int32), C.c_int32(n_prefix), C.c_int32(n))
        tail = (P_(out["action"], C.c_int32), P_(out["key"], C.c_double), P_(out["q"], C.c_double), P_(out["done"], C.c_uint8))
        return head, tail, out, n

    def plan(self, mode, horizon, traces, tid, off, prefix, forecast, pos=None):
        """mode 0: the planner's walk; 1: brute force on an explicit constant trace entered at pos."""
        head, tail, out, n = self._args(traces, tid, off, prefix)
        forecast = np.ascontiguousarray(forecast, np.float64)
        pos = np.zeros(n, np.int32) if pos is None else np.ascontiguousarray(pos, np.int32)
        assert forecast.shape == (n,)
        rc = self.PH.pl_run(self.h, C.c_int32(mode), C.c_int32(horizon), *head, P_(forecast, C.c_double), C.c_int32(CONST_LEN),
                            P_(pos, C.c_int32), *tail)
        assert rc == 0
        return out

    def lookahead(self, horizon, traces, tid, off, prefix):
        """the existing lookahead walk on the real traces (la_run, mode 0)"""
        head, tail, out, n = self._args(traces, tid, off, prefix)
        assert self.PH.la_run(self.h, C.c_int32(0), C.c_int32(horizon), *head, *tail, None, None, None) == 0
        return out

    def close(self):
        self.PH.la_destroy(self.h)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same(a, b, what):
    assert np.array_equal(a["action"], b["action"]), what
    assert np.array_equal(a["done"], b["done"]), what
    assert np.array_equal(bits(a["key"]), bits(b["key"])), what          # one NaN pattern on both sides; -0.0 != +0.0
    assert np.array_equal(bits(a["q"]), bits(b["q"])), what


def forecasts(rng, n):
    """log-uniform over 1e-12 .. 1e6, the two ends included"""
    f = 10.0 ** rng.uniform(-12.0, 6.0, n)
    f[rng.integers(0, n)] = 1e-12
    f[rng.integers(0, n)] = 1e6
    return f


# ---- the walk on a forecast against brute force on an explicit constant trace ----
V_DEEP = 11


@pytest.mark.parametrize("M", [1, 2, 3, 6, 16])
def test_forecast_walk_equals_brute_force_on_a_constant_trace(PH, M):
    seen = dict(answers=0, none=0, shrunk=0, actions=set())
    ctx = Ctx(PH, M, V_DEEP, max_ticks=120_000)
    try:
        for fi, family in enumerate(TF.FAMILIES[:3]):
            rng = np.random.default_rng([M, fi, 78])
            traces = TF.make_pool(family, rng, [int(rng.integers(20, 120)) for _ in range(4)])
            for H in range(1, 9):
                leaves = M ** H
                if leaves > MAX_LEAVES:
                    continue
                n = int(max(2, min(8, 20_000 // leaves)))
                for c in (0, 1, 2, V_DEEP - 1):
                    tid = rng.integers(0, len(traces), n).astype(np.int32)
                    off = rng.integers(0, 200, n).astype(np.int32)
                    prefix = rng.integers(0, M, (n, c)).astype(np.int32).reshape(n, c)
                    F = forecasts(rng, n)
                    w = ctx.plan(0, H, traces, tid, off, prefix, F)
                    b = ctx.plan(1, H, traces, tid, off, prefix, F, pos=rng.integers(0, 100, n))
                    same(w, b, (family, M, H, c))
                    live = w["done"] == 0
                    seen["answers"] += int((w["action"] >= 0).sum())
                    seen["none"] += int((live & (w["action"] < 0)).sum())
                    seen["shrunk"] += int(c == V_DEEP - 1 and H > 1)
                    seen["actions"] |= set(w["action"].tolist())
    finally:
        ctx.close()
    assert seen["answers"] > 0 and seen["shrunk"] > 0
    assert seen["none"] > 0                                     # 1e-12: 4 Mbit never arrive within max_ticks
    if M > 1:
        assert len(seen["actions"] - {-1}) > 1


def test_forecast_walk_equals_brute_force_with_a_quality_model(PH):
    M, H = 3, 3
    ctx = Ctx(PH, M, 6, max_ticks=60_000)
    try:
        rng = np.random.default_rng(6)
        traces = TF.make_pool("outage", rng, [60, 90, 120])
        u = np.tile(np.log(np.array(ctx.ladder) / ctx.ladder[0]), (6, 1)) * rng.uniform(0.5, 1.5, (6, 1))
        n = 48
        tid, off = rng.integers(0, 3, n), rng.integers(0, 60, n)
        prefix = rng.integers(0, M, (n, 2))
        F = forecasts(rng, n)
        plain = ctx.plan(0, H, traces, tid, off, prefix, F)
        ctx.quality(3.0, u)
        w, b = ctx.plan(0, H, traces, tid, off, prefix, F), ctx.plan(1, H, traces, tid, off, prefix, F)
        same(w, b, "quality")
        assert not np.array_equal(bits(w["key"]), bits(plain["key"]))       # the keys carry the term
        assert (w["action"] > plain["action"]).any()                        # and it pays for higher rates
        ctx.quality(0.0, None)
        same(ctx.plan(0, H, traces, tid, off, prefix, F), plain, "model removed")
    finally:
        ctx.close()


def test_unusable_forecasts_take_no_decision(PH):
    ctx = Ctx(PH, 3, 6, max_ticks=60_000)
    try:
        traces = [np.full(50, 2.0)]
        F = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 2.0, np.finfo(np.float64).max, 5e-324])
        n = len(F)
        assert [PH.pl_usable(C.c_double(f)) for f in F] == [0, 0, 0, 0, 0, 0, 1, 1, 1]
        w = ctx.plan(0, 2, traces, np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 1), np.int32), F)
        b = ctx.plan(1, 2, traces, np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 1), np.int32), F)
        same(w, b, "unusable")
        assert (w["done"] == 0).all()
        assert (w["action"][:6] == -1).all() and np.isnan(w["key"][:6]).all() and np.isnan(w["q"][:, :6]).all()
        assert w["action"][6] >= 0 and np.isfinite(w["key"][6])
        assert w["action"][8] == -1                              # usable, but every sequence times out
    finally:
        ctx.close()


@pytest.mark.parametrize("M,H", [(3, 3), (6, 2), (2, 8)])
def test_constant_traces_the_forecast_walk_is_the_lookahead_walk(PH, M, H):
    """A corpus whose traces are constant per trace: planning on P = that constant is looking into the real future."""
    V = 10
    ctx = Ctx(PH, M, V, max_ticks=120_000)
    try:
        rng = np.random.default_rng([M, H, 11])
        level = rng.uniform(0.2, 8.0, 6)
        traces = [np.full(int(rng.integers(1, 40)), v) for v in level]     # a one-sample trace among them, maybe
        traces[0] = np.full(1, level[0])
        u = rng.uniform(0.0, 2.0, (V, M))
        for quality in (False, True):
            ctx.quality(3.0, u) if quality else ctx.quality(0.0, None)
            for c in (0, 1, 2, V - 1):
                n = 24
                tid = rng.integers(0, len(traces), n).astype(np.int32)
                off = rng.integers(0, 50, n).astype(np.int32)
                prefix = rng.integers(0, M, (n, c)).astype(np.int32).reshape(n, c)
                la = ctx.lookahead(H, traces, tid, off, prefix)
                pl = ctx.plan(0, H, traces, tid, off, prefix, level[tid])
                same(pl, la, (M, H, c, quality))
                assert (la["action"] >= 0).all()
    finally:
        ctx.close()


# ---- the built-in forecast against the numpy twin ----
def run_forecast(PH, W_, done, c, hist, state):
    n = len(c)
    P = np.full(n, -7.0)
    PH.pl_forecast(C.c_int64(n), C.c_int32(W_), P_(done, C.c_uint8), P_(np.asarray(c, np.int32), C.c_int32),
                   P_(hist, C.c_double), P_(state, C.c_uint8), P_(P, C.c_double))
    return P


@pytest.mark.parametrize("robust", [0, 1])
@pytest.mark.parametrize("W_", [1, 3, 5, 16])
def test_forecast_equals_the_twin(PH, W_, robust):
    """A script of selects over 40 lanes: select, select again, a download between selects, a gap (two downloads and no
    select), finished lanes, an episode restart (chunk 0), a zero and an infinite throughput in the history."""
    N, T = 40, 24
    rng = np.random.default_rng([W_, robust, 3])
    hist = np.ascontiguousarray(rng.uniform(0.2, 8.0, (T, N)))
    hist[3, 7], hist[4, 6], hist[:, 5] = 0.0, np.inf, 0.0       # lane 5 never measures any throughput
    c = np.zeros(N, np.int64)
    done = np.zeros(N, np.uint8)
    twin = RT.empty_state(N, W_)
    state = np.zeros(RT.state_nbytes(N, W_), np.uint8) if robust else None
    seen = dict(discounted=0, none=0)

    def check(what):
        P = run_forecast(PH, W_, done, c, hist, state)
        ref = RT.estimate_vec(W_, c, hist, twin if robust else RT.empty_state(N, W_), active=done == 0)
        assert np.array_equal(bits(P), bits(ref)), what
        if robust:
            assert np.array_equal(state, RT.state_bytes(twin)), what
        assert (P[done != 0] == 0.0).all() and (P[c == 0] == 0.0).all()
        return P

    check("chunk 0")
    for step in range(1, 20):
        move = rng.random(N) < 0.8
        if step == 7:
            c = np.where(move, c + 2, c)                         # a gap: two downloads between two selects
        elif step == 12:
            c = np.where(np.arange(N) % 4 == 0, 0, c + move)     # an episode restart for every fourth lane
            hist[:, np.arange(N) % 4 == 0] = rng.uniform(0.2, 8.0, (T, (N + 3) // 4))
        else:
            c = c + move
        if step == 9:
            done[::5] = 1                                        # finished lanes keep their state
        if step == 14:
            done[:] = 0
        P = check(step)
        P2 = check((step, "again"))                              # selecting twice: the same answer, the same state
        assert np.array_equal(bits(P), bits(P2))
        hm = RT.estimate_vec(W_, c, hist, RT.empty_state(N, W_), active=done == 0)
        seen["discounted"] += int((P < hm).sum())
        seen["none"] += int(((P == 0.0) & (done == 0) & (c > 0)).sum())
        if not robust:
            assert np.array_equal(bits(P), bits(hm))             # P = hm
    assert seen["none"] > 0                                      # the zero throughput: hm = 0
    assert (seen["discounted"] > 0) == bool(robust)


# ---- the struct, the symbols, the refusals, the Python checks ----
def test_struct_matches_the_header(L):
    fields = ["horizon", "window", "robust", "reserved_", "max_nodes_per_launch", "forecast_dev", "state_dev", "state_bytes"]
    prog = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "abr_env.h"
    int main(void) {
        printf("%zu", sizeof(abr_plan_config));
    """ + "".join(f'    printf(" %zu", offsetof(abr_plan_config, {f}));\n' for f in fields) + r"""
        printf(" %d %d %d\n", ABR_ABI_VERSION, ABR_MAX_HORIZON, ABR_ROBUST_MAX_WINDOW);
        return 0;
    }"""
    got = list(map(int, c_abi_output(prog)[0].split()))
    S = L.PlanConfig
    assert got[:9] == [C.sizeof(S)] + [getattr(S, f).offset for f in fields] == [48, 0, 4, 8, 12, 16, 24, 32, 40]
    assert got[9] == 4 == L.ABI_VERSION and got[10] == 8 == L.MAX_HORIZON and got[11] == 16 == L.ROBUST_MAX_WINDOW


def test_symbols_declared_exported_and_bound(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "abr_env.h")).read()
    for sym in ("abr_env_plan_select", "abr_env_step_plan"):
        assert hasattr(lib, sym) and sym in {n for n, _, _ in L.SYMBOLS} and sym + "(" in header
    assert lib.abr_abi_version() == 4                            # additive: the ABI version stays
    import abrsimulator_amd as A
    assert A.ForecastMPCController is __import__("abrsimulator_amd.planner", fromlist=["x"]).ForecastMPCController
    assert "ForecastMPCController" in A.__all__ and hasattr(A.BatchedABREnv, "step_plan")


def test_refusals_that_need_no_device(L):
    """The documented order: cfg, action_out_dev (select), horizon, reserved_, max_nodes_per_launch, robust, window (without a
    forecast), n_steps (step), then the handle."""
    lib = L.lib()
    one = C.c_void_p(256)
    E = lambda: lib.abr_last_error()
    select = lambda cfg, act: lib.abr_env_plan_select(None, cfg, act, None, None, None, None)
    step = lambda cfg, n: lib.abr_env_step_plan(None, cfg, n, None, None, None, None, None)
    cfg = lambda h=3, w=5, rb=1, r=0, n=0, f=None: C.byref(L.PlanConfig(h, w, rb, r, n, f, None, 0))
    assert select(None, None) == -1 and b"cfg is NULL" in E()
    assert step(None, 0) == -1 and b"cfg is NULL" in E()
    assert select(cfg(0, 0, 2, 1, -1), None) == -1 and b"action_out_dev" in E()
    for h in (0, -1, 9):
        assert select(cfg(h, 0, 2, 1, -1), one) == -1 and b"horizon" in E()
        assert step(cfg(h, 0, 2, 1, -1), 0) == -1 and b"horizon" in E()          # a step has no action_out_dev to miss
    assert select(cfg(3, 0, 2, 1, -1), one) == -1 and b"reserved_" in E()
    assert step(cfg(8, 0, 2, 7, -1), 0) == -1 and b"reserved_" in E()
    assert select(cfg(3, 0, 2, 0, -1), one) == -1 and b"max_nodes_per_launch" in E()
    assert step(cfg(3, 0, 2, 0, -1), 0) == -1 and b"max_nodes_per_launch" in E()
    for rb in (2, -1):
        assert select(cfg(3, 0, rb), one) == -1 and b"robust must be 0 or 1" in E()
        assert step(cfg(3, 0, rb), 0) == -1 and b"robust must be 0 or 1" in E()
    for w in (0, -1, 17):
        for rb in (0, 1):
            assert select(cfg(3, w, rb), one) == -1 and b"window" in E()
            assert step(cfg(3, w, rb), 0) == -1 and b"window" in E()
        # a caller's forecast: the window is not looked at
        assert select(cfg(3, w, 1, f=256), one) == -1 and b"env is NULL" in E()
        assert step(cfg(3, w, 0, f=256), 0) == -1 and b"n_steps" in E()
    for n in (0, -3):
        assert step(cfg(), n) == -1 and b"n_steps" in E()
    for h, w in ((1, 1), (8, 16)):
        assert select(cfg(h, w, 0), one) == -1 and b"env is NULL" in E()
        assert select(cfg(h, w, 1), one) == -1 and b"env is NULL" in E()         # the state is checked against the handle's lanes
        assert step(cfg(h, w, 1, n=2 ** 40), 1) == -1 and b"env is NULL" in E()


def test_python_value_errors():
    import torch
    import abrsimulator_amd as A

    class Env:
        n_lanes, device = 4, torch.device("cuda", 0)

    class Player:
        env = Env()

    for kw in (dict(horizon=0), dict(horizon=9), dict(horizon=2.5), dict(horizon=3, window=0), dict(horizon=3, window=17),
               dict(horizon=3, window=2.5), dict(horizon=3, max_nodes_per_launch=-1)):
        with pytest.raises(ValueError):
            A.ForecastMPCController(Player(), **kw)
    ctl = A.ForecastMPCController(Player(), 3, window=16, robust=False)
    assert (ctl.horizon, ctl.window, ctl.robust, ctl.max_nodes_per_launch) == (3, 16, False, 0)
    cfg = ctl.config()                                           # robust=False: no state, no forecast
    assert (cfg.horizon, cfg.window, cfg.robust, cfg.reserved_, cfg.forecast_dev, cfg.state_dev, cfg.state_bytes) == \
        (3, 16, 0, 0, None, None, 0)
    for bad in (torch.zeros(4, dtype=torch.float32), torch.zeros(3, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.float64),
                torch.zeros(4, dtype=torch.float64), [1.0, 2.0, 3.0, 4.0]):     # dtype, shape, shape, device, not a tensor
        with pytest.raises(ValueError):
            ctl.config(bad)
        with pytest.raises(ValueError):
            ctl.select(forecast=bad)
        with pytest.raises(ValueError):
            ctl.next_bitrate(forecast=bad)
