"""Forecast MPC on the device (include/abr_env.h: abr_env_plan_select, abr_env_step_plan; ForecastMPCController,
BatchedABREnv.step_plan).

The reference is always existing code, never the planner.  The walk: LookaheadExpert in a constant world -- the
environment's traces overwritten in place so that lane i's trace is F[i] everywhere (or an environment whose real traces
are constant) -- must answer what select(forecast=F) answers, on the bit pattern.  The built-in forecast: the numpy twin of
RobustMPC's estimate (robust_twin.estimate_vec) on env.history().  The rollout: select + step in a Python loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import abrsimulator_amd as A
from abrsimulator_amd import _lib
import fork_twin
import robust_twin as RT

pytestmark = pytest.mark.gpu

LADDER16 = [0.3, 0.5, 0.75, 1.0, 1.2, 1.5, 1.85, 2.3, 2.85, 3.5, 4.3, 5.2, 6.0, 7.0, 8.0, 9.5]
L, MB, SU, W = 4.0, 20.0, 8.0, [4.3, 1.0, 1.0, 0.1]


def ladder(M):
    return [0.3, 1.2, 2.85] if M == 3 else [LADDER16[(16 * k) // M] for k in range(M)]


def corpus(n, seed=0, lo=30, hi=60):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.5, 6.0, int(rng.integers(lo, hi))) for _ in range(n)]


def make(N, M=3, V=6, traces=None, **kw):
    """one trace per lane unless the caller brings a corpus"""
    return A.BatchedABREnv(A.MPD(V, L, MB, SU, A.Chunk(ladder(M))), A.QOEMetric(*W), A.NetworkInfo(1.0, traces or corpus(N)), N,
                           device="cuda", **kw)


def start(env, seed=3):
    N = env.n_lanes
    tid = (np.arange(N) % env.n_traces).astype(np.int32)
    off = np.random.default_rng(seed).integers(0, 30, N).astype(np.int32)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    return tid, off


def advance(env, steps, seed=5):
    acts = np.random.default_rng(seed).integers(0, env.n_rates, (max(steps, 1), env.n_lanes)).astype(np.int32)
    for t in range(steps):
        env.step(torch.from_numpy(acts[t]).cuda())


def planner(env, H=3, **kw):
    return A.ForecastMPCController(A.EnvPlayer(env), H, **kw)


def raw(t):
    return t.cpu().numpy().view(np.uint8)


def same_answer(got, want, what=""):
    """action, key and q on the bit pattern (both sides write the same quiet NaN)"""
    for k in ("action", "key", "q"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(raw(got[k]), raw(want[k])), (what, k)


def lookahead_in_a_constant_world(env, F, H, **kw):
    """LookaheadExpert's labels with the traces overwritten in place so that lane i's trace (trace_id = arange) is F[i]
    everywhere; the traces are put back and their bytes checked."""
    N = env.n_lanes
    assert env.n_traces == N and np.array_equal(env.trace_id.cpu().numpy(), np.arange(N))
    saved = env.traces.clone()
    ln = env.trace_len.cpu().numpy().astype(np.int64)
    off = env.trace_off.cpu().numpy().astype(np.int64)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(ln)[:-1]])) and int(ln.sum()) == saved.numel()
    env.traces.copy_(torch.from_numpy(np.repeat(np.asarray(F, np.float64), ln)).to(saved.dtype))
    lab = A.LookaheadExpert(A.EnvPlayer(env), H, **kw).labels(want_q=True)
    env.traces.copy_(saved)
    assert np.array_equal(raw(env.traces), raw(saved))
    return lab


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def state_bytes_of(env):
    """The workspace without the rollouts' scratch (the fused MPC rollouts' action row and predictor scratch, which carry
    nothing between calls): every table and per-lane region, and the layout tag."""
    v, ws = env.state_view(), env.workspace
    o = fork_twin.workspace_offsets(env.video_length, env.n_lanes, v.buffer_level - ws.data_ptr())
    return torch.cat([ws[:o["mpc_action"][0]], ws[-256:]]).cpu().numpy()


def vivid(act, chunk, done):
    """The non-vacuity conditions: every live lane past chunk 0 carries an action, and at least two actions occur."""
    live = (done == 0) & (chunk > 0)
    assert live.any() and (act[live] >= 0).all()
    return set(act[live].tolist())


def chunks(env):
    return env.mpc_inputs()[0].cpu().numpy().copy()


def dones(env):
    return env.done_after_reset().cpu().numpy().copy()


# ---- 1. a caller's forecast against the lookahead in a constant world ----
def test_callers_forecast_equals_the_lookahead_in_a_constant_world():
    N = 200
    env = make(N)
    env.set_quality(3.0, "log")
    start(env)
    F = np.random.default_rng(21).uniform(0.5, 6.0, N)
    ctl = planner(env)
    acts = np.random.default_rng(5).integers(0, 3, (5, N)).astype(np.int32)
    seen, t = set(), 0
    for upto in (0, 2, 4, 5):                                             # 4 and 5: the horizon shrinks to 2 and 1
        while t < upto:
            env.step(torch.from_numpy(acts[t]).cuda())
            t += 1
        want = lookahead_in_a_constant_world(env, F, 3)
        got = ctl.select(want_q=True, want_forecast=True, forecast=dev(F))
        same_answer(got, want, upto)
        assert np.array_equal(got["forecast"].cpu().numpy(), F)
        a = got["action"].cpu().numpy()
        assert (a >= 0).all()                                             # a caller's forecast decides at chunk 0 as well
        if upto:
            seen |= vivid(a, chunks(env), dones(env))
    assert len(seen) >= 2
    assert ctl._state is None                                             # a caller's forecast touches no state


# ---- 2. the built-in forecast against the twin ----
@pytest.mark.parametrize("robust", [0, 1])
def test_builtin_forecast_equals_the_twin_through_a_script(robust):
    N, Wd = 200, 3
    env = make(N, auto_reset=True)
    tid, off = start(env)
    ctl = planner(env, window=Wd, robust=bool(robust))
    twin = RT.empty_state(N, Wd)
    seen = dict(discounted=0, restarted=0)

    def select(what):
        got = ctl.select(want_forecast=True)
        c, d, hist = chunks(env), dones(env), env.history()[1].cpu().numpy()
        P = RT.estimate_vec(Wd, c, hist, twin if robust else RT.empty_state(N, Wd), active=d == 0)
        assert np.array_equal(raw(got["forecast"]), P.view(np.uint8)), what
        if robust:
            assert np.array_equal(ctl.state.cpu().numpy(), RT.state_bytes(twin)), what
        else:
            assert ctl._state is None, what                               # robust == 0 needs no state and touches none
        a = got["action"].cpu().numpy()
        assert ((a >= 0) == (P > 0.0)).all(), what                        # nothing times out here
        hm = RT.estimate_vec(Wd, c, hist, RT.empty_state(N, Wd), active=d == 0)
        seen["discounted"] += int((P < hm).sum())
        return got

    select("chunk 0")
    for step in range(1, 9):
        a = select(step)
        b = select((step, "again"))                                       # the same answer and the same state
        for k in ("action", "key", "forecast"):
            assert np.array_equal(raw(a[k]), raw(b[k])), (step, k)
        if step == 3:                                                     # a masked reset: those lanes restart at chunk 0
            mask = (np.arange(N) % 3 == 0).astype(np.uint8)
            env.reset(torch.from_numpy(tid), torch.from_numpy(off), mask=torch.from_numpy(mask))
            select((step, "masked reset"))
        if step == 5:
            advance(env, 1, seed=40)                                      # a gap: a download without a select before it
        before = chunks(env)
        advance(env, 1, seed=50 + step)
        seen["restarted"] += int(((chunks(env) == 0) & (before > 0)).sum())  # auto_reset: the episode ended and restarted
    assert seen["restarted"] > 0
    assert (seen["discounted"] > 0) == bool(robust)
    if robust:
        ctl.reset_state()
        assert not ctl.state.any()
        i32, f64 = ctl.state_rows()
        assert tuple(i32.shape) == (2, N) and tuple(f64.shape) == (1 + Wd, N) and i32.data_ptr() == ctl.state.data_ptr()


# ---- 3. select is read-only ----
def test_select_leaves_the_workspace_the_quality_sums_and_the_ledger_alone():
    env = make(200)
    env.set_episode_ledger(2)
    env.set_quality(3.0, "log", rows=2)
    start(env)
    advance(env, 4)                                                       # horizon 3 crosses the episode's end
    ws, qb, lb = env.workspace.clone(), env.quality.blob.clone(), env.episode_ledger.blob.clone()
    hist = [h.clone() for h in env.history()]
    F = dev(np.full(200, 2.0))
    for ctl, kw in ((planner(env), {}), (planner(env, robust=False), {}), (planner(env), dict(forecast=F))):
        got = ctl.select(want_q=True, want_forecast=True, **kw)
        assert (got["action"] >= 0).all()
    torch.cuda.synchronize()
    assert torch.equal(env.workspace, ws) and torch.equal(env.quality.blob, qb) and torch.equal(env.episode_ledger.blob, lb)
    assert all(torch.equal(a, b) for a, b in zip(env.history(), hist))    # action_hist and bw_hist
    assert (env.episode_ledger.count() == 0).all()


# ---- 4. no decision ----
def nothing(got, lanes=slice(None), forecast=0.0):
    assert (got["action"][lanes] == -1).all() and torch.isnan(got["key"][lanes]).all() and torch.isnan(got["q"][:, lanes]).all()
    if forecast is not None:
        assert (got["forecast"][lanes] == forecast).all()


def test_no_decision():
    N = 130
    env = make(N)
    F = dev(np.full(N, 2.0))
    ctl = planner(env)
    nothing(ctl.select(want_q=True, want_forecast=True, forecast=F))      # never reset: ABR_DONE_EPISODE
    nothing(ctl.select(want_q=True, want_forecast=True))
    start(env)
    for c in (ctl, planner(env, robust=False)):                           # chunk 0: the built-in forecast has no history
        nothing(c.select(want_q=True, want_forecast=True))
    assert not ctl.state.any()                                            # and the state stays empty
    bad = np.full(N, 2.0)
    bad[0::5], bad[1::5], bad[2::5], bad[3::5] = 0.0, -1.0, np.nan, np.inf
    got = ctl.select(want_q=True, want_forecast=True, forecast=dev(bad))
    none = torch.from_numpy(np.arange(N) % 5 != 4).cuda()
    nothing(got, none)
    assert (got["action"][~none] >= 0).all() and torch.isfinite(got["key"][~none]).all() and (got["forecast"][~none] == 2.0).all()
    advance(env, 6)                                                       # every lane finished
    assert (dones(env) != 0).all()
    nothing(ctl.select(want_q=True, want_forecast=True, forecast=F))
    nothing(ctl.select(want_q=True, want_forecast=True))
    # 1e-12 under 40 s of ticks: every sequence times out; the forecast was usable and is reported
    env = make(64, max_ticks=4_000)
    start(env)
    env.step(torch.zeros(64, dtype=torch.int32, device="cuda"))           # 1.2 Mbit at 0.5 Mbit/s or more: a few seconds
    got = planner(env).select(want_q=True, want_forecast=True, forecast=dev(np.full(64, 1e-12)))
    nothing(got, forecast=1e-12)
    assert (dones(env) == 0).all()


# ---- 5. the rollout against select + step in a Python loop ----
@pytest.mark.parametrize("auto_reset,dressed,robust", [(False, False, True), (True, False, True), (True, True, True),
                                                        (False, True, False)])
def test_step_plan_equals_select_and_step(auto_reset, dressed, robust):
    N, n, Wd = 200, 9, 3                                                  # 9 decisions: one and a half episodes
    envs = [make(N, auto_reset=auto_reset) for _ in range(2)]
    for e in envs:
        if dressed:
            e.set_episode_ledger(2)
            e.set_quality(3.0, "log", rows=2)
        start(e)
    fused, loop = envs
    cf, cl = planner(fused, window=Wd, robust=robust), planner(loop, window=Wd, robust=robust)
    out = fused.step_plan(cf, n)
    seen = set()
    for s in range(n):
        sel = cl.select()
        a = sel["action"].cpu().numpy()
        if dressed:
            seen |= vivid(a, chunks(loop), dones(loop)) if ((dones(loop) == 0) & (chunks(loop) > 0)).any() else set()
        act = cl.next_bitrate()
        assert np.array_equal(act.cpu().numpy(), np.maximum(a, 0))        # -1 -> 0
        obs, rew, dn = loop.step(act)
        assert np.array_equal(raw(out["obs"][s]), raw(obs)), s
        assert np.array_equal(raw(out["reward"][s]), raw(rew)), s
        assert np.array_equal(raw(out["done"][s]), raw(dn)), s
        assert np.array_equal(out["actions"][s].cpu().numpy(), act.cpu().numpy()), s
    if dressed:
        assert len(seen) >= 2
    assert np.array_equal(state_bytes_of(fused), state_bytes_of(loop))
    sf, sl = fused.state_dict(), loop.state_dict()
    assert torch.equal(sf["trace_id"], sl["trace_id"]) and torch.equal(sf["start_offset"], sl["start_offset"])
    if robust:
        assert torch.equal(cf.state, cl.state) and cf.state.any()
    else:
        assert cf._state is None and cl._state is None
    if dressed:
        assert torch.equal(fused.quality.blob, loop.quality.blob)
        rf, rl = fused.episode_ledger.records(), loop.episode_ledger.records()
        assert len(rf["lane"]) >= N                                       # every lane finished an episode
        for k in rf:
            assert np.array_equal(raw(rf[k]), raw(rl[k])), k
    # the outputs are optional, and a fixed belief rides along unchanged
    F = dev(np.random.default_rng(2).uniform(0.5, 6.0, N))
    for e in envs:
        start(e)
    o2 = fused.step_plan(cf, 3, want_obs=False, want_actions=False, forecast=F)
    assert o2["obs"] is None and o2["actions"] is None
    for s in range(3):
        _, rew, dn = loop.step(cl.next_bitrate(forecast=F))
        assert np.array_equal(raw(o2["reward"][s]), raw(rew)) and np.array_equal(raw(o2["done"][s]), raw(dn))
    assert np.array_equal(state_bytes_of(fused), state_bytes_of(loop))


# ---- 6. closed loop in a constant world ----
def test_closed_loop_in_a_constant_world_is_the_lookahead_expert():
    N, V, H = 200, 6, 3
    level = np.random.default_rng(31).uniform(0.5, 6.0, 16)
    traces = [np.full(20 + k, v) for k, v in enumerate(level)]
    a, b = make(N, traces=traces), make(N, traces=traces)
    for e in (a, b):
        e.set_quality(3.0, "log")
        tid, _ = start(e)
    F = dev(level[tid])
    out = a.step_plan(planner(a, H), V + 1, forecast=F)                   # the last decision finds every lane finished
    exp = A.LookaheadExpert(A.EnvPlayer(b), H)
    seen = set()
    for s in range(V + 1):
        lab = exp.next_bitrate()
        act = lab.cpu().numpy()
        if 0 < s < V:
            seen |= vivid(act, chunks(b), dones(b))
        if s == V:
            assert (act == -1).all()
        obs, rew, dn = b.step(lab.clamp(min=0))
        assert np.array_equal(raw(out["obs"][s]), raw(obs)), s
        assert np.array_equal(raw(out["reward"][s]), raw(rew)) and np.array_equal(raw(out["done"][s]), raw(dn)), s
        assert np.array_equal(out["actions"][s].cpu().numpy(), np.maximum(act, 0)), s
    assert len(seen) >= 2
    assert np.array_equal(state_bytes_of(a), state_bytes_of(b))
    assert torch.equal(a.episode_qoe(quality=True), b.episode_qoe(quality=True))


# ---- 7. shapes and refusals ----
def check_shape(env, H, steps=1, **kw):
    start(env)
    advance(env, steps)
    F = np.random.default_rng(env.n_lanes).uniform(0.5, 6.0, env.n_lanes)
    want = lookahead_in_a_constant_world(env, F, H)
    got = planner(env, H, **kw).select(want_q=True, forecast=dev(F))
    same_answer(got, want, (env.n_lanes, H, kw))
    assert (got["action"] >= 0).all()
    return got


@pytest.mark.parametrize("N", [1, 64, 65, 200])
def test_lane_counts(N):
    check_shape(make(N), 3)


@pytest.mark.parametrize("M,H,V", [(1, 2, 6), (16, 2, 6), (2, 8, 9)])
def test_rate_counts_and_the_deepest_instance(M, H, V):
    check_shape(make(100, M=M, V=V), H)                                   # (2, 8, 9): eight decisions left, 256 sequences


def test_launch_splitting():
    """39 nodes per lane at 3 rates and horizon 3: a bound of 64 lanes' worth splits 200 lanes into four launches."""
    env = make(200)
    one = check_shape(env, 3, steps=2)
    F = np.random.default_rng(200).uniform(0.5, 6.0, 200)
    nodes = 3 + 9 + 27
    for cap in (nodes * 64, nodes * 64 + nodes * 63, 1):
        ctl = planner(env, 3, max_nodes_per_launch=cap)
        same_answer(ctl.select(want_q=True, forecast=dev(F)), one, cap)
    # the built-in forecast is computed once for all launches
    a, b = planner(env, 3).select(want_q=True, want_forecast=True), planner(env, 3, max_nodes_per_launch=1).select(want_q=True, want_forecast=True)
    same_answer(a, b, "built-in")
    assert torch.equal(a["forecast"], b["forecast"]) and (a["action"] >= 0).all()


def test_every_accepted_implementation():
    sel, roll = {}, {}
    acts = np.random.default_rng(5).integers(0, 3, (2, 200)).astype(np.int32)
    for impl in ("jump", "split", "split3", "tick"):
        env = make(200, impl=impl)
        start(env)
        env.step_script(torch.from_numpy(acts).cuda())
        ctl = planner(env)
        sel[impl] = ctl.select(want_q=True, want_forecast=True)
        if impl == "tick":                                                # the rollout's kernel choice is abr_env_step_mpc's
            with pytest.raises(_lib.AbrError, match="-4"):
                env.step_plan(ctl, 2)
            continue
        roll[impl] = env.step_plan(ctl, 5)
        roll[impl]["state"] = torch.from_numpy(state_bytes_of(env))
    assert (sel["jump"]["action"] >= 0).all()
    for impl in ("split", "split3", "tick"):
        same_answer(sel[impl], sel["jump"], impl)
        assert torch.equal(sel[impl]["forecast"], sel["jump"]["forecast"])
    for impl in ("split", "split3"):
        for k in ("obs", "reward", "done", "actions", "state"):
            assert np.array_equal(raw(roll[impl][k]), raw(roll["jump"][k])), (impl, k)


def test_refusals():
    N = 64
    rule = A.LatencySpeedController((2.0, 6.0), (1.0, 8.0), ((0.9, 1.0, 1.0), (0.9, 1.1, 1.25), (0.75, 1.5, 2.0)))
    for speed in (torch.full((N,), 1.1, dtype=torch.float64), torch.full((2, N), 1.05, dtype=torch.float64), rule):
        env = make(N, speed=speed)
        start(env)
        with pytest.raises(_lib.AbrError, match="-4.*speed"):
            planner(env, 2).select()
        with pytest.raises(_lib.AbrError, match="-4.*speed"):
            env.step_plan(planner(env, 2), 1)
    env = make(N)
    start(env)
    ctl = planner(env, 2)
    ctl.select()
    sp = torch.full((N,), 1.1, dtype=torch.float64, device="cuda")
    env._check(env.lib.abr_env_set_lane_speeds(env._h, _lib.ptr(sp)))      # pending ones refuse as well
    with pytest.raises(_lib.AbrError, match="-4.*pending"):
        ctl.select()
    env._check(env.lib.abr_env_set_lane_speeds(env._h, None))
    ctl.select()
    env = make(N, M=6, speed=1.25)                                        # a constant play speed is fine
    check_shape(env, 2)
    with pytest.raises(_lib.AbrError, match="-4.*leaves"):                # 6^7 = 279 936 leaves
        planner(env, 7).select()
    with pytest.raises(_lib.AbrError, match="-4.*leaves"):
        env.step_plan(planner(env, 7), 1)
    planner(env, 6).select()                                              # 46 656: the cap admits it
    # the state is checked against the handle's lanes, after the handle and before the unsupported cases
    ctl = planner(env, 7, window=4)
    act = torch.empty(N, dtype=torch.int32, device="cuda")
    st = ctl.state
    for ptr_, nbytes, what in ((None, st.numel(), "NULL"), (st.data_ptr() + 4, st.numel(), "aligned"),
                               (st.data_ptr(), st.numel() - 1, "bytes")):
        cfg = ctl.config()
        cfg.state_dev, cfg.state_bytes = ptr_, nbytes
        with pytest.raises(_lib.AbrError, match="-1.*" + what):
            env._call(env.lib.abr_env_plan_select, env._h, C.byref(cfg), _lib.ptr(act), None, None, None)
        with pytest.raises(_lib.AbrError, match="-1.*" + what):
            env._call(env.lib.abr_env_step_plan, env._h, C.byref(cfg), 1, None, None, None, None)
    torch.cuda.synchronize()
