"""Variable-bitrate video on the device (include/abr_env.h: abr_env_set_size_table; BatchedABREnv(chunk_sizes=...)).

The exact reference without touching the oracle, which knows bitrate tables only: draw an effective-bitrate table E (the
nominal B times uniform(0.6, 1.6) per entry, rows not sorted) and set S = E * L in float64.  oracle.env_batch with
br_table = E downloads exactly S -- the same single multiplication -- so it gives every clock, buffer and bandwidth frame
of a run under size table S; the rewards follow from those frames with the NOMINAL table, oracle.step_rewards(...,
br_table=B).  Each half is the reference's own arithmetic.

Tolerances: everything is compared on the bit pattern except episode_qoe / the ledger's qoe against the value formed from
the oracle's terms, which carry the oracle's average_latency: the kernels' latency integral differs from the reference's
recurrence by float64 drift (1e-9 relative on the latency, 1e-10 on the qoe), the tolerance every ledger
test of the project uses.  The variance term, which is what this feature could get wrong, is compared with ==."""
import itertools

import numpy as np
import pytest
import torch

import abrsimulator_amd as A
from abrsimulator_amd import _lib
import helpers
import policy_gru_twin as GT
import policy_twin as T
import rules_twin
import test_lookahead_gpu as TL

pytestmark = pytest.mark.gpu

V, L, MB, SU, W = 6, 4.0, 20.0, 8.0, [4.3, 1.0, 1.0, 0.1]        # TL.reference forms its keys with the same weights
N = 200                                                          # not a multiple of 64: the last workgroup is partial
LADDER16 = [0.3, 0.5, 0.75, 1.0, 1.2, 1.5, 1.85, 2.3, 2.85, 3.5, 4.3, 5.2, 6.0, 7.0, 8.0, 9.5]
assert TL.W == W and TL.L == L


def corpus():
    rng = np.random.default_rng(1)
    return [rng.uniform(0.2, 6.0, int(n)).astype(np.float32).astype(np.float64) for n in rng.integers(30, 201, 8)]


TRACES = corpus()


def tables(M=3, seed=0, Vv=V):
    """(ladder, B [V][M] nominal, E effective, S = E * L)"""
    rng = np.random.default_rng(seed)
    ladder = [0.75, 1.2, 1.85] if M == 3 else LADDER16[:M]
    B = np.tile(np.asarray(ladder, np.float64), (Vv, 1))
    E = B * rng.uniform(0.6, 1.6, B.shape)
    return ladder, B, E, E * L


def make(n=N, ladder=None, sizes=None, br=None, Vv=V, traces=None, **kw):
    chunks = A.Chunk(ladder) if br is None else [A.Chunk(list(r)) for r in br]
    return A.BatchedABREnv(A.MPD(Vv, L, MB, SU, chunks), A.QOEMetric(*W), A.NetworkInfo(1.0, traces or TRACES), n,
                           device="cuda", chunk_sizes=sizes, **kw)


def pairs(n=N, seed=3):
    rng = np.random.default_rng(seed)
    return (np.arange(n) % len(TRACES)).astype(np.int32), rng.integers(0, 30, n).astype(np.int32)


def start(env, seed=3):
    tid, off = pairs(env.n_lanes, seed)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    return tid, off


def npy(t):
    return t.detach().cpu().numpy()


def same(a, b):
    a, b = np.ascontiguousarray(npy(a) if torch.is_tensor(a) else a), np.ascontiguousarray(npy(b) if torch.is_tensor(b) else b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def variance_in_order(a, Btab):
    """sum over the episode of |br[c][a_c] - br[c+1][a_(c+1)]| added in chunk order (Simulator.py:82), a: [n, V]"""
    v = np.zeros(a.shape[0])
    for c in range(a.shape[1] - 1):
        v = v + np.abs(Btab[c][a[:, c]] - Btab[c + 1][a[:, c + 1]])
    return v


def qoe_from(fin, var):
    return W[0] * fin["rebuffer_time"] + W[1] * var + W[2] * fin["start_up_time"] + W[3] * fin["average_latency"]


def check_frame(env, steps, bw, s):
    """observe_f64 at call site s against the oracle's frame s"""
    f = env.observe_f64()
    for k in helpers.F64_EXACT:
        assert same(f[k], np.ascontiguousarray(steps[k][:, s])), (s, k)
    want_bw = bw[:, s - 1] if s else np.zeros(bw.shape[0])
    assert same(f["last_bandwidth"], np.ascontiguousarray(want_bw)), (s, "last_bandwidth")


# ---------------------------------------------------------------------------------------------------------------------
# 1. oracle parity

IMPLS = ("jump", "split", "split3", "tick")


@pytest.mark.parametrize("M,impl", [(3, i) for i in IMPLS] + [(16, "jump")])
@pytest.mark.parametrize("mode", ("step", "script", "random"))
def test_oracle_parity(oracle, impl, mode, M):
    ladder, B, E, S = tables(M)
    auto = mode == "random"
    env = make(ladder=ladder, sizes=S, impl=impl, auto_reset=auto)
    assert env.general_instance() and env.general_instance(fused=True)
    tid, off = start(env)
    cfg = oracle.env_cfg(ladder, L, V, MB, SU, 1.0, W, 1.0, br_table=E)
    rng = np.random.default_rng(7)
    if not auto:
        acts = rng.integers(0, M, (N, V)).astype(np.int32)
        steps, bw, fin, _ = oracle.env_batch(cfg, TRACES, tid, off, acts)
        rew = oracle.step_rewards(steps["rebuffer_time"], steps["start_up_time"], fin["rebuffer_time"], fin["start_up_time"],
                                  acts, W, br_table=B)
        dev = torch.from_numpy(np.ascontiguousarray(acts.T)).cuda()                # [V, N]
        if mode == "step":
            for s in range(V):
                check_frame(env, steps, bw, s)
                _, r, _ = env.step(dev[s].contiguous())
                assert same(r, rew[:, s]), s
        else:                                                                      # two fused pieces, a frame between them
            out = [env.step_script(dev[:3].contiguous())]
            check_frame(env, steps, bw, 3)
            out.append(env.step_script(dev[3:].contiguous()))
            got = torch.cat([o["reward"] for o in out])
            assert same(got, np.ascontiguousarray(rew.T))
            obs = torch.cat([o["obs"] for o in out])                               # obs[s]: call site s + 1
            for s in range(V - 1):
                for row, k in ((_lib.OBS_ROWS.index("buffer_level"), "buffer_level"),
                               (_lib.OBS_ROWS.index("global_time"), "global_time")):
                    assert same(obs[s, row], steps[k][:, s + 1].astype(np.float32)), (s, k)
                assert same(obs[s, _lib.OBS_ROWS.index("last_bandwidth")], bw[:, s].astype(np.float32)), s
        f = env.observe_f64()
        for k in ("global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level"):
            assert same(f[k], np.ascontiguousarray(fin[k])), k
        assert same(f["last_bandwidth"], np.ascontiguousarray(bw[:, V - 1]))
        assert (npy(env.done_after_reset()) == _lib.DONE_EPISODE).all()
        var = variance_in_order(acts, B)
        assert not np.array_equal(var, variance_in_order(acts, E))
        np.testing.assert_allclose(npy(env.episode_qoe()), qoe_from(fin, var), rtol=1e-10, atol=0)
        return
    # fused random decisions under auto_reset, across two episode ends, with a ledger
    led = env.set_episode_ledger(2)
    n_steps = 2 * V + 2
    out = env.step_random(n_steps, seed=99)
    acts = npy(out["actions"])
    want = helpers.auto_reset_rollout_rewards(oracle, cfg, TRACES, tid, off, acts, W, br_table=B)
    assert same(out["reward"], want)
    a3 = np.zeros((N, V), np.int32)
    a3[:, :2] = acts[2 * V:].T
    steps, bw, _, _ = oracle.env_batch(cfg, TRACES, tid, off, a3)
    check_frame(env, steps, bw, 2)
    rec = led.records()
    for k in range(2):
        a = np.ascontiguousarray(acts[k * V:(k + 1) * V].T)
        _, _, fin, _ = oracle.env_batch(cfg, TRACES, tid, off, a)
        var = variance_in_order(a, B)
        got_var = npy(rec["variance"]).reshape(N, 2)[:, k]
        assert same(got_var, var), k
        for f in ("rebuffer_time", "start_up_time"):
            assert same(npy(rec[f]).reshape(N, 2)[:, k], np.ascontiguousarray(fin[f])), (k, f)
        np.testing.assert_allclose(npy(rec["qoe"]).reshape(N, 2)[:, k], qoe_from(fin, var), rtol=1e-10, atol=0)
    assert same(npy(rec["qoe"]).reshape(N, 2)[:, 1], npy(env.episode_qoe()))


# ---------------------------------------------------------------------------------------------------------------------
# 2. CBR sizes are the identity

def twins(build_a, build_b):
    """two environments that start from the same bytes (the workspace is allocated uninitialised)"""
    first = build_a()
    start(first)
    sd = first.state_dict()
    first.close()
    envs = [build_a(), build_b()]
    for e in envs:
        e.load_state_dict(sd)
    return envs


@pytest.mark.parametrize("impl", IMPLS)
def test_cbr_sizes_are_the_identity(impl):
    ladder, B, _, _ = tables()
    for auto in (False, True):
        plain, sized = twins(lambda: make(ladder=ladder, impl=impl, auto_reset=auto),
                             lambda: make(ladder=ladder, sizes=B * L, impl=impl, auto_reset=auto))
        assert sized.general_instance() and not plain.general_instance()
        assert sized.sz_table is not None and plain.sz_table is None
        acts = torch.from_numpy(np.random.default_rng(2).integers(0, 3, (V, N)).astype(np.int32)).cuda()
        for e in (plain, sized):
            e.out1 = e.step_script(acts[:4].contiguous())
            e.out2 = e.step_random(V + 3, seed=5) if auto else e.step_script(acts[4:].contiguous())
        torch.cuda.synchronize()
        for o in ("out1", "out2"):
            for k, v in getattr(plain, o).items():
                assert same(v, getattr(sized, o)[k]), (auto, o, k)
        assert torch.equal(plain.workspace, sized.workspace), auto


# ---------------------------------------------------------------------------------------------------------------------
# 3. separation: the size table moves the state, the bitrate table moves the score

def test_separation(oracle):
    """(B, S) against (B' = E, no size table) on the same lanes and actions: both download E * L, so every state row is
    equal; the first scores the variance on B, the second on E.  Read as: the rewards are each run's own table's on the
    SAME frames, equal where the variance terms agree (step 0 has none) and different wherever they differ by more than
    float32's resolution of the reward."""
    ladder, B, E, S = tables(seed=6)
    one, two = make(ladder=ladder, sizes=S), make(br=E)
    assert one.general_instance() and not two.general_instance()
    tid, off = start(one)
    start(two)
    acts = np.random.default_rng(4).integers(0, 3, (N, V)).astype(np.int32)
    dev = torch.from_numpy(np.ascontiguousarray(acts.T)).cuda()
    rew = []
    for s in range(V):
        fa, fb = one.observe_f64(), two.observe_f64()
        for k in helpers.F64_EXACT + ["last_bandwidth", "chunk_id", "hist_n", "hist_sum_inv"]:
            assert same(fa[k], fb[k]), (s, k)
        rew.append((npy(one.step(dev[s].contiguous())[1]).copy(), npy(two.step(dev[s].contiguous())[1]).copy()))
    cfg = oracle.env_cfg(ladder, L, V, MB, SU, 1.0, W, 1.0, br_table=E)
    steps, _, fin, _ = oracle.env_batch(cfg, TRACES, tid, off, acts)
    args = (steps["rebuffer_time"], steps["start_up_time"], fin["rebuffer_time"], fin["start_up_time"], acts, W)
    wantB, wantE = oracle.step_rewards(*args, br_table=B), oracle.step_rewards(*args, br_table=E)
    r1, r2 = np.stack([r[0] for r in rew], 1), np.stack([r[1] for r in rew], 1)
    assert same(r1, wantB) and same(r2, wantE)
    idx = np.arange(V)[None, :]
    vB, vE = np.zeros((N, V)), np.zeros((N, V))
    vB[:, 1:] = np.abs(B[idx, acts][:, 1:] - B[idx, acts][:, :-1])
    vE[:, 1:] = np.abs(E[idx, acts][:, 1:] - E[idx, acts][:, :-1])
    assert np.array_equal(r1[:, 0], r2[:, 0])
    far = np.abs(vB - vE) > 1e-3
    assert far.any() and (r1[far] != r2[far]).all() and (r1[vB == vE] == r2[vB == vE]).all()
    # the nominal score alone: switching between rungs costs exactly the ladder's step, staying costs nothing
    stay = np.zeros((N, V), bool)
    stay[:, 1:] = acts[:, 1:] == acts[:, :-1]
    base = oracle.step_rewards(*args[:4], np.zeros_like(acts), W, br_table=B)
    assert np.array_equal(r1[stay], base[stay]) and (r1[~stay][vB[~stay] > 0] != base[~stay][vB[~stay] > 0]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. latching

def test_latching_and_checkpoints():
    ladder, B, E, S = tables(seed=8)
    env, plain, sized = make(ladder=ladder), make(ladder=ladder), make(ladder=ladder, sizes=S)
    acts = torch.from_numpy(np.random.default_rng(3).integers(0, 3, (V, N)).astype(np.int32)).cuda()
    for e in (env, plain, sized):
        tid, off = start(e)
    keys = ("obs", "reward", "done")
    a, b = env.step_script(acts[:2].contiguous()), plain.step_script(acts[:2].contiguous())
    assert all(same(a[k], b[k]) for k in keys)
    t = env.set_chunk_sizes(S)                                   # mid-episode: pending, nothing changes
    assert env.sz_table is t and env.general_instance()          # 0x100 already while pending
    a, b = env.step_script(acts[2:].contiguous()), plain.step_script(acts[2:].contiguous())
    assert all(same(a[k], b[k]) for k in keys)
    assert same(env.episode_qoe(), plain.episode_qoe())
    mask = torch.zeros(N, dtype=torch.uint8)
    mask[::2] = 1
    with pytest.raises(_lib.AbrError, match="abr_env_set_size_table"):
        env.reset(torch.from_numpy(tid), torch.from_numpy(off), mask=mask)
    start(env)                                                   # the full reset adopts it
    a, c = env.step_script(acts[:3].contiguous()), sized.step_script(acts[:3].contiguous())
    assert all(same(a[k], c[k]) for k in keys) and not same(a["reward"], b["reward"][:3])
    # state_dict / load_state_dict with the table set, mid-episode
    sd = env.state_dict()
    again = make(ladder=ladder, sizes=S)
    again.load_state_dict(sd)
    a, c = env.step_script(acts[3:].contiguous()), again.step_script(acts[3:].contiguous())
    assert all(same(a[k], c[k]) for k in keys)
    assert same(env.observe_f64()["global_time"], again.observe_f64()["global_time"])
    assert same(env.episode_qoe(), again.episode_qoe())
    # None restores bitrate x chunk_length, again at the next full reset
    assert env.set_chunk_sizes(None) is None and env.sz_table is None
    start(env)
    start(plain)
    assert not env.general_instance()
    a, b = env.step_script(acts), plain.step_script(acts)
    assert all(same(a[k], b[k]) for k in keys) and same(env.episode_qoe(), plain.episode_qoe())


def test_mpd_sizes_are_opt_in(oracle):
    """an MPD carrying Chunk.sizes: ignored by default (CBR downloads, as ever), downloaded under chunk_sizes='mpd'"""
    ladder, B, E, S = tables(seed=9)
    chunks = [A.Chunk(ladder, list(S[c])) for c in range(V)]
    mk = lambda **kw: A.BatchedABREnv(A.MPD(V, L, MB, SU, chunks), A.QOEMetric(*W), A.NetworkInfo(1.0, TRACES), N, device="cuda", **kw)
    default, opted, plain = mk(), mk(chunk_sizes="mpd"), make(ladder=ladder)
    assert default.sz_table is None and not default.general_instance()
    assert same(opted.sz_table, S)
    acts = torch.from_numpy(np.random.default_rng(3).integers(0, 3, (V, N)).astype(np.int32)).cuda()
    for e in (default, opted, plain):
        tid, off = start(e)
        e.out = e.step_script(acts)
    assert same(default.out["reward"], plain.out["reward"]) and same(default.out["obs"], plain.out["obs"])
    cfg = oracle.env_cfg(ladder, L, V, MB, SU, 1.0, W, 1.0, br_table=E)
    steps, bw, fin, _ = oracle.env_batch(cfg, TRACES, tid, off, np.ascontiguousarray(npy(acts).T))
    assert same(opted.observe_f64()["global_time"], np.ascontiguousarray(fin["global_time"]))


# ---------------------------------------------------------------------------------------------------------------------
# 5. tree walks

@pytest.mark.parametrize("H", (2, 3))
@pytest.mark.parametrize("quality", (False, True))
def test_lookahead_under_a_size_table(H, quality):
    ladder, B, E, S = tables(seed=10)
    env, plain = make(ladder=ladder, sizes=S), make(ladder=ladder)
    if quality:
        env.set_quality(3.0, "log")
        plain.set_quality(3.0, "log")
    for e in (env, plain):
        start(e)
        TL.advance(e, 2)
    lab, _ = TL.expect(env, H)                                   # restore, step_script every sequence, the key in numpy
    assert (lab["action"] >= 0).all()
    base = A.LookaheadExpert(A.EnvPlayer(plain), H).labels()
    assert not torch.equal(lab["key"], base["key"])
    TL.advance(env, 3, seed=8)                                   # chunk 5: the horizon shrinks to 1
    TL.expect(env, H)


def constant_world_reference(env, F, H):
    """TL.reference with the traces overwritten in place so that lane i's trace (trace_id = arange) is F[i] everywhere:
    what a walk on the forecast F must answer.  The traces are put back."""
    n = env.n_lanes
    assert env.n_traces == n and np.array_equal(npy(env.trace_id), np.arange(n))
    saved = env.traces.clone()
    ln = npy(env.trace_len).astype(np.int64)
    env.traces.copy_(torch.from_numpy(np.repeat(np.asarray(F, np.float64), ln)))
    ref = TL.reference(env, H)
    env.traces.copy_(saved)
    return ref


@pytest.mark.parametrize("quality", (False, True))
def test_forecast_mpc_under_a_size_table(quality):
    ladder, B, E, S = tables(seed=11)
    rng = np.random.default_rng(12)
    traces = [rng.uniform(0.5, 6.0, int(rng.integers(30, 60))) for _ in range(N)]       # one trace per lane
    env = make(ladder=ladder, sizes=S, traces=traces)
    if quality:
        env.set_quality(3.0, "log")
    env.reset(torch.arange(N, dtype=torch.int32), torch.from_numpy(rng.integers(0, 30, N).astype(np.int32)))
    TL.advance(env, 2)
    ctl = A.ForecastMPCController(A.EnvPlayer(env), 2, window=3, robust=False)
    given = rng.uniform(0.4, 5.0, N)
    for forecast in (given, None):
        got = ctl.select(want_q=True, want_forecast=True,
                         forecast=None if forecast is None else torch.from_numpy(forecast).cuda())
        F = npy(got["forecast"])
        if forecast is not None:
            assert same(F, forecast)
        assert (F > 0).all()
        a, k, q = constant_world_reference(env, F, 2)
        assert np.array_equal(npy(got["action"]), a) and (a >= 0).all()
        assert same(got["key"], k) and same(got["q"], q)
    # step_plan over 6 decisions == select + step
    loop, fused = make(ladder=ladder, sizes=S), make(ladder=ladder, sizes=S)
    for e in (loop, fused):
        if quality:
            e.set_quality(3.0, "log")
        start(e)
    out = fused.step_plan(A.ForecastMPCController(A.EnvPlayer(fused), 2, window=3, robust=False), V)
    lc = A.ForecastMPCController(A.EnvPlayer(loop), 2, window=3, robust=False)
    for s in range(V):
        act = lc.next_bitrate()
        obs, r, d = loop.step(act)
        assert same(out["actions"][s], act) and same(out["reward"][s], r) and same(out["done"][s], d), s
        assert same(out["obs"][s], obs), s
    if quality:                                                  # (a pure cost is minimised by bitrate 0 throughout)
        assert len(np.unique(npy(out["actions"]))) > 1


# ---------------------------------------------------------------------------------------------------------------------
# 6. rules

def rule_cases(env):
    p = A.EnvPlayer(env)
    return [(A.BufferBasedController(p, reservoir=2.0, cushion=10.0), dict(kind=rules_twin.BUFFER, reservoir=2.0, cushion=10.0)),
            (A.RateBasedController(p, window=3, safety=0.9), dict(kind=rules_twin.RATE, window=3, safety=0.9)),
            (A.BolaController(p, gamma_p=1.0, v=4.0), dict(kind=rules_twin.BOLA, v=4.0, gp=1.0))]


def twin_rule(env, params, Btab, Stab, utility):
    f = {k: npy(v) for k, v in env.observe_f64().items()}
    hist = npy(env.history()[1])                                 # [V, N]
    dn = npy(env.done_after_reset())
    out = np.full(env.n_lanes, -1, np.int32)
    for i in range(env.n_lanes):
        if dn[i]:
            continue
        c = int(f["chunk_id"][i])
        br = Btab[c] if params["kind"] == rules_twin.BUFFER else Stab[c] / L
        out[i] = rules_twin.rule_scalar(params, c, f["buffer_level"][i], hist[:, i], br, None if utility is None else utility[c])
    return out


@pytest.mark.parametrize("which", (0, 1, 2))
@pytest.mark.parametrize("impl", ("jump", "tick"))
def test_rules_under_a_size_table(which, impl):
    ladder, B, E, S = tables(seed=4)
    assert any(np.any(np.diff(S[c] / L) < 0) for c in range(V))  # e is not ascending on some chunk
    fused, loop = make(ladder=ladder, sizes=S, impl=impl), make(ladder=ladder, sizes=S, impl=impl)
    start(fused)
    start(loop)
    ctl, params = rule_cases(loop)[which]
    fctl = rule_cases(fused)[which][0]
    out = fused.step_rule(fctl, V)
    util = getattr(ctl, "utility", None)
    nominal_differs = 0
    for s in range(V):
        want = twin_rule(loop, params, B, S, util)
        nominal_differs += int((want != twin_rule(loop, params, B, B * L, util)).sum())
        got = ctl.next_bitrate()                                 # rule_select
        assert np.array_equal(npy(got), want), s
        assert np.array_equal(npy(out["actions"][s]), want), s
        _, r, _ = loop.step(got)
        assert same(out["reward"][s], r), s
    assert len(np.unique(npy(out["actions"]))) > 1
    assert (nominal_differs > 0) == (params["kind"] != rules_twin.BUFFER)


# ---------------------------------------------------------------------------------------------------------------------
# 7. learned policy

def mlp_layers(rng, F, widths, M):
    out, fan = [], F
    for w in widths + [M]:
        out.append((rng.normal(0, 1.5 / np.sqrt(fan), (w, fan)).astype(np.float32), rng.normal(0, 0.2, w).astype(np.float32)))
        fan = w
    return out


def gru_parts(rng, F, H, M, scale=0.6):
    f32 = np.float32
    cell = tuple((rng.standard_normal(s) * scale).astype(f32) for s in ((3 * H, F), (3 * H, H), (3 * H,), (3 * H,)))
    head = tuple((rng.standard_normal(s) * scale).astype(f32) for s in ((M, H), (M,)))
    return cell, head


def expected_features(env, Wn, Btab, Stab, norm):
    """(x [F, N] under the size table, x on the nominal table, cc, live, episode)"""
    f = {k: npy(v) for k, v in env.observe_f64().items()}
    hist = npy(env.history()[1])
    M = env.n_rates
    c = f["chunk_id"].astype(np.int64)
    live = (npy(env.done_after_reset()) == 0) & (c < V)
    cc = np.clip(c, 0, V - 1)
    nominal = T.features(Wn, M, V, cc, f["last_bitrate"].astype(np.int64), f["buffer_level"], f["global_time"],
                         f["play_time"], hist, lambda r: Btab[r], norm)
    x = nominal.copy()
    for m in range(M):
        i = 4 + Wn + m
        x[i] = ((Stab[cc, m] - norm[0][i]) * norm[1][i]).astype(np.float32)
    return x, nominal, cc, live, npy(env.episodes()["episode"]).astype(np.int64)


@pytest.mark.parametrize("kind", ("lane", "matrix", "gru", "gru_matrix", "population"))
def test_policy_features_under_a_size_table(kind):
    ladder, B, E, S = tables(seed=13)
    n = 300 if kind == "population" else N                       # two members of 256 lanes, the second partial
    M, Wn = 3, 4
    F = 4 + Wn + M
    rng = np.random.default_rng(21)
    norm = np.stack([rng.uniform(-0.5, 0.5, F), rng.uniform(0.05, 0.5, F)])
    env, plain = make(n, ladder=ladder, sizes=S), make(n, ladder=ladder)
    kw = dict(window=Wn, norm=(norm[0], norm[1]), seed=5)
    members = None
    if kind in ("lane", "matrix"):
        layers = mlp_layers(rng, F, [16], M)
        mk = lambda e: A.PolicyController(A.EnvPlayer(e), layers, engine=kind, **kw)
    elif kind == "population":
        members = [mlp_layers(rng, F, [16], M) for _ in range(2)]
        mk = lambda e: A.PolicyPopulation(A.EnvPlayer(e), members, group=256, **kw)
    else:
        cell, head = gru_parts(rng, F, 8, M)
        mk = lambda e: A.RecurrentPolicyController(A.EnvPlayer(e), cell, head, engine="matrix" if kind == "gru_matrix" else "lane", **kw)
    ctl, pctl = mk(env), mk(plain)
    seen = set()
    for e in (env, plain):
        start(e)
    for upto in (0, 2):
        if upto:
            acts = torch.from_numpy(np.random.default_rng(3).integers(0, M, (upto, n)).astype(np.int32)).cuda()
            env.step_script(acts)
            plain.step_script(acts)
        out = ctl.select()
        x, nominal, cc, live, ep = expected_features(env, Wn, B, S, norm)
        assert live.all()
        got = npy(out["features"])
        for i in range(F):
            assert same(got[i], x[i]), (upto, i)
        assert same(got[:4 + Wn], nominal[:4 + Wn]) and not same(got[4 + Wn:], nominal[4 + Wn:])
        lane = np.arange(n)
        if kind in ("lane", "matrix"):
            a, s, _ = T.decide(layers, x, 5, 0, lane, cc, ep, M)
        elif kind == "population":
            a, s = np.zeros(n, np.int64), np.zeros((M, n), np.float32)
            for m in range(2):
                sl = slice(256 * m, min(256 * (m + 1), n))
                a[sl], s[:, sl], _ = T.decide(members[m], x[:, sl], 5, 0, lane[sl], cc[sl], ep[sl], M)
        else:
            o, _ = GT.select(list(cell) + list(head), x, npy(ctl.hidden), live, 5, 0, lane, cc, ep, M)
            a, s = o["actions"], o["scores"]
        assert same(out["scores"], np.asarray(s, np.float32)), upto
        assert np.array_equal(npy(out["actions"]), a), upto
        seen.update(np.unique(a).tolist())
        # the plain environment's features 4 + W + m are the bitrates
        pout = npy(pctl.select()["features"])
        pstate = expected_features(plain, Wn, B, S, norm)[1]
        assert same(pout, pstate)
    assert len(seen) > 1


# ---------------------------------------------------------------------------------------------------------------------
# 8. hindsight search

def test_hindsight_search_is_exhaustive_under_a_size_table():
    Vv, M = 4, 3
    ladder, B, E, S = tables(seed=14, Vv=Vv)
    beam = M ** (Vv - 1)
    n = beam * M                                                 # 81 lanes: one group
    env, brute = make(n, ladder=ladder, sizes=S, Vv=Vv), make(n, ladder=ladder, sizes=S, Vv=Vv)
    for e in (env, brute):
        e.set_quality(1.0, "identity")
    got = A.HindsightSearch(env, beam).run([5], [17])
    brute.reset(torch.full((n,), 5, dtype=torch.int32), torch.full((n,), 17, dtype=torch.int32))
    seqs = np.array(list(itertools.product(range(M), repeat=Vv)), np.int32)            # [81, V]
    brute.step_script(torch.from_numpy(np.ascontiguousarray(seqs.T)).cuda())
    assert (npy(brute.done_after_reset()) == _lib.DONE_EPISODE).all()
    q = npy(brute.episode_qoe(quality=True))
    assert int(npy(got["valid"])[0]) == 1
    assert same(npy(got["qoe"])[:1], np.array([q.min()]))
    best = seqs[int(np.argmin(q))]
    assert q[(seqs == npy(got["actions"])[:, 0]).all(1)][0] == q.min() and len(np.unique(q)) > 1
    # and the table matters: the same search without it finds another optimum value
    other = make(n, ladder=ladder, Vv=Vv)
    other.set_quality(1.0, "identity")
    assert npy(A.HindsightSearch(other, beam).run([5], [17])["qoe"])[0] != q.min()
    assert best.shape == (Vv,)


# ---------------------------------------------------------------------------------------------------------------------
# 9. fork

def test_fork_under_a_size_table():
    ladder, B, E, S = tables(seed=15)
    a, b = make(ladder=ladder, sizes=S), make(ladder=ladder, sizes=S)
    acts = np.random.default_rng(6).integers(0, 3, (V, N)).astype(np.int32)
    for e in (a, b):
        start(e)
        e.step_script(torch.from_numpy(acts[:2]).cuda())
    src = (np.arange(N) + 1) % N                                 # lane i continues as lane i + 1: a cycle
    b.fork(torch.from_numpy(src.astype(np.int32)).cuda())
    rest = acts[2:]
    oa = a.step_script(torch.from_numpy(rest).cuda())
    ob = b.step_script(torch.from_numpy(np.ascontiguousarray(rest[:, src])).cuda())
    idx = torch.from_numpy(src).cuda()
    assert same(ob["reward"], oa["reward"][:, idx]) and same(ob["done"], oa["done"][:, idx])
    assert same(ob["obs"], oa["obs"][:, :, idx])
    fa, fb = a.observe_f64(), b.observe_f64()
    for k in helpers.F64_EXACT + ["last_bandwidth"]:
        assert same(fb[k], fa[k][idx]), k
    assert same(b.episode_qoe(), a.episode_qoe()[idx])


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals and validation

def test_validation_and_refusals():
    ladder, B, E, S = tables(seed=16)
    for bad in ("sizes", S[:5], S[:, :2], np.where(np.arange(3) == 1, 0.0, S), -S, S * np.nan,
                np.where(np.arange(3) == 2, np.inf, S), np.where(np.arange(3) == 0, 2.0 ** 960, S)):
        with pytest.raises(ValueError):
            make(ladder=ladder, sizes=bad)
    env = make(ladder=ladder)
    with pytest.raises(ValueError):
        env.set_chunk_sizes(S[:, ::-1][:, :2])
    assert env.sz_table is None and not env.general_instance()
    env.set_chunk_sizes(S)                                       # no episode in flight: at once
    assert env.general_instance()
    sh = A.ShardedABREnv(A.MPD(V, L, MB, SU, A.Chunk(ladder)), A.QOEMetric(*W), A.NetworkInfo(1.0, TRACES), total_lanes=N,
                         fuse=V, rank=0, world=1, gather=False, chunk_sizes=S)
    assert same(sh.env.sz_table, S)


@pytest.mark.parametrize("impl", ("async", "ring3", "pair3"))
def test_diagnostic_pipelines_refuse_a_size_table(impl):
    lib = helpers.diag_lib()
    ladder, B, E, S = tables(seed=16)
    env = make(ladder=ladder, sizes=S, impl=impl, library=lib)
    start(env)                                                   # the reset is the one-thread-per-lane kernel's
    with pytest.raises(_lib.AbrError, match="size table"):
        env.step_random(4, seed=1)
