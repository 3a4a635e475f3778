"""The episode sampler on the device (include/abr_env.h: abr_episode_sampler): fused auto-reset rollouts of every launch kind,
on every implementation each runs on, replayed episode by episode through the oracle from the numpy twin's drawn
(trace, offset) and the reported actions -- rewards, done bytes and float32 observations element by element across every
episode boundary, MPC's actions too; episodes() after each launch; shards, checkpoints, time-outs, masked sampled resets
and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import oracle_rewards
import abrsimulator_amd as A
from abrsimulator_amd import _lib
from abrsimulator_amd.episodes import EpisodeSampler

pytestmark = pytest.mark.gpu

LADDER = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
V, L, MB, SU, W = 8, 4.0, 20.0, 4.0, [4.3, 1.0, 1.0, 0.1]
N = 200                      # three full workgroups of 64 and a partial one
T = 3 * V + 3                # every lane crosses three episode boundaries
OBS = _lib.OBS_ROWS


def corpus(seed=0, n=7):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.3, 6.0, int(rng.integers(20, 300))) for _ in range(n)]


TRACES = corpus()
TL = np.array([len(t) for t in TRACES], np.int32)


def make(impl="auto", n=N, base=0, traces=TRACES, **kw):
    return A.BatchedABREnv(A.MPD(V, L, MB, SU, A.Chunk(LADDER)), A.QOEMetric(*W), A.NetworkInfo(1.0, traces), n,
                           device="cuda", auto_reset=True, impl=impl, lane_id_base=base, **kw)


def armed(env, smp, pool=None, span=0):
    env.set_episode_sampler(smp.seed, pool, span)
    env.reset(sample=True)
    return env


def np_out(out):
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def check_episodes(env, smp, base=0):
    ep = {k: v.cpu().numpy() for k, v in env.episodes().items()}
    t, off = smp.draw(base + np.arange(env.n_lanes, dtype=np.uint64), ep["episode"], TL)
    assert np.array_equal(ep["trace_id"], t) and np.array_equal(ep["start_offset"], off)
    return ep


def check_rollout(oracle, out, smp, e0, base=0, mpc_cfg=None, mpc_tables=None):
    """out: numpy outputs of fused decisions that start at chunk 0 of episode e0 (every lane); every episode ends after
    exactly V decisions.  Each episode k runs the twin's pair for episode e0 + k."""
    acts, rew, done, obs = out["actions"], out["reward"], out["done"], out["obs"]
    n_steps, n = rew.shape
    g = base + np.arange(n, dtype=np.uint64)
    cfg = oracle.env_cfg(LADDER, L, V, MB, SU, 1.0, W, 1.0)
    assert (done & ~np.uint8(_lib.DONE_EPISODE) == 0).all(), "a lane timed out or was frozen"
    n_ep = -(-n_steps // V)
    reps = []
    for k in range(n_ep + 1):
        tid, off = smp.draw(g, e0 + k, TL)
        s0, m = k * V, max(0, min(V, n_steps - k * V))
        a = np.zeros((n, V), np.int32)
        a[:, :m] = np.clip(acts[s0:s0 + m].T, 0, len(LADDER) - 1)
        steps, bw, fin, _ = oracle.env_batch(cfg, TRACES, tid, off, a)
        reps.append((s0, m, a, steps, fin))
        if mpc_cfg is not None and m:
            _, _, want, _ = oracle.env_batch_mpc(cfg, mpc_cfg, *mpc_tables, TRACES, tid, off)
            assert np.array_equal(acts[s0:s0 + m].T, want[:, :m]), k
    for k in range(n_ep):
        s0, m, a, steps, fin = reps[k]
        rw = oracle_rewards(steps, fin, a, W, ladder=LADDER)
        for s in range(m):
            t = s0 + s
            assert np.array_equal(rew[t], rw[:, s]), ("reward", t)
            assert np.array_equal(done[t], np.full(n, 1 if s == V - 1 else 0, np.uint8)), ("done", t)
            nxt = reps[k][3] if s < V - 1 else reps[k + 1][3]
            col = s + 1 if s < V - 1 else 0
            for r, key in enumerate(OBS):
                assert np.array_equal(obs[t, r], nxt[key][:, col].astype(np.float32)), ("obs." + key, t)


def rollout_and_check(oracle, env, smp, launch, n_steps=T, **kw):
    e0 = env.episodes()["episode"].cpu().numpy()
    assert (e0 == e0[0]).all() and (env.observe_f64()["chunk_id"].cpu().numpy() == 0).all()
    out = np_out(launch(env, n_steps))
    check_rollout(oracle, out, smp, int(e0[0]), **kw)
    ep = check_episodes(env, smp)
    assert (ep["episode"] == e0 + n_steps // V).all()
    return out


SMP = EpisodeSampler(0x5EED_0F_EB150DE5, offset_span=0)
ALL = ["tick", "jump", "split", "split3"]


@pytest.mark.parametrize("impl", ALL)
def test_step_random_and_step_script(oracle, impl):
    env = armed(make(impl), SMP)
    check_episodes(env, SMP)
    out = rollout_and_check(oracle, env, SMP, lambda e, n: e.step_random(n, 77))
    ref = np_out(armed(make("jump"), SMP).step_random(T, 77))
    for k in ("reward", "done", "obs", "actions"):
        assert np.array_equal(out[k], ref[k]), (impl, k)           # every implementation, bit for bit
    script = np.random.default_rng(3).integers(0, 6, (T, N)).astype(np.int32)
    env = armed(make(impl), SMP)
    out = np_out(env.step_script(torch.from_numpy(script).cuda()))
    out["actions"] = script
    check_rollout(oracle, out, SMP, 0)
    check_episodes(env, SMP)


@pytest.mark.parametrize("impl", ["jump", "tick"])
@pytest.mark.parametrize("kind", ["rate", "fastmpc"])
def test_step_rule(oracle, impl, kind):
    env = armed(make(impl), SMP)
    ctl = (A.RateBasedController(A.EnvPlayer(env), window=3) if kind == "rate"
           else A.FastMPCController(A.EnvPlayer(env), horizon=3, device="cuda"))
    rollout_and_check(oracle, env, SMP, lambda e, n: e.step_rule(ctl, n))


@pytest.mark.parametrize("impl", ["jump", "split", "split3"])
@pytest.mark.parametrize("method", ["harmonic", "robust"])
def test_step_mpc(oracle, impl, method):
    env = armed(make(impl), SMP)
    ctl = A.BatchedMPCController(A.EnvPlayer(env), horizon=3, clip_horizon=True, method=method)
    kw = {}
    if method == "harmonic":
        br = np.tile(np.asarray(LADDER), (V, 1))
        kw = dict(mpc_cfg=oracle.mpc_cfg(6, 3, V, L, MB, W[1], W[0], 0.0), mpc_tables=(br, br * L))
    rollout_and_check(oracle, env, SMP, lambda e, n: e.step_mpc(ctl, n), **kw)


@pytest.mark.parametrize("impl", ["jump", "split", "split3"])
def test_step_policy(oracle, impl):
    smp = EpisodeSampler(SMP.seed, pool=[1, 4, 6], offset_span=50)
    env = armed(make(impl), smp, pool=[1, 4, 6], span=50)
    rng = np.random.default_rng(5)
    layers, fan = [], 4 + 4 + 6
    for w in (16, 6):
        layers.append((rng.normal(0, 1.5 / np.sqrt(fan), (w, fan)).astype(np.float32), rng.normal(0, 0.2, w).astype(np.float32)))
        fan = w
    ctl = A.PolicyController(A.EnvPlayer(env), layers, window=4, explore=0.25, seed=9)
    out = rollout_and_check(oracle, env, smp, lambda e, n: e.step_policy(ctl, n))
    tid = env.episodes()["trace_id"].cpu().numpy()
    assert np.isin(tid, [1, 4, 6]).all() and (env.episodes()["start_offset"].cpu().numpy() < 50).all()
    assert len(np.unique(out["actions"])) > 1


def test_fused_launch_equals_single_steps_and_sampling_off_restores_the_old_rearm():
    script = np.random.default_rng(8).integers(0, 6, (T, N)).astype(np.int32)
    a = armed(make(), SMP)
    fused = np_out(a.step_script(torch.from_numpy(script).cuda()))
    b = armed(make(), SMP)
    for t in range(T):
        o, r, d = b.step(torch.from_numpy(script[t]).cuda())
        assert np.array_equal(r.cpu().numpy(), fused["reward"][t]) and np.array_equal(d.cpu().numpy(), fused["done"][t])
        assert np.array_equal(o.cpu().numpy(), fused["obs"][t]), t
    assert np.array_equal(a.episodes()["trace_id"].cpu().numpy(), b.episodes()["trace_id"].cpu().numpy())
    # set_episode_sampler(None): re-arms go back to the lane's current pair
    b.set_episode_sampler(None)
    before = {k: v.cpu().numpy() for k, v in b.episodes().items()}
    b.step_random(2 * V, 1)
    after = {k: v.cpu().numpy() for k, v in b.episodes().items()}
    assert np.array_equal(before["trace_id"], after["trace_id"]) and np.array_equal(before["start_offset"], after["start_offset"])
    assert (after["episode"] >= before["episode"] + 1).all()


@pytest.mark.parametrize("impl", ["auto", "split3"])
def test_two_shards_reproduce_the_unsharded_env(impl):
    whole = armed(make(impl), SMP)
    want = np_out(whole.step_random(T, 4))
    got = []
    for base, n in ((0, 120), (120, 80)):
        sh = A.ShardedABREnv(A.MPD(V, L, MB, SU, A.Chunk(LADDER)), A.QOEMetric(*W), A.NetworkInfo(1.0, TRACES),
                             total_lanes=n, device="cuda", rank=0, world=1, gather=False,
                             env=make(impl, n=n, base=base))
        sh.set_episode_sampler(SMP.seed)
        sh.reset(sample=True)
        got.append((base, n, np_out(sh.env.step_random(T, 4)), sh.env))
    for base, n, o, e in got:
        for k in ("reward", "done", "obs", "actions"):
            assert np.array_equal(o[k], want[k][..., base:base + n]), (base, k)
        check_episodes(e, SMP, base=base)


def test_checkpoint_mid_rollout_continues_identically():
    a = armed(make(), SMP)
    a.step_random(V + 3, 11)
    sd = a.state_dict()
    want = np_out(a.step_random(T, 12))
    b = make()
    b.set_episode_sampler(SMP.seed)
    b.load_state_dict(sd)
    got = np_out(b.step_random(T, 12))
    for k in ("reward", "done", "obs", "actions"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("trace_id", "start_offset", "episode"):
        assert torch.equal(a.episodes()[k], b.episodes()[k]), k


def test_timeouts_are_not_rearmed_and_a_masked_sampled_reset_touches_only_masked_lanes():
    traces = [np.full(40, 0.01), np.random.default_rng(1).uniform(4.0, 8.0, 100)]       # trace 0 cannot finish in time
    env = make("jump", traces=traces, max_ticks=(V + 2) * 400)
    smp = EpisodeSampler(3, pool=[0, 1])
    env.set_episode_sampler(3, pool=[0, 1])
    env.reset(sample=True)
    out = np_out(env.step_random(T, 2))
    d = out["done"]
    slow = env.episodes()["trace_id"].cpu().numpy() == 0
    timed = ((d & _lib.DONE_TIMEOUT) != 0).any(0)
    assert timed.any() and (timed == slow).all()
    ends = ((d & _lib.DONE_EPISODE) != 0).sum(0)
    ep = {k: v.cpu().numpy() for k, v in env.episodes().items()}
    assert np.array_equal(ep["episode"], ends)                                            # one re-arm per finished episode
    for i in np.flatnonzero(timed):
        t0 = int(np.argmax((d[:, i] & _lib.DONE_TIMEOUT) != 0))
        assert (d[t0:, i] == d[t0, i]).all() and (out["actions"][t0 + 1:, i] == -1).all()
    lens = np.array([len(t) for t in traces], np.int32)
    t, off = smp.draw(np.arange(N, dtype=np.uint64), ep["episode"], lens)
    assert np.array_equal(ep["trace_id"], t) and np.array_equal(ep["start_offset"], off)
    # masked sampled reset
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    f_before = env.observe_f64()
    env.reset(sample=True, mask=torch.from_numpy(mask))
    ep2 = {k: v.cpu().numpy() for k, v in env.episodes().items()}
    f_after = env.observe_f64()
    m = mask.astype(bool)
    assert np.array_equal(ep2["episode"][~m], ep["episode"][~m]) and np.array_equal(ep2["episode"][m], ep["episode"][m] + 1)
    t, off = smp.draw(np.arange(N, dtype=np.uint64), ep2["episode"], lens)
    assert np.array_equal(ep2["trace_id"], t) and np.array_equal(ep2["start_offset"], off)
    for k in ("global_time", "buffer_level", "chunk_id"):
        assert torch.equal(f_before[k][torch.from_numpy(~m).cuda()], f_after[k][torch.from_numpy(~m).cuda()]), k
    assert (f_after["chunk_id"].cpu().numpy()[m] == 0).all()
    assert np.array_equal(env.trace_id.cpu().numpy(), ep2["trace_id"])


def test_refusals():
    env = make()
    with pytest.raises(ValueError):
        env.set_episode_sampler(1, pool=[0, len(TRACES)])
    with pytest.raises(ValueError):
        env.set_episode_sampler(1, offset_span=-1)
    with pytest.raises(ValueError):
        env.reset(sample=True)                                        # no sampler
    env.set_episode_sampler(1)
    with pytest.raises(ValueError):
        env.reset(torch.zeros(N, dtype=torch.int32), sample=True)
    # the C ABI checks the pool itself (read back from the device) and refuses before storing anything
    lib = env.lib
    bad = torch.tensor([0, 99], dtype=torch.int32, device="cuda")
    s = _lib.EpisodeSampler(seed=1, pool=bad.data_ptr(), n_pool=2, offset_span=0)
    assert lib.abr_env_set_episode_sampler(env._h, C.byref(s)) == -1 and b"pool[1]" in lib.abr_last_error()
    env.set_episode_sampler(None)
    assert lib.abr_env_reset(env._h, None, None, None, None, None) == -1          # NULL ids without a sampler
