"""The bitrate rules on the device (abr_env_step_rule / abr_env_rule_select): episodes against the C oracle driven by the
numpy twin (tests/rules_twin.py), full-size replays, the fused rollout against the host-driven loop and a script, the
tick kernel as a cross-check, auto-reset, per-chunk ladders, per-lane speeds, mixed policies, frozen lanes, refusals."""
import numpy as np
import pytest
import torch

import abrsimulator_amd as A
from helpers import golden_workload, make_env, oracle_env_cfg, oracle_rewards, threads
from rules_twin import params_of, rule_scalar, rule_vec

pytestmark = pytest.mark.gpu

# the defaults and a second parameter set each.  The workload is a live stream (a chunk becomes available only as the clock
# reaches it), so the buffer stays below ~2 chunks: the default BOLA (v ~ 2.1) and BBA-0 (reservoir 5 s) answer rate 0 almost
# everywhere; the second sets spread the answers over the ladder, and the single-set tests below use them (VARIED).
RULES = [("buffer", {}), ("buffer", dict(reservoir=1.0, cushion=6.0)),
         ("rate", {}), ("rate", dict(window=3, safety=0.8)),
         ("bola", {}), ("bola", dict(gamma_p=1.0, v=5.0))]
VARIED = {"buffer": dict(reservoir=1.0, cushion=6.0), "rate": {}, "bola": dict(gamma_p=1.0, v=5.0)}
CLS = {"buffer": A.BufferBasedController, "rate": A.RateBasedController, "bola": A.BolaController}
F64_FINAL = ["global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level"]


def _ctl(env, kind, kw):
    return CLS[kind](A.EnvPlayer(env), **kw)


def _rows(ctl, c, table):
    """Each lane's chunk-c bitrates and utilities for the vectorised twin."""
    c = np.minimum(np.asarray(c), table.shape[0] - 1)
    return table[c], (ctl.utility[c] if hasattr(ctl, "utility") else None)


def _twin_over_replay(ctl, steps, bw, table, s0=0):
    """The twin's action at every call site s >= s0 of the replayed frames: [V - s0, N]."""
    p = params_of(ctl)
    out = []
    for s in range(s0, steps.shape[1]):
        c = steps["chunk_id"][:, s]
        br, u = _rows(ctl, c, table)
        out.append(rule_vec(p, c, steps["buffer_level"][:, s], bw.T, br, u))
    return np.stack(out)


def _table(m, V):
    return np.tile(np.asarray(m["ladder"], np.float64), (V, 1))


@pytest.mark.parametrize("kind,kw", RULES)
def test_episodes_match_oracle_driven_by_twin(oracle, kind, kw):
    m, traces, tid, off = golden_workload(256)
    N, V = 256, m["video_length"]
    env = make_env(m, traces, N)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    ctl = _ctl(env, kind, kw)
    out = env.step_rule(ctl, V)
    acts = out["actions"].cpu().numpy()
    obs, rew, done = out["obs"].cpu().numpy(), out["reward"].cpu().numpy(), out["done"].cpu().numpy()
    p, table = params_of(ctl), _table(m, V)
    cfg = oracle_env_cfg(oracle, m)
    steps = np.zeros((N, V), oracle.STEP_DTYPE)
    fin = np.zeros(N, oracle.FINAL_DTYPE)
    want_a = np.zeros((N, V), np.int32)
    for i in range(N):
        pol = (lambda o, h: rule_scalar(p, o["chunk_id"], o["buffer_level"], h, table[o["chunk_id"]],
                                        ctl.utility[o["chunk_id"]] if kind == "bola" else None))
        st, _, a, f = oracle.env_episode_policy(cfg, traces[tid[i]], off[i], pol)
        steps[i], want_a[i], fin[i] = st, a, f
    assert np.array_equal(acts.T, want_a), (kind, kw)
    if kw or kind == "rate":
        assert len(np.unique(want_a)) >= 3, np.unique(want_a)
    assert np.array_equal(done, np.where(np.arange(V)[:, None] == V - 1, 1, 0).repeat(N, 1))
    assert np.array_equal(rew.T, oracle_rewards(steps, fin, want_a, m["weights"], ladder=m["ladder"]))
    for s in range(V - 1):
        assert np.array_equal(obs[s, 3], steps["buffer_level"][:, s + 1].astype(np.float32)), s
        assert np.array_equal(obs[s, 4], steps["global_time"][:, s + 1].astype(np.float32)), s
        assert np.array_equal(obs[s, 0], steps["chunk_id"][:, s + 1].astype(np.float32)), s
        assert np.array_equal(obs[s, 1], steps["last_bitrate"][:, s + 1].astype(np.float32)), s
    f = env.observe_f64()
    for k in F64_FINAL:
        assert np.array_equal(f[k].cpu().numpy(), fin[k]), k
    assert np.allclose(env.episode_qoe().cpu().numpy(), fin["qoe"], rtol=1e-10)


@pytest.mark.parametrize("kind", ["buffer", "rate", "bola"])
def test_full_size_replay(oracle, kind):
    N = 65536
    m, traces, tid, off = golden_workload(N, seed=11)
    V = m["video_length"]
    env = make_env(m, traces, N)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    ctl = _ctl(env, kind, VARIED[kind])
    out = env.step_rule(ctl, V)
    acts = out["actions"].cpu().numpy()
    assert (acts >= 0).all() and len(np.unique(acts)) >= 3
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid, off, np.ascontiguousarray(acts.T),
                                         threads=threads())
    assert np.array_equal(_twin_over_replay(ctl, steps, bw, _table(m, V)), acts)
    obs = out["obs"].cpu().numpy()
    for s in range(V - 1):
        for r, k in ((3, "buffer_level"), (4, "global_time"), (5, "play_time"), (6, "rebuffer_time"), (2, "last_bandwidth")):
            assert np.array_equal(obs[s, r], steps[k][:, s + 1].astype(np.float32)), (s, k)
    assert np.array_equal(env.observe_f64()["buffer_level"].cpu().numpy(), fin["buffer_level"])


def _same_state(a, b):
    """Every lane's state: the float64 frame, both history lists, the MPC-facing views (the workspace bytes of two handles
    also hold their tables' alignment padding, which nothing writes)."""
    fa, fb = a.observe_f64(), b.observe_f64()
    for k in fa:
        assert torch.equal(fa[k], fb[k]), k
    for x, y in zip(a.history(), b.history()):
        assert torch.equal(x, y)
    for x, y in zip(a.mpc_inputs(), b.mpc_inputs()):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind,kw", [RULES[1], RULES[3], RULES[5]])
def test_fused_equals_host_loop_and_script(kind, kw):
    m, traces, tid, off = golden_workload(1024, seed=3)
    N, n = 1024, 20
    envs = [make_env(m, traces, N) for _ in range(3)]
    for e in envs:
        e.reset(torch.from_numpy(tid), torch.from_numpy(off))
    out = envs[0].step_rule(_ctl(envs[0], kind, kw), n)
    ctl1 = _ctl(envs[1], kind, kw)
    for s in range(n):
        a = ctl1.next_bitrate()
        assert torch.equal(a, out["actions"][s]), s
        obs, rew, done = envs[1].step(a)
        assert torch.equal(obs, out["obs"][s]) and torch.equal(rew, out["reward"][s]) and torch.equal(done, out["done"][s])
    _same_state(envs[0], envs[1])
    # a script of the same actions under `auto` (the three-wave kernel at this size)
    assert envs[2].effective_impl(fused=True) == "split3"
    sc = envs[2].step_script(out["actions"])
    for k in ("obs", "reward", "done"):
        assert torch.equal(sc[k], out[k]), k
    _same_state(envs[0], envs[2])


@pytest.mark.parametrize("kind,kw", RULES)
def test_jump_equals_tick(kind, kw):
    m, traces, tid, off = golden_workload(512, seed=5)
    outs = []
    for impl in ("jump", "tick"):
        env = make_env(m, traces, 512, impl=impl)
        env.reset(torch.from_numpy(tid), torch.from_numpy(off))
        outs.append((env.step_rule(_ctl(env, kind, kw), m["video_length"]), env.observe_f64()))
    for k in ("obs", "reward", "done", "actions"):
        assert torch.equal(outs[0][0][k], outs[1][0][k]), k
    for k in F64_FINAL:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


@pytest.mark.parametrize("kind", ["buffer", "rate", "bola"])
def test_auto_reset_repeats_the_first_episode(kind):
    m, traces, tid, off = golden_workload(256, seed=9)
    V = m["video_length"]
    env = make_env(m, traces, 256, auto_reset=True)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    out = env.step_rule(_ctl(env, kind, VARIED[kind]), 2 * V + 10)
    a = out["actions"].cpu().numpy()
    assert (a >= 0).all()
    assert np.array_equal(a[V:2 * V], a[:V]) and np.array_equal(a[2 * V:], a[:10])
    d = out["done"].cpu().numpy()
    assert (d[V - 1] == 1).all() and (d[2 * V - 1] == 1).all() and (np.delete(d, [V - 1, 2 * V - 1], 0) == 0).all()
    assert torch.equal(out["reward"][V:2 * V], out["reward"][:V])


@pytest.mark.parametrize("kind", ["buffer", "rate", "bola"])
def test_per_chunk_bitrate_table(oracle, kind):
    m, traces, tid, off = golden_workload(128, seed=13)
    V, N = m["video_length"], 128
    rng = np.random.default_rng(2)
    table = np.sort(np.asarray(m["ladder"]) * rng.uniform(0.7, 1.3, (V, 1)) * rng.uniform(0.9, 1.1, (V, 6)), axis=1)
    mpd = A.MPD(V, m["chunk_length"], m["max_buffer"], m["start_up_length"], [A.Chunk(list(r)) for r in table])
    env = A.BatchedABREnv(mpd, A.QOEMetric(*m["weights"]), A.NetworkInfo(m["interval"], traces), N, device="cuda")
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    ctl = _ctl(env, kind, VARIED[kind])
    out = env.step_rule(ctl, V)
    acts = out["actions"].cpu().numpy()
    cfg = oracle_env_cfg(oracle, m, br_table=table)
    p = params_of(ctl)
    gt = env.observe_f64()["global_time"].cpu().numpy()
    for i in range(N):
        pol = (lambda o, h: rule_scalar(p, o["chunk_id"], o["buffer_level"], h, table[o["chunk_id"]],
                                        ctl.utility[o["chunk_id"]] if kind == "bola" else None))
        st, _, a, f = oracle.env_episode_policy(cfg, traces[tid[i]], off[i], pol)
        assert np.array_equal(acts[:, i], a), i
        assert gt[i] == f["global_time"], i


@pytest.mark.parametrize("kind", ["buffer", "rate", "bola"])
def test_per_lane_speeds(oracle, kind):
    m, traces, tid, off = golden_workload(512, seed=17)
    V, N = m["video_length"], 512
    speeds = np.random.default_rng(4).uniform(0.8, 1.3, N)
    env = make_env(dict(m, speed=torch.from_numpy(speeds)), traces, N)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    ctl = _ctl(env, kind, VARIED[kind])
    out = env.step_rule(ctl, V)
    acts = out["actions"].cpu().numpy()
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid, off, np.ascontiguousarray(acts.T),
                                         speeds=speeds, threads=threads())
    assert np.array_equal(_twin_over_replay(ctl, steps, bw, _table(m, V)), acts)
    obs = out["obs"].cpu().numpy()
    for s in range(V - 1):
        assert np.array_equal(obs[s, 3], steps["buffer_level"][:, s + 1].astype(np.float32)), s
    for k in F64_FINAL:
        assert np.array_equal(env.observe_f64()[k].cpu().numpy(), fin[k]), k


def test_random_then_rule_sees_the_random_history(oracle):
    m, traces, tid, off = golden_workload(512, seed=19)
    V, N, k = m["video_length"], 512, 7
    env = make_env(m, traces, N)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    r = env.step_random(k, 1234)
    ctl = _ctl(env, "rate", dict(window=10))
    out = env.step_rule(ctl, V - k)
    acts = np.concatenate([r["actions"].cpu().numpy(), out["actions"].cpu().numpy()])
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid, off, np.ascontiguousarray(acts.T),
                                         threads=threads())
    assert np.array_equal(_twin_over_replay(ctl, steps, bw, _table(m, V), s0=k), acts[k:])
    want = oracle_rewards(steps, fin, acts.T, m["weights"], ladder=m["ladder"])
    assert np.array_equal(out["reward"].cpu().numpy(), want.T[k:])
    assert np.allclose(env.episode_qoe().cpu().numpy(), fin["qoe"], rtol=1e-10)


def test_frozen_lanes_and_refusals():
    m, traces, tid, off = golden_workload(256, seed=23)
    tid = tid.copy()
    tid[::5] = 99                                       # out of range: frozen with ABR_DONE_BADARG
    env = make_env(m, traces, 256)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    ctl = _ctl(env, "bola", {})
    sel = ctl.next_bitrate().cpu().numpy()
    assert (sel[::5] == -1).all() and (np.delete(sel, np.s_[::5]) >= 0).all()
    out = env.step_rule(ctl, 5)
    a, d = out["actions"].cpu().numpy(), out["done"].cpu().numpy()
    assert (a[:, ::5] == -1).all() and (d[:, ::5] == A._lib.DONE_BADARG).all()
    assert (np.delete(a, np.s_[::5], 1) >= 0).all() and (np.delete(d, np.s_[::5], 1) == 0).all()
    assert (env.observe_f64()["chunk_id"].cpu().numpy()[::5] == 0).all()
    for impl in ("split", "split3"):
        e = make_env(m, traces, 64, impl=impl)
        e.reset()
        with pytest.raises(A._lib.AbrError, match="error -4"):
            e.step_rule(_ctl(e, "rate", VARIED["rate"]), 4)
