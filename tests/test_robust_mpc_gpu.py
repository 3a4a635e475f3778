"""RobustMPC on the device (abr_mpc_select_robust / abr_env_step_mpc_robust) against the numpy twin of its estimate
(tests/robust_twin.py) and the C oracle's brute-force search: standalone selects with their edges and the whole state,
idempotence, episodes driven through the oracle, the fused rollout against the host loop on every event-driven kernel,
auto-reset, a robust controller after random steps, a full-size replay, and the tick refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import abrsimulator_amd as A
from abrsimulator_amd import _lib
from helpers import golden_workload, make_env, oracle_env_cfg, oracle_rewards, thread_map, threads
from robust_twin import copy_state, empty_state, select_scalar, state_bytes, state_from_bytes

pytestmark = pytest.mark.gpu

F64_FINAL = ["global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level"]
H = 5


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


def _ocfg(oracle, m):
    w = m["weights"]          # QOEMetric(rebuffer, variance, startup, latency)
    return oracle.mpc_cfg(len(m["ladder"]), H, m["video_length"], m["chunk_length"], m["max_buffer"], w[1], w[0], w[2])


def _tables(m):
    br = np.tile(np.asarray(m["ladder"], np.float64), (m["video_length"], 1))
    return br, br * m["chunk_length"]


def _env_ctl(m, traces, tid, off, N, window=5, **kw):
    env = make_env(m, traces, N, **kw)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    return env, A.BatchedMPCController(A.EnvPlayer(env), horizon=H, clip_horizon=True, method="robust", window=window)


def _state(ctl, N):
    return state_from_bytes(ctl.robust_state(N).cpu().numpy(), N, ctl.window)


def _same_state(a, b):
    return (np.array_equal(a["cs1"], b["cs1"]) and np.array_equal(a["cnt"], b["cnt"])
            and np.array_equal(a["ps"].view(np.uint64), b["ps"].view(np.uint64))
            and np.array_equal(a["err"].view(np.uint64), b["err"].view(np.uint64)))


def _policy(oracle, ocfg, br, sz, W, st):
    """The oracle's policy callback for one lane: twin estimate + brute search, carrying the twin state `st` (1 lane)."""
    def pol(o, h):
        a, _, _ = select_scalar(oracle, ocfg, br, sz, W, int(o["chunk_id"]), int(o["last_bitrate"]),
                                float(o["buffer_level"]), h, st, 0)
        return max(a, 0)                                    # no decision downloads bitrate 0
    return pol


# ---------------------------------------------------------------------------------------------------------------------
# 1. / 2.  standalone select

def _select_inputs(seed, N=2000, B=6, V=30, W=5):
    rng = np.random.default_rng(seed)
    br = np.sort(rng.uniform(0.2, 6.0, B))[None, :] * rng.uniform(0.8, 1.2, (V, B))
    sz = br * 4.0 * rng.uniform(0.7, 1.3, (V, B))
    chunk = rng.integers(0, V, N).astype(np.int32)
    chunk[:40] = np.arange(40) % 3                                 # c = 0, 1, 2
    chunk[40:80] = V - 1 - np.arange(40) % (H - 1)                 # every clipped horizon (D12)
    prev = rng.integers(-1, B, N).astype(np.int32)
    prev[80:100] = rng.choice([-B - 1, -B, -3, B, B + 2], 20)       # Python's negative index and out-of-range values
    buf = rng.uniform(0.0, 20.0, N)
    buf[100:120] = 0.0
    hist = rng.uniform(0.2, 6.0, (V, N))
    chunk[120:140] = 10
    hist[:, 120:140] = 1e-300                                      # tiny throughputs: P underflows with a big error
    st = empty_state(N, W)
    rel = rng.random(N)
    st["cs1"][:] = np.where(rel < 0.2, 0, np.where(rel < 0.6, chunk, np.where(rel < 0.8, chunk + 1, chunk + 3)))
    st["cnt"][:] = rng.integers(0, W + 1, N)
    st["ps"][:] = rng.uniform(0.2, 6.0, N)
    st["err"][:] = rng.uniform(0.0, 1.5, (W, N))
    st["err"][:, 120:140] = 1e300
    st["cnt"][120:140] = W
    return br, sz, chunk, prev, buf, hist, st


def _controller(br, sz, chunk, prev, buf, hist, W, clip, mask=None, done=None):
    V = len(br)
    mpd = A.MPD(V, 4.0, 20.0, 0.0, [A.Chunk(list(b), list(s)) for b, s in zip(br, sz)])
    ci = _Info()
    ci.chunk_number = torch.as_tensor(chunk).cuda()
    ci.previous_bitrate = torch.as_tensor(prev).cuda()
    ci.buffer_level = torch.as_tensor(buf).cuda()
    ci.previous_bandwidths = torch.as_tensor(hist).cuda().contiguous()
    if mask is not None:
        ci.mask = torch.as_tensor(mask).cuda()
    if done is not None:
        ci.done = torch.as_tensor(done).cuda()
    return A.BatchedMPCController(_Player(mpd, A.QOEMetric(4.3, 1.0, 0.0), ci), horizon=H, clip_horizon=clip,
                                  method="robust", window=W), ci


def _select_raw(ctl, N, sentinel=-777):
    """One abr_mpc_select_robust through the controller's bound state, outputs pre-filled with sentinels."""
    ci = ctl.player.get_next_chunk_info()
    action = torch.full((N,), sentinel, dtype=torch.int32, device="cuda")
    flat = torch.full((N,), sentinel, dtype=torch.int32, device="cuda")
    J = torch.full((N,), -7.25, dtype=torch.float64, device="cuda")
    mask, mid = (ci.mask, 0) if hasattr(ci, "mask") else ((ci.done, 1) if hasattr(ci, "done") else (None, 0))
    br, sz = ctl._tables()
    cfg = ctl.config()
    need = C.c_size_t()
    _lib.check(ctl.lib.abr_mpc_scratch_bytes(C.byref(cfg), N, C.byref(need)))
    scratch = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    r = ctl.robust_options(N, scratch)
    r.hist_dev, r.hist_stride, r.mask_is_done = ci.previous_bandwidths.data_ptr(), N, mid
    _lib.check(ctl.lib.abr_mpc_select_robust(
        C.byref(cfg), C.byref(r), _lib.ptr(ci.chunk_number), _lib.ptr(ci.previous_bitrate), _lib.ptr(ci.buffer_level),
        _lib.ptr(br), _lib.ptr(sz), _lib.ptr(mask), _lib.ptr(action), _lib.ptr(flat), _lib.ptr(J), N, None))
    torch.cuda.synchronize()
    return action.cpu().numpy(), flat.cpu().numpy(), J.cpu().numpy()


def _expect(oracle, br, sz, chunk, prev, buf, hist, st, W, clip, active):
    V, B = br.shape
    ocfg = oracle.mpc_cfg(B, H, V, 4.0, 20.0, 1.0, 4.3, 0.0)
    N = len(chunk)
    act, flat, J = np.full(N, -777, np.int32), np.full(N, -777, np.int64), np.full(N, -7.25)
    for i in np.flatnonzero(active):
        act[i], flat[i], J[i] = select_scalar(oracle, ocfg, br, sz, W, int(chunk[i]), int(prev[i]), float(buf[i]),
                                              hist[:, i], st, i, clip=clip)
    return act, flat, J


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("masking", ["none", "mask", "done"])
def test_standalone_select_matches_twin_and_brute(oracle, clip, masking):
    W = 5
    br, sz, chunk, prev, buf, hist, st0 = _select_inputs(31 + clip)
    N = len(chunk)
    rng = np.random.default_rng(5)
    mask = done = None
    active = np.ones(N, bool)
    if masking == "mask":
        mask = (rng.random(N) < 0.85).astype(np.uint8)
        active = mask != 0
    elif masking == "done":
        done = np.where(rng.random(N) < 0.15, rng.choice([1, 2, 4], N), 0).astype(np.uint8)
        active = done == 0
    ctl, _ = _controller(br, sz, chunk, prev, buf, hist, W, clip, mask=mask, done=done)
    ctl.load_state_dict({"window": W, "n_lanes": N, "state": torch.from_numpy(state_bytes(st0))})
    a, f, J = _select_raw(ctl, N)
    want_st = copy_state(st0)
    wa, wf, wJ = _expect(oracle, br, sz, chunk, prev, buf, hist, want_st, W, clip, active)
    if masking == "done":
        wa[~active] = -1                   # a lane with done bits reports -1 (abr_mpc_options.mask_is_done); flat, J untouched
    assert np.array_equal(a, wa), np.flatnonzero(a != wa)[:8]
    assert np.array_equal(f, wf), np.flatnonzero(f != wf)[:8]
    assert np.array_equal(J, wJ, equal_nan=True)
    assert _same_state(_state(ctl, N), want_st)
    # the edges occurred: decisions, no decisions, D12 clips and refusals, pushes, keeps and clears
    assert (wa >= 0).sum() > N // 2 and (wa[active] == -1).sum() > 50
    if not clip:
        assert (wa[40:80][active[40:80]] == -1).all()
    assert (st0["cnt"] != want_st["cnt"]).any() and (want_st["cs1"][120:140][active[120:140]] > 0).all()


def test_select_twice_on_the_same_state_gives_the_same_answer(oracle):
    W = 4
    br, sz, chunk, prev, buf, hist, st0 = _select_inputs(44, N=1500, W=W)
    N = len(chunk)
    ctl, _ = _controller(br, sz, chunk, prev, buf, hist, W, True)
    ctl.load_state_dict({"window": W, "n_lanes": N, "state": torch.from_numpy(state_bytes(st0))})
    a1 = ctl.next_bitrate(want_details=True).cpu().numpy()
    f1, J1 = ctl.last_flat.cpu().numpy(), ctl.last_J.cpu().numpy()
    s1 = _state(ctl, N)
    a2 = ctl.next_bitrate(want_details=True).cpu().numpy()
    assert np.array_equal(a1, a2) and np.array_equal(f1, ctl.last_flat.cpu().numpy())
    assert np.array_equal(J1, ctl.last_J.cpu().numpy(), equal_nan=True)
    assert _same_state(s1, _state(ctl, N))
    want = copy_state(st0)
    wa, _, _ = _expect(oracle, br, sz, chunk, prev, buf, hist, want, W, True, np.ones(N, bool))
    assert np.array_equal(a1, wa) and _same_state(s1, want)
    # reset_state forgets every lane
    ctl.reset_state()
    assert not ctl.robust_state(N).any()


# ---------------------------------------------------------------------------------------------------------------------
# 3.  episodes against the oracle

@pytest.mark.parametrize("window", [5, 1, 16])
def test_episodes_match_oracle_driven_by_twin(oracle, window):
    N = 64
    m, traces, tid, off = golden_workload(N)
    V = m["video_length"]
    env, ctl = _env_ctl(m, traces, tid, off, N, window=window)
    out = env.step_mpc(ctl, V)
    acts = out["actions"].cpu().numpy()
    obs, rew, done = out["obs"].cpu().numpy(), out["reward"].cpu().numpy(), out["done"].cpu().numpy()
    ocfg, (br, sz), cfg = _ocfg(oracle, m), _tables(m), oracle_env_cfg(oracle, m)
    steps = np.zeros((N, V), oracle.STEP_DTYPE)
    fin = np.zeros(N, oracle.FINAL_DTYPE)
    want_a = np.zeros((N, V), np.int32)
    dev_st = _state(ctl, N)
    for i in range(N):
        st = empty_state(1, window)
        s, _, a, f = oracle.env_episode_policy(cfg, traces[tid[i]], off[i], _policy(oracle, ocfg, br, sz, window, st))
        steps[i], want_a[i], fin[i] = s, a, f
        one = {k: (v[..., i:i + 1] if k == "err" else v[i:i + 1]) for k, v in dev_st.items()}
        assert _same_state(one, st), i
    assert np.array_equal(acts.T, want_a)
    assert len(np.unique(want_a)) >= 2                     # live stream, low buffer: mostly rate 0
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


# ---------------------------------------------------------------------------------------------------------------------
# 4. - 6.  the fused rollout

@pytest.mark.parametrize("impl", ["jump", "split", "split3", "auto"])
def test_fused_rollout_matches_host_loop(impl):
    N = 1000
    m, traces, tid, off = golden_workload(N, seed=3)
    V = m["video_length"]
    env, ctl = _env_ctl(m, traces, tid, off, N, impl=impl)
    out = env.step_mpc(ctl, V)
    env2, ctl2 = _env_ctl(m, traces, tid, off, N, impl=impl)
    acts, rews, obs = [], [], []
    for _ in range(V):
        a = ctl2.next_bitrate().clamp_min(0)            # "no decision" downloads bitrate 0
        o, r, _ = env2.step(a)
        acts.append(a.clone()), rews.append(r.clone()), obs.append(o.clone())
    assert torch.equal(out["actions"], torch.stack(acts))
    assert torch.equal(out["reward"], torch.stack(rews))
    assert torch.equal(out["obs"], torch.stack(obs))
    assert torch.equal(ctl.robust_state(N), ctl2.robust_state(N))
    assert torch.equal(env.episode_qoe(), env2.episode_qoe())


def test_auto_reset_repeats_the_first_episode():
    m, traces, tid, off = golden_workload(256, seed=9)
    V = m["video_length"]
    env, ctl = _env_ctl(m, traces, tid, off, 256, auto_reset=True)
    out = env.step_mpc(ctl, 2 * V + 10)
    a = out["actions"].cpu().numpy()
    assert (a >= 0).all() and len(np.unique(a)) >= 2
    assert np.array_equal(a[V:2 * V], a[:V]) and np.array_equal(a[2 * V:], a[:10])
    assert torch.equal(out["reward"][V:2 * V], out["reward"][:V])


def test_robust_after_random_steps_starts_with_empty_errors(oracle):
    N, k = 512, 7
    m, traces, tid, off = golden_workload(N, seed=21)
    V = m["video_length"]
    env, ctl = _env_ctl(m, traces, tid, off, N)
    env.step_random(k, seed=99)
    chunk, prev, buf = (t.cpu().numpy().copy() for t in env.mpc_inputs()[:3])
    hist = env.history()[1].cpu().numpy().copy()
    assert (chunk == k).all()
    ocfg, (br, sz) = _ocfg(oracle, m), _tables(m)
    want = empty_state(N, 5)
    for step in range(2):
        out = env.step_mpc(ctl, 1)
        wa = np.array([max(select_scalar(oracle, ocfg, br, sz, 5, int(chunk[i]), int(prev[i]), float(buf[i]),
                                         hist[:, i], want, i)[0], 0) for i in range(N)])
        assert np.array_equal(out["actions"][0].cpu().numpy(), wa), step
        got = _state(ctl, N)
        assert _same_state(got, want) and (got["cnt"] == step).all(), step
        chunk, prev, buf = (t.cpu().numpy().copy() for t in env.mpc_inputs()[:3])
        hist = env.history()[1].cpu().numpy().copy()


# ---------------------------------------------------------------------------------------------------------------------
# 7.  full size

def test_full_size_replay_and_sampled_decisions(oracle):
    N = 65536
    m, traces, tid, off = golden_workload(N, seed=11)
    V = m["video_length"]
    env, ctl = _env_ctl(m, traces, tid, off, N)
    out = env.step_mpc(ctl, V)
    acts = out["actions"].cpu().numpy()
    assert (acts >= 0).all() and len(np.unique(acts)) >= 2
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid, off, np.ascontiguousarray(acts.T),
                                         threads=threads())
    obs = out["obs"].cpu().numpy()
    for s in range(V - 1):
        for r, k in ((3, "buffer_level"), (4, "global_time"), (5, "play_time"), (6, "rebuffer_time"), (2, "last_bandwidth")):
            assert np.array_equal(obs[s, r], steps[k][:, s + 1].astype(np.float32)), (s, k)
    assert np.array_equal(env.observe_f64()["buffer_level"].cpu().numpy(), fin["buffer_level"])
    # the decisions of a 1 024-lane sample, replayed through twin + brute on the oracle's call sites
    ocfg, (br, sz) = _ocfg(oracle, m), _tables(m)
    sample = np.random.default_rng(0).choice(N, 1024, replace=False)

    def lane(i):
        st = empty_state(1, 5)
        return np.array([max(select_scalar(oracle, ocfg, br, sz, 5, int(steps["chunk_id"][i, s]),
                                           int(steps["last_bitrate"][i, s]), float(steps["buffer_level"][i, s]),
                                           bw[i], st, 0)[0], 0) for s in range(V)])
    want = np.stack(thread_map(lane, sample), 1)
    assert np.array_equal(acts[:, sample], want)


# ---------------------------------------------------------------------------------------------------------------------
# 8.  refusals

def test_tick_kernel_is_refused():
    m, traces, tid, off = golden_workload(64)
    env, ctl = _env_ctl(m, traces, tid, off, 64, impl="tick")
    with pytest.raises(_lib.AbrError, match="-4"):
        env.step_mpc(ctl, 2)
    assert not ctl.robust_state(64).any()                     # nothing ran


def test_state_follows_lane_count_and_window():
    m, traces, tid, off = golden_workload(128)
    env, ctl = _env_ctl(m, traces, tid, off, 128)
    env.step_mpc(ctl, 3)
    sd = ctl.state_dict()
    assert sd["n_lanes"] == 128 and sd["state"].any()
    ctl.window = 3                                            # a new layout: a new, empty state
    assert ctl.robust_state(128).numel() == 128 * 8 * 5 and not ctl.robust_state(128).any()
    ctl.window = 5
    ctl.load_state_dict(sd)
    assert torch.equal(ctl.robust_state(128), sd["state"].cuda())
