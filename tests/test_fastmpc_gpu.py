"""FastMPC on the device: every built entry against the oracle's brute-force search, the two layouts against each other,
the standalone lookup against RobustMPC on a zeroed state (on grid points) and against the twin reading the built table
(off them), fused rollouts against the oracle driven by the twin (jump, tick, auto, auto-reset, per-chunk ladders,
per-lane speeds, frozen lanes), the fused rollout against the host loop, a full-size replay, and the refusals."""
import numpy as np
import pytest
import torch

import abrsimulator_amd as A
from abrsimulator_amd import _lib
from conftest import load_golden
from fastmpc_twin import chunk_of_row, entry_oracle, lookup, lookup_lanes, row_of
from helpers import golden_workload, make_env, oracle_env_cfg, oracle_rewards, thread_map, threads

pytestmark = pytest.mark.gpu


class _Info:
    pass


class _Player:
    def __init__(self, mpd, qoe, ci=None):
        self.mpd, self.qoe, self.ci = mpd, qoe, ci

    def get_mpd(self):
        return self.mpd

    def get_qoe_metric(self):
        return self.qoe

    def get_next_chunk_info(self):
        return self.ci


def _mpd(br, sz, L, mb):
    return A.MPD(br.shape[0], L, mb, 0.0, [A.Chunk(list(b), list(s)) for b, s in zip(br, sz)])


def _tables(rng, M, V, L, vbr):
    if vbr:
        br = np.sort(rng.uniform(0.2, 6.0, M))[None, :] * rng.uniform(0.8, 1.2, (V, 1))
        br = np.sort(br * rng.uniform(0.95, 1.05, (V, M)), axis=1)
        sz = br * L * rng.uniform(0.7, 1.3, (V, M))
    else:
        br = np.tile(np.sort(rng.uniform(0.2, 6.0, M)), (V, 1))
        sz = br * L
    return br, sz


def _ocfg(oracle, M, H, V, L, mb, qoe):
    return oracle.mpc_cfg(M, H, V, L, mb, qoe.variance_weight, qoe.rebuffer_weight, qoe.startup_weight)


def _host(ctl):
    e = ctl.entries().cpu().numpy()
    torch.cuda.synchronize()
    return e


def _check_all_entries(oracle, ctl, br, sz, ocfg, rows=None):
    e = _host(ctl)
    R, M, Nb, Nq = e.shape
    V = br.shape[0]
    bad = []
    for r in (range(R) if rows is None else rows):
        c = chunk_of_row(r, V, ctl.uniform)
        for p in range(M):
            for bi in range(Nb):
                for qi in range(Nq):
                    want = entry_oracle(oracle, ocfg, br, sz, c, p, ctl.buffer_points[bi], ctl.tput_points[qi],
                                        ctl.clip_horizon)
                    if e[r, p, bi, qi] != want:
                        bad.append((r, p, bi, qi, int(e[r, p, bi, qi]), want))
    assert not bad, bad[:10]
    return e


# ---------------------------------------------------------------------------------------------------------------------
# 1.  every entry equals the brute-force search

SMALL = [  # (M, H, V, clip, layout, vbr)
    (2, 2, 5, True, "uniform", False), (3, 3, 7, False, "uniform", False), (4, 4, 6, True, "per_chunk", True),
    (5, 2, 4, False, "per_chunk", True), (6, 5, 8, True, "uniform", False), (6, 3, 5, False, "per_chunk", False),
    (6, 5, 6, True, "per_chunk", True), (3, 5, 4, True, "per_chunk", False),
]


@pytest.mark.parametrize("M,H,V,clip,layout,vbr", SMALL)
def test_every_entry_equals_brute_force(oracle, M, H, V, clip, layout, vbr):
    rng = np.random.default_rng(M * 100 + H * 10 + V)
    L, mb = 4.0, 12.0
    br, sz = _tables(rng, M, V, L, vbr)
    qoe = A.QOEMetric(4.3, 1.0, 0.0)
    bp = np.array([0.0, 0.5, 3.0, 7.5, 12.0, 15.5])
    tp = np.geomspace(br.min() / 4, br.max() * 4, 5)
    ctl = A.FastMPCController(_Player(_mpd(br, sz, L, mb), qoe), horizon=H, clip_horizon=clip, layout=layout,
                              buffer_points=bp, tput_points=tp, device="cuda")
    e = _check_all_entries(oracle, ctl, br, sz, _ocfg(oracle, M, H, V, L, mb, qoe))
    assert len(np.unique(e)) >= 2
    if not clip:
        # rows whose horizon runs past the video end hold "no decision": 0
        for r in range(e.shape[0]):
            if chunk_of_row(r, V, ctl.uniform) + H > V:
                assert not e[r].any(), r


def test_bench_size_table_sampled(oracle):
    """The 64 x 64 default grid of the bench workload: >= 20 000 sampled entries, every corner included."""
    m, _ = load_golden("env_bench_shape")
    V, L, mb, M, H = m["video_length"], m["chunk_length"], m["max_buffer"], len(m["ladder"]), 5
    br = np.tile(np.asarray(m["ladder"], np.float64), (V, 1))
    sz = br * L
    qoe = A.QOEMetric(*m["weights"])
    ctl = A.FastMPCController(_Player(A.MPD(V, L, mb, 0.0, A.Chunk(m["ladder"])), qoe), device="cuda")
    e = _host(ctl)
    assert e.shape == (H, M, 64, 64)
    ocfg = _ocfg(oracle, M, H, V, L, mb, qoe)
    rng = np.random.default_rng(5)
    idx = {tuple(int(x) for x in rng.integers(0, [H, M, 64, 64])) for _ in range(26000)}
    idx |= {(r, p, b, q) for r in range(H) for p in range(M) for b in (0, 63) for q in (0, 63)}
    idx = sorted(idx)
    assert len(idx) >= 20000

    def run(part):
        return [(k, entry_oracle(oracle, ocfg, br, sz, chunk_of_row(k[0], V, True), k[1], ctl.buffer_points[k[2]],
                                 ctl.tput_points[k[3]])) for k in part]
    res = [x for part in thread_map(run, np.array_split(np.array(idx), threads())) for x in part]
    bad = [(tuple(k), int(e[tuple(k)]), w) for k, w in res if e[tuple(k)] != w]
    assert not bad, bad[:10]


# ---------------------------------------------------------------------------------------------------------------------
# 2.  the layouts agree on a uniform ladder

@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("utility", ["identity", "log"])
def test_layouts_agree(clip, utility):
    m, _ = load_golden("env_bench_shape")
    V, L, mb = m["video_length"], m["chunk_length"], m["max_buffer"]
    p = _Player(A.MPD(V, L, mb, 0.0, A.Chunk(m["ladder"])), A.QOEMetric(*m["weights"]))
    kw = dict(clip_horizon=clip, utility=utility, buffer_points=np.linspace(0, 24, 16),
              tput_points=np.geomspace(0.05, 20, 16), device="cuda")
    u = _host(A.FastMPCController(p, layout="uniform", **kw))
    pc = _host(A.FastMPCController(p, layout="per_chunk", **kw))
    assert u.shape[0] == 5 and pc.shape[0] == V
    for c in range(V):
        assert np.array_equal(u[row_of(c, V, 5, True)], pc[c]), c


# ---------------------------------------------------------------------------------------------------------------------
# 3.  on-grid exactness: the lookup equals RobustMPC on a zeroed state, which equals the oracle

@pytest.mark.parametrize("utility", ["identity", "log"])
@pytest.mark.parametrize("clip", [True, False])
def test_standalone_select_on_and_off_grid(oracle, utility, clip):
    rng = np.random.default_rng(11)
    M, H, V, L, mb, W, N = 6, 5, 30, 4.0, 20.0, 5, 3000
    br, sz = _tables(rng, M, V, L, vbr=True)
    qoe = A.QOEMetric(4.3, 1.0, 0.0)
    bp = np.linspace(0.0, 24.0, 25)                       # multiples of 1.0: exact
    tp = 2.0 ** np.arange(-4, 5, dtype=np.float64)        # powers of two
    mpd = _mpd(br, sz, L, mb)
    ctl = A.FastMPCController(_Player(mpd, qoe), horizon=H, window=W, utility=utility, clip_horizon=clip,
                              buffer_points=bp, tput_points=tp, device="cuda")
    assert not ctl.uniform
    chunk = rng.integers(1, V, N).astype(np.int32)
    prev = rng.integers(-M, M, N).astype(np.int32)
    on = np.arange(N) < N // 2
    buf = np.where(on, rng.choice(bp, N), rng.uniform(0.0, 26.0, N))
    x = rng.choice(tp, N)
    hist = np.where(on[None, :], np.broadcast_to(x, (V, N)), rng.uniform(0.05, 20.0, (V, N))).copy()
    hist[:, N - 50:] = rng.choice([np.inf, 1e-310], (V, 50))      # P = 0 or inf off the grid
    chunk[N - 60:N - 50] = 0
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    got = ctl.select(d(chunk, torch.int32), d(prev, torch.int32), d(buf, torch.float64), d(hist, torch.float64))
    got = got.cpu().numpy()
    e = _host(ctl)
    want = lookup_lanes(e, ctl.buffer_edges, ctl.tput_edges, W, V, H, False, chunk, prev, buf, hist)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    # on the grid: RobustMPC's exact search on a zeroed state (its estimate is the same harmonic mean)
    ci = _Info()
    ci.chunk_number, ci.previous_bitrate, ci.buffer_level = d(chunk, torch.int32), d(prev, torch.int32), d(buf, torch.float64)
    ci.previous_bandwidths = d(hist, torch.float64)
    rob = A.BatchedMPCController(_Player(mpd, qoe, ci), horizon=H, clip_horizon=clip, method="robust", window=W,
                                 utility=utility, device="cuda")
    ra = rob.next_bitrate().cpu().numpy()
    ra = np.where(ra < 0, 0, ra)
    assert np.array_equal(got[on], ra[on]), np.flatnonzero(got[on] != ra[on])[:5]
    if utility == "identity":
        ocfg = _ocfg(oracle, M, H, V, L, mb, qoe)
        for i in np.flatnonzero(on)[:300]:
            assert got[i] == entry_oracle(oracle, ocfg, br, sz, chunk[i], prev[i] % M, buf[i], x[i], clip), i
    # masks: a plain mask skips lanes (outputs untouched); mask_is_done reports -1 for done lanes
    done = (rng.random(N) < 0.2).astype(np.uint8)
    out2 = ctl.select(d(chunk, torch.int32), d(prev, torch.int32), d(buf, torch.float64), d(hist, torch.float64),
                      mask=d(done, torch.uint8), mask_is_done=True).cpu().numpy()
    assert np.array_equal(out2, np.where(done != 0, -1, want))


# ---------------------------------------------------------------------------------------------------------------------
# 4. - 6.  rollouts

def _twin_over_replay(ctl, e, steps, bw, V):
    """The twin's action at every call site of the replayed episodes: [V, N]."""
    N = steps.shape[0]
    out = np.zeros((V, N), np.int32)
    for i in range(N):
        for s in range(V):
            out[s, i] = lookup(e, ctl.buffer_edges, ctl.tput_edges, ctl.window, V, ctl.horizon, ctl.uniform, s,
                               int(steps["last_bitrate"][i, s]), float(steps["buffer_level"][i, s]), bw[i, :s])
    return out


@pytest.mark.parametrize("impl", ["jump", "tick", "auto"])
def test_rollout_equals_oracle_driven_by_twin(oracle, impl):
    N = 96
    m, traces, tid, off = golden_workload(N)
    V = m["video_length"]
    env = make_env(m, traces, N, impl=impl)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    # a controller that weighs rebuffering less than the environment does, so that the episodes use the whole ladder
    ctl = A.FastMPCController(A.EnvPlayer(env, qoe=A.QOEMetric(0.3, 1.0, 0.0)), window=3)
    out = env.step_rule(ctl, V + 2)                                   # two steps past the end: frozen lanes
    acts = out["actions"].cpu().numpy()
    e = _host(ctl)
    assert (acts[V:] == -1).all()
    cfg = oracle_env_cfg(oracle, m)
    # a few lanes literally driven by the twin through the oracle
    for i in range(8):
        pol = lambda o, h: lookup(e, ctl.buffer_edges, ctl.tput_edges, 3, V, 5, True, int(o["chunk_id"]),
                                  int(o["last_bitrate"]), float(o["buffer_level"]), h)
        st, _, a, f = oracle.env_episode_policy(cfg, traces[tid[i]], off[i], pol)
        assert np.array_equal(acts[:V, i], a), i
    steps, bw, fin, _ = oracle.env_batch(cfg, traces, tid, off, np.ascontiguousarray(acts[:V].T), threads=threads())
    assert np.array_equal(_twin_over_replay(ctl, e, steps, bw, V), acts[:V])
    assert len(np.unique(acts[:V])) >= 3
    rew = out["reward"].cpu().numpy()
    assert np.array_equal(rew[:V].T, oracle_rewards(steps, fin, acts[:V].T, m["weights"], ladder=m["ladder"]))
    obs = out["obs"].cpu().numpy()
    for s in range(V - 1):
        assert np.array_equal(obs[s, 3], steps["buffer_level"][:, s + 1].astype(np.float32)), s
    for k in ("global_time", "rebuffer_time", "buffer_level"):
        assert np.array_equal(env.observe_f64()[k].cpu().numpy(), fin[k]), k
    d = out["done"].cpu().numpy()
    assert (d[V - 1:] == 1).all() and (d[:V - 1] == 0).all()


def test_auto_reset_repeats_the_first_episode():
    m, traces, tid, off = golden_workload(128)
    V = m["video_length"]
    env = make_env(m, traces, 128, auto_reset=True)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    ctl = A.FastMPCController(A.EnvPlayer(env))
    out = env.step_rule(ctl, 2 * V + 7)
    a = out["actions"].cpu().numpy()
    assert np.array_equal(a[V:2 * V], a[:V]) and np.array_equal(a[2 * V:], a[:7])
    assert torch.equal(out["reward"][V:2 * V], out["reward"][:V])


def test_per_chunk_ladder_and_lane_speeds(oracle):
    N = 128
    m, traces, tid, off = golden_workload(N, seed=13)
    V, L = m["video_length"], m["chunk_length"]
    rng = np.random.default_rng(2)
    table = np.sort(np.asarray(m["ladder"]) * rng.uniform(0.7, 1.3, (V, 1)) * rng.uniform(0.9, 1.1, (V, 6)), axis=1)
    mpd = A.MPD(V, L, m["max_buffer"], m["start_up_length"], [A.Chunk(list(r)) for r in table])
    speeds = rng.uniform(0.8, 1.3, N)
    env = A.BatchedABREnv(mpd, A.QOEMetric(*m["weights"]), A.NetworkInfo(m["interval"], traces), N, device="cuda",
                          speed=torch.from_numpy(speeds))
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    ctl = A.FastMPCController(A.EnvPlayer(env, qoe=A.QOEMetric(0.3, 1.0, 0.0)), tput_points=np.geomspace(0.05, 25, 40))
    assert not ctl.uniform
    out = env.step_rule(ctl, V)
    acts = out["actions"].cpu().numpy()
    e = _host(ctl)
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m, br_table=table), traces, tid, off,
                                         np.ascontiguousarray(acts.T), speeds=speeds, threads=threads())
    assert np.array_equal(_twin_over_replay(ctl, e, steps, bw, V), acts)
    assert len(np.unique(acts)) >= 3
    assert np.array_equal(env.observe_f64()["global_time"].cpu().numpy(), fin["global_time"])


@pytest.mark.parametrize("impl", ["jump", "tick"])
def test_fused_equals_host_loop(impl):
    N = 256
    m, traces, tid, off = golden_workload(N, seed=3)
    V = m["video_length"]
    envs = [make_env(m, traces, N, impl=impl) for _ in range(2)]
    for env in envs:
        env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    ctls = [A.FastMPCController(A.EnvPlayer(env), window=4) for env in envs]
    out = envs[0].step_rule(ctls[0], V + 1)
    for s in range(V + 1):
        a = ctls[1].next_bitrate()
        assert torch.equal(a, out["actions"][s]), s
        if s < V:
            obs, rew, done = envs[1].step(a)
            assert torch.equal(obs, out["obs"][s]) and torch.equal(rew, out["reward"][s]), s
            assert torch.equal(done, out["done"][s]), s
    assert (out["actions"][V] == -1).all()


def test_full_size_replay(oracle):
    N = 65536
    m, traces, tid, off = golden_workload(N, seed=21)
    V = m["video_length"]
    env = make_env(m, traces, N)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    ctl = A.FastMPCController(A.EnvPlayer(env))
    out = env.step_rule(ctl, V)
    acts = out["actions"].cpu().numpy()
    e = _host(ctl)
    lanes = np.sort(np.random.default_rng(0).choice(N, 512, replace=False))
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid[lanes], off[lanes],
                                         np.ascontiguousarray(acts[:, lanes].T), threads=threads())
    assert np.array_equal(_twin_over_replay(ctl, e, steps, bw, V), acts[:, lanes])
    assert np.array_equal(env.observe_f64()["global_time"].cpu().numpy()[lanes], fin["global_time"])


# ---------------------------------------------------------------------------------------------------------------------
# 7.  refusals

@pytest.mark.parametrize("impl", ["split", "split3"])
def test_role_split_is_refused(impl):
    m, traces, tid, off = golden_workload(64)
    env = make_env(m, traces, 64, impl=impl)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    ctl = A.FastMPCController(A.EnvPlayer(env))
    with pytest.raises(_lib.AbrError, match="-4"):
        env.step_rule(ctl, 4)


def test_uniform_layout_refused_with_per_chunk_table():
    m, traces, tid, off = golden_workload(64)
    V = m["video_length"]
    table = np.tile(np.asarray(m["ladder"]), (V, 1)) * np.linspace(1.0, 1.1, V)[:, None]
    mpd = A.MPD(V, m["chunk_length"], m["max_buffer"], m["start_up_length"], [A.Chunk(list(r)) for r in table])
    env = A.BatchedABREnv(mpd, A.QOEMetric(*m["weights"]), A.NetworkInfo(m["interval"], traces), 64, device="cuda")
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    # a controller that believes in one ladder (the MPD it was given is uniform) against the per-chunk environment
    ctl = A.FastMPCController(_Player(A.MPD(V, m["chunk_length"], m["max_buffer"], 0.0, A.Chunk(m["ladder"])),
                                      A.QOEMetric(*m["weights"])), device="cuda")
    ctl.player.env = env
    assert ctl.uniform
    with pytest.raises(_lib.AbrError, match="uniform"):
        env.step_rule(ctl, 4)
    with pytest.raises(_lib.AbrError, match="uniform"):
        ctl.next_bitrate()
