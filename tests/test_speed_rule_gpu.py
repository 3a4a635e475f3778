"""The closed-loop speed rule on the device (abr_env_set_speed_rule) against the tick-loop twin
(tests/speed_twin.py) and the C oracle replaying the device's own log as a speed schedule: every event-driven kernel
under every rollout, auto-reset, per-chunk ladders, a checkpoint resumed in a fresh handle, latching, a 65 536-lane
run, the tick kernels' refusal, and Simulator with a LatencySpeedController."""

import numpy as np
import pytest
import torch

import abrsimulator_amd as A
from abrsimulator_amd import _lib
from helpers import make_env, oracle_env_cfg
from speed_twin import rule_arrays, twin_batch

pytestmark = pytest.mark.gpu

FRAME = ["global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level", "play_id"]
LADDER = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
CTL = A.LatencySpeedController((2.0, 6.0), (1.0, 8.0), ((0.9, 1.0, 1.0), (0.9, 1.1, 1.25), (0.75, 1.5, 2.0)))


def _workload(N, seed=5, V=12, max_buffer=12.0, start_up=4.0):
    rng = np.random.default_rng(seed)
    traces = [rng.uniform(0.3, 7.0, 800).astype(np.float32).astype(np.float64) for _ in range(8)]
    meta = dict(ladder=LADDER, chunk_length=4.0, video_length=V, max_buffer=max_buffer, start_up_length=start_up,
                interval=1.0, weights=[4.3, 1, 1, 0.1])
    tid = rng.integers(0, 8, N).astype(np.int32)
    off = rng.integers(0, 800, N).astype(np.int32)
    return meta, traces, tid, off


def _env(m, traces, N, ctl=CTL, rows=None, **kw):
    env = make_env(m, traces, N, **kw)
    env.set_speed_controller(ctl, log_rows=m["video_length"] + 4 if rows is None else rows)
    return env


def _sched(log):
    """The device log [rows, N] as an oracle schedule [N, rows]: rows a lane never reached (still 0) are never read."""
    log = log.cpu().numpy()
    return np.ascontiguousarray(np.where(log == 0.0, 1.0, log).T)


def _rollout(env, kind, V, chunk):
    """Run V decisions in pieces of `chunk`; returns (actions [V, N], observe_f64 after each piece)."""
    N = env.n_lanes
    acts, frames = [], []
    rng = np.random.default_rng(99)
    ctl = None
    if kind in ("mpc", "robust"):
        ctl = A.BatchedMPCController(A.EnvPlayer(env), horizon=5, clip_horizon=True,
                                     **(dict(method="robust", window=5) if kind == "robust" else {}))
    elif kind == "rule":
        ctl = A.BufferBasedController(A.EnvPlayer(env), reservoir=2.0, cushion=8.0)
    s = 0
    while s < V:
        n = min(chunk, V - s)
        if kind == "step":
            for _ in range(n):
                a = torch.from_numpy(rng.integers(0, env.n_rates, N).astype(np.int32)).to(env.device)
                env.step(a)
                acts.append(a.cpu().numpy())
        elif kind == "random":
            acts.extend(env.step_random(n, 1234 + s)["actions"].cpu().numpy())
        elif kind == "script":
            a = rng.integers(0, env.n_rates, (n, N)).astype(np.int32)
            env.step_script(torch.from_numpy(a).to(env.device))
            acts.extend(a)
        elif kind in ("mpc", "robust"):
            acts.extend(env.step_mpc(ctl, n)["actions"].cpu().numpy())
        else:
            acts.extend(env.step_rule(ctl, n)["actions"].cpu().numpy())
        s += n
        frames.append((s, {k: v.cpu().numpy().copy() for k, v in env.observe_f64().items()}))
    return np.asarray(acts, np.int32), frames


def _check_frames(frames, steps, fin, V):
    for s, f in frames:
        for k in FRAME:
            want = fin[k] if s == V else steps[k][:, s]
            assert np.array_equal(f[k], want), (s, k)
        want = fin["average_latency"] if s == V else steps["average_latency"][:, s]
        assert np.allclose(f["average_latency"], want, rtol=1e-9, atol=0), s


def _check_twin(m, traces, tid, off, acts, log, n=24, ctl=CTL):
    rows = log.shape[0]
    steps, final, bws, tlog, _ = twin_batch(m, traces, tid[:n], off[:n], acts.T[:n], rule_arrays(ctl), rows)
    dlog = log[:, :n].cpu().numpy().T
    assert np.array_equal(np.where(np.isnan(tlog), 0.0, tlog), dlog)
    return steps, final


# every rollout on every event-driven kernel; step_rule only where it runs (the role-split kernels refuse it)
CASES = [(impl, kind) for impl in ("jump", "split", "split3", "auto")
         for kind in ("step", "random", "script", "mpc", "robust")] + [("jump", "rule"), ("auto", "rule")]


@pytest.mark.parametrize("impl,kind", CASES)
def test_rollouts_match_twin_and_oracle_replay(oracle, impl, kind):
    N = 512
    m, traces, tid, off = _workload(N)
    V = m["video_length"]
    env = _env(m, traces, N, impl=impl)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    acts, frames = _rollout(env, kind, V, chunk=5)
    log = env.speed_log()
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid, off, np.ascontiguousarray(acts.T),
                                         speeds=_sched(log))
    _check_frames(frames, steps, fin, V)
    assert np.allclose(env.episode_qoe().cpu().numpy(), fin["qoe"], rtol=1e-9)
    tsteps, tfin = _check_twin(m, traces, tid, off, acts, log)
    for k in FRAME:
        assert np.array_equal(tfin[k], fin[k][:24]), k
    # the rule really steers: more than one answer in the log
    assert len(np.unique(log.cpu().numpy())) >= 3


def test_rule_rollouts_still_refused_on_the_split_kernels():
    m, traces, tid, off = _workload(64)
    for impl in ("split", "split3"):
        env = _env(m, traces, 64, impl=impl)
        env.reset(torch.from_numpy(tid), torch.from_numpy(off))
        with pytest.raises(_lib.AbrError):
            env.step_rule(A.BufferBasedController(A.EnvPlayer(env)), 2)


@pytest.mark.parametrize("impl", ["jump", "auto"])
def test_auto_reset_logs_the_current_episode(oracle, impl):
    N = 256
    m, traces, tid, off = _workload(N, seed=8)
    V = m["video_length"]
    env = _env(m, traces, N, impl=impl, auto_reset=True)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    a1 = env.step_random(V, 7)["actions"].cpu().numpy()
    q1 = env.episode_qoe().cpu().numpy()
    log1 = env.speed_log().clone()
    a2 = env.step_random(V, 7)["actions"].cpu().numpy()
    q2 = env.episode_qoe().cpu().numpy()
    for a, q, log in ((a1, q1, log1), (a2, q2, env.speed_log())):
        steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid, off, np.ascontiguousarray(a.T),
                                             speeds=_sched(log))
        assert np.allclose(q, fin["qoe"], rtol=1e-9)
    _check_twin(m, traces, tid, off, a2, env.speed_log(), n=16)


def test_per_chunk_ladders_with_a_rule(oracle):
    N = 256
    m, traces, tid, off = _workload(N, seed=9)
    V = m["video_length"]
    rng = np.random.default_rng(2)
    table = np.sort(np.asarray(LADDER) * rng.uniform(0.7, 1.3, (V, 1)) * rng.uniform(0.9, 1.1, (V, 6)), axis=1)
    mpd = A.MPD(V, m["chunk_length"], m["max_buffer"], m["start_up_length"], [A.Chunk(list(r)) for r in table])
    env = A.BatchedABREnv(mpd, A.QOEMetric(*m["weights"]), A.NetworkInfo(m["interval"], traces), N, device="cuda",
                          speed=CTL)
    env.set_speed_controller(CTL, log_rows=V + 4)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    acts, frames = _rollout(env, "mpc", V, chunk=4)
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m, br_table=table), traces, tid, off,
                                         np.ascontiguousarray(acts.T), speeds=_sched(env.speed_log()))
    _check_frames(frames, steps, fin, V)
    assert np.allclose(env.episode_qoe().cpu().numpy(), fin["qoe"], rtol=1e-9)


def test_checkpoint_mid_episode_resumes_in_a_fresh_handle(oracle):
    N = 256
    m, traces, tid, off = _workload(N, seed=10)
    V = m["video_length"]
    env = _env(m, traces, N)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    a1 = env.step_random(5, 3)["actions"].cpu().numpy()
    sd = env.state_dict()
    log_mid = env.speed_log().clone()
    env2 = make_env(m, traces, N)
    env2.set_speed_controller(CTL, log_rows=V + 4)
    env2.speed_log().copy_(log_mid)               # the log is the caller's: it travels with the checkpoint if wanted
    env2.load_state_dict(sd)
    a2 = env2.step_random(V - 5, 4)["actions"].cpu().numpy()
    acts = np.concatenate([a1, a2])
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid, off, np.ascontiguousarray(acts.T),
                                         speeds=_sched(env2.speed_log()))
    f = env2.observe_f64()
    for k in FRAME:
        assert np.array_equal(f[k].cpu().numpy(), fin[k]), k
    _check_twin(m, traces, tid, off, acts, env2.speed_log(), n=16)


def test_latching_and_last_setter_wins(oracle):
    N = 128
    m, traces, tid, off = _workload(N, seed=11)
    V = m["video_length"]
    env = make_env(m, traces, N)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    # armed handle: the rule waits for the next full reset
    env.set_speed_controller(CTL, log_rows=V + 4)
    a = env.step_random(V, 5)["actions"].cpu().numpy()
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid, off, np.ascontiguousarray(a.T))
    assert np.array_equal(env.observe_f64()["global_time"].cpu().numpy(), fin["global_time"])
    assert not env.speed_log().any()
    with pytest.raises(_lib.AbrError):                    # a partial reset cannot adopt it
        env.reset(torch.from_numpy(tid), torch.from_numpy(off), mask=torch.ones(N, dtype=torch.uint8))
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    a = env.step_random(V, 5)["actions"].cpu().numpy()
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid, off, np.ascontiguousarray(a.T),
                                         speeds=_sched(env.speed_log()))
    assert np.array_equal(env.observe_f64()["global_time"].cpu().numpy(), fin["global_time"])
    assert env.speed_log().any()
    # a schedule set after the rule replaces it at the next full reset
    sched = torch.full((3, N), 1.25, dtype=torch.float64, device="cuda")
    assert env.lib.abr_env_set_speed_schedule(env._h, _lib.ptr(sched), 3) == 0
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    a = env.step_random(V, 6)["actions"].cpu().numpy()
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid, off, np.ascontiguousarray(a.T),
                                         speeds=np.full((N, 3), 1.25))
    assert np.array_equal(env.observe_f64()["play_time"].cpu().numpy(), fin["play_time"])
    # rule == NULL restores the config speed
    env.set_speed_controller(None)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    a = env.step_random(V, 6)["actions"].cpu().numpy()
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid, off, np.ascontiguousarray(a.T))
    assert np.array_equal(env.observe_f64()["play_time"].cpu().numpy(), fin["play_time"])


def test_tick_kernels_refuse_both_ways():
    m, traces, tid, off = _workload(64)
    env = make_env(m, traces, 64, impl="tick")
    with pytest.raises(_lib.AbrError, match="event-driven"):
        env.set_speed_controller(CTL)
    env = _env(m, traces, 64, impl="jump")                 # unarmed: the rule is in force at once
    assert env.lib.abr_env_set_impl(env._h, 1) != 0
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    env.set_speed_controller(None)                         # removal pending: the episodes still run the rule
    assert env.lib.abr_env_set_impl(env._h, 1) != 0
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    assert env.lib.abr_env_set_impl(env._h, 1) == 0
    with pytest.raises(_lib.AbrError, match="event-driven"):
        env.set_speed_controller(CTL)
    assert env.lib.abr_env_set_impl(env._h, 0) == 0
    env.set_speed_controller(CTL)                          # pending on an armed handle: refused as well
    assert env.lib.abr_env_set_impl(env._h, 1) != 0


def test_large_run_sampled_lanes_replayed(oracle):
    N = 65536
    m, traces, tid, off = _workload(N, seed=13)
    V = m["video_length"]
    env = _env(m, traces, N)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    assert env.effective_impl(fused=True) == "split3"
    acts = env.step_random(V, 77)["actions"].cpu().numpy()
    f = env.observe_f64()
    pick = np.random.default_rng(0).choice(N, 2048, replace=False)
    log = env.speed_log()[:, torch.from_numpy(pick).cuda()]
    steps, bw, fin, _ = oracle.env_batch(oracle_env_cfg(oracle, m), traces, tid[pick], off[pick],
                                         np.ascontiguousarray(acts.T[pick]), speeds=_sched(log))
    for k in FRAME:
        assert np.array_equal(f[k].cpu().numpy()[pick], fin[k]), k
    assert np.allclose(f["average_latency"].cpu().numpy()[pick], fin["average_latency"], rtol=1e-9)


def test_simulator_with_a_latency_controller(oracle):
    N = 128
    m, traces, tid, off = _workload(N, seed=14)
    V = m["video_length"]

    class Abr:
        def get_next_bitrate(self, chunk_id, prev_bitrates, prev_bandwidths, buffer_level):
            return (chunk_id % 6).to(torch.int32)

    sim = A.Simulator(Abr(), speed_controller=CTL, n_lanes=N)
    sim.set_qoe_metric(A.QOEMetric(*m["weights"]))
    sim.set_network_info(m["interval"], A.NetworkInfo(m["interval"], traces))
    sim.set_mpd(m["chunk_length"], m["max_buffer"], m["start_up_length"],
                A.MPD(V, m["chunk_length"], m["max_buffer"], m["start_up_length"], A.Chunk(LADDER)))
    sim.set_lanes(torch.from_numpy(tid), torch.from_numpy(off))
    qoe = sim.run().cpu().numpy()
    acts = np.tile(np.arange(V, dtype=np.int32) % 6, (N, 1))
    steps, final, bws, log, _ = twin_batch(m, traces, tid, off, acts, rule_arrays(CTL), V + 4)
    assert np.allclose(qoe, final["qoe"], rtol=1e-9)
    with pytest.raises(RuntimeError, match="device"):
        CTL.get_next_speed()
