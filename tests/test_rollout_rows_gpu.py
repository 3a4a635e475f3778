"""Where a per-launch rollout keeps its decisions when the caller wants no actions back (want_actions=False: the C entry
gets actions_out_dev == NULL and decides into the workspace's mpc_action row).

Two environments that start from the same bytes run the same rollout, one with want_actions=True and one with
want_actions=False.  obs, reward and done must agree on the bit pattern, the workspaces must agree outside the rollouts'
scratch (the action row, which only the second environment writes, and the predictor scratch carry nothing between
calls), and so must every controller's own state.

Shape: 130 lanes (two full waves and a partial one), 3 rates, horizon 2, traces of 40 points, video_length 6 without
auto_reset and 8 decisions, so that every lane finishes at decision 6 (an episode is exactly video_length downloads, which
the test asserts on the done rows) and the last two rows come from masked lanes.  Bandwidths well above the ladder, light
QoE penalties and a quality model make every controller take more than one action (asserted), so that a rollout that
read its decisions from the wrong row would not go unnoticed."""
import numpy as np
import pytest
import torch

import abrsimulator_amd as A
import fork_twin

pytestmark = pytest.mark.gpu

N, M, V, H, STEPS, POINTS, WINDOW = 130, 3, 6, 2, 8, 40, 3
LADDER = [0.3, 1.2, 2.85]


def _env():
    rng = np.random.default_rng(11)
    traces = [rng.uniform(1.0, 16.0, POINTS) for _ in range(N)]
    env = A.BatchedABREnv(A.MPD(V, 4.0, 20.0, 8.0, A.Chunk(LADDER)), A.QOEMetric(1.0, 0.2, 0.2, 0.1),
                          A.NetworkInfo(1.0, traces), N, device="cuda")
    env.set_quality(3.0, "log")
    env.reset(torch.arange(N, dtype=torch.int32), torch.from_numpy(rng.integers(0, POINTS, N).astype(np.int32)))
    return env


def _pair():
    """the workspace is allocated uninitialised: both environments load the bytes of a third"""
    sd = _env().state_dict()
    envs = [_env(), _env()]
    for e in envs:
        e.load_state_dict(sd)
    return envs


def _mpc(method):
    def go(env, want_actions):
        ctl = A.BatchedMPCController(A.EnvPlayer(env), horizon=H, clip_horizon=True, method=method)
        out = env.step_mpc(ctl, STEPS, want_actions=want_actions)
        return out, [] if method == "harmonic" else [ctl.robust_state(N)]
    return go


def _plan(env, want_actions):
    ctl = A.ForecastMPCController(A.EnvPlayer(env), H, window=WINDOW, robust=True)
    return env.step_plan(ctl, STEPS, want_actions=want_actions), [ctl.state]


def _policy(env, want_actions):
    rng, layers, fan = np.random.default_rng(5), [], 4 + WINDOW + M
    for w in (8, M):
        layers.append((rng.normal(0, 1.5 / np.sqrt(fan), (w, fan)).astype(np.float32), rng.normal(0, 0.2, w).astype(np.float32)))
        fan = w
    ctl = A.PolicyController(A.EnvPlayer(env), layers, window=WINDOW)
    return env.step_policy(ctl, STEPS, want_actions=want_actions), []


def _gru(env, want_actions):
    rng, F, Hd = np.random.default_rng(7), 4 + WINDOW + M, 8
    cell = tuple((rng.standard_normal(s) * 0.6).astype(np.float32) for s in ((3 * Hd, F), (3 * Hd, Hd), (3 * Hd,), (3 * Hd,)))
    head = tuple((rng.standard_normal(s) * 0.6).astype(np.float32) for s in ((M, Hd), (M,)))
    ctl = A.RecurrentPolicyController(A.EnvPlayer(env), cell, head, window=WINDOW)
    out = env.step_policy(ctl, STEPS, want_actions=want_actions)
    assert ctl.hidden.any()
    return out, [ctl.hidden]


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.uint8)


@pytest.mark.parametrize("rollout", [_mpc("harmonic"), _mpc("robust"), _plan, _policy, _gru],
                         ids=["mpc_harmonic", "mpc_robust", "plan_robust", "policy_mlp", "policy_gru"])
def test_a_rollout_without_an_action_output_is_the_same_rollout(rollout):
    with_rows, without = _pair()
    (a, state_a), (b, state_b) = rollout(with_rows, True), rollout(without, False)
    assert a["actions"].shape == (STEPS, N) and b["actions"] is None
    done = a["done"].cpu().numpy()
    assert (done[:V - 1] == 0).all() and (done[V - 1:] & fork_twin.DONE_EPISODE).all()    # rows V.. are masked lanes'
    acts = a["actions"].cpu().numpy()
    assert len(set(acts[1:V].ravel().tolist())) >= 2
    for k in ("obs", "reward", "done"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    off = fork_twin.workspace_offsets(V, N, with_rows.state_view().buffer_level - with_rows.workspace.data_ptr())
    lo = off["mpc_action"][0]
    for e in (with_rows, without):
        assert e.workspace.numel() > lo + 4 * N + 256
    assert torch.equal(with_rows.workspace[:lo], without.workspace[:lo])
    assert torch.equal(with_rows.workspace[-256:], without.workspace[-256:])
    assert torch.equal(with_rows.quality.blob, without.quality.blob)
    assert len(state_a) == len(state_b)
    for u, v in zip(state_a, state_b):
        assert torch.equal(u, v)
