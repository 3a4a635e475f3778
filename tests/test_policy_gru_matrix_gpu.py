"""The recurrent policy's matrix engine on the device (include/abr_env.h: abr_policy_gru_mx): abr_env_gru_mx_select
against the lane engine bit for bit on every shape both run, and against the numpy twin (tests/policy_gru_twin.py) above
the lane engine's width and at the column-tile edges; commit and no commit; the fused rollout against select + step and
against the lane engine's rollout; the episode-boundary rule; last_value; two launches against one; non-finite numbers at
H = 128; and the controllers that were there before, untouched by it.

The helpers, the MODES list and the sizes are tests/test_policy_gru_gpu.py's: golden traces, video_length 6, at most 16
steps and 300 lanes.  Every comparison is over all cells, on bits (NaN equal to NaN), and each test asserts the number of
(launch, lane) cells it compared."""
import numpy as np
import pytest
import torch

import policy_gru_twin as GT
import policy_sample_twin as ST
import test_policy_gru_gpu as G
from test_policy_gru_gpu import MODES, SLABS, STEPS, V, _bits_eq, _np

pytestmark = pytest.mark.gpu

f32 = np.float32
MX = dict(engine="matrix")


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _two_engines(N, H, W, M, mode, value, seed, **envkw):
    """Two environments from the same bytes, a lane controller on the first and a matrix controller on the second,
    built from the same weights."""
    envs = G._pair(N, M=M, seed=seed, **envkw)
    lane = G._ctl(envs[0], np.random.default_rng(seed), H, W, M, value=value, **mode)[0]
    mx = G._ctl(envs[1], np.random.default_rng(seed), H, W, M, value=value, **dict(mode, **MX))[0]
    assert lane.engine == "lane" and mx.engine == "matrix" and _same(lane.weights, mx.weights)
    return envs, lane, mx


def _check_engines_agree(N, H, W, M, mode, value, seed):
    """select on both engines after scripted prefixes of 0, 1 and 3 committed steps: every output and the committed slab,
    bit for bit.  Returns the number of (launch, lane) cells compared."""
    envs, lane, mx = _two_engines(N, H, W, M, mode, value, seed)
    kw = dict(want_probs=True, want_value=value, want_hidden=True)
    keys = ("actions", "features", "scores", "probs", "hidden") + (("value",) if value else ())
    cells = done_steps = 0
    for prefix in (0, 1, 3):
        while done_steps < prefix:
            a, b = lane.select(commit=True, **kw), mx.select(commit=True, **kw)
            for k in keys:
                assert _same(a[k], b[k]), (H, W, M, "prefix", done_steps, k)
            assert _same(lane.hidden, mx.hidden), (H, W, M, "committed state", done_steps)
            envs[0].step(a["actions"])
            envs[1].step(b["actions"])
            done_steps += 1
            cells += N
        before = mx.hidden.clone()
        a, b = lane.select(**kw), mx.select(**kw)
        for k in keys:
            assert _same(a[k], b[k]), (H, W, M, "select", prefix, k)
        assert _same(before, mx.hidden)                                       # commit=False
        if prefix:
            assert float(b["hidden"].abs().max()) > 0
        cells += N
    assert torch.equal(envs[0].workspace, envs[1].workspace)
    for e in envs:
        e.close()
    return cells


@pytest.mark.parametrize("H", [1, 7, 31, 32, 33, 64])
@pytest.mark.parametrize("W", [0, 8, 16])
@pytest.mark.parametrize("M", [1, 6, 16])
def test_select_equals_the_lane_engine_on_every_shared_shape(H, W, M):
    k = H + W + M
    cells = _check_engines_agree(65, H, W, M, MODES[k % len(MODES)], value=bool((k // 2) % 2), seed=k)
    assert cells == 6 * 65


@pytest.mark.parametrize("k", range(len(MODES)))
@pytest.mark.parametrize("value", [False, True])
def test_select_equals_the_lane_engine_in_every_mode(k, value):
    cells = _check_engines_agree(257, 33, 8, 6, MODES[k], value=value, seed=70 + k)
    assert cells == 6 * 257


@pytest.mark.parametrize("H", [65, 96, 127, 128])
@pytest.mark.parametrize("k", range(len(MODES)))
def test_select_matches_twin_above_the_lane_engines_width(H, k):
    W, M = [(8, 6), (16, 16), (0, 1), (16, 6), (0, 16)][(k + H) % 5]
    cells = G._check_select_after_prefixes(65, H, W, M, dict(MODES[k], **MX), value=bool((k + H) % 2), seed=H + k)
    assert cells == 6 * 65


@pytest.mark.parametrize("k,N", list(enumerate([1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300])))
def test_select_matches_twin_at_column_tile_wave_and_workgroup_edges(k, N):
    H, W, M = [(128, 8, 6), (65, 16, 16), (1, 0, 1), (96, 16, 16), (33, 8, 6), (127, 0, 6), (7, 0, 16), (128, 8, 6),
               (64, 8, 6), (96, 0, 1), (65, 8, 6)][k]
    cells = G._check_select_after_prefixes(N, H, W, M, dict(MODES[k % len(MODES)], **MX), value=bool(k % 2), seed=40 + k)
    assert cells == 6 * N


def test_a_finished_lane_inside_a_column_tile_of_live_neighbours():
    N, H = 70, 96
    env, meta = G._env(N)
    ctl, parts, head = G._ctl(env, np.random.default_rng(23), H, 8, 6, value=True, sample="softmax", **MX)
    env.step(ctl.select(commit=True)["actions"])
    a = ctl.select(commit=True)["actions"].clone()
    frozen = [4, 37, 63, 64]                                              # both column tiles of wave 0, and wave 1's first lane
    a[frozen] = 99
    env.step(a)                                                           # these lanes are frozen from here on
    kept = ctl.hidden[:, frozen].clone()
    assert float(kept.abs().max()) > 0
    cells = 0
    for s in range(3):
        want, new = G._twin_select(env, ctl, meta, parts, head, commit=True)
        out = ctl.select(want_probs=True, want_value=True, want_hidden=True, commit=True)
        G._assert_select(out, want, s)
        acts = _np(out["actions"])
        assert (acts[frozen] == -1).all() and (np.delete(acts, frozen) >= 0).all()
        assert not _np(out["hidden"])[:, frozen].view(np.uint32).any()
        assert _same(ctl.hidden[:, frozen], kept)                         # a frozen lane's column is untouched
        assert _bits_eq(_np(ctl.hidden), new)
        env.step(out["actions"])
        cells += N
    assert cells == 3 * N
    env.close()


def test_commit_writes_the_twins_state_on_live_lanes_only():
    rng = np.random.default_rng(3)
    N, H = 300, 65
    env, meta = G._env(N)
    ctl, parts, head = G._ctl(env, rng, H, 8, 6, sample="softmax", **MX)
    live_cells = dead_cells = 0
    for s in range(STEPS):                                                # no auto_reset: lanes finish after 6 steps
        if s == 8:
            env.reset()                                                   # every lane starts again
        before = _np(ctl.hidden).copy()
        want, _ = G._twin_select(env, ctl, meta, parts, head, commit=False)
        out = ctl.select(want_probs=True, want_hidden=True, commit=False)
        G._assert_select(out, want, (s, "no commit"))
        assert np.array_equal(_np(ctl.hidden).view(np.uint32), before.view(np.uint32)), s      # byte for byte
        want, new = G._twin_select(env, ctl, meta, parts, head, commit=True)
        out = ctl.select(want_probs=True, want_hidden=True, commit=True)
        G._assert_select(out, want, s)
        after = _np(ctl.hidden)
        dead = want["actions"] < 0
        assert _bits_eq(after, new), s
        assert np.array_equal(after[:, dead].view(np.uint32), before[:, dead].view(np.uint32)), s   # not touched
        live_cells += int((~dead).sum())
        dead_cells += int(dead.sum())
        env.step(out["actions"])
    assert live_cells + dead_cells == STEPS * N
    assert live_cells == 12 * N and dead_cells == 4 * N              # 6 of every 8 steps
    env.close()


@pytest.mark.parametrize("impl", ["auto", "jump", "split", "split3"])
def test_fused_rollout_equals_select_plus_step(impl):
    N, H = 257, 96
    envs = G._pair(N, impl=impl, auto_reset=True)
    ctls = [G._ctl(e, np.random.default_rng(9), H, 8, 6, value=True, sample="softmax", explore=0.2, seed=99, **MX)[0]
            for e in envs]
    fused = envs[0].step_policy(ctls[0], STEPS, want_features=True, want_scores=True, want_probs=True, want_values=True,
                                want_hidden=True)
    cells = 0
    for s in range(STEPS):
        sel = ctls[1].select(want_probs=True, want_value=True, want_hidden=True, commit=True)
        obs, rew, dn = envs[1].step(sel["actions"])
        for k, v in (("actions", sel["actions"]), ("features", sel["features"]), ("scores", sel["scores"]),
                     ("probs", sel["probs"]), ("values", sel["value"]), ("hidden", sel["hidden"]), ("obs", obs),
                     ("reward", rew), ("done", dn)):
            assert _same(fused[k][s], v), (impl, s, k)
        cells += N
    assert cells == STEPS * N and int((fused["actions"] >= 0).sum()) == STEPS * N          # auto_reset: every cell live
    assert torch.equal(envs[0].workspace, envs[1].workspace)
    assert _same(ctls[0].hidden, ctls[1].hidden)
    last = ctls[1].select(False, False, want_value=True)["value"]
    assert _same(fused["last_value"], last)
    for e in envs:
        e.close()


def test_fused_rollout_equals_the_lane_engines_at_64_units():
    N = 257
    envs, lane, mx = _two_engines(N, 64, 8, 6, dict(sample="softmax", explore=0.2, seed=99), True, 9, auto_reset=True)
    kw = dict(want_features=True, want_scores=True, want_probs=True, want_values=True, want_hidden=True)
    a, b = envs[0].step_policy(lane, STEPS, **kw), envs[1].step_policy(mx, STEPS, **kw)
    for k in SLABS + ("last_value",):
        assert _same(a[k], b[k]), k
    assert a["actions"].numel() == STEPS * N and int((b["actions"] >= 0).sum()) == STEPS * N
    assert torch.equal(envs[0].workspace, envs[1].workspace)
    assert _same(lane.hidden, mx.hidden)
    for e in envs:
        e.close()


def test_tick_is_refused():
    from abrsimulator_amd import _lib
    env, _ = G._env(64, impl="tick")
    ctl, _, _ = G._ctl(env, np.random.default_rng(1), 96, 8, 6, **MX)
    with pytest.raises(_lib.AbrError, match=r"-4"):
        env.step_policy(ctl, 2)
    env.close()


@pytest.mark.parametrize("sampler", [False, True])
def test_episode_boundaries_restart_the_recurrence(sampler):
    N, H = 255, 65
    env, meta = G._env(N, auto_reset=True)
    if sampler:
        env.set_episode_sampler(1234, offset_span=50)
        env.reset(sample=True)
    rng = np.random.default_rng(21)
    ctl, parts, head = G._ctl(env, rng, H, 8, 6, norm=None, sample="softmax", explore=0.3, seed=8, **MX)
    ep0 = _np(env.episodes()["episode"]).astype(np.int64)
    fused = env.step_policy(ctl, STEPS, want_features=True, want_scores=True, want_probs=True, want_hidden=True)
    feats, hid = _np(fused["features"]), _np(fused["hidden"])
    first = feats[:, 2, :] == V                                           # norm=None: feature 2 is V - c
    assert first[0].all() and first[6].all() and first[12].all() and int(first.sum()) == 3 * N
    assert not hid[first.nonzero()[0], :, first.nonzero()[1]].view(np.uint32).any()
    assert np.abs(hid[5]).max() > 0 and np.abs(hid[11]).max() > 0        # the previous episode's state was not zero
    cells, state = G._replay(fused, parts, head, ctl, ep0, N, 6, ST.SOFTMAX)
    assert cells == STEPS * N
    assert _bits_eq(_np(ctl.hidden), state)
    env.close()


def test_masked_reset_restarts_the_masked_lanes_only():
    N, H = 64, 96
    env, meta = G._env(N)
    ctl, parts, head = G._ctl(env, np.random.default_rng(22), H, 8, 6, explore=0.3, seed=4, **MX)
    mask = torch.arange(N, device=env.device) % 2 == 1
    cells = live = 0
    for s in range(STEPS):
        if s in (4, 10):
            env.reset(mask=mask)                                          # mid-episode (s = 4) and after the end (s = 10)
        want, new = G._twin_select(env, ctl, meta, parts, head, commit=True)
        out = ctl.select(want_probs=True, want_hidden=True, commit=True)
        G._assert_select(out, want, s)
        assert _bits_eq(_np(ctl.hidden), new), s
        if s in (4, 10):
            assert (_np(out["actions"])[1::2] >= 0).all()
            assert not _np(out["hidden"])[:, 1::2].view(np.uint32).any(), s       # restarted: +0.0f
        if s == 4:
            assert np.abs(_np(out["hidden"])[:, 0::2]).max() > 0                  # the others carry on
        live += int((_np(out["actions"]) >= 0).sum())
        env.step(out["actions"])
        cells += N
    assert cells == STEPS * N
    assert live == 6 * (N // 2) + (4 + 6 + 6) * (N // 2)                  # even lanes: 6 steps; odd: 4, then 6, then 6
    env.close()


def test_last_value_is_a_forward_only_select():
    N = 300
    env, _ = G._env(N, auto_reset=True)
    ctl, _, _ = G._ctl(env, np.random.default_rng(31), 128, 8, 6, value=True, sample="softmax", **MX)
    out = env.step_policy(ctl, STEPS, want_values=True)
    left = ctl.hidden.clone()
    sel = ctl.select(False, False, want_value=True, commit=False)
    assert _same(out["last_value"], sel["value"])
    assert _same(left, ctl.hidden)
    assert float(out["values"].abs().max()) > 0 and int((out["actions"] >= 0).sum()) == STEPS * N
    assert out["last_value"].numel() == N
    env.close()


def test_two_launches_equal_one():
    N = 257
    envs = G._pair(N, auto_reset=True)
    ctls = [G._ctl(e, np.random.default_rng(32), 96, 8, 6, value=True, sample="softmax", explore=0.1, seed=6, **MX)[0]
            for e in envs]
    kw = dict(want_features=True, want_scores=True, want_probs=True, want_values=True, want_hidden=True)
    one = envs[0].step_policy(ctls[0], STEPS, **kw)
    a = envs[1].step_policy(ctls[1], STEPS // 2, **kw)
    b = envs[1].step_policy(ctls[1], STEPS // 2, **kw)
    for k in SLABS:
        assert _same(one[k], torch.cat([a[k], b[k]])), k
    assert _same(one["last_value"], b["last_value"])
    assert _same(ctls[0].hidden, ctls[1].hidden)
    assert torch.equal(envs[0].workspace, envs[1].workspace)
    assert one["actions"].numel() == STEPS * N
    for e in envs:
        e.close()


def test_non_finite_weights_and_state_at_128_units():
    import abrsimulator_amd as A
    N, H, W, M = 65, 128, 8, 6
    rng = np.random.default_rng(33)
    env, meta = G._env(N)
    cell, head, vh = G._weights(rng, 4 + W + M, H, M, scale=0.3)
    pool = np.array([np.nan, np.inf, -np.inf, 1e-40, -3e-42, -0.0], f32)
    cells = 0
    for special in pool:
        cell2 = tuple(t.copy() for t in cell)
        head2 = tuple(t.copy() for t in head)
        for t in cell2 + head2:
            t.ravel()[rng.integers(t.size)] = special
        ctl = A.RecurrentPolicyController(A.EnvPlayer(env), cell2, head2, window=W, value_head=vh, sample="softmax", **MX)
        state = np.tanh(rng.standard_normal((H, N))).astype(f32)
        state[rng.integers(H), ::2] = special                             # a row of the state, every other lane
        state[:, rng.integers(N)] = special                               # and a whole column
        ctl.hidden.copy_(torch.from_numpy(state))
        parts, hd = list(cell2) + list(head2), np.concatenate([vh[0], [vh[1]]]).astype(f32)
        if cells == 0:
            env.step(ctl.select(commit=True)["actions"])                  # c = 1 from here on: the state is read
            ctl.hidden.copy_(torch.from_numpy(state))
        want, _ = G._twin_select(env, ctl, meta, parts, hd, commit=False)
        out = ctl.select(want_probs=True, want_value=True, want_hidden=True)
        G._assert_select(out, want, float(special))
        cells += N
    assert cells == len(pool) * N
    # a NaN state: NaN scores, the first argmax answers 0
    ctl = A.RecurrentPolicyController(A.EnvPlayer(env), cell, head, window=W, **MX)
    ctl.hidden.fill_(float("nan"))
    out = ctl.select(want_hidden=True)
    live = _np(out["actions"]) >= 0
    assert live.all() and np.isnan(_np(out["scores"])).all() and not _np(out["actions"]).any()
    assert np.isnan(_np(out["hidden"])).all()
    env.close()


def test_other_controllers_are_untouched():
    import abrsimulator_amd as A
    N = 512
    env, _ = G._env(N)
    rng = np.random.default_rng(34)
    F = 4 + 8 + 6
    layers = [((rng.standard_normal((16, F)) * 0.5).astype(f32), rng.standard_normal(16).astype(f32)),
              ((rng.standard_normal((6, 16)) * 0.5).astype(f32), rng.standard_normal(6).astype(f32))]
    layers2 = [(w * f32(0.5), b) for w, b in layers]
    mlp = A.PolicyController(A.EnvPlayer(env), layers, window=8, sample="softmax", explore=0.2, seed=3)
    pop = A.PolicyPopulation(A.EnvPlayer(env), [layers, layers2], group=256, window=8, sample="softmax", seed=3)
    lane, _, _ = G._ctl(env, np.random.default_rng(35), 64, 8, 6, value=True, sample="softmax")
    env.step_random(2, seed=1)
    kw = dict(want_probs=True, want_value=True, want_hidden=True)
    before = [mlp.select(want_probs=True), pop.select(want_probs=True), lane.select(**kw)]
    ws = env.workspace.clone()
    kept = lane.hidden.clone()
    mx, _, _ = G._ctl(env, rng, 128, 8, 6, value=True, sample="softmax", **MX)
    mx.select(commit=True, **kw)
    assert torch.equal(ws, env.workspace)                                 # the state lives in the controller
    assert _same(kept, lane.hidden) and float(mx.hidden.abs().max()) > 0
    after = [mlp.select(want_probs=True), pop.select(want_probs=True), lane.select(**kw)]
    for b, a in zip(before, after):
        for k in b:
            if b[k] is not None:
                assert _same(b[k], a[k]), k
    env.step_policy(mx, 3)
    out = env.step_policy(mlp, 2, want_scores=True)
    assert out["scores"].shape == (2, 6, N)
    out = env.step_policy(lane, 2, want_hidden=True)
    assert out["hidden"].shape == (2, 64, N)
    with pytest.raises(ValueError):
        env.step_policy(mlp, 2, want_hidden=True)
    env.close()
