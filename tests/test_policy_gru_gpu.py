"""The recurrent policy on the device (include/abr_env.h: abr_policy_gru): abr_env_policy_select_gru against the numpy
twin (tests/policy_gru_twin.py) bit for bit; commit and no commit; the fused rollout against select + step; the
episode-boundary rule under auto_reset, the episode sampler, a masked reset and a frozen lane; last_value; two launches
against one; non-finite numbers; and the controllers that were there before, untouched by it.

Small on purpose: golden traces, video_length 6 so that episodes turn over, 16 steps, a few hundred lanes at most."""
import numpy as np
import pytest
import torch

import policy_gru_twin as GT
import policy_sample_twin as ST
import policy_twin as T
from helpers import golden_workload, make_env

pytestmark = pytest.mark.gpu

f32 = np.float32
V, STEPS = 6, 16
LADDERS = {1: [1.2], 6: [0.3, 0.75, 1.2, 1.85, 2.85, 4.3], 16: list(np.round(np.linspace(0.3, 6.0, 16), 3))}


def _bits_eq(u, v):
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    return bool(((u.view(np.uint32) == v.view(np.uint32)) | (np.isnan(u) & np.isnan(v))).all())


def _np(t):
    return t.detach().cpu().numpy()


def _env(N, M=6, seed=7, **kw):
    m, traces, tid, off = golden_workload(N, seed=seed)
    meta = dict(m, video_length=V, ladder=LADDERS[M])
    env = make_env(meta, traces, N, **kw)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    return env, meta


def _pair(N, **kw):
    """Two environments that start from the same bytes (the workspace is allocated uninitialised, and the regions no
    kernel writes would otherwise differ by chance)."""
    first = _env(N, **kw)[0]
    sd = first.state_dict()
    first.close()
    envs = [_env(N, **kw)[0] for _ in range(2)]
    for e in envs:
        e.load_state_dict(sd)
    return envs


def _weights(rng, F, H, M, scale=0.6):
    cell = tuple((rng.standard_normal(s) * scale).astype(f32) for s in ((3 * H, F), (3 * H, H), (3 * H,), (3 * H,)))
    head = tuple((rng.standard_normal(s) * scale).astype(f32) for s in ((M, H), (M,)))
    vh = ((rng.standard_normal(H) * scale).astype(f32), f32(rng.standard_normal() * scale))
    return cell, head, vh


def _ctl(env, rng, H, W, M, value=False, **kw):
    import abrsimulator_amd as A
    cell, head, vh = _weights(rng, 4 + W + M, H, M)
    ctl = A.RecurrentPolicyController(A.EnvPlayer(env), cell, head, window=W, value_head=vh if value else None, **kw)
    parts = list(cell) + list(head)
    return ctl, parts, (np.concatenate([vh[0], [vh[1]]]).astype(f32) if value else None)


def _twin_inputs(env, ctl, meta):
    """(x [F, N], c [N], live [N], episode [N]) of the environment's current state, from its float64 observation."""
    f = {k: _np(v) for k, v in env.observe_f64().items()}
    hist = _np(env.history()[1])
    N, M = env.n_lanes, env.n_rates
    c = f["chunk_id"].astype(np.int64)
    dn = _np(env.mpc_inputs()[5])
    live = (dn == 0) & (c >= 0) & (c < V)
    cc = np.clip(c, 0, V - 1)
    lad = np.tile(np.asarray(meta["ladder"], np.float64), (N, 1))
    norm = _np(ctl.norm) if ctl.norm is not None else None
    x = T.features(ctl.window, M, V, cc, f["last_bitrate"].astype(np.int64), f["buffer_level"], f["global_time"],
                   f["play_time"], hist, lambda r: lad, norm)
    return x, cc, live, _np(env.episodes()["episode"]).astype(np.int64)


def _twin_select(env, ctl, meta, parts, head, commit):
    """The twin's outputs for one launch on the current state and the state slab it leaves."""
    x, c, live, ep = _twin_inputs(env, ctl, meta)
    mode = ST.SOFTMAX if ctl.sample == "softmax" else ST.ARGMAX
    return GT.select(parts, x, _np(ctl.hidden), live, ctl.seed, ctl.explore_threshold, np.arange(env.n_lanes), c, ep,
                     env.n_rates, mode, ctl.inv_temperature, head, commit)


def _assert_select(out, want, tag):
    assert np.array_equal(_np(out["actions"]), want["actions"]), tag
    for k in ("features", "scores", "probs", "hidden"):
        assert _bits_eq(_np(out[k]), want[k]), (tag, k)
    if want["value"] is not None:
        assert _bits_eq(_np(out["value"]), want["value"]), (tag, "value")


MODES = [dict(), dict(sample="softmax", temperature=0.7), dict(explore=0.3, seed=11), dict(explore=1.0, seed=5),
         dict(sample="softmax", explore=0.3, seed=3, temperature=1.5)]


def _check_select_after_prefixes(N, H, W, M, mode, value, seed):
    """select against the twin after scripted prefixes of 0, 1 and 3 steps (c = 0, 1, 3; the state nonzero after the
    first).  Returns the number of (launch, lane) cells compared."""
    rng = np.random.default_rng(seed)
    env, meta = _env(N, M, seed=seed)
    ctl, parts, head = _ctl(env, rng, H, W, M, value=value, **mode)
    cells, done_steps = 0, 0
    for prefix in (0, 1, 3):
        while done_steps < prefix:                                       # the scripted prefix commits, as a rollout does
            want, new = _twin_select(env, ctl, meta, parts, head, commit=True)
            out = ctl.select(want_probs=True, want_value=value, want_hidden=True, commit=True)
            _assert_select(out, want, (N, H, W, M, "prefix", done_steps))
            assert _bits_eq(_np(ctl.hidden), new), (N, H, W, M, "committed state", done_steps)
            env.step(out["actions"])
            done_steps += 1
            cells += N
        before = ctl.hidden.clone()
        want, _ = _twin_select(env, ctl, meta, parts, head, commit=False)
        out = ctl.select(want_probs=True, want_value=value, want_hidden=True)
        _assert_select(out, want, (N, H, W, M, "select", prefix))
        assert torch.equal(before.view(torch.int32), ctl.hidden.view(torch.int32))      # commit=False
        if prefix:
            assert np.abs(_np(out["hidden"])).max() > 0
        else:
            assert not _np(out["hidden"]).view(np.uint32).any()          # c == 0: +0.0f in every unit
        cells += N
    env.close()
    return cells


@pytest.mark.parametrize("k,N", list(enumerate([1, 63, 64, 65, 255, 256, 257, 300])))
def test_select_matches_twin_at_wave_and_workgroup_edges(k, N):
    H, W, M = [(64, 8, 6), (7, 16, 16), (1, 0, 1), (64, 16, 16), (7, 8, 6), (64, 0, 6), (7, 0, 16), (64, 8, 6)][k]
    cells = _check_select_after_prefixes(N, H, W, M, MODES[k % len(MODES)], value=bool(k % 2), seed=40 + k)
    assert cells == 6 * N


@pytest.mark.parametrize("H", [1, 7, 64])
@pytest.mark.parametrize("W", [0, 8, 16])
@pytest.mark.parametrize("M", [1, 6, 16])
def test_select_matches_twin_on_every_shape(H, W, M):
    k = H + W + M
    cells = _check_select_after_prefixes(65, H, W, M, MODES[k % len(MODES)], value=bool((k // 2) % 2), seed=k)
    assert cells == 6 * 65


@pytest.mark.parametrize("k", range(len(MODES)))
@pytest.mark.parametrize("value", [False, True])
def test_select_matches_twin_in_every_mode(k, value):
    cells = _check_select_after_prefixes(257, 7, 8, 6, MODES[k], value=value, seed=70 + k)
    assert cells == 6 * 257


def test_commit_writes_the_twins_state_on_live_lanes_only():
    rng = np.random.default_rng(3)
    N = 300
    env, meta = _env(N)
    ctl, parts, head = _ctl(env, rng, 7, 8, 6, sample="softmax")
    live_cells = dead_cells = 0
    for s in range(STEPS):                                                # no auto_reset: lanes finish after 6 steps
        if s == 8:
            env.reset()                                                   # every lane starts again
        before = _np(ctl.hidden).copy()
        want, new = _twin_select(env, ctl, meta, parts, head, commit=True)
        out = ctl.select(want_probs=True, want_hidden=True, commit=True)
        _assert_select(out, want, s)
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


SLABS = ("actions", "features", "scores", "probs", "values", "hidden", "obs", "reward", "done")


@pytest.mark.parametrize("impl", ["auto", "jump", "split", "split3"])
def test_fused_rollout_equals_select_plus_step(impl):
    N = 257
    envs = _pair(N, impl=impl, auto_reset=True)
    ctls = [_ctl(e, np.random.default_rng(9), 7, 8, 6, value=True, sample="softmax", explore=0.2, seed=99)[0] for e in envs]
    fused = envs[0].step_policy(ctls[0], STEPS, want_features=True, want_scores=True, want_probs=True, want_values=True,
                                want_hidden=True)
    cells = 0
    for s in range(STEPS):
        sel = ctls[1].select(want_probs=True, want_value=True, want_hidden=True, commit=True)
        obs, rew, dn = envs[1].step(sel["actions"])
        for k, v in (("actions", sel["actions"]), ("features", sel["features"]), ("scores", sel["scores"]),
                     ("probs", sel["probs"]), ("values", sel["value"]), ("hidden", sel["hidden"]), ("obs", obs),
                     ("reward", rew), ("done", dn)):
            assert torch.equal(fused[k][s].view(torch.uint8), v.view(torch.uint8)), (impl, s, k)
        cells += N
    assert cells == STEPS * N and int((fused["actions"] >= 0).sum()) == STEPS * N          # auto_reset: every cell live
    assert torch.equal(envs[0].workspace, envs[1].workspace)
    assert torch.equal(ctls[0].hidden.view(torch.int32), ctls[1].hidden.view(torch.int32))
    last = ctls[1].select(False, False, want_value=True)["value"]
    assert torch.equal(fused["last_value"].view(torch.int32), last.view(torch.int32))
    for e in envs:
        e.close()


def test_tick_is_refused():
    from abrsimulator_amd import _lib
    env, _ = _env(64, impl="tick")
    ctl, _, _ = _ctl(env, np.random.default_rng(1), 7, 8, 6)
    with pytest.raises(_lib.AbrError, match=r"-4"):
        env.step_policy(ctl, 2)
    env.close()


def _replay(fused, parts, head, ctl, ep0, N, M, mode):
    """The sequential twin over a rollout's slabs with norm=None: x is the features slab, c = V - features[2], the episode
    number advances where done was set (auto_reset).  Returns the cells compared and the final state."""
    feats, acts, hid, done = (_np(fused[k]) for k in ("features", "actions", "hidden", "done"))
    state = np.zeros_like(hid[0])
    ep = ep0.copy()
    cells = 0
    for t in range(feats.shape[0]):
        live = acts[t] >= 0
        c = np.where(live, V - feats[t][2].astype(np.int64), 1)
        want, state = GT.select(parts, feats[t], state, live, ctl.seed, ctl.explore_threshold, np.arange(N), c, ep, M,
                                mode, ctl.inv_temperature, head, commit=True)
        assert np.array_equal(acts[t], want["actions"]), t
        for k, slab in (("hidden", hid), ("scores", _np(fused["scores"])), ("probs", _np(fused["probs"]))):
            assert _bits_eq(slab[t], want[k]), (t, k)
        first = live & (c == 0)
        assert not hid[t][:, first].view(np.uint32).any(), t              # +0.0f at every episode start
        ep = ep + (done[t] != 0)
        cells += N
    return cells, state


@pytest.mark.parametrize("sampler", [False, True])
def test_episode_boundaries_restart_the_recurrence(sampler):
    N = 255
    env, meta = _env(N, auto_reset=True)
    if sampler:
        env.set_episode_sampler(1234, offset_span=50)
        env.reset(sample=True)
    rng = np.random.default_rng(21)
    ctl, parts, head = _ctl(env, rng, 7, 8, 6, norm=None, sample="softmax", explore=0.3, seed=8)
    ep0 = _np(env.episodes()["episode"]).astype(np.int64)
    fused = env.step_policy(ctl, STEPS, want_features=True, want_scores=True, want_probs=True, want_hidden=True)
    feats, hid = _np(fused["features"]), _np(fused["hidden"])
    first = feats[:, 2, :] == V                                           # norm=None: feature 2 is V - c
    assert first[0].all() and first[6].all() and first[12].all() and int(first.sum()) == 3 * N
    assert not hid[first.nonzero()[0], :, first.nonzero()[1]].view(np.uint32).any()
    assert np.abs(hid[5]).max() > 0 and np.abs(hid[11]).max() > 0        # the previous episode's state was not zero
    cells, state = _replay(fused, parts, head, ctl, ep0, N, 6, ST.SOFTMAX)
    assert cells == STEPS * N
    assert _bits_eq(_np(ctl.hidden), state)
    env.close()


def test_masked_reset_restarts_the_masked_lanes_only():
    N = 64
    env, meta = _env(N)
    ctl, parts, head = _ctl(env, np.random.default_rng(22), 7, 8, 6, explore=0.3, seed=4)
    mask = torch.arange(N, device=env.device) % 2 == 1
    cells = live = 0
    for s in range(STEPS):
        if s in (4, 10):
            env.reset(mask=mask)                                          # mid-episode (s = 4) and after the end (s = 10)
        want, new = _twin_select(env, ctl, meta, parts, head, commit=True)
        out = ctl.select(want_probs=True, want_hidden=True, commit=True)
        _assert_select(out, want, s)
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


def test_a_frozen_lanes_state_is_not_touched():
    N = 64
    env, meta = _env(N)
    ctl, parts, head = _ctl(env, np.random.default_rng(23), 7, 8, 6)
    out = ctl.select(commit=True)
    env.step(out["actions"])
    out = ctl.select(commit=True)
    a = out["actions"].clone()
    a[4] = 99
    env.step(a)                                                           # lane 4 is frozen from here on
    kept = ctl.hidden[:, 4].clone()
    assert float(kept.abs().max()) > 0
    for s in range(3):
        want, new = _twin_select(env, ctl, meta, parts, head, commit=True)
        out = ctl.select(want_probs=True, want_hidden=True, commit=True)
        _assert_select(out, want, s)
        assert int(out["actions"][4]) == -1 and not _np(out["hidden"])[:, 4].view(np.uint32).any()
        assert torch.equal(ctl.hidden[:, 4].view(torch.int32), kept.view(torch.int32))
        assert _bits_eq(_np(ctl.hidden), new)
        env.step(out["actions"])
    env.close()


def test_last_value_is_a_forward_only_select():
    N = 300
    env, _ = _env(N, auto_reset=True)
    ctl, _, _ = _ctl(env, np.random.default_rng(31), 64, 8, 6, value=True, sample="softmax")
    out = env.step_policy(ctl, STEPS, want_values=True)
    left = ctl.hidden.clone()
    sel = ctl.select(False, False, want_value=True, commit=False)
    assert torch.equal(out["last_value"].view(torch.int32), sel["value"].view(torch.int32))
    assert torch.equal(left.view(torch.int32), ctl.hidden.view(torch.int32))
    assert float(out["values"].abs().max()) > 0 and int((out["actions"] >= 0).sum()) == STEPS * N
    env.close()


def test_two_launches_equal_one():
    N = 257
    envs = _pair(N, auto_reset=True)
    ctls = [_ctl(e, np.random.default_rng(32), 7, 8, 6, value=True, sample="softmax", explore=0.1, seed=6)[0] for e in envs]
    kw = dict(want_features=True, want_scores=True, want_probs=True, want_values=True, want_hidden=True)
    one = envs[0].step_policy(ctls[0], STEPS, **kw)
    a = envs[1].step_policy(ctls[1], STEPS // 2, **kw)
    b = envs[1].step_policy(ctls[1], STEPS // 2, **kw)
    for k in SLABS:
        assert torch.equal(one[k].view(torch.uint8), torch.cat([a[k], b[k]]).view(torch.uint8)), k
    assert torch.equal(one["last_value"].view(torch.int32), b["last_value"].view(torch.int32))
    assert torch.equal(ctls[0].hidden.view(torch.int32), ctls[1].hidden.view(torch.int32))
    assert torch.equal(envs[0].workspace, envs[1].workspace)
    assert one["actions"].numel() == STEPS * N
    for e in envs:
        e.close()


def test_non_finite_weights_and_state():
    import abrsimulator_amd as A
    N, H, W, M = 65, 7, 8, 6
    rng = np.random.default_rng(33)
    env, meta = _env(N)
    cell, head, vh = _weights(rng, 4 + W + M, H, M)
    pool = np.array([np.nan, np.inf, -np.inf, 1e-40, -3e-42, -0.0], f32)
    cells = 0
    for special in pool:
        cell2 = tuple(t.copy() for t in cell)
        head2 = tuple(t.copy() for t in head)
        for t in cell2 + head2:
            t.ravel()[rng.integers(t.size)] = special
        ctl = A.RecurrentPolicyController(A.EnvPlayer(env), cell2, head2, window=W, value_head=vh, sample="softmax")
        ctl.hidden.copy_(torch.from_numpy(np.tanh(rng.standard_normal((H, N))).astype(f32)))
        parts, hd = list(cell2) + list(head2), np.concatenate([vh[0], [vh[1]]]).astype(f32)
        if cells == 0:
            env.step(ctl.select(commit=True)["actions"])                  # c = 1 from here on: the state is read
        want, _ = _twin_select(env, ctl, meta, parts, hd, commit=False)
        out = ctl.select(want_probs=True, want_value=True, want_hidden=True)
        _assert_select(out, want, float(special))
        cells += N
    assert cells == len(pool) * N
    # a NaN state: NaN scores, the first argmax answers 0
    ctl = A.RecurrentPolicyController(A.EnvPlayer(env), cell, head, window=W)
    ctl.hidden.fill_(float("nan"))
    out = ctl.select(want_hidden=True)
    live = _np(out["actions"]) >= 0
    assert live.all() and np.isnan(_np(out["scores"])).all() and not _np(out["actions"]).any()
    assert np.isnan(_np(out["hidden"])).all()
    env.close()


def test_existing_controllers_are_untouched():
    import abrsimulator_amd as A
    N = 512
    env, _ = _env(N)
    rng = np.random.default_rng(34)
    F = 4 + 8 + 6
    layers = [((rng.standard_normal((16, F)) * 0.5).astype(f32), rng.standard_normal(16).astype(f32)),
              ((rng.standard_normal((6, 16)) * 0.5).astype(f32), rng.standard_normal(6).astype(f32))]
    layers2 = [(w * f32(0.5), b) for w, b in layers]
    mlp = A.PolicyController(A.EnvPlayer(env), layers, window=8, sample="softmax", explore=0.2, seed=3)
    pop = A.PolicyPopulation(A.EnvPlayer(env), [layers, layers2], group=256, window=8, sample="softmax", seed=3)
    env.step_random(2, seed=1)
    before = [mlp.select(want_probs=True), pop.select(want_probs=True)]
    ws = env.workspace.clone()
    gru, _, _ = _ctl(env, rng, 64, 8, 6, value=True, sample="softmax")
    gru.select(want_probs=True, want_value=True, want_hidden=True, commit=True)
    assert torch.equal(ws, env.workspace)                                 # the state lives in the controller
    after = [mlp.select(want_probs=True), pop.select(want_probs=True)]
    for b, a in zip(before, after):
        for k in ("actions", "features", "scores", "probs"):
            assert torch.equal(b[k].view(torch.uint8), a[k].view(torch.uint8)), k
    env.step_policy(gru, 3)
    out = env.step_policy(mlp, 2, want_scores=True)
    assert out["scores"].shape == (2, 6, N)
    with pytest.raises(ValueError):
        env.step_policy(mlp, 2, want_hidden=True)
    env.close()
