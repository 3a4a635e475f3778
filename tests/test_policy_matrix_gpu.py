"""The matrix engine of the learned policy on the device (include/abr_env.h: abr_policy_mx; abr_env.hip: policy_mx_kernel):
bit for bit the lane engine on every shape both can run -- the test of the hardware's accumulation order inside
v_mfma_f32_32x32x2_f32 -- and bit for bit the numpy twins on the shapes only it can run, with special weights, at the
lane-count edges, with finished lanes inside a 32-column tile, in fused rollouts on every event-driven kernel, and after
load_weights."""
import ctypes as C

import numpy as np
import pytest
import torch

import actor_critic_twin as AC
from test_actor_critic_gpu import _head
from test_policy_cpu import _layers as _special_layers
from test_policy_gpu import LADDER, _env, _layers
from test_policy_gpu import _twin_select as _twin_argmax
from test_policy_sample_gpu import _bits_eq, _twin_select

pytestmark = pytest.mark.gpu

f32 = np.float32
FLOATS = ("features", "scores", "probs", "value")


def _ladder(M):
    return LADDER if M == 6 else [1.2] if M == 1 else list(np.round(np.geomspace(0.2, 8.0, M), 3))


def _same(a, b, tag):
    """Two select() / step_policy() dicts, bit for bit (any NaN equal to any NaN)."""
    assert a.keys() == b.keys(), tag
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (tag, k)
        elif a[k].dtype == torch.float32:
            assert _bits_eq(a[k].cpu().numpy(), b[k].cpu().numpy()), (tag, k)
        else:
            assert torch.equal(a[k], b[k]), (tag, k)


def _pair(A, env, layers, head, W, **kw):
    return [A.PolicyController(A.EnvPlayer(env), layers, window=W, value_head=head, engine=e, **kw)
            for e in ("lane", "matrix")]


# ---------------------------------------------------------------------------------------------------------------------
# matrix engine == lane engine

SHARED = ([], [1], [5], [31], [32], [33], [64], [64, 64], [64, 1], [1, 64], [33, 17])


@pytest.mark.parametrize("M", (1, 6, 16))
def test_matrix_engine_equals_lane_engine_bit_for_bit(M):
    import abrsimulator_amd as A
    rng = np.random.default_rng(200 + M)
    V, N = 12, 1000
    env = _env(A, V, N, rng, br=np.tile(_ladder(M), (V, 1)))
    env.step_random(2, seed=5, want_actions=False)
    distinct = 0
    for W in (0, 8, 16):
        F = 4 + W + M
        for hidden in SHARED:
            layers = _layers(rng, F, list(hidden), M)
            head = _head(rng, list(hidden), F)
            seed = int(rng.integers(1 << 62))
            lane, mx = _pair(A, env, layers, head, W, seed=seed, temperature=0.7)
            assert type(mx.bound(env)) is A._lib.PolicyMx and type(lane.bound(env)) is A._lib.Policy
            for sample, explore, probs, value in (("argmax", 0.0, False, False), ("softmax", 0.3, True, True),
                                                  ("argmax", 0.3, True, False), ("softmax", 0.0, False, True)):
                for c in (lane, mx):
                    c.sample, c.explore = sample, explore
                a = lane.select(want_probs=probs, want_value=value)
                b = mx.select(want_probs=probs, want_value=value)
                _same(a, b, (M, W, hidden, sample, explore))
            distinct = max(distinct, len(torch.unique(b["scores"])))
        env.step_random(3, seed=W, want_actions=False)                     # other rollout states for the next window
    assert distinct > N // 2                                               # scores worth comparing
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
# the shapes only the matrix engine runs == the twins

def _check_twin(env, ctl, layers, head, br, episode, tag):
    out = ctl.select(want_probs=True, want_value=True)
    x, sc, a, p = _twin_select(env, ctl, layers, br, episode=episode)
    live = a >= 0
    assert _bits_eq(out["features"].cpu().numpy(), x), tag
    assert _bits_eq(out["scores"].cpu().numpy(), sc), tag
    assert _bits_eq(out["probs"].cpu().numpy(), p), tag
    assert np.array_equal(out["actions"].cpu().numpy(), a), tag
    want_v = np.where(live, AC.value(layers, head, x), f32(0)).astype(np.float32)
    assert _bits_eq(out["value"].cpu().numpy(), want_v), tag
    return out, live


WIDE = ([65], [96, 33], [128], [128, 128], [128, 128, 128], [1, 1, 1], [128, 1, 128])


@pytest.mark.parametrize("hidden", WIDE, ids=lambda h: "x".join(map(str, h)))
def test_wide_shapes_match_the_twin(hidden):
    import abrsimulator_amd as A
    rng = np.random.default_rng(300 + sum(hidden))
    V, N = 10, 257
    W, M = (16, 16) if hidden == [128, 128, 128] else (7, 6) if len(hidden) == 2 else (8, 6)   # F = 36, 17, 18
    F = 4 + W + M
    br = np.tile(_ladder(M), (V, 1))
    env = _env(A, V, N, rng, br=br)
    env.step_random(3, seed=1, want_actions=False)
    for special in (False, True):
        layers = _special_layers(rng, F, list(hidden), M, special)
        hl = _special_layers(rng, hidden[-1], [], 1, special)[0]
        head = (hl[0][0], hl[1][0])
        if special:                                                         # every kind of special value at least once
            layers[0][0][0, :5] = [np.nan, np.inf, -np.inf, -0.0, 1e-41]
            layers[-1][1][0] = f32(1e-41)
            head[0][:3] = [-0.0, 1e-41, np.inf if len(hidden) == 3 else 1e-40][:head[0].size]
        ctl = A.PolicyController(A.EnvPlayer(env), layers, window=W, value_head=head, engine="matrix", sample="softmax",
                                 temperature=0.9, explore=0.25, seed=int(rng.integers(1 << 62)))
        assert ctl.bound(env).weights_bytes == 4 * sum(w.size + b.size for w, b in layers)
        out, live = _check_twin(env, ctl, layers, head, br, 0, (hidden, special))
        assert live.all()
        if not special:
            assert np.isfinite(out["scores"].cpu().numpy()).all()
            assert len(torch.unique(out["value"])) > N // 2 or min(hidden) == 1     # a width of 1 may sit at ReLU's 0
    env.close()


@pytest.mark.parametrize("N", (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000))
def test_lane_count_edges(N):
    import abrsimulator_amd as A
    rng = np.random.default_rng(400)
    V, W, M = 8, 8, 6
    env = _env(A, V, N, rng)
    env.step_random(2, seed=3, want_actions=False)
    layers = _layers(rng, 4 + W + M, [128, 128], M)
    head = _head(rng, [128, 128], 4 + W + M)
    ctl = A.PolicyController(A.EnvPlayer(env), layers, window=W, value_head=head, engine="matrix", sample="softmax", seed=7)
    br = np.tile(LADDER, (V, 1))
    out, live = _check_twin(env, ctl, layers, head, br, 0, N)
    assert live.all()
    # nothing is written past lane N - 1: every output with a guard behind it
    pol, smp, val = ctl.bound(env), ctl.sampling(), ctl.value()
    dev = env.device
    act = torch.full((N + 64,), -7, dtype=torch.int32, device=dev)
    guards = {k: torch.full((rows * N + 64,), 123.0, device=dev) for k, rows in
              (("features", 4 + W + M), ("scores", M), ("probs", M), ("value", 1))}
    env._call(env.lib.abr_env_policy_select_mx, env._h, C.byref(pol), C.byref(smp), C.byref(val), A._lib.ptr(act),
              *(A._lib.ptr(guards[k]) for k in FLOATS))
    assert (act[N:] == -7).all() and torch.equal(act[:N], out["actions"])
    for k in FLOATS:
        assert (guards[k][-64:] == 123.0).all(), k
        assert _bits_eq(guards[k][:-64].cpu().numpy(), out[k].reshape(-1).cpu().numpy()), k
    env.close()


def test_finished_lanes_inside_a_column_tile():
    import abrsimulator_amd as A
    rng = np.random.default_rng(500)
    V, N, W, M = 6, 200, 4, 6
    env = _env(A, V, N, rng, auto_reset=False)
    env.step_random(V, seed=1, want_actions=False)                          # every lane has finished
    again = (np.arange(N) % 3 != 1) & (np.arange(N) % 7 != 0)               # live and finished lanes interleaved
    env.reset(mask=torch.from_numpy(again.astype(np.uint8)).to(env.device))
    env.step_random(2, seed=2, want_actions=False)
    layers = _layers(rng, 4 + W + M, [128, 33], M)
    head = _head(rng, [128, 33], 4 + W + M)
    ctl = A.PolicyController(A.EnvPlayer(env), layers, window=W, value_head=head, engine="matrix")
    out = ctl.select(want_probs=True, want_value=True)
    x, sc, a = _twin_argmax(env, ctl, layers, np.tile(LADDER, (V, 1)))
    live = a >= 0
    assert np.array_equal(live, again)
    for t in range(0, N - 31, 32):
        assert 0 < live[t:t + 32].sum() < 32                                # both kinds in every tile
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["actions"], a) and (got["actions"][~live] == -1).all()
    for k in ("features", "scores", "probs"):
        assert (got[k][:, ~live].view(np.uint32) == 0).all(), k             # +0.0f columns
    assert (got["value"][~live].view(np.uint32) == 0).all()
    assert _bits_eq(got["features"], x) and _bits_eq(got["scores"], sc)
    assert _bits_eq(got["value"], np.where(live, AC.value(layers, head, x), f32(0)).astype(np.float32))
    g = np.argmax(got["probs"][:, live], axis=0)
    assert np.array_equal(g, a[live]) and (got["probs"][:, live].sum(0) == 1).all()   # argmax: one-hot at the action
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
# fused rollouts

def _start(A, impl, V, N, sampler):
    """Two environments that start from the same bytes (the workspace is allocated uninitialised)."""
    first = _env(A, V, N, np.random.default_rng(5), impl=impl, auto_reset=True)
    sd = first.state_dict()
    first.close()
    envs = [_env(A, V, N, np.random.default_rng(5), impl=impl, auto_reset=True) for _ in range(2)]
    for e in envs:
        e.load_state_dict(sd)
        if sampler:
            e.set_episode_sampler(4242, offset_span=100)
    return envs


@pytest.mark.parametrize("impl", ("auto", "jump", "split", "split3"))
def test_fused_rollouts(impl):
    import abrsimulator_amd as A
    rng = np.random.default_rng(600)
    V, N, W, M = 10, 1000, 4, 6
    F = 4 + W + M
    want = dict(want_features=True, want_scores=True, want_probs=True, want_values=True)
    # a wide shape: step_policy == select + step
    layers, head = _layers(rng, F, [96, 33], M), _head(rng, [96, 33], F)
    envs = _start(A, impl, V, N, False)
    ctls = [A.PolicyController(A.EnvPlayer(e), layers, window=W, value_head=head, engine="matrix", sample="softmax",
                               temperature=0.8, explore=0.2, seed=99) for e in envs]
    n = 13
    fused = envs[0].step_policy(ctls[0], n, **want)
    for s in range(n):
        sel = ctls[1].select(want_probs=True, want_value=True)
        obs, rew, dn = envs[1].step(sel["actions"])
        for k, ref in (("actions", sel["actions"]), ("features", sel["features"]), ("scores", sel["scores"]),
                       ("probs", sel["probs"]), ("values", sel["value"]), ("obs", obs), ("reward", rew), ("done", dn)):
            assert torch.equal(fused[k][s], ref), (impl, s, k)
    assert torch.equal(fused["last_value"], ctls[1].select(want_value=True)["value"])
    assert (fused["done"] != 0).any() and len(torch.unique(fused["values"])) > N
    for e in envs:
        e.close()
    # 64 x 64: every output and the workspace == the lane engine's rollout, over three sampled episodes
    layers, head = _layers(rng, F, [64, 64], M), _head(rng, [64, 64], F)
    n = 3 * V + 2
    for sample, explore, kw in (("softmax", 0.2, want), ("argmax", 0.3, dict(want_scores=True)),
                                ("argmax", 0.0, dict(want_values=True))):
        envs = _start(A, impl, V, N, True)
        outs = [e.step_policy(A.PolicyController(A.EnvPlayer(e), layers, window=W, value_head=head, engine=eng,
                                                 sample=sample, temperature=0.8, explore=explore, seed=99), n, **kw)
                for e, eng in zip(envs, ("lane", "matrix"))]
        _same(outs[0], outs[1], (impl, sample, explore))
        assert torch.equal(envs[0].workspace, envs[1].workspace), (impl, sample, explore)
        assert ((outs[1]["done"] != 0).sum(0) >= 3).all()
        if "want_values" in kw:
            assert outs[1]["values"].shape == (n, N) and outs[1]["last_value"].shape == (N,)
        for e in envs:
            e.close()


def test_tick_is_refused_and_sizes_are_checked():
    import abrsimulator_amd as A
    from abrsimulator_amd import _lib
    rng = np.random.default_rng(700)
    V, N = 6, 300
    tick = _env(A, V, N, np.random.default_rng(2), impl="tick")
    layers, head = _layers(rng, 13, [128], 6), _head(rng, [128], 13)
    ctl = A.PolicyController(A.EnvPlayer(tick), layers, window=3, value_head=head, engine="matrix")
    for kw in (dict(), dict(want_values=True), dict(want_probs=True)):
        with pytest.raises(_lib.AbrError, match=r"-4"):
            tick.step_policy(ctl, 2, **kw)
    assert (ctl.select(want_value=True)["actions"] >= 0).all()             # select runs on every impl
    act = torch.empty(N, dtype=torch.int32, device=tick.device)
    pol, val = ctl.bound(tick), ctl.value()
    pol.weights_bytes -= 4
    rc = tick.lib.abr_env_policy_select_mx(tick._h, C.byref(pol), None, None, _lib.ptr(act), None, None, None, None, None)
    assert rc == -1 and b"weights_bytes" in tick.lib.abr_last_error()
    pol = ctl.bound(tick)
    val.head_bytes += 4
    rc = tick.lib.abr_env_step_policy_mx(tick._h, C.byref(pol), None, C.byref(val), 1, None, None, None, None, None, None,
                                         None, None, None, None)
    assert rc == -1 and b"head_bytes" in tick.lib.abr_last_error()
    # smp == NULL is the first argmax
    rc = tick.lib.abr_env_policy_select_mx(tick._h, C.byref(pol), None, None, _lib.ptr(act), None, None, None, None, None)
    assert rc == 0 and torch.equal(act, ctl.select()["actions"])
    tick.close()


def test_load_weights_changes_the_next_decision():
    import abrsimulator_amd as A
    V, N = 16, 1024
    env = _env(A, V, N, np.random.default_rng(6))
    nn = torch.nn
    net = nn.Sequential(nn.Linear(18, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(),
                        nn.Linear(128, 6)).cuda()
    ctl = A.PolicyController.from_module(A.EnvPlayer(env), net, window=8, engine="matrix")
    env.step_policy(ctl, 3)
    first = ctl.select()
    with torch.no_grad():
        for prm in net.parameters():
            prm.add_(0.3 * torch.randn_like(prm))
    ctl.load_weights(net)                                                  # in place, on the stream
    layers = [(Wt.detach().cpu().numpy(), b.detach().cpu().numpy()) for Wt, b in ctl.layers()]
    second = ctl.select()
    x, s, a = _twin_argmax(env, ctl, layers, np.tile(LADDER, (V, 1)))
    assert torch.equal(first["features"], second["features"]) and not torch.equal(first["scores"], second["scores"])
    assert _bits_eq(second["scores"].cpu().numpy(), s) and np.array_equal(second["actions"].cpu().numpy(), a)
    assert not torch.equal(first["actions"], second["actions"])
    env.close()
