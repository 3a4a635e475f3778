"""Actor-critic rollouts on the device: select(want_value=True) against the numpy twin (tests/actor_critic_twin.py) bit
for bit on states reached by random rollouts; the workgroup edge; the fused rollout with values against select + step and
against a run without values; A.gae on the rollout's own slabs and on the CPU tests' edge slabs against the twin, and
against the float64 meaning checks of tests/test_actor_critic_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import actor_critic_twin as AC
from test_actor_critic_cpu import check_lambda_zero_is_the_td_error, check_returns_are_episode_sums
from test_policy_gpu import LADDER, _env, _layers
from test_policy_sample_gpu import _bits_eq, _twin_select

pytestmark = pytest.mark.gpu

f32 = np.float32


def _head(rng, widths, F):
    n_in = widths[-1] if widths else F
    return rng.normal(0, 1.0 / np.sqrt(n_in), n_in).astype(np.float32), f32(rng.normal())


def _twin_value(x, live, layers, head):
    """The twin's value [N] on the twin's features x [F, N] (zero columns on lanes that are not live)."""
    return np.where(live, AC.value(layers, head, x), f32(0)).astype(np.float32)


def _check_select(env, ctl, layers, head, br, episode, tag):
    """select(want_value=True) == the twins, in both sampling modes, and its other outputs == the entries without a
    value.  Returns the softmax actions and the values."""
    out = ctl.select(want_probs=True, want_value=True)
    ref = ctl.select(want_probs=True)
    for k in ("actions", "features", "scores", "probs"):
        assert torch.equal(out[k], ref[k]), (tag, k)
    x, sc, a, p = _twin_select(env, ctl, layers, br, episode=episode)
    assert np.array_equal(out["actions"].cpu().numpy(), a), tag
    assert _bits_eq(out["scores"].cpu().numpy(), sc), tag
    live = a >= 0
    v = out["value"].cpu().numpy()
    assert _bits_eq(v, _twin_value(x, live, layers, head)), tag
    assert (v[~live].view(np.uint32) == 0).all(), tag                      # +0.0f on done lanes
    mode = ctl.sample
    ctl.sample = "argmax"                                                  # without probs: the plain instance with a value
    plain, ref = ctl.select(want_value=True), ctl.select()
    ctl.sample = mode
    for k in ("actions", "features", "scores"):
        assert torch.equal(plain[k], ref[k]), (tag, k)
    assert plain["probs"] is None and torch.equal(plain["value"], out["value"]), tag
    return a, v


def test_select_value_matches_twin_on_random_rollout_states():
    import abrsimulator_amd as A
    rng = np.random.default_rng(81)
    V, N = 20, 4096
    br = np.sort(np.tile(LADDER, (V, 1)) * rng.uniform(0.8, 1.2, (V, 6)), axis=1)
    speeds = rng.choice([0.75, 1.0, 1.25, 1.5], N)
    env = _env(A, V, N, rng, br=br, speeds=speeds)
    shapes = ((8, [64, 64], 0.0, 1.0), (16, [5], 0.25, 0.3), (0, [], 0.0, 2.0), (1, [64, 1], 1.0, 1.0),
              (4, [16, 16], 0.25, 0.05))
    for ep, (W, widths, explore, temp) in enumerate(shapes):
        env.reset()                                                        # the lanes' episode number is now ep + 1
        layers = _layers(rng, 4 + W + 6, widths, 6)
        head = _head(rng, widths, 4 + W + 6)
        ctl = A.PolicyController(A.EnvPlayer(env), layers, window=W, explore=explore, seed=int(rng.integers(1 << 62)),
                                 sample="softmax", temperature=temp, value_head=head)
        seen, distinct = set(), 0
        for s in range(0, V + 2, 3):
            a, v = _check_select(env, ctl, layers, head, br, ep + 1, (W, widths, s))
            seen.update(np.unique(a).tolist())
            distinct = max(distinct, len(np.unique(v)))
            env.step_random(3, seed=int(rng.integers(1 << 62)), want_actions=False)
        assert -1 in seen and len(seen) >= 3, seen
        assert distinct > N // 2 or widths != [64, 64], distinct             # a value worth comparing
    env.close()


@pytest.mark.parametrize("N", (1, 255, 256, 257, 1000))
def test_value_at_the_workgroup_edge(N):
    import abrsimulator_amd as A
    rng = np.random.default_rng(82)
    V = 8
    env = _env(A, V, N, rng)
    layers = _layers(rng, 4 + 8 + 6, [64, 64], 6)
    head = _head(rng, [64, 64], 18)
    ctl = A.PolicyController(A.EnvPlayer(env), layers, window=8, seed=3, sample="softmax", value_head=head)
    br = np.tile(LADDER, (V, 1))
    guard = torch.full((N + 64,), 123.0, device=env.device)                # a value vector with a guard behind it
    for s in range(3):
        _check_select(env, ctl, layers, head, br, 0, (N, s))
        pol, smp, val = ctl.bound(env), ctl.sampling(), ctl.value()
        act = torch.empty(N, dtype=torch.int32, device=env.device)
        env._call(env.lib.abr_env_policy_select_ac, env._h, C.byref(pol), C.byref(smp), C.byref(val), A._lib.ptr(act), None,
                  None, None, A._lib.ptr(guard))
        assert (guard[N:] == 123.0).all()
        env.step_random(3, seed=s, want_actions=False)
    env.close()


FUSED = (("softmax", 0.2, True), ("softmax", 0.0, True), ("argmax", 0.2, False), ("argmax", 0.0, True))   # .., want_probs


@pytest.fixture(scope="module")
def rollouts():
    """The fused test's rollouts with values (softmax with exploration), kept for the GAE test: {impl: numpy slabs}."""
    return {}


def _rollout(A, impl, auto_reset, sample, explore, n, want_values, layers, head, V=10, N=1000, want_probs=True, start=None):
    """start: a state_dict to begin from -- the same bytes also in the regions of the workspace that no kernel of the
    rollout writes (the workspace is allocated uninitialised)."""
    env = _env(A, V, N, np.random.default_rng(5), impl=impl, auto_reset=auto_reset)
    if start is not None:
        env.load_state_dict(start)
    ctl = A.PolicyController(A.EnvPlayer(env), layers, window=4, explore=explore, seed=99, sample=sample, temperature=0.8,
                             value_head=head)
    out = env.step_policy(ctl, n, want_features=True, want_scores=True, want_probs=want_probs, want_values=want_values)
    return env, ctl, out


@pytest.mark.parametrize("impl", ("auto", "jump", "split", "split3"))
def test_fused_values_equal_select_plus_step(impl, rollouts):
    import abrsimulator_amd as A
    rng = np.random.default_rng(83)
    V, N, n = 10, 1000, 23
    layers = _layers(rng, 4 + 4 + 6, [32], 6)
    head = _head(rng, [32], 14)
    for sample, explore, probs in FUSED:
        start = _env(A, V, N, np.random.default_rng(5), impl=impl, auto_reset=True)
        ref_env, ref_ctl, ref = _rollout(A, impl, True, sample, explore, n, False, layers, head, want_probs=probs,
                                         start=start.state_dict())
        env, ctl, fused = _rollout(A, impl, True, sample, explore, n, True, layers, head, want_probs=probs,
                                   start=start.state_dict())
        start.close()
        assert ref_ctl.uses_sampled_entries(probs) == (sample == "softmax" or probs)
        assert fused["values"].shape == (n, N) and fused["last_value"].shape == (N,)
        assert "values" not in ref
        for k in ("obs", "reward", "done", "actions", "features", "scores", "probs"):
            if k == "probs" and not probs:
                assert fused[k] is None and ref[k] is None
                continue
            assert torch.equal(fused[k], ref[k]), (impl, sample, explore, k)
        assert torch.equal(env.workspace, ref_env.workspace), (impl, sample, explore)
        after = ctl.select(want_value=True)["value"]
        assert torch.equal(fused["last_value"], after), (impl, sample, explore)
        step_env = _env(A, V, N, np.random.default_rng(5), impl=impl, auto_reset=True)
        step_ctl = A.PolicyController(A.EnvPlayer(step_env), layers, window=4, explore=explore, seed=99, sample=sample,
                                      temperature=0.8, value_head=head)
        for s in range(n):
            sel = step_ctl.select(want_probs=True, want_value=True)
            step_env.step(sel["actions"])
            assert torch.equal(fused["values"][s], sel["value"]), (impl, sample, explore, s)
            assert torch.equal(fused["actions"][s], sel["actions"]), (impl, sample, explore, s)
        assert (fused["done"] != 0).sum(0).min() >= 2                      # two episode ends per lane
        assert len(torch.unique(fused["values"])) > N
        if sample == "softmax" and explore:
            rollouts[impl] = {k: v.cpu().numpy() for k, v in fused.items() if v is not None}
        for e in (env, ref_env, step_env):
            e.close()


def _device_gae(A, dev="cuda"):
    def fn(reward, values, last, done, actions, gamma, lam):
        t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        adv, ret = A.gae(t(reward), t(values), t(last), t(done), t(actions), gamma, lam)
        return adv.cpu().numpy(), ret.cpu().numpy()
    return fn


def test_gae_on_the_rollouts_own_slabs(rollouts):
    import abrsimulator_amd as A
    rng = np.random.default_rng(84)
    layers = _layers(rng, 4 + 4 + 6, [32], 6)
    head = _head(rng, [32], 14)
    gae = _device_gae(A)
    cases = []
    if "auto" in rollouts:                                                 # the fused test's rollout, when it ran first
        cases.append(("auto_reset/shared", rollouts["auto"]))
    env, ctl, out = _rollout(A, "auto", True, "softmax", 0.2, 23, True, layers, head)
    cases.append(("auto_reset", {k: v.cpu().numpy() for k, v in out.items() if v is not None}))
    env.close()
    env, ctl, out = _rollout(A, "auto", False, "softmax", 0.2, 23, True, layers, head)
    cases.append(("dead tails", {k: v.cpu().numpy() for k, v in out.items() if v is not None}))
    env.close()
    for tag, o in cases:
        if tag == "dead tails":
            assert (o["actions"][11:] == -1).all() and (o["values"][11:] == 0).all() and (o["last_value"] == 0).all()
        else:
            assert ((o["done"] != 0).sum(0) >= 2).all() and (o["actions"] >= 0).all()
        for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0)):
            want = AC.gae(o["reward"], o["values"], o["last_value"], o["done"], o["actions"], gamma, lam)
            got = gae(o["reward"], o["values"], o["last_value"], o["done"], o["actions"], gamma, lam)
            assert _bits_eq(got[0], want[0]) and _bits_eq(got[1], want[1]), (tag, gamma, lam)
            assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 0
        s = dict(reward=o["reward"], values=o["values"], last_value=o["last_value"], done=o["done"], actions=o["actions"])
        check_returns_are_episode_sums(gae, s)
        check_lambda_zero_is_the_td_error(gae, s)


@pytest.mark.parametrize("N", (1, 63, 64, 65, 1000))
def test_gae_on_the_edge_slabs(N):
    import abrsimulator_amd as A
    gae = _device_gae(A)
    for T_ in (1, 2, 5, 48):
        s = AC.edge_slabs(T_, N, seed=600 + T_)
        for gamma, lam in ((0.99, 0.95), (0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)):
            want = AC.gae(s["reward"], s["values"], s["last_value"], s["done"], s["actions"], gamma, lam)
            got = gae(s["reward"], s["values"], s["last_value"], s["done"], s["actions"], gamma, lam)
            assert _bits_eq(got[0], want[0]) and _bits_eq(got[1], want[1]), (T_, N, gamma, lam)
            ok = ~s["poison"]
            assert np.isfinite(got[0][ok]).all() and np.isfinite(got[1][ok]).all()
        fin = {k: (np.where(np.isfinite(v), v, f32(1.5)).astype(np.float32) if v.dtype == np.float32 else v)
               for k, v in s.items()}
        want = AC.gae(fin["reward"], fin["values"], fin["last_value"], fin["done"], None, 0.99, 0.95)
        got = gae(fin["reward"], fin["values"], fin["last_value"], fin["done"], None, 0.99, 0.95)
        assert _bits_eq(got[0], want[0]) and _bits_eq(got[1], want[1]), (T_, N)
        if N >= 12:
            check_returns_are_episode_sums(gae, s)
            check_lambda_zero_is_the_td_error(gae, s)
    # out= is filled in place, with a guard row behind it left alone; bool done bytes are taken as they are
    s = AC.edge_slabs(5, N, seed=9)
    t = lambda x: torch.from_numpy(x).cuda()
    buf = torch.full((2, 6, N), 55.0, device="cuda")
    adv, ret = A.gae(t(s["reward"]), t(s["values"]), t(s["last_value"]), t(s["done"]) != 0, t(s["actions"]),
                     out=(buf[0, :5], buf[1, :5]))
    want = AC.gae(s["reward"], s["values"], s["last_value"], s["done"], s["actions"], 0.99, 0.95)
    assert adv.data_ptr() == buf.data_ptr() and (buf[:, 5] == 55.0).all()
    assert _bits_eq(adv.cpu().numpy(), want[0]) and _bits_eq(ret.cpu().numpy(), want[1])


def test_values_need_a_head_and_the_heads_size_is_checked():
    import abrsimulator_amd as A
    from abrsimulator_amd import _lib
    rng = np.random.default_rng(85)
    V, N = 6, 300
    env = _env(A, V, N, rng)
    layers = _layers(rng, 4 + 3 + 6, [8], 6)
    plain = A.PolicyController(A.EnvPlayer(env), layers, window=3)
    with pytest.raises(ValueError):
        env.step_policy(plain, 2, want_values=True)
    with pytest.raises(ValueError):
        plain.select(want_value=True)
    out = env.step_policy(plain, 2)                                        # nothing was launched by the refused calls
    assert "values" not in out and (out["actions"] >= 0).all()
    ctl = A.PolicyController(A.EnvPlayer(env), layers, window=3, value_head=_head(rng, [8], 13))
    pol, smp, val = ctl.bound(env), ctl.sampling(), ctl.value()
    act = torch.empty(N, dtype=torch.int32, device=env.device)
    for nbytes in (val.head_bytes - 4, val.head_bytes + 4, 0):
        bad = ctl.value()
        bad.head_bytes = nbytes
        rc = env.lib.abr_env_policy_select_ac(env._h, C.byref(pol), C.byref(smp), C.byref(bad), _lib.ptr(act), None, None,
                                              None, None, None)
        assert rc == -1 and b"head_bytes" in env.lib.abr_last_error()
        rc = env.lib.abr_env_step_policy_ac(env._h, C.byref(pol), C.byref(smp), C.byref(bad), 1, None, None, None, None,
                                            None, None, None, None, None, None)
        assert rc == -1 and b"head_bytes" in env.lib.abr_last_error()
    # past the end of the episode: values 0, and a rollout on 'tick' is refused as step_policy is
    out = env.step_policy(ctl, V + 2, want_values=True)
    assert (out["values"][V - 2:] == 0).all() and (out["last_value"] == 0).all()
    assert (out["values"][V - 2:].view(torch.int32) == 0).all()
    env.close()
    tick = _env(A, V, N, np.random.default_rng(2), impl="tick")
    ctl = A.PolicyController(A.EnvPlayer(tick), layers, window=3, value_head=_head(rng, [8], 13))
    with pytest.raises(_lib.AbrError, match=r"-4"):
        tick.step_policy(ctl, 2, want_values=True)
    assert (ctl.select(want_value=True)["actions"] >= 0).all()             # select runs on every impl
    tick.close()
