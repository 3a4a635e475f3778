"""Policy populations on the device (include/abr_env.h: abr_policy_pop; abr_env.hip: the POP instances of
policy_select_kernel and policy_mx_kernel).  The yardstick everywhere is the existing single-network path: for every
member m, what the population gives on lanes_of(m) is bit for bit (any NaN equal to any NaN) what member m's weights give
there through PolicyController on an identically built environment -- in select on rollout states, in fused rollouts on
every event-driven kernel, at P = 1, across the two engines, after load_member, and in the ledger's per-member read-out.
One member's blob and head hold NaN, infinities, -0 and subnormals: nothing of it may show in a neighbour's lanes."""
import math

import numpy as np
import pytest
import torch

from test_actor_critic_gpu import _head
from test_policy_cpu import _layers as _special_layers
from test_policy_gpu import _env, _layers
from test_policy_sample_gpu import _bits_eq

pytestmark = pytest.mark.gpu

f32 = np.float32
V, W, M = 8, 8, 6
F = 4 + W + M
PAIRS = ((256, 256), (257, 256), (700, 256), (1024, 256), (1000, 512))     # (n_lanes, group)
LANE_SHAPES = ([], [5], [64, 64])
MX_SHAPES = ([33], [128, 128], [128, 128, 128])
MODES = (("argmax", 0.0, False, False), ("softmax", 0.3, True, True), ("argmax", 0.3, True, False),
         ("softmax", 0.0, False, True))                                     # sample, explore, probs, value
ALL = dict(want_features=True, want_scores=True, want_probs=True, want_values=True)


def _eq(a, b):
    """Bit for bit, any NaN equal to any NaN, compared on the device."""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return bool(((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) |
                     (torch.isnan(a) & torch.isnan(b))).all())
    if a.dtype == torch.float64:
        return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
    return torch.equal(a, b)


def _same_on(sl, got, ref, tag):
    """Two select() / step_policy() dicts on a slice of lanes (the last axis of every entry)."""
    assert got.keys() == ref.keys(), tag
    for k in got:
        a, b = got[k], ref[k]
        assert _eq(None if a is None else a[..., sl], None if b is None else b[..., sl]), (tag, k)


def _members(rng, hidden, P):
    """P independently drawn members and heads; member 1 (where there is one) holds every kind of special value."""
    hidden = list(hidden)
    layers = [_layers(rng, F, hidden, M) for _ in range(P)]
    heads = [_head(rng, hidden, F) for _ in range(P)]
    if P >= 2:
        sp = _special_layers(rng, F, hidden, M, True)
        sp[0][0][0, :5] = [np.nan, np.inf, -np.inf, -0.0, 1e-41]
        sp[-1][1][0] = f32(1e-41)
        hv = heads[1][0].copy()
        hv[:4] = [-0.0, 1e-41, np.inf, np.nan]
        layers[1], heads[1] = sp, (hv, f32(-0.0))
    return layers, heads


def _pop(A, env, hidden, group, rng, engine, **kw):
    P = -(-env.n_lanes // group)
    layers, heads = _members(rng, hidden, P)
    kw = dict(dict(window=W, temperature=0.8, seed=int(rng.integers(1 << 62))), **kw)
    return A.PolicyPopulation(A.EnvPlayer(env), layers, group, value_heads=heads, engine=engine, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. select on rollout states

@pytest.mark.parametrize("N,group", PAIRS)
def test_select_equals_each_member_on_its_lanes(N, group):
    import abrsimulator_amd as A
    rng = np.random.default_rng(1000 + N)
    env = _env(A, V, N, rng, auto_reset=True)
    env.step_random(3, seed=5, want_actions=False)
    for engine, shapes in (("lane", LANE_SHAPES), ("matrix", MX_SHAPES)):
        for hidden in shapes:
            pop = _pop(A, env, hidden, group, rng, engine)
            P = pop.n_members
            assert pop.member_of_lane().tolist() == [i // group for i in range(N)]
            for sample, explore, probs, value in MODES:
                pop.sample, pop.explore = sample, explore
                got = pop.select(want_probs=probs, want_value=value)
                refs = [pop.member(m).select(want_probs=probs, want_value=value) for m in range(P)]
                for m in range(P):
                    _same_on(pop.lanes_of(m), got, refs[m], (engine, hidden, sample, explore, m))
                if P >= 2:                                                  # members that differ: the comparison says something
                    assert not _eq(refs[0]["scores"], refs[1]["scores"]), (engine, hidden)
                    assert not _eq(refs[0]["scores"], refs[P - 1]["scores"]), (engine, hidden)
                    sc = got["scores"][:, pop.lanes_of(0)]
                    assert torch.isfinite(sc).all() and len(torch.unique(sc)) > group   # and nothing leaked from member 1
        env.step_random(2, seed=7, want_actions=False)                      # other states for the other engine
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. fused rollouts

def _start(A, impl, N, n_envs):
    """Environments that start from the same bytes (the workspace is allocated uninitialised), with the same sampler and
    the same step_random warm-up."""
    first = _env(A, V, N, np.random.default_rng(5), impl=impl, auto_reset=True)
    sd = first.state_dict()
    first.close()
    envs = [_env(A, V, N, np.random.default_rng(5), impl=impl, auto_reset=True) for _ in range(n_envs)]
    for e in envs:
        e.load_state_dict(sd)
        e.set_episode_sampler(4242, offset_span=100)
        e.step_random(2, seed=3, want_actions=False)
    return envs


def _rollout_case(A, impl, N, group, engine, hidden, sample, explore, want, n=12):
    rng = np.random.default_rng(2000 + N + len(hidden))
    P = -(-N // group)
    envs = _start(A, impl, N, 1 + P)
    pop = _pop(A, envs[0], hidden, group, rng, engine, sample=sample, explore=explore)
    got = envs[0].step_policy(pop, n, **want)
    assert (got["done"] != 0).any()                                         # the launch crossed an episode end
    state, eps = envs[0].observe_f64(), envs[0].episodes()
    for m in range(P):
        ref_env, sl = envs[1 + m], pop.lanes_of(m)
        tag = (impl, N, group, engine, hidden, sample, m)
        ref = ref_env.step_policy(pop.member(m), n, **want)
        _same_on(sl, got, ref, tag)
        if want.get("want_values"):
            assert got["last_value"].shape == (N,) and got["values"].shape == (n, N)
        for k, v in ref_env.observe_f64().items():
            assert _eq(state[k][sl], v[sl]), (tag, k)
        for k, v in ref_env.episodes().items():
            assert torch.equal(eps[k][sl], v[sl]), (tag, k)
    for e in envs:
        e.close()


@pytest.mark.parametrize("impl", ("auto", "jump", "split", "split3"))
@pytest.mark.parametrize("pair", range(len(PAIRS)), ids=lambda k: "%dx%d" % PAIRS[k])
def test_fused_rollout_equals_each_member_on_its_lanes(impl, pair):
    import abrsimulator_amd as A
    N, group = PAIRS[pair]
    k = (pair + ("auto", "jump", "split", "split3").index(impl)) % 3          # every shape on every kernel and pair over the grid
    # softmax with exploration and every slab; then the first argmax without probs and values (the other instances)
    _rollout_case(A, impl, N, group, "lane", LANE_SHAPES[k], "softmax", 0.2, ALL)
    _rollout_case(A, impl, N, group, "matrix", MX_SHAPES[k], "softmax", 0.2, ALL)
    engine, shapes = (("lane", LANE_SHAPES), ("matrix", MX_SHAPES))[pair % 2]
    _rollout_case(A, impl, N, group, engine, shapes[(k + 1) % 3], "argmax", 0.3, dict(want_scores=True))


def test_tick_refuses_the_rollouts():
    import abrsimulator_amd as A
    from abrsimulator_amd import _lib
    rng = np.random.default_rng(7)
    tick = _env(A, V, 300, np.random.default_rng(2), impl="tick")
    for engine, hidden in (("lane", [5]), ("matrix", [33])):
        pop = _pop(A, tick, hidden, 256, rng, engine)
        for kw in (dict(), dict(want_values=True), dict(want_probs=True)):
            with pytest.raises(_lib.AbrError, match=r"-4"):
                tick.step_policy(pop, 2, **kw)
        got = pop.select(want_value=True)                                   # select runs on every impl
        for m in range(2):
            _same_on(pop.lanes_of(m), got, pop.member(m).select(want_value=True), (engine, m))
    tick.close()


def test_sizes_are_checked_after_the_handle():
    import ctypes as C

    import abrsimulator_amd as A
    from abrsimulator_amd import _lib
    rng = np.random.default_rng(8)
    env = _env(A, V, 700, np.random.default_rng(2))
    act = torch.empty(700, dtype=torch.int32, device=env.device)
    for engine, hidden, sel in (("lane", [5], env.lib.abr_env_policy_select_pop),
                                ("matrix", [33], env.lib.abr_env_policy_select_mx_pop)):
        pop = _pop(A, env, hidden, 256, rng, engine)
        call = lambda pol, pp, val: sel(env._h, C.byref(pol), C.byref(pp), None, C.byref(val) if val is not None else None,
                                        _lib.ptr(act), None, None, None, None, None)
        pol, pp, val = pop.bound(env), pop.population(), pop.value()
        assert call(pol, pp, val) == 0
        pol.weights_bytes *= 3                                              # the whole blob's size is not one member's
        assert call(pol, pp, val) == -1 and b"weights_bytes" in env.lib.abr_last_error()
        pol = pop.bound(env)
        val.head_bytes *= 3
        assert call(pol, pp, val) == -1 and b"head_bytes" in env.lib.abr_last_error()
        for P, group in ((2, 256), (4, 256), (3, 512), (2, 1024)):
            pp.n_members, pp.group = P, group
            assert call(pol, pp, None) == -1 and b"n_members" in env.lib.abr_last_error(), (P, group)
        pp.n_members, pp.group = 2, 512                                     # another cover of the same lanes is accepted
        assert call(pol, pp, None) == 0
    torch.cuda.synchronize()
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. P = 1 is the plain controller, workspace included

@pytest.mark.parametrize("engine,hidden", (("lane", [64, 64]), ("matrix", [128, 128])))
@pytest.mark.parametrize("N", (200, 256))
def test_one_member_is_the_plain_controller_byte_for_byte(engine, hidden, N):
    import abrsimulator_amd as A
    rng = np.random.default_rng(31)
    layers, head = _layers(rng, F, list(hidden), M), _head(rng, list(hidden), F)
    for sample, explore, want in (("softmax", 0.2, ALL), ("argmax", 0.0, dict(want_scores=True))):
        envs = _start(A, "auto", N, 2)
        kw = dict(window=W, engine=engine, sample=sample, explore=explore, temperature=0.7, seed=99)
        pop = A.PolicyPopulation(A.EnvPlayer(envs[0]), [layers], 256, value_heads=[head], **kw)
        ctl = A.PolicyController(A.EnvPlayer(envs[1]), layers, value_head=head, **kw)
        assert pop.n_members == 1 and torch.equal(pop.weights[0], ctl.weights)
        a, b = envs[0].step_policy(pop, 12, **want), envs[1].step_policy(ctl, 12, **want)
        _same_on(slice(None), a, b, (engine, N, sample))
        assert torch.equal(envs[0].workspace, envs[1].workspace), (engine, N, sample)
        assert (a["done"] != 0).any()
        for e in envs:
            e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the engines agree

@pytest.mark.parametrize("N,group", ((700, 256), (1000, 512)))
def test_matrix_population_equals_lane_population(N, group):
    import abrsimulator_amd as A
    P = -(-N // group)
    layers, heads = _members(np.random.default_rng(41), [64, 64], P)
    envs = _start(A, "auto", N, 2)
    pops = [A.PolicyPopulation(A.EnvPlayer(e), layers, group, value_heads=heads, window=W, engine=eng, sample="softmax",
                               explore=0.2, temperature=0.9, seed=5) for e, eng in zip(envs, ("lane", "matrix"))]
    assert torch.equal(pops[0].weights.view(torch.int32), pops[1].weights.view(torch.int32))
    _same_on(slice(None), pops[0].select(want_probs=True, want_value=True),
             pops[1].select(want_probs=True, want_value=True), "select")
    outs = [e.step_policy(p, 12, **ALL) for e, p in zip(envs, pops)]
    _same_on(slice(None), outs[0], outs[1], "rollout")
    assert torch.equal(envs[0].workspace, envs[1].workspace)
    for e in envs:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. load_member between launches

@pytest.mark.parametrize("engine,hidden", (("lane", [64, 64]), ("matrix", [128, 128])))
def test_load_member_changes_exactly_that_members_lanes(engine, hidden):
    import abrsimulator_amd as A
    rng = np.random.default_rng(51)
    N, group = 1000, 256
    env = _env(A, V, N, rng, auto_reset=True)
    env.step_random(3, seed=1, want_actions=False)
    layers = [_layers(rng, F, list(hidden), M) for _ in range(4)]
    heads = [_head(rng, list(hidden), F) for _ in range(4)]
    pop = A.PolicyPopulation(A.EnvPlayer(env), layers, group, value_heads=heads, window=W, engine=engine)
    first = pop.select(want_value=True)
    pop.load_member(2, _layers(rng, F, list(hidden), M), value_head=_head(rng, list(hidden), F))   # in place, on the stream
    second = pop.select(want_value=True)
    for m in range(4):
        sl = pop.lanes_of(m)
        _same_on(sl, second, pop.member(m).select(want_value=True), (engine, m))
        if m == 2:
            assert not _eq(first["scores"][:, sl], second["scores"][:, sl])
            assert not _eq(first["value"][sl], second["value"][sl])
        else:
            _same_on(sl, first, second, (engine, m, "untouched"))
    out = env.step_policy(pop, 3, want_scores=True)                         # and the next rollout sees the new member
    assert out["scores"].shape == (3, M, N)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the read-out an evolution strategy ranks its members by

def test_ledger_per_member_after_a_population_rollout():
    import abrsimulator_amd as A
    from abrsimulator_amd.ledger import FLOAT_FIELDS
    rng = np.random.default_rng(61)
    N, group = 700, 256
    env = _env(A, V, N, rng, auto_reset=True)
    env.set_episode_sampler(77, offset_span=100)
    led = env.set_episode_ledger(8)
    pop = _pop(A, env, [64, 64], group, rng, "lane", sample="softmax", explore=0.1)
    P = pop.n_members
    env.step_policy(pop, 24, want_obs=False, want_actions=False)
    pm = led.per_member(group, P)
    cnt = led.count().cpu().numpy().astype(np.int64)
    assert cnt.min() >= 3 and cnt.max() <= 8                                # nothing has left the ring: records() has all
    assert pm["count"].tolist() == [int(cnt[pop.lanes_of(m)].sum()) for m in range(P)]
    rec = {k: v.cpu().numpy() for k, v in led.records().items()}
    u = 2.0 ** -53
    for k in FLOAT_FIELDS:
        for m in range(P):
            sl = pop.lanes_of(m)
            x = rec[k][(rec["lane"] >= sl.start) & (rec["lane"] < sl.stop)].astype(np.float64)
            c = x.size
            assert c == int(pm["count"][m])
            # a float64 sum of c terms in any order, the mean's division and the multiplication that undoes it
            bound = c * u * math.fsum(np.abs(x)) / (1 - c * u)
            exact = math.fsum(x)
            got = float(pm[k][m])
            assert abs(got * c - exact) <= bound + 2 * u * abs(exact), (k, m)
            # numpy's own mean is such a sum as well: the two may differ by both errors
            assert abs(got - float(np.mean(x))) * c <= 2 * (bound + 2 * u * abs(exact)), (k, m)
    env.close()
