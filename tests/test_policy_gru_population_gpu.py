"""Recurrent policy populations on the device (include/abr_env.h: abr_env_gru_select_pop and its three siblings;
abr_env.hip: the POP instances of policy_gru_kernel and policy_gru_mx_kernel).  The yardstick everywhere is the
single-network path: for every member m, what the population gives on lanes_of(m) -- every output, and the committed
columns of the one state slab -- is bit for bit (any NaN equal to any NaN) what a RecurrentPolicyController over member
m's blob and head gives there on an identically built environment.  One member's blob and head are full of NaN,
infinities, -0 and subnormals, so a workgroup that picks the wrong blob cannot pass.

Small on purpose: golden traces, video_length 5 so that a 12-decision rollout crosses two episode ends on every lane, at
most 1 000 lanes.  The shapes are the smallest at which the mapping can go wrong: one member; a second member that owns a
single lane; a ragged last member; a group that spans two workgroups with a ragged tail."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import golden_workload, make_env
from test_policy_gru_gpu import LADDERS, _weights
from test_policy_population_gpu import _eq, _same_on

pytestmark = pytest.mark.gpu

f32 = np.float32
V, STEPS = 5, 12
PAIRS = ((256, 256), (257, 256), (700, 256), (1000, 512))                  # (n_lanes, group)
LANE_H, MX_H = (1, 7, 33, 64), (32, 65, 128)
SHAPES = [("lane", H) for H in LANE_H] + [("matrix", H) for H in MX_H]
IMPLS = ("auto", "jump", "split", "split3")
ALL = dict(want_features=True, want_scores=True, want_probs=True, want_values=True, want_hidden=True)
POOL = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-41, -3e-42, 6e-39, -np.nan], f32)


def _env(N, M=6, seed=7, **kw):
    m, traces, tid, off = golden_workload(N, seed=seed)
    env = make_env(dict(m, video_length=V, ladder=LADDERS[M]), traces, N, **kw)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    return env


def _envs(n, N, sampler=False, **kw):
    """n environments that start from the same bytes (the workspace is allocated uninitialised)."""
    first = _env(N, **kw)
    sd = first.state_dict()
    first.close()
    envs = [_env(N, **kw) for _ in range(n)]
    for e in envs:
        e.load_state_dict(sd)
        if sampler:
            e.set_episode_sampler(4242, offset_span=100)
    return envs


def _members(rng, H, P, W=8, M=6):
    """P independently drawn (cell, head, value head); one of them -- member 1, or member 0 of two, so that the last
    member's few lanes are still compared on finite numbers -- holds nothing but special values."""
    mem = [_weights(rng, 4 + W + M, H, M) for _ in range(P)]
    if P >= 2:
        k = 1 if P >= 3 else 0
        cell, head, vh = mem[k]
        draw = lambda t: rng.choice(POOL, np.shape(t)).astype(f32)
        mem[k] = (tuple(draw(t) for t in cell), tuple(draw(t) for t in head), (draw(vh[0]), f32(-0.0)))
    return mem


def _build(envs, H, group, engine, rng, W=8, M=6, **kw):
    """The population on envs[0] and member m's plain controller on envs[1 + m], from the same weights."""
    import abrsimulator_amd as A
    N = envs[0].n_lanes
    P = -(-N // group)
    mem = _members(rng, H, P, W, M)
    kw = dict(dict(window=W, engine=engine, explore=0.2, seed=11, temperature=0.8), **kw)
    pop = A.RecurrentPolicyPopulation(A.EnvPlayer(envs[0]), [(c, h) for c, h, _ in mem], group,
                                      value_heads=[v for _, _, v in mem], **kw)
    refs = [A.RecurrentPolicyController(A.EnvPlayer(envs[1 + m]), mem[m][0], mem[m][1], value_head=mem[m][2], **kw)
            for m in range(P)]
    assert pop.n_members == P == len(refs) and pop.hidden.shape == (H, N)
    for m in range(P):
        assert _eq(pop.weights[m], refs[m].weights) and _eq(pop.value_heads[m], refs[m].value_head)
    return pop, refs


def _close(envs):
    for e in envs:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. select in four modes, after 0 and 3 committed steps

def _select_case(N, group, engine, H, W=8, M=6):
    P = -(-N // group)
    envs = _envs(1 + P, N, M=M)
    pop, refs = _build(envs, H, group, engine, np.random.default_rng(1000 + N + H), W, M)
    kw = dict(want_probs=True, want_value=True, want_hidden=True)
    done_steps = cells = 0
    for prefix in (0, 3):
        while done_steps < prefix:                                          # commit=True, then the step of those actions
            got = pop.select(commit=True, **kw)
            envs[0].step(got["actions"])
            for m in range(P):
                ref, sl = refs[m].select(commit=True, **kw), pop.lanes_of(m)
                _same_on(sl, got, ref, (engine, H, "prefix", done_steps, m))
                assert _eq(pop.hidden[:, sl], refs[m].hidden[:, sl]), (engine, H, "committed slab", done_steps, m)
                envs[1 + m].step(ref["actions"])
            done_steps += 1
        for sample in ("argmax", "softmax"):
            for value in (False, True):
                pop.sample = sample
                before = pop.hidden.clone()
                got = pop.select(want_probs=sample == "softmax", want_value=value, want_hidden=True)
                assert torch.equal(before.view(torch.int32), pop.hidden.view(torch.int32))       # commit=False
                for m in range(P):
                    refs[m].sample = sample
                    ref = refs[m].select(want_probs=sample == "softmax", want_value=value, want_hidden=True)
                    _same_on(pop.lanes_of(m), got, ref, (engine, H, prefix, sample, value, m))
                cells += N
                if prefix:
                    assert float(torch.nan_to_num(got["hidden"]).abs().max()) > 0
                else:
                    assert not got["hidden"].view(torch.int32).any()       # c == 0: +0.0f in every unit
                if P >= 2:                                                  # the poisoned member shows on its own lanes only
                    bad, fine = (1, 0) if P >= 3 else (0, 1)
                    assert not torch.isfinite(got["scores"][:, pop.lanes_of(bad)]).any()
                    assert torch.isfinite(got["scores"][:, pop.lanes_of(fine)]).all()
                    assert torch.isfinite(got["scores"][:, pop.lanes_of(P - 1)]).all() or P - 1 == bad
    assert cells == 8 * N
    _close(envs)


@pytest.mark.parametrize("N,group", PAIRS)
@pytest.mark.parametrize("engine,H", SHAPES)
def test_select_equals_each_member_on_its_lanes(N, group, engine, H):
    _select_case(N, group, engine, H)


@pytest.mark.parametrize("engine,H", (("lane", 7), ("matrix", 65)))
def test_select_without_a_window_and_with_one_rate(engine, H):
    _select_case(700, 256, engine, H, W=0, M=1)


# ---------------------------------------------------------------------------------------------------------------------
# 2. fused rollouts across two episode ends

def _rollout_case(impl, N, group, engine, H, sample, want):
    P = -(-N // group)
    envs = _envs(1 + P, N, sampler=True, impl=impl, auto_reset=True)
    pop, refs = _build(envs, H, group, engine, np.random.default_rng(2000 + N + H), sample=sample)
    got = envs[0].step_policy(pop, STEPS, **want)
    assert int((got["done"] != 0).sum(0).min()) >= 2                        # every lane crossed two episode ends
    assert got["hidden"].shape == (STEPS, H, N)
    state, eps = envs[0].observe_f64(), envs[0].episodes()
    for m in range(P):
        sl, tag = pop.lanes_of(m), (impl, N, group, engine, H, sample, m)
        ref = envs[1 + m].step_policy(refs[m], STEPS, **want)
        _same_on(sl, got, ref, tag)
        if want.get("want_values"):
            assert got["last_value"].shape == (N,) and got["values"].shape == (STEPS, N)
        for k, v in envs[1 + m].observe_f64().items():
            assert _eq(state[k][sl], v[sl]), (tag, k)
        for k, v in envs[1 + m].episodes().items():
            assert torch.equal(eps[k][sl], v[sl]), (tag, k)
        assert _eq(pop.hidden[:, sl], refs[m].hidden[:, sl]), (tag, "final state slab")
    _close(envs)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("pair", range(len(PAIRS)), ids=lambda k: "%dx%d" % PAIRS[k])
def test_fused_rollout_equals_each_member_on_its_lanes(impl, pair):
    N, group = PAIRS[pair]
    k = pair + IMPLS.index(impl)                                            # every hidden size on every kernel and pair over the grid
    # softmax with exploration and every slab; then the first argmax without probs and values (the other instances)
    _rollout_case(impl, N, group, "lane", LANE_H[k % 4], "softmax", ALL)
    _rollout_case(impl, N, group, "matrix", MX_H[k % 3], "softmax", ALL)
    engine, hs = (("lane", LANE_H), ("matrix", MX_H))[pair % 2]
    _rollout_case(impl, N, group, engine, hs[(k + 1) % len(hs)], "argmax", dict(want_scores=True, want_hidden=True))


def test_tick_refuses_the_rollouts_and_runs_the_select():
    from abrsimulator_amd import _lib
    envs = [_env(300, impl="tick") for _ in range(3)]
    for engine, H in (("lane", 7), ("matrix", 65)):
        pop, refs = _build(envs, H, 256, engine, np.random.default_rng(7))
        for kw in (dict(), dict(want_values=True), dict(want_probs=True, want_hidden=True)):
            with pytest.raises(_lib.AbrError, match=r"-4"):
                envs[0].step_policy(pop, 2, **kw)
        got = pop.select(want_value=True, want_hidden=True)                 # select runs on every impl
        for m in range(2):
            _same_on(pop.lanes_of(m), got, refs[m].select(want_value=True, want_hidden=True), (engine, m))
    _close(envs)


def test_sizes_are_checked_after_the_handle():
    from abrsimulator_amd import _lib
    envs = [_env(700) for _ in range(4)]
    env = envs[0]
    act = torch.empty(700, dtype=torch.int32, device=env.device)
    for engine, H, sel in (("lane", 7, env.lib.abr_env_gru_select_pop),
                           ("matrix", 65, env.lib.abr_env_gru_mx_select_pop)):
        pop, _ = _build(envs, H, 256, engine, np.random.default_rng(8))
        err = env.lib.abr_last_error
        call = lambda pol, pp, val: sel(env._h, C.byref(pol), C.byref(pp), None, C.byref(val) if val is not None else None,
                                        0, _lib.ptr(act), None, None, None, None, None, None)
        pol, pp, val = pop.bound(env), pop.population(), pop.value()
        assert call(pol, pp, val) == 0
        pol.weights_bytes *= 3                                              # the whole blob's size is not one member's
        pol.state_bytes += 4
        val.head_bytes *= 3
        pp.n_members = 2
        assert call(pol, pp, val) == -1 and b"weights_bytes" in err()       # in this order
        pol.weights_bytes //= 3
        assert call(pol, pp, val) == -1 and b"state_bytes" in err()
        pol.state_bytes -= 4
        assert call(pol, pp, val) == -1 and b"head_bytes" in err()
        val.head_bytes //= 3
        for P, group in ((2, 256), (4, 256), (3, 512), (2, 1024)):
            pp.n_members, pp.group = P, group
            assert call(pol, pp, val) == -1 and b"n_members" in err(), (P, group)
        pp.n_members, pp.group = 2, 512                                     # another cover of the same lanes is accepted
        assert call(pol, pp, None) == 0
    torch.cuda.synchronize()
    _close(envs)


# ---------------------------------------------------------------------------------------------------------------------
# 3. P = 1 is the plain controller, workspace and state slab included

@pytest.mark.parametrize("engine,H", (("lane", 64), ("matrix", 128)))
@pytest.mark.parametrize("N", (200, 256))
def test_one_member_is_the_plain_controller_byte_for_byte(engine, H, N):
    for sample, want in (("softmax", ALL), ("argmax", dict(want_scores=True, want_hidden=True))):
        envs = _envs(2, N, sampler=True, auto_reset=True)
        pop, (ctl,) = _build(envs, H, 256, engine, np.random.default_rng(31), sample=sample)
        assert pop.n_members == 1
        a, b = envs[0].step_policy(pop, STEPS, **want), envs[1].step_policy(ctl, STEPS, **want)
        _same_on(slice(None), a, b, (engine, N, sample))
        assert torch.equal(envs[0].workspace, envs[1].workspace), (engine, N, sample)
        assert torch.equal(pop.hidden.view(torch.int32), ctl.hidden.view(torch.int32)), (engine, N, sample)
        _same_on(slice(None), pop.select(want_probs=True, want_value=True, want_hidden=True),
                 ctl.select(want_probs=True, want_value=True, want_hidden=True), (engine, N, sample, "select"))
        assert (a["done"] != 0).any() and float(pop.hidden.abs().max()) > 0
        _close(envs)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the engines agree

@pytest.mark.parametrize("N,group", ((700, 256), (1000, 512)))
def test_matrix_population_equals_lane_population_at_64_units(N, group):
    envs = _envs(2, N, sampler=True, auto_reset=True)
    import abrsimulator_amd as A
    P = -(-N // group)
    mem = _members(np.random.default_rng(41), 64, P)
    pops = [A.RecurrentPolicyPopulation(A.EnvPlayer(e), [(c, h) for c, h, _ in mem], group,
                                        value_heads=[v for _, _, v in mem], window=8, engine=eng, sample="softmax",
                                        explore=0.2, temperature=0.9, seed=5) for e, eng in zip(envs, ("lane", "matrix"))]
    assert torch.equal(pops[0].weights.view(torch.int32), pops[1].weights.view(torch.int32))
    kw = dict(want_probs=True, want_value=True, want_hidden=True)
    _same_on(slice(None), pops[0].select(**kw), pops[1].select(**kw), "select")
    outs = [e.step_policy(p, STEPS, **ALL) for e, p in zip(envs, pops)]
    _same_on(slice(None), outs[0], outs[1], "rollout")
    assert torch.equal(envs[0].workspace, envs[1].workspace)
    assert _eq(pops[0].hidden, pops[1].hidden)
    _close(envs)


# ---------------------------------------------------------------------------------------------------------------------
# 5. load_member between launches; a masked reset

@pytest.mark.parametrize("engine,H", (("lane", 33), ("matrix", 65)))
def test_load_member_changes_exactly_that_members_lanes(engine, H):
    import abrsimulator_amd as A
    rng = np.random.default_rng(51)
    N, group = 1000, 256
    env = _env(N, auto_reset=True)
    mem = [_weights(rng, 18, H, 6) for _ in range(4)]
    pop = A.RecurrentPolicyPopulation(A.EnvPlayer(env), [(c, h) for c, h, _ in mem], group,
                                      value_heads=[v for _, _, v in mem], engine=engine)
    env.step_policy(pop, 3)                                                 # a state that is not zero
    kw = dict(want_value=True, want_hidden=True)
    first = pop.select(**kw)
    state = pop.hidden.clone()
    cell, head, vh = _weights(rng, 18, H, 6)
    pop.load_member(2, cell, head, value_head=vh)                           # in place, on the stream
    assert torch.equal(state, pop.hidden)
    second = pop.select(**kw)
    ref_env = _env(N, auto_reset=True)
    ref_env.load_state_dict(env.state_dict())
    for m in range(4):
        sl = pop.lanes_of(m)
        ctl = A.RecurrentPolicyController(A.EnvPlayer(ref_env), *pop.member_parts(m), value_head=(pop.value_heads[m, :H],
                                          pop.value_heads[m, H]), engine=engine)
        ctl.hidden.copy_(pop.hidden)
        _same_on(sl, second, ctl.select(**kw), (engine, m))
        if m == 2:
            assert not _eq(first["scores"][:, sl], second["scores"][:, sl])
            assert not _eq(first["value"][sl], second["value"][sl])
            assert _eq(first["hidden"][:, sl], second["hidden"][:, sl])
        else:
            _same_on(sl, first, second, (engine, m, "untouched"))
    out = env.step_policy(pop, 3, want_scores=True)                         # and the next rollout sees the new member
    assert out["scores"].shape == (3, 6, N)
    env.close()
    ref_env.close()


@pytest.mark.parametrize("engine,H", (("lane", 33), ("matrix", 65)))
def test_masked_reset_of_half_a_members_lanes_restarts_only_those(engine, H):
    N, group = 700, 256
    envs = _envs(4, N)
    pop, refs = _build(envs, H, group, engine, np.random.default_rng(61))
    mask = torch.zeros(N, dtype=torch.bool, device=envs[0].device)
    mask[512:700:2] = True                                                  # half of member 2's lanes
    kw = dict(want_probs=True, want_value=True, want_hidden=True)
    envs[0].step_policy(pop, 2)
    for m in range(3):
        envs[1 + m].step_policy(refs[m], 2)
    for e in envs:
        e.reset(mask=mask)
    for s in range(3):
        got = pop.select(commit=True, **kw)
        if s == 0:
            assert (got["actions"][mask] >= 0).all()
            assert not got["hidden"][:, mask].view(torch.int32).any()       # restarted: +0.0f
            rest = torch.nan_to_num(got["hidden"][:, ~mask]).abs().amax(0)
            assert (rest[:256] > 0).all() and (rest[-94:] > 0).all()        # the others carry on (member 1 holds NaN)
        envs[0].step(got["actions"])
        for m in range(3):
            ref, sl = refs[m].select(commit=True, **kw), pop.lanes_of(m)
            _same_on(sl, got, ref, (engine, s, m))
            assert _eq(pop.hidden[:, sl], refs[m].hidden[:, sl]), (engine, s, m)
            envs[1 + m].step(ref["actions"])
    # reset_hidden(mask) zeroes the masked columns of the one slab and nothing else
    before = pop.hidden.clone()
    pop.reset_hidden(mask)
    assert not pop.hidden[:, mask].view(torch.int32).any() and _eq(pop.hidden[:, ~mask], before[:, ~mask])
    _close(envs)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the read-out an evolution strategy ranks its members by

def test_ledger_per_member_after_a_population_rollout():
    from abrsimulator_amd.ledger import FLOAT_FIELDS
    N, group = 700, 256
    env = _env(N, auto_reset=True)
    env.set_episode_sampler(77, offset_span=100)
    led = env.set_episode_ledger(8)
    pop, _ = _build([env] * 4, 33, group, "lane", np.random.default_rng(71), sample="softmax", explore=0.1)
    P = pop.n_members
    env.step_policy(pop, 24, want_obs=False, want_actions=False)
    pm = led.per_member(group, P)
    cnt = led.count().cpu().numpy().astype(np.int64)
    assert cnt.min() >= 4 and cnt.max() <= 8                                # nothing has left the ring: records() has all
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
            assert abs(got - float(np.mean(x))) * c <= 2 * (bound + 2 * u * abs(exact)), (k, m)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the controllers that were there before

def test_other_controllers_are_untouched():
    import abrsimulator_amd as A
    N = 512
    env = _env(N)
    rng = np.random.default_rng(81)
    F = 4 + 8 + 6
    layers = [((rng.standard_normal((16, F)) * 0.5).astype(f32), rng.standard_normal(16).astype(f32)),
              ((rng.standard_normal((6, 16)) * 0.5).astype(f32), rng.standard_normal(6).astype(f32))]
    layers2 = [(w * f32(0.5), b) for w, b in layers]
    mlp = A.PolicyController(A.EnvPlayer(env), layers, window=8, sample="softmax", explore=0.2, seed=3)
    mpop = A.PolicyPopulation(A.EnvPlayer(env), [layers, layers2], group=256, window=8, sample="softmax", seed=3)
    cell, head, vh = _weights(rng, F, 64, 6)
    gru = A.RecurrentPolicyController(A.EnvPlayer(env), cell, head, value_head=vh, sample="softmax")
    env.step_random(2, seed=1)
    kw = dict(want_probs=True, want_value=True, want_hidden=True)
    before = [mlp.select(want_probs=True), mpop.select(want_probs=True), gru.select(**kw)]
    ws, kept = env.workspace.clone(), gru.hidden.clone()
    for engine, H in (("lane", 64), ("matrix", 128)):
        pop, _ = _build([env] * 3, H, 256, engine, rng, sample="softmax")
        pop.select(commit=True, **kw)
        assert torch.equal(ws, env.workspace)                               # the state lives in the population
        assert torch.equal(kept, gru.hidden) and float(torch.nan_to_num(pop.hidden).abs().max()) > 0
        after = [mlp.select(want_probs=True), mpop.select(want_probs=True), gru.select(**kw)]
        for b, a in zip(before, after):
            for k in b:
                if b[k] is not None:
                    assert _eq(b[k], a[k]), (engine, k)
    env.step_policy(pop, 3, want_hidden=True)
    assert env.step_policy(mlp, 2, want_scores=True)["scores"].shape == (2, 6, N)
    assert env.step_policy(mpop, 2, want_scores=True)["scores"].shape == (2, 6, N)
    assert env.step_policy(gru, 2, want_hidden=True)["hidden"].shape == (2, 64, N)
    for c in (mlp, mpop):
        with pytest.raises(ValueError):
            env.step_policy(c, 2, want_hidden=True)
    with pytest.raises(ValueError, match="recurrent"):
        A.PolicyPopulation(A.EnvPlayer(env), [torch.nn.GRUCell(F, 8)], group=256)
    env.close()
