"""The lookahead expert on the device (include/abr_env.h: abr_env_lookahead_select; LookaheadExpert).

The reference is the existing kernels, never the code under test: from a saved state_dict(), every one of the n_rates^H
sequences is restored, stepped with step_script (the sequence tiled over the lanes) and read back with observe_f64; the key
is then formed in numpy float64 in the contract's order.  A finished lane reports reward 0 and a frozen state under
auto_reset=False, so the trailing steps of a horizon the episode's end has shrunk add nothing.  q, key and action must
equal the reference's on the bit pattern; ties go to the smaller index."""
import itertools

import numpy as np
import pytest
import torch

import abrsimulator_amd as A
from abrsimulator_amd import _lib

pytestmark = pytest.mark.gpu

LADDER16 = [0.3, 0.5, 0.75, 1.0, 1.2, 1.5, 1.85, 2.3, 2.85, 3.5, 4.3, 5.2, 6.0, 7.0, 8.0, 9.5]
L, MB, SU, W = 4.0, 20.0, 8.0, [4.3, 1.0, 1.0, 0.1]
TIMEOUT = _lib.DONE_TIMEOUT


def ladder(M):
    return [0.3, 1.2, 2.85] if M == 3 else [LADDER16[(16 * k) // M] for k in range(M)]


def corpus():
    rng = np.random.default_rng(0)
    return [rng.uniform(0.5, 6.0, int(rng.integers(30, 200))) for _ in range(8)]


TRACES = corpus()


def make(N, M=3, V=6, traces=None, **kw):
    return A.BatchedABREnv(A.MPD(V, L, MB, SU, A.Chunk(ladder(M))), A.QOEMetric(*W), A.NetworkInfo(1.0, traces or TRACES), N,
                           device="cuda", **kw)


def start(env, seed=3):
    N = env.n_lanes
    rng = np.random.default_rng(seed)
    tid = (np.arange(N) % env.n_traces).astype(np.int32)
    off = rng.integers(0, 30, N).astype(np.int32)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    return tid, off


def advance(env, steps, seed=5):
    acts = np.random.default_rng(seed).integers(0, env.n_rates, (max(steps, 1), env.n_lanes)).astype(np.int32)
    for t in range(steps):
        env.step(torch.from_numpy(acts[t]).cuda())
    return acts


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if torch.is_tensor(t) else t, np.float64).view(np.uint64)


def reference(env, H):
    """(action int32 [N], key [N], q [M, N]) of the environment's current state from step_script and observe_f64; the
    environment is left as it was found."""
    M, N, wl = env.n_rates, env.n_lanes, W[3]
    sd = env.state_dict()
    root_done = env.done_after_reset().cpu().numpy().copy()
    q = np.full((M, N), np.nan)
    for seq in itertools.product(range(M), repeat=H):                     # lexicographic: the tie rule's order
        env.load_state_dict(sd)
        out = env.step_script(torch.tensor(seq, dtype=torch.int32).reshape(H, 1).repeat(1, N))
        lat = env.observe_f64()["average_latency"].cpu().numpy()
        rew, dn = out["reward"].cpu().numpy(), out["done"].cpu().numpy()
        R = np.zeros(N)
        for j in range(H):
            R = R + rew[j].astype(np.float64)
        key = R + wl * lat
        ok = (root_done == 0) & ((dn & TIMEOUT) == 0).all(0) & ~np.isnan(key)
        row = q[seq[0]]
        take = ok & ~(row <= key)                                         # NaN or larger: replaced; equal: the earlier stays
        row[take] = key[take]
    env.load_state_dict(sd)
    action, key = np.full(N, -1, np.int32), np.full(N, np.nan)
    for m in range(M):
        take = ~np.isnan(q[m]) & ~(key <= q[m])
        action[take], key[take] = m, q[m][take]
    return action, key, q


def expect(env, H, lab=None, **kw):
    lab = lab or A.LookaheadExpert(A.EnvPlayer(env), H, **kw).labels(want_q=True)
    a, k, q = reference(env, H)
    torch.cuda.synchronize()
    assert lab["action"].dtype == torch.int32 and lab["key"].dtype == torch.float64 and tuple(lab["q"].shape) == q.shape
    assert np.array_equal(lab["action"].cpu().numpy(), a)
    nan = np.isnan(k)
    assert np.array_equal(np.isnan(lab["key"].cpu().numpy()), nan) and np.array_equal(np.isnan(lab["q"].cpu().numpy()), np.isnan(q))
    assert np.array_equal(bits(lab["key"])[~nan], bits(k)[~nan])
    assert np.array_equal(bits(lab["q"])[~np.isnan(q)], bits(q)[~np.isnan(q)])
    assert ((a == -1) == nan).all()
    return lab, (a, k, q)


def test_core_equals_the_existing_kernels():
    """200 lanes, V = 6, 3 rates, horizon 3 at the states after 0, 2, 4 and 5 steps: the last two shrink the horizon."""
    env = make(200)
    start(env)
    acts = np.random.default_rng(5).integers(0, 3, (5, 200)).astype(np.int32)
    t = 0
    for upto in (0, 2, 4, 5):
        while t < upto:
            env.step(torch.from_numpy(acts[t]).cuda())
            t += 1
        lab, (a, k, q) = expect(env, 3)
        assert (a >= 0).all()
        if upto == 5:                                                     # one decision left: q is that step's cost
            assert len(np.unique(q, axis=0)) > 1
    env.step(torch.from_numpy(acts[4]).cuda())                            # every lane finished: no label
    lab = A.LookaheadExpert(A.EnvPlayer(env), 3).labels(want_q=True)
    assert (lab["action"] == -1).all() and torch.isnan(lab["key"]).all() and torch.isnan(lab["q"]).all()


def test_never_armed_lanes_have_no_label_and_next_bitrate_is_the_action():
    env = make(70)
    exp = A.LookaheadExpert(A.EnvPlayer(env), 2)
    lab = exp.labels(want_key=False)
    assert lab["key"] is None and lab["q"] is None and (lab["action"] == -1).all()
    start(env)
    advance(env, 1)
    assert torch.equal(exp.next_bitrate(), exp.labels()["action"])


def test_read_only_workspace_quality_and_ledger():
    env = make(200)
    env.set_episode_ledger(2)
    env.set_quality(3.0, "log", rows=2)
    start(env)
    advance(env, 4)                                                       # horizon 3 crosses the episode's end
    ws, qb, lb = env.workspace.clone(), env.quality.blob.clone(), env.episode_ledger.blob.clone()
    A.LookaheadExpert(A.EnvPlayer(env), 3).labels(want_q=True)
    torch.cuda.synchronize()
    assert torch.equal(env.workspace, ws) and torch.equal(env.quality.blob, qb) and torch.equal(env.episode_ledger.blob, lb)
    assert (env.episode_ledger.count() == 0).all()                        # no record appears


@pytest.mark.parametrize("N", [1, 64, 65, 200])
def test_lane_counts(N):
    env = make(N)
    start(env)
    advance(env, 1)
    expect(env, 3)


@pytest.mark.parametrize("M,H,V", [(1, 2, 6), (16, 2, 6), (2, 8, 9)])
def test_rate_counts_and_the_deepest_instance(M, H, V):
    env = make(100, M=M, V=V)
    start(env)
    advance(env, 1)                                                       # (2, 8, 9): eight decisions left, 256 sequences
    expect(env, H)


def test_staggered_lanes():
    """After two steps half the lanes are reset: one wave then holds lanes at chunk 0 and chunk 2, and near the end their
    horizons differ."""
    env = make(200)
    tid, off = start(env)
    advance(env, 2)
    mask = (np.arange(200) % 2).astype(np.uint8)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off), mask=torch.from_numpy(mask))
    c = env.observe_f64()["chunk_id"].cpu().numpy()
    assert set(c[mask == 1]) == {0.0} and set(c[mask == 0]) == {2.0}
    expect(env, 3)
    advance(env, 2, seed=8)                                               # chunks 2 and 4: h = 3 and 2
    expect(env, 3)
    advance(env, 1, seed=9)                                               # chunks 3 and 5: h = 3 and 1
    expect(env, 3)


def test_with_a_quality_model():
    env, plain = make(200), make(200)
    q = env.set_quality(3.0, "log")
    for e in (env, plain):
        start(e)
        advance(e, 2)
    run0 = q.running().clone()
    lab, _ = expect(env, 3)
    assert torch.equal(q.running(), run0)                                 # q_run is unchanged
    base = A.LookaheadExpert(A.EnvPlayer(plain), 3).labels()
    assert not torch.equal(lab["key"], base["key"])                       # the keys carry the term
    assert (lab["action"] > base["action"]).any()                         # and it pays for higher rates


def test_timeouts():
    # an all-zero trace next to live ones: those lanes answer -1 and NaN
    traces = [np.zeros(40)] + TRACES[:3]
    env = make(130, traces=traces, max_ticks=20_000)
    tid, _ = start(env)
    lab, _ = expect(env, 2)
    dead = torch.from_numpy(tid == 0).cuda()
    assert (lab["action"][dead] == -1).all() and torch.isnan(lab["key"][dead]).all() and torch.isnan(lab["q"][:, dead]).all()
    assert (lab["action"][~dead] >= 0).all()
    # 0.3 throughout and 40 s of ticks: one top-rate chunk is 38 s of download and the two cheapest after it 8 s, so every
    # sequence that starts at the top rate times out; a middle-rate start (16 s + 8 s) and a bottom-rate one fit
    env = make(64, traces=[np.full(40, 0.3)], max_ticks=4_000)
    start(env)
    lab, (a, k, q) = expect(env, 3)
    assert np.isnan(q[2]).all() and np.isfinite(q[:2]).all() and (a >= 0).all() and np.isfinite(k).all()


def test_auto_reset_makes_no_difference():
    a, b = make(200, auto_reset=False), make(200, auto_reset=True)
    for e in (a, b):
        start(e)
        advance(e, 4)                                                     # chunk 4 of 6: horizon 3 crosses the end
    la, _ = expect(a, 3)
    lb = A.LookaheadExpert(A.EnvPlayer(b), 3).labels(want_q=True)
    for k in ("action", "key", "q"):
        assert np.array_equal(la[k].cpu().numpy().view(np.uint8), lb[k].cpu().numpy().view(np.uint8)), k


@pytest.mark.parametrize("N,launches", [(200, 4), (192, 3)])
def test_launch_splitting(N, launches):
    """39 nodes per lane at 3 rates and horizon 3: a bound of 64 lanes' worth makes every launch one wave group.  Ranges
    are multiples of 64, so 200 lanes split into four launches (64, 64, 64, 8) and 192 into three."""
    env = make(N)
    start(env)
    advance(env, 2)
    nodes = 3 + 9 + 27
    assert -(-N // 64) == launches
    one = A.LookaheadExpert(A.EnvPlayer(env), 3).labels(want_q=True)
    for cap in (nodes * 64, nodes * 64 + nodes * 63, 1):
        many = A.LookaheadExpert(A.EnvPlayer(env), 3, max_nodes_per_launch=cap).labels(want_q=True)
        for k in ("action", "key", "q"):
            assert np.array_equal(one[k].cpu().numpy().view(np.uint8), many[k].cpu().numpy().view(np.uint8)), (k, cap)
    if N == 200:
        expect(env, 3, lab=one)


def test_every_environment_implementation_leaves_the_same_state():
    labs = {}
    for impl in ("jump", "split", "split3", "tick"):
        env = make(200, impl=impl)
        start(env)
        acts = np.random.default_rng(5).integers(0, 3, (3, 200)).astype(np.int32)
        env.step_script(torch.from_numpy(acts).cuda())                    # the fused kernels of each implementation
        env.step(torch.from_numpy(acts[0]).cuda())
        labs[impl] = A.LookaheadExpert(A.EnvPlayer(env), 3).labels(want_q=True)
        if impl == "jump":
            expect(env, 3, lab=labs[impl])
    for impl in ("split", "split3", "tick"):
        for k in ("action", "key", "q"):
            assert np.array_equal(labs[impl][k].cpu().numpy().view(np.uint8), labs["jump"][k].cpu().numpy().view(np.uint8)), (impl, k)


def test_refusals():
    N = 64
    rule = A.LatencySpeedController((2.0, 6.0), (1.0, 8.0), ((0.9, 1.0, 1.0), (0.9, 1.1, 1.25), (0.75, 1.5, 2.0)))
    for speed in (torch.full((N,), 1.1, dtype=torch.float64), torch.full((2, N), 1.05, dtype=torch.float64), rule):
        env = make(N, speed=speed)
        start(env)
        with pytest.raises(_lib.AbrError, match="-4.*speed"):
            A.LookaheadExpert(A.EnvPlayer(env), 2).labels()
    env = make(N)
    start(env)
    exp = A.LookaheadExpert(A.EnvPlayer(env), 2)
    exp.labels()
    sp = torch.full((N,), 1.1, dtype=torch.float64, device="cuda")
    env._check(env.lib.abr_env_set_lane_speeds(env._h, _lib.ptr(sp)))      # pending ones refuse as well
    with pytest.raises(_lib.AbrError, match="-4.*pending"):
        exp.labels()
    env._check(env.lib.abr_env_set_lane_speeds(env._h, None))             # taking them back lifts the refusal
    exp.labels()
    env = make(N, M=6, speed=1.25)                                        # a constant play speed is fine
    start(env)
    advance(env, 1)
    expect(env, 2)
    with pytest.raises(_lib.AbrError, match="-4.*leaves"):                # 6^7 = 279 936 leaves
        A.LookaheadExpert(A.EnvPlayer(env), 7).labels()
    A.LookaheadExpert(A.EnvPlayer(env), 6).labels()                       # 46 656: the cap admits it
    torch.cuda.synchronize()


def test_replay_reproduces_the_key():
    """Stepping the returned actions for h decisions, re-deciding each time with the horizon one shorter, ends on the key:
    the first action of an optimal sequence is followed by an optimal remainder."""
    env = make(200)
    start(env)
    advance(env, 1)
    H = 3
    lab = A.LookaheadExpert(A.EnvPlayer(env), H).labels()
    key0 = lab["key"].cpu().numpy()
    R = np.zeros(200)
    act = lab["action"]
    for j in range(H):
        _, rew, dn = env.step(act)
        assert (dn.cpu().numpy() & TIMEOUT == 0).all()
        R = R + rew.cpu().numpy().astype(np.float64)
        if j + 1 < H:
            act = A.LookaheadExpert(A.EnvPlayer(env), H - 1 - j).next_bitrate()
    key = R + W[3] * env.observe_f64()["average_latency"].cpu().numpy()
    assert np.array_equal(key.view(np.uint64), key0.view(np.uint64))
