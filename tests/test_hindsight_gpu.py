"""The hindsight beam search on the device (abrsimulator_amd/search.py: HindsightSearch; abr_beam_select, abr_env_fork).

Workload (the one checked on the CPU, tests/test_fork_cpu.py): ladder [0.3, 1.2, 2.85], 5 chunks of 4 s, max buffer 20,
start-up 4, weights [4.3, 1, 1, 0.1], eight uniform(0.5, 6.0) traces, log utility with wq = 3; group g runs trace g % 8
from offset (g * 7) % 13.  The reference is pre-existing code: all 243 sequences of a pair run by step_script on a second
environment, scored by episode_qoe(quality=True).

Recorded, not asserted (MI355X): width 4 finds the exhaustive optimum in 24 of 24 groups and greedy is worse than it in
23 of 24 -- the figures test_greedy_is_worse_somewhere_and_width_4_is_recorded prints, and the ones the oracle gave on the
CPU."""
import itertools

import numpy as np
import pytest
import torch

import abrsimulator_amd as A
import fork_twin as T

pytestmark = pytest.mark.gpu

LADDER = [0.3, 1.2, 2.85]
V, L, MB, SU, W, WQ = 5, 4.0, 20.0, 4.0, [4.3, 1.0, 1.0, 0.1], 3.0
M = len(LADDER)
SEQS = np.array(list(itertools.product(range(M), repeat=V)), np.int32)          # [243, V]


def corpus():
    rng = np.random.default_rng(0)
    return [rng.uniform(0.5, 6.0, int(rng.integers(30, 200))) for _ in range(8)]


TRACES = corpus()


def pairs(G):
    g = np.arange(G)
    return (g % 8).astype(np.int32), ((g * 7) % 13).astype(np.int32)


def make(n_lanes):
    env = A.BatchedABREnv(A.MPD(V, L, MB, SU, A.Chunk(LADDER)), A.QOEMetric(*W), A.NetworkInfo(1.0, TRACES), n_lanes,
                          device="cuda")
    env.set_quality(WQ, "log")
    return env


@pytest.fixture(scope="module")
def exhaustive():
    """qoe_q of all 243 sequences of each of 24 groups, [24, 243], by step_script on an environment of its own: computed
    once and shared."""
    G = 24
    env = make(G * len(SEQS))
    tid, off = pairs(G)
    env.reset(torch.from_numpy(np.repeat(tid, len(SEQS))), torch.from_numpy(np.repeat(off, len(SEQS))))
    out = env.step_script(torch.from_numpy(np.ascontiguousarray(np.tile(SEQS, (G, 1)).T)).cuda())
    assert (out["done"][-1] == 1).all()
    return env.episode_qoe(quality=True).cpu().numpy().reshape(G, len(SEQS))


def replay(actions, G):
    """qoe_q of one sequence per group ([V, G]) by step_script on a fresh environment."""
    env = make(G)
    tid, off = pairs(G)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    out = env.step_script(actions.to(torch.int32).contiguous())
    assert (out["done"][-1] == 1).all()
    return env.episode_qoe(quality=True).cpu().numpy()


def search(beam, G):
    env = make(G * beam * M)
    hs = A.HindsightSearch(env, beam)
    tid, off = pairs(G)
    res = hs.run(torch.from_numpy(tid), torch.from_numpy(off))
    return env, hs, res


def test_exhaustive_width_finds_the_minimum_over_all_sequences(exhaustive):
    G = 8
    _, _, res = search(81, G)                                     # 243 slots, 8 groups = 1 944 lanes: nothing is pruned
    assert res["valid"].cpu().numpy().all()
    qoe = res["qoe"].cpu().numpy()
    assert np.array_equal(qoe, exhaustive[:G].min(1)), (qoe, exhaustive[:G].min(1))
    acts = res["actions"].cpu().numpy()
    for g in range(G):                                            # the optimum is unique: the sequence is the arg-min
        assert acts[:, g].tolist() == SEQS[exhaustive[g].argmin()].tolist()


@pytest.mark.parametrize("beam", [1, 4, 81])
def test_replaying_the_returned_actions_reproduces_the_returned_qoe(beam):
    G = 8
    _, _, res = search(beam, G)
    assert np.array_equal(replay(res["actions"], G), res["qoe"].cpu().numpy())


@pytest.mark.parametrize("beam", [1, 4, 81])
def test_every_iteration_equals_the_select_twin_on_the_devices_own_inputs(beam):
    G = 8
    S = beam * M
    env = make(G * S + 5)                                         # five lanes past the last group: ignored
    hs = A.HindsightSearch(env, beam)
    tid, off = pairs(G)
    hs.begin(torch.from_numpy(tid), torch.from_numpy(off))
    R = np.zeros(env.n_lanes)
    valid = ((np.arange(env.n_lanes) % S < M) & (np.arange(env.n_lanes) < G * S)).astype(np.uint8)
    for t in range(V):
        src, Ro, vo, reward, lat, done = [x.cpu().numpy() for x in hs.step()]
        n = G * S
        w_src, w_R, w_v = T.select(S, M, W[3], R[:n], reward[:n], lat[:n], done[:n], valid[:n])
        assert np.array_equal(src[:n], w_src) and np.array_equal(Ro[:n].view(np.uint64), w_R.view(np.uint64)), t
        assert np.array_equal(vo[:n], w_v), t
        assert (src[n:] == -1).all()
        assert int(w_v.reshape(G, S).sum(1).min()) == min(beam, M ** (t + 1)) * M, t     # survivors fill up, then the beam binds
        if t + 1 < V:
            R[:n], valid[:n] = w_R, w_v
    res = hs.finish()
    qoe = env.episode_qoe(quality=True).cpu().numpy()
    f_src, _, f_v = T.select(S, M, W[3], R[:n], reward[:n], None, done[:n], valid[:n], key_override=qoe[:n])
    assert np.array_equal(res["lane"].cpu().numpy(), f_src[::S]) and f_v[::S].all()
    assert np.array_equal(res["qoe"].cpu().numpy(), qoe[f_src[::S]])


def test_greedy_is_worse_somewhere_and_width_4_is_recorded(exhaustive):
    G = 24
    opt = exhaustive.min(1)
    _, _, r1 = search(1, G)
    _, _, r4 = search(4, G)
    q1, q4 = r1["qoe"].cpu().numpy(), r4["qoe"].cpu().numpy()
    print(f"hindsight: greedy worse than the optimum in {int((q1 > opt).sum())} of {G} groups; width 4 finds it in "
          f"{int((q4 == opt).sum())} of {G}")
    assert (q1 >= opt).all() and (q4 >= opt).all()                # a search result is one of the 243 sequences
    assert (q1 > opt).any()
