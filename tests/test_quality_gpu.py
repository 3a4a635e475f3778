"""The quality model on the device (include/abr_env.h: abr_episode_quality): the reward, the quality blob and nothing else.

The shape is the smallest that reaches every path: 200 lanes (three full 64-lane groups and a partial one), 5-chunk
episodes over 3 rates, auto_reset on, 13 decisions per launch -- every live lane closes two episodes inside a launch and
carries q_run out of it -- a ledger of 2 rows, so the ring wraps in the second launch, an all-zero trace whose lanes time
out in mid-download, and (scripted launches) one lane fed an out-of-range action.

Expectations.  Rewards: float32(oracle.step_rewards(..., dtype=float64) - wq * u[c][a]) with c and a from the oracle replay
of the launch's own actions, `==`; a timed-out or bad-action step equals the run without a model.  Everything else:
byte-identical to a run from the same starting bytes without a model.  The blob: the numpy twin (tests/quality_twin.py)
driven by the launch's actions and done bytes, byte for byte."""
import ctypes as C

import numpy as np
import pytest
import torch

import abrsimulator_amd as A
from abrsimulator_amd import _lib
from abrsimulator_amd.episodes import EpisodeSampler
from helpers import DIAG_IMPLS, diag_lib
from quality_twin import TwinQuality

pytestmark = pytest.mark.gpu

LADDER = [0.3, 1.2, 2.85]
V, L, MB, SU, W = 5, 4.0, 20.0, 4.0, [4.3, 1.0, 1.0, 0.1]
M = len(LADDER)
N = 200
T = 2 * V + 3                                 # two episodes closed, three chunks into the third
MAX_TICKS = 4000                              # a live episode takes about V * L / 0.01 = 2000 ticks
DEAD = 6                                      # the all-zero trace
IMPLS = ["jump", "split", "split3", "tick"]
WQ = 0.37
SMP = EpisodeSampler(0x5EED)
BAD = (17, 3)                                 # (lane, step) of the out-of-range scripted action


def corpus():
    rng = np.random.default_rng(0)
    return [rng.uniform(3.0, 8.0, int(rng.integers(30, 200))) for _ in range(DEAD)] + [np.zeros(40)]


TRACES = corpus()
TL = np.array([len(t) for t in TRACES], np.int32)
TID = (np.arange(N) % len(TRACES)).astype(np.int32)
OFF = (np.arange(N) % 13).astype(np.int32)
TABLE = np.sort(np.random.default_rng(4).uniform(0.2, 4.0, (V, M)), axis=1)      # a per-chunk bitrate table


def make(impl, auto_reset=True, table=None, **kw):
    chunks = A.Chunk(LADDER) if table is None else [A.Chunk(list(r)) for r in table]
    return A.BatchedABREnv(A.MPD(V, L, MB, SU, chunks), A.QOEMetric(*W), A.NetworkInfo(1.0, TRACES), N, device="cuda",
                           auto_reset=auto_reset, impl=impl, max_ticks=MAX_TICKS, **kw)


def start(env, sampled):
    if sampled:
        env.set_episode_sampler(SMP.seed)
        env.reset(sample=True)
    else:
        env.reset(torch.from_numpy(TID), torch.from_numpy(OFF))
    return env


def pair_fn(sampled):
    """e -> (trace ids, offsets) of every lane's episode number e."""
    if sampled:
        g = np.arange(N, dtype=np.uint64)
        return lambda e: SMP.draw(g, e, TL)
    return lambda e: (TID, OFF)


def script(seed=3, t=2 * T):
    a = np.random.default_rng(seed).integers(0, M, (t, N)).astype(np.int32)
    a[BAD[1], BAD[0]] = M + 4
    return a


def np_out(out):
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def launch(env, kind, n, t0=0, acts=None, ctl=None):
    """n decisions of `kind`; returns numpy (actions, reward, done, obs)."""
    if kind == "random":
        o = np_out(env.step_random(n, 77 + t0))
    elif kind == "script":
        o = np_out(env.step_script(torch.from_numpy(acts[t0:t0 + n]).cuda()))
        o["actions"] = acts[t0:t0 + n]
    elif kind == "step":
        rs = []
        for t in range(t0, t0 + n):
            ob, r, d = env.step(torch.from_numpy(acts[t]).cuda())
            rs.append((ob.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()))
        o = dict(obs=np.stack([x[0] for x in rs]), reward=np.stack([x[1] for x in rs]), done=np.stack([x[2] for x in rs]),
                 actions=acts[t0:t0 + n])
    elif kind == "rule":
        o = np_out(env.step_rule(ctl, n))
    elif kind == "mpc":
        o = np_out(env.step_mpc(ctl, n))
    else:
        o = np_out(env.step_policy(ctl, n, **({"want_values": True} if kind == "policy_ac" else {})))
    return o


def replay(oracle, acts, hit, cs, ep, pairs, wq, u, lanes=None, table=None):
    """The float64 rewards without a model and the expected float32 rewards with one, [n_steps, n], at the steps that
    completed a download (`hit`); elsewhere NaN.  acts, hit, cs (the chunk each step downloaded) and ep (the lane's
    episode number at each step) are [n_steps, n]; every lane starts at chunk 0.  pairs(e) -> (trace ids, offsets) of
    episode e.  Each episode is replayed through the oracle with the lane's own actions; a partial episode is padded with
    rate 0 (a step's reward depends on the actions up to that step only), and a lane whose episode runs on the all-zero
    trace is replayed on trace 0 (it never completes a download: nothing of that replay is used)."""
    n_steps, n = acts.shape
    lanes = np.arange(N) if lanes is None else lanes
    cfg = oracle.env_cfg(LADDER, L, V, MB, SU, 1.0, W, 1.0, br_table=table)
    want = np.full((n_steps, n), np.nan, np.float32)
    for e in sorted(set(ep[hit].tolist())):
        a = np.zeros((n, V), np.int32)
        sel = hit & (ep == e)
        tt, ii = np.nonzero(sel)
        a[ii, cs[tt, ii]] = acts[tt, ii]
        tid, off = pairs(e)
        tid = np.where(tid[lanes] == DEAD, 0, tid[lanes]).astype(np.int32)
        steps, _, fin, _ = oracle.env_batch(cfg, TRACES, tid, off[lanes], a)
        from oracle.oracle import step_rewards
        r64 = step_rewards(steps["rebuffer_time"], steps["start_up_time"], fin["rebuffer_time"], fin["start_up_time"], a, W,
                           ladder=LADDER, br_table=table, dtype=np.float64)
        want[tt, ii] = (r64[ii, cs[tt, ii]] - np.float64(wq) * u[cs[tt, ii], acts[tt, ii]]).astype(np.float32)
    return want


class Case:
    """One environment with a quality model (`q`) and one without (`p`, the parent's behaviour) started from the same
    bytes, each with a ledger of `rows`; and the twin of the quality blob."""

    def __init__(self, impl, sampled=False, wq=WQ, utility="identity", rows=2, auto_reset=True, table=None, ledger=True):
        self.p = start(make(impl, auto_reset, table), sampled)
        self.q = make(impl, auto_reset, table)
        if sampled:
            self.q.set_episode_sampler(SMP.seed)
        self.q.load_state_dict(self.p.state_dict())
        assert torch.equal(self.p.workspace, self.q.workspace)
        self.lp = self.p.set_episode_ledger(rows) if ledger else None
        self.lq = self.q.set_episode_ledger(rows) if ledger else None
        self.ql = self.q.set_quality(wq, utility) if ledger else self.q.set_quality(wq, utility, rows=rows)
        assert self.q.quality is self.ql and self.ql.rows == rows and self.ql.blob.data_ptr() % 256 == 0
        self.u = self.ql.table.cpu().numpy()
        self.twin = TwinQuality(N, rows, wq, self.u)
        self.auto_reset, self.sampled, self.wq, self.table, self.utility = auto_reset, sampled, wq, table, utility
        self.frozen = np.zeros(N, bool)
        self.hist = []                        # (acts, hit, cs, ep, reward with, reward without) per launch

    def chunk0(self):
        return self.q.mpc_inputs()[0].cpu().numpy().astype(np.int64)

    def run(self, kind, n, t0=0, acts=None, ctl=None):
        """One launch of both environments; the twin follows.  Checks that nothing but the rewards differs."""
        c0 = self.chunk0()
        ep0 = self.q.episodes()["episode"].cpu().numpy().astype(np.int64)
        cp, cq = (ctl(self.p), ctl(self.q)) if ctl is not None else (None, None)
        op, oq = launch(self.p, kind, n, t0, acts, cp), launch(self.q, kind, n, t0, acts, cq)
        for k in op:
            if k != "reward":
                assert np.array_equal(op[k], oq[k], equal_nan=True), k
        assert torch.equal(self.p.workspace, self.q.workspace), "the workspace differs"
        if self.lp is not None:
            assert torch.equal(self.lp.blob, self.lq.blob), "the ledger differs"
        acts_r = np.where(oq["actions"] < 0, 0, oq["actions"])
        _, hit, cs, _, frozen = self.twin.launch(c0, acts_r, oq["done"], self.auto_reset, frozen=self.frozen)
        # the lane's episode number at each step: the number at the launch's start plus the re-arms so far
        rearm = hit & (cs == V - 1) & self.auto_reset
        ep = ep0[None, :] + np.concatenate([np.zeros((1, N), np.int64), np.cumsum(rearm, 0)[:-1]])
        self.frozen = frozen
        self.hist.append((acts_r, hit, cs, ep, oq["reward"], op["reward"]))
        return oq

    def check_blob(self):
        got = self.ql.blob.cpu().numpy()
        t = self.twin
        for name, a, b in (("count", self.ql.count(), t.count), ("q_run", self.ql.running(), t.q_run),
                           ("q_last", self.ql.last(), t.q_last), ("total_q", self.ql.totals(), t.total_q),
                           ("rec_q", self.ql.ring(), t.rec_q)):
            assert a.cpu().numpy().tobytes() == b.tobytes(), name
        assert got.tobytes() == t.blob.tobytes()

    def check_rewards(self, oracle):
        """Every reward of every launch so far.  The launches together must start at chunk 0 of every lane."""
        acts, hit, cs, ep = (np.concatenate([h[k] for h in self.hist]) for k in range(4))
        rq, rp = (np.concatenate([h[k] for h in self.hist]) for k in (4, 5))
        want = replay(oracle, acts, hit, cs, ep, pair_fn(self.sampled), self.wq, self.u, table=self.table)
        assert hit.any() and (~hit).any()
        assert np.array_equal(rq[hit], want[hit]), "a reward with a completed download"
        assert rq[~hit].tobytes() == rp[~hit].tobytes(), "a reward without a completed download moved"
        if self.wq != 0.0:                    # non-vacuity ("log" scores the lowest rate 0.0: a third of random actions)
            assert (rq[hit] != rp[hit]).mean() > (0.99 if self.utility == "identity" else 0.5)
        return acts, hit, cs, ep, rq, rp


# ---- 1, 2, 3: rewards, nothing else moves, the blob equals the twin; two launches, the ring wraps ----
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("kind", ["random", "script"])
@pytest.mark.parametrize("impl", IMPLS)
def test_rewards_blob_and_nothing_else(oracle, impl, kind, sampled):
    c = Case(impl, sampled, utility="log" if sampled else "identity")
    acts = script() if kind == "script" else None
    o1 = c.run(kind, T, 0, acts)
    c.check_blob()
    live = ~c.frozen
    if not sampled:
        dead = TID == DEAD
        assert ((o1["done"][0] & _lib.DONE_TIMEOUT) != 0)[dead].all() and not c.hist[0][1][:, dead].any()
        assert (c.twin.count[dead] == 1).all() and (c.twin.count[live] == 2).all() and live.sum() > 150
        assert (c.twin.q_run[live] != 0).all() and (c.twin.q_run[dead] == 0).all()      # carried out of the launch
    if kind == "script":
        assert o1["done"][BAD[1], BAD[0]] & _lib.DONE_BADACT and c.frozen[BAD[0]] and c.twin.count[BAD[0]] == 0
        assert o1["reward"][BAD[1], BAD[0]] == 0.0
    o2 = c.run(kind, T, T, acts)
    c.check_blob()
    # the ring of 2 wrapped twice (under the sampler a lane re-armed onto the all-zero trace adds a timed-out record and stops)
    assert (c.twin.count[~c.frozen] == 5).all() and (~c.frozen).sum() > 50 and 5 <= c.twin.count.max() <= 6
    c.check_rewards(oracle)
    # 5: the last episode's combined figure is the newest joined record's
    rec = {k: v.cpu().numpy() for k, v in c.ql.records(c.lq).items()}
    newest = np.r_[np.nonzero(np.diff(rec["lane"]))[0], rec["lane"].size - 1]
    has = c.twin.count > 0
    assert np.array_equal(rec["lane"][newest], np.nonzero(has)[0])
    got = c.q.episode_qoe(quality=True).cpu().numpy()
    assert got[has].tobytes() == rec["qoe_q"][newest].tobytes()
    assert np.array_equal(rec["qoe_q"], rec["qoe"] - c.wq * rec["quality"])
    assert np.array_equal(c.q.episode_qoe().cpu().numpy(), c.p.episode_qoe().cpu().numpy())


@pytest.mark.parametrize("impl", IMPLS)
def test_weight_zero_leaves_every_reward_byte(impl):
    c = Case(impl, wq=0.0, utility="identity")
    o = c.run("random", T)
    assert o["reward"].tobytes() == c.hist[0][5].tobytes()
    c.check_blob()
    assert (c.twin.total_q[~c.frozen] > 0).all()


@pytest.mark.parametrize("impl", IMPLS)
def test_fused_single_steps_and_pieces_agree(impl):
    acts = script(8, T)
    a, b, d = Case(impl), Case(impl), Case(impl)
    ra = a.run("script", T, 0, acts)["reward"]
    rb = b.run("step", T, 0, acts)["reward"]
    rd = np.concatenate([d.run("script", 7, 0, acts)["reward"], d.run("script", 6, 7, acts)["reward"]])
    a.check_blob(), b.check_blob(), d.check_blob()
    assert torch.equal(a.ql.blob, b.ql.blob) and torch.equal(a.ql.blob, d.ql.blob)
    assert ra.tobytes() == rb.tobytes() == rd.tobytes()


# ---- 4: launch kinds ----
def _policy(critic=False, **kw):
    def build(env):
        rng = np.random.default_rng(5)
        layers, fan = [], 4 + 4 + M
        for w in (16, M):
            layers.append((rng.normal(0, 1.5 / np.sqrt(fan), (w, fan)).astype(np.float32),
                           rng.normal(0, 0.2, w).astype(np.float32)))
            fan = w
        head = (rng.normal(0, 0.3, 16).astype(np.float32), np.float32(0.1)) if critic else None
        return A.PolicyController(A.EnvPlayer(env), layers, window=4, explore=0.25, seed=9, value_head=head, **kw)
    return build


CLOSED = {
    "rule": ("rule", lambda env: A.RateBasedController(A.EnvPlayer(env), window=3), ("jump", "tick")),
    "mpc": ("mpc", lambda env: A.BatchedMPCController(A.EnvPlayer(env), horizon=3, clip_horizon=True),
            ("jump", "split", "split3")),
    "policy": ("policy", _policy(), ("jump", "split", "split3")),
    "policy_sampled": ("policy", _policy(sample="softmax", temperature=0.7), ("jump", "split", "split3")),
    "policy_ac": ("policy_ac", _policy(critic=True, sample="softmax", temperature=0.7), ("jump", "split", "split3")),
}


@pytest.mark.parametrize("name,impl", [(k, i) for k, v in CLOSED.items() for i in v[2]])
def test_closed_loop_launches(oracle, name, impl):
    kind, ctl, _ = CLOSED[name]
    c = Case(impl)
    c.run(kind, T, ctl=ctl)
    c.check_blob()
    assert (c.twin.count[~c.frozen] == 2).all() and (~c.frozen).sum() > 150
    c.check_rewards(oracle)


@pytest.mark.parametrize("impl", IMPLS)
def test_a_masked_reset_zeroes_the_masked_running_sums_only(oracle, impl):
    c = Case(impl)
    c.run("random", 7)
    c.check_blob()
    before = c.ql.blob.clone()
    run0 = c.ql.running().clone()
    mask = (np.arange(N) % 3 == 0)
    tid2, off2 = ((TID + 1) % DEAD).astype(np.int32), ((OFF + 5) % 11).astype(np.int32)
    for env in (c.p, c.q):
        env.reset(torch.from_numpy(tid2), torch.from_numpy(off2), mask=torch.from_numpy(mask.astype(np.uint8)))
    m = torch.from_numpy(mask).cuda()
    assert (c.ql.running()[m] == 0).all() and torch.equal(c.ql.running()[~m], run0[~m]) and (run0[m] != 0).any()
    c.ql.running().copy_(run0)
    assert torch.equal(c.ql.blob, before), "a reset wrote more than q_run: a record, a count"
    c.ql.running()[m] = 0.0
    c.twin.reset(mask)
    c.frozen = c.frozen & ~mask                              # a reset revives a frozen lane
    first = c.hist.pop()
    o = c.run("random", 6, 7)
    c.check_blob()
    # unmasked lanes: 7 + 6 decisions on the first pair; masked lanes: 6 decisions from chunk 0 on the second pair
    u, wq = c.u, c.wq
    acts, hit, cs, ep = (np.concatenate([first[k], c.hist[0][k]]) for k in range(4))
    rq, rp = (np.concatenate([first[k], c.hist[0][k]]) for k in (4, 5))
    un = np.nonzero(~mask)[0]
    want = replay(oracle, acts[:, un], hit[:, un], cs[:, un], ep[:, un], pair_fn(False), wq, u, lanes=un)
    assert np.array_equal(rq[:, un][hit[:, un]], want[hit[:, un]])
    ma = np.nonzero(mask)[0]
    a2, h2, c2, e2 = (c.hist[0][k][:, ma] for k in range(4))
    want = replay(oracle, a2, h2, c2, e2, lambda e: (tid2, off2), wq, u, lanes=ma)
    assert h2.all() and np.array_equal(c.hist[0][4][:, ma][h2], want[h2])
    assert rq[~hit].tobytes() == rp[~hit].tobytes()
    assert (c.twin.count[ma] == 2).all()                     # one record before the reset, one after: none for the abandoned episode


@pytest.mark.parametrize("impl", IMPLS)
def test_without_auto_reset_one_record_then_a_frozen_lane(oracle, impl):
    c = Case(impl, auto_reset=False, rows=1, ledger=False)
    o = c.run("random", T)
    c.check_blob()
    assert (c.twin.count == 1).all() and c.frozen.all()
    live = TID != DEAD
    assert c.hist[0][1][:V, live].all() and not c.hist[0][1][V:].any()
    assert np.array_equal(c.twin.q_run, c.twin.q_last)       # no re-arm: the sum stays until a reset
    c.check_rewards(oracle)
    before = c.ql.blob.clone()
    c.run("random", 3, T)
    assert torch.equal(c.ql.blob, before)


@pytest.mark.parametrize("impl", IMPLS)
def test_per_chunk_table_with_the_identity_utility(oracle, impl):
    c = Case(impl, utility="identity", table=TABLE)
    assert np.array_equal(c.u, TABLE)
    c.run("random", T)
    c.check_blob()
    c.check_rewards(oracle)


# ---- 6: refusals ----
def test_refusals_and_off_again():
    c = Case("jump")
    env, lib = c.q, c.q.lib
    ql = c.ql
    ok = dict(wq=1.0, u_dev=ql.table.data_ptr(), base_dev=ql.blob.data_ptr(), rows=2, reserved_=0)
    other = A.EpisodeQuality(N, 2, 5.0, ql.table.cpu().numpy(), "cuda")
    for change, word in ((dict(wq=float("nan")), b"finite"), (dict(wq=float("inf")), b"finite"),
                         (dict(u_dev=None), b"u_dev is NULL"), (dict(u_dev=ok["u_dev"] + 4), b"8-byte"),
                         (dict(base_dev=None), b"base_dev is NULL"), (dict(base_dev=ok["base_dev"] + 64), b"256-byte"),
                         (dict(rows=0), b"rows")):
        st = _lib.EpisodeQuality(**{**ok, "base_dev": other.blob.data_ptr(), **change})
        assert lib.abr_env_set_episode_quality(env._h, C.byref(st)) == -1 and word in lib.abr_last_error(), change
    c.run("random", V)                                       # nothing was stored: the installed model is still the one in force
    c.check_blob()
    assert not other.blob.any()
    with pytest.raises(ValueError):
        env.set_quality(1.0, "sqrt")
    with pytest.raises(ValueError):
        env.set_quality(float("nan"))
    with pytest.raises(ValueError):
        env.set_quality(1.0, np.zeros((V, M + 1)))
    with pytest.raises(ValueError):
        env.set_quality(A.EpisodeQuality(N + 1, 2, 1.0, ql.table.cpu().numpy(), "cuda"))
    assert "quality" in env.state_dict() and "quality" not in c.p.state_dict()
    # set_quality(None): today's rewards again, and the blob stands still
    assert env.set_quality(None) is None and env.quality is None
    before = ql.blob.clone()
    rp, rq = c.p.step_random(T, 5)["reward"], env.step_random(T, 5)["reward"]
    assert torch.equal(rp, rq) and torch.equal(ql.blob, before)
    with pytest.raises(ValueError):
        env.episode_qoe(quality=True)
    q = torch.empty(N, dtype=torch.float64, device="cuda")
    assert lib.abr_env_episode_quality(env._h, C.c_void_p(q.data_ptr()), None) == -1


def test_rows_default_to_the_ledgers_and_shards_pass_through():
    env = make("jump")
    assert env.set_quality().rows == 1
    env.set_episode_ledger(3)
    assert env.set_quality(2.0, "log_top").rows == 3 and env.quality.weight == 2.0
    sh = A.ShardedABREnv(A.MPD(V, L, MB, SU, A.Chunk(LADDER)), A.QOEMetric(*W), A.NetworkInfo(1.0, TRACES),
                         total_lanes=N, device="cuda", rank=0, world=1, gather=False, env=env)
    ql = sh.set_quality(0.5, "identity", rows=2)
    assert sh.quality is ql is env.quality and ql.rows == 2 and ql.n_lanes == N
    assert sh.set_quality(None) is None and env.quality is None


@pytest.mark.parametrize("impl", DIAG_IMPLS)
def test_the_diagnostic_pipelines_refuse_a_quality_model(impl):
    env = make(impl, library=diag_lib())
    env.reset(torch.from_numpy(TID), torch.from_numpy(OFF))
    env.set_quality()
    with pytest.raises(_lib.AbrError, match="quality model"):
        env.step_random(4, 1)
    env.set_quality(None)
    env.step_random(4, 1)
