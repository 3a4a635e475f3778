"""The episode ledger on the device (include/abr_env.h: abr_episode_ledger): every finished episode of a fused launch
leaves one record.  The shape of test_episode_sampler_gpu.py -- 200 lanes, 8-chunk episodes, 7 ragged traces, 3 * V + 3
decisions, so that every lane finishes exactly three episodes in one launch -- and its helpers.  The expected records
are the oracle's `fin` of each (lane, episode), replayed with the launch's own actions from the sampler twin's pairs.

Tolerances: rebuffer_time, start_up_time, variance and the int fields ==; average_latency 1e-9
relative; qoe 1e-10 relative; total[f] == the in-order sum of the device's own records, and against the oracle the
per-field tolerance times the episode count."""
import ctypes as C

import numpy as np
import pytest
import torch

import abrsimulator_amd as A
from abrsimulator_amd import _lib
from abrsimulator_amd.episodes import EpisodeSampler
from speed_twin import rule_arrays
from test_episode_sampler_gpu import ALL, L, LADDER, MB, N, SMP, SU, T, TL, TRACES, V, W, armed, make, np_out

pytestmark = pytest.mark.gpu

FLOATS = ("rebuffer_time", "start_up_time", "average_latency", "variance", "qoe")
INTS = ("episode", "trace_id", "start_offset", "chunks", "done")
RTOL = {"rebuffer_time": 0.0, "start_up_time": 0.0, "variance": 0.0, "average_latency": 1e-9, "qoe": 1e-10}
N_EP = T // V


def variance_in_order(a, ladder=LADDER):
    """sum over the episode of |br[a_c] - br[a_(c+1)]| added in chunk order (Simulator.py:82), a: [n, V]."""
    br = np.asarray(ladder, np.float64)
    v = np.zeros(a.shape[0])
    for c in range(a.shape[1] - 1):
        v = v + np.abs(br[a[:, c]] - br[a[:, c + 1]])
    return v


def expected(oracle, acts, pairs, n_ep=N_EP, episodes=None, **kw):
    """acts [n_steps, n] as the launch reported them; pairs(k) -> (trace ids, offsets) of the lanes' k-th episode.
    Returns dict field -> [n, n_ep]."""
    n = acts.shape[1]
    cfg = oracle.env_cfg(LADDER, L, V, MB, SU, 1.0, W, 1.0)
    out = {k: np.zeros((n, n_ep), np.float64) for k in FLOATS}
    out.update({k: np.zeros((n, n_ep), np.int32) for k in INTS})
    for k in range(n_ep):
        tid, off = pairs(k)
        a = np.ascontiguousarray(acts[k * V:(k + 1) * V].T).astype(np.int32)
        _, _, fin, _ = oracle.env_batch(cfg, kw.get("traces", TRACES), tid, off, a,
                                        **{x: y for x, y in kw.items() if x != "traces"})
        for f in ("rebuffer_time", "start_up_time", "average_latency", "qoe"):
            out[f][:, k] = fin[f]
        out["variance"][:, k] = variance_in_order(a)
        out["episode"][:, k] = k if episodes is None else episodes[k]
        out["trace_id"][:, k], out["start_offset"][:, k] = tid, off
        out["chunks"][:, k], out["done"][:, k] = V, _lib.DONE_EPISODE
    return out


def records(led, n_ep):
    """records() of a ledger whose every lane holds exactly n_ep valid records, as dict field -> [n, n_ep]."""
    rec = {k: v.cpu().numpy() for k, v in led.records().items()}
    n = led.n_lanes
    assert rec["lane"].size == n * n_ep and np.array_equal(rec["lane"], np.repeat(np.arange(n), n_ep))
    return {k: rec[k].reshape(n, n_ep) for k in FLOATS + INTS}


def check_records(got, want, what=""):
    for k in INTS:
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in FLOATS:
        g, w = got[k], want[k]
        err = float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300)))
        print(f"{what} {k}: max relative error {err:.3e} (bound {RTOL[k]:.0e})")
        if RTOL[k] == 0.0:
            assert np.array_equal(g, w), (what, k)
        else:
            assert np.all(np.abs(g - w) <= RTOL[k] * np.abs(w)), (what, k, err)


def check_totals(led, got, want, wrapped=False):
    """total[f] == the in-order sum of the device's own records (when nothing wrapped); against the oracle: exact for
    the exact fields, the field's tolerance times the episode count for the others."""
    tot = {k: v.cpu().numpy() for k, v in led.totals().items()}
    n_ep = want["qoe"].shape[1]
    in_order = lambda x: sum((x[:, e] for e in range(1, x.shape[1])), x[:, 0] + 0.0)
    for k in FLOATS:
        if not wrapped:
            assert np.array_equal(tot[k], in_order(got[k])), ("total in order", k)
        if RTOL[k] == 0.0:
            assert np.array_equal(tot[k], in_order(want[k])), ("total", k)
        else:
            assert np.all(np.abs(tot[k] - in_order(want[k])) <= n_ep * RTOL[k] * in_order(np.abs(want[k]))), ("total", k)


def twin_pairs(smp, n=N, base=0, e0=0):
    g = base + np.arange(n, dtype=np.uint64)
    return lambda k: smp.draw(g, e0 + k, TL)


def script(seed=3, t=T, n=N):
    return np.random.default_rng(seed).integers(0, 6, (t, n)).astype(np.int32)


def run(impl, kind, rows=8, smp=SMP):
    env = armed(make(impl), smp)
    led = env.set_episode_ledger(rows)
    assert env.episode_ledger is led and led.blob.is_cuda and led.blob.data_ptr() % 256 == 0
    if kind == "random":
        acts = env.step_random(T, 77)["actions"].cpu().numpy()
    else:
        acts = script()
        env.step_script(torch.from_numpy(acts).cuda())
    return env, led, acts


_ref = {}


def jump_blob(kind, rows=8):
    if (kind, rows) not in _ref:
        _ref[kind, rows] = run("jump", kind, rows)[1].blob.clone()
    return _ref[kind, rows]


# ---- 1: three records per lane, each equal to the oracle; every impl's blob equal to jump's ----
@pytest.mark.parametrize("kind", ["random", "script"])
@pytest.mark.parametrize("impl", ALL)
def test_three_records_per_lane_equal_the_oracle(oracle, impl, kind):
    env, led, acts = run(impl, kind)
    assert (led.count().cpu().numpy() == 3).all()
    got = records(led, N_EP)
    want = expected(oracle, acts, twin_pairs(SMP))
    check_records(got, want, f"{impl}/{kind}")
    check_totals(led, got, want)
    # non-vacuity: at least two distinct traces among a lane's three records for >= 90 % of the lanes; all 7 occur
    distinct = np.array([len(set(r)) for r in got["trace_id"].tolist()])
    assert (distinct >= 2).mean() >= 0.9 and set(got["trace_id"].ravel().tolist()) == set(range(7))
    assert torch.equal(led.blob, jump_blob(kind)), "the blob differs from the one-thread-per-lane kernel's"
    # 9: a lane's newest record's qoe is episode_qoe(), bit for bit
    assert np.array_equal(got["qoe"][:, -1], env.episode_qoe().cpu().numpy())


# ---- 2: a ring of two keeps episodes 1 and 2; the totals keep everything ----
@pytest.mark.parametrize("impl", ALL)
def test_ring_of_two_keeps_the_last_two_and_all_totals(oracle, impl):
    env, led, acts = run(impl, "random", rows=2)
    assert (led.count().cpu().numpy() == 3).all()
    got = records(led, 2)
    want = expected(oracle, acts, twin_pairs(SMP))
    assert (got["episode"] == np.array([1, 2])).all()
    check_records(got, {k: v[:, 1:] for k, v in want.items()}, f"{impl}/rows2")
    big = A.EpisodeLedger(N, 8, "cuda")
    big.blob.copy_(jump_blob("random"))
    for k in FLOATS:
        assert torch.equal(led.totals()[k], big.totals()[k]), k
    check_totals(led, got, want, wrapped=True)
    ring = led.ring()["episode"].cpu().numpy()
    assert (ring[0] == 2).all() and (ring[1] == 1).all()          # record 2 went to slot 2 % 2 == 0


# ---- 3: one fused launch, T single steps, pieces of 5: identical blobs ----
@pytest.mark.parametrize("impl", ["auto", "split3", "split"])
def test_fused_single_steps_and_pieces_give_identical_blobs(impl):
    acts = script(8)
    a = armed(make(impl), SMP)
    la = a.set_episode_ledger(8)
    a.step_script(torch.from_numpy(acts).cuda())
    b = armed(make(impl), SMP)
    lb = b.set_episode_ledger(8)
    for t in range(T):
        b.step(torch.from_numpy(acts[t]).cuda())
    c = armed(make(impl), SMP)
    lc = c.set_episode_ledger(8)
    for s in range(0, T, 5):
        c.step_script(torch.from_numpy(acts[s:s + 5]).cuda())
    assert (la.count() == 3).all()
    assert torch.equal(la.blob, lb.blob) and torch.equal(la.blob, lc.blob)


# ---- 4: every closed-loop launch kind on every impl that accepts it ----
def _policy(env, **kw):
    rng = np.random.default_rng(5)
    layers, fan = [], 4 + 4 + 6
    for w in (16, 6):
        layers.append((rng.normal(0, 1.5 / np.sqrt(fan), (w, fan)).astype(np.float32), rng.normal(0, 0.2, w).astype(np.float32)))
        fan = w
    return A.PolicyController(A.EnvPlayer(env), layers, window=4, explore=0.25, seed=9, **kw)


CLOSED = ([("rate", i) for i in ("jump", "tick", "auto")] + [("fastmpc", i) for i in ("jump", "tick", "auto")] +
          [(k, i) for k in ("mpc", "robust", "argmax", "softmax") for i in ("jump", "split", "split3", "auto")])


@pytest.mark.parametrize("kind,impl", CLOSED)
def test_closed_loop_launches(oracle, kind, impl):
    env = armed(make(impl), SMP)
    led = env.set_episode_ledger(8)
    if kind == "rate":
        out = env.step_rule(A.RateBasedController(A.EnvPlayer(env), window=3), T)
    elif kind == "fastmpc":
        out = env.step_rule(A.FastMPCController(A.EnvPlayer(env), horizon=3, device="cuda"), T)
    elif kind in ("mpc", "robust"):
        ctl = A.BatchedMPCController(A.EnvPlayer(env), horizon=3, clip_horizon=True,
                                     method="robust" if kind == "robust" else "harmonic")
        out = env.step_mpc(ctl, T)
    else:
        out = env.step_policy(_policy(env, **(dict(sample="softmax", temperature=0.7) if kind == "softmax" else {})), T)
    acts = out["actions"].cpu().numpy()
    assert (out["done"].cpu().numpy() & ~np.uint8(_lib.DONE_EPISODE) == 0).all()
    assert (led.count().cpu().numpy() == 3).all()
    got = records(led, N_EP)
    want = expected(oracle, acts, twin_pairs(SMP))
    check_records(got, want, f"{kind}/{impl}")
    check_totals(led, got, want)
    assert np.array_equal(got["qoe"][:, -1], env.episode_qoe().cpu().numpy())


# ---- 5: explicit pairs without a sampler; a masked reset mid-episode adds no record and leaves a gap ----
@pytest.mark.parametrize("impl", ["jump", "split3", "split", "tick"])
def test_explicit_pairs_and_a_masked_reset(oracle, impl):
    rng = np.random.default_rng(12)
    tid, off = rng.integers(0, 7, N).astype(np.int32), rng.integers(0, 20, N).astype(np.int32)
    tid2, off2 = rng.integers(0, 7, N).astype(np.int32), rng.integers(0, 20, N).astype(np.int32)
    env = make(impl)
    led = env.set_episode_ledger(4)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    a1 = env.step_random(V + 3, 5)["actions"].cpu().numpy()
    assert (led.count().cpu().numpy() == 1).all()
    before = led.blob.clone()
    mask = (np.arange(N) % 3 == 0)
    env.reset(torch.from_numpy(tid2), torch.from_numpy(off2), mask=torch.from_numpy(mask.astype(np.uint8)))
    assert torch.equal(led.blob, before), "a reset touched the ledger"
    a2 = env.step_random(V, 6)["actions"].cpu().numpy()
    assert (led.count().cpu().numpy() == 2).all()
    got = records(led, 2)
    m, u = mask, ~mask
    assert (got["episode"][u] == [0, 1]).all() and (got["episode"][m] == [0, 2]).all()       # episode 1 was abandoned
    # unmasked lanes: two episodes on the reset's pair; the second one's actions span both launches
    acts_u = np.concatenate([a1[:, u], a2[:V - 3, u]])
    want = expected(oracle, acts_u, lambda k: (tid[u], off[u]), n_ep=2)
    check_records({k: v[u] for k, v in got.items()}, want, f"{impl}/unmasked")
    # masked lanes: episode 0 on the first pair, episode 2 on the masked reset's pair, V decisions of the second launch
    want0 = expected(oracle, a1[:V, m], lambda k: (tid[m], off[m]), n_ep=1)
    want2 = expected(oracle, a2[:, m], lambda k: (tid2[m], off2[m]), n_ep=1, episodes=[2])
    check_records({k: v[m][:, :1] for k, v in got.items()}, want0, f"{impl}/masked ep0")
    check_records({k: v[m][:, 1:] for k, v in got.items()}, want2, f"{impl}/masked ep2")


# ---- 6: auto_reset off: one record when the lane finishes, none afterwards ----
@pytest.mark.parametrize("impl", ["jump", "split3", "split", "tick"])
def test_without_auto_reset_one_record(oracle, impl):
    env = A.BatchedABREnv(A.MPD(V, L, MB, SU, A.Chunk(LADDER)), A.QOEMetric(*W), A.NetworkInfo(1.0, TRACES), N,
                          device="cuda", auto_reset=False, impl=impl)
    led = env.set_episode_ledger(3)
    tid = (np.arange(N) % 7).astype(np.int32)
    off = (np.arange(N) % 11).astype(np.int32)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    acts = env.step_random(V + 3, 9)["actions"].cpu().numpy()
    assert (led.count().cpu().numpy() == 1).all()
    got = records(led, 1)
    check_records(got, expected(oracle, acts[:V], lambda k: (tid, off), n_ep=1), f"{impl}/no auto_reset")
    assert np.array_equal(got["qoe"][:, 0], env.episode_qoe().cpu().numpy())
    before = led.blob.clone()
    env.step_random(5, 10)
    env.step(torch.zeros(N, dtype=torch.int32, device="cuda"))
    assert torch.equal(led.blob, before)


# ---- 7: a dead trace times out: exactly one record, once; the live lanes of the same wave are unaffected ----
@pytest.mark.parametrize("impl", ALL)
def test_a_timed_out_lane_records_once(oracle, impl):
    traces = [np.zeros(40), np.random.default_rng(1).uniform(4.0, 8.0, 100)]        # trace 0 never delivers a byte
    env = make(impl, traces=traces, max_ticks=(V + 2) * 400)
    led = env.set_episode_ledger(4)
    tid = (np.arange(N) % 2).astype(np.int32)                                        # dead and live lanes interleaved
    off = (np.arange(N) % 13).astype(np.int32)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    out = np_out(env.step_random(V, 2))
    dead, live = tid == 0, tid == 1
    timed = ((out["done"] & _lib.DONE_TIMEOUT) != 0).any(0)
    assert timed.any() and (~timed).any() and np.array_equal(timed, dead)           # non-vacuity: both kinds occur
    cnt = led.count().cpu().numpy()
    assert (cnt[dead] == 1).all() and (cnt[live] == 1).all()
    ring = {k: v.cpu().numpy() for k, v in led.ring().items()}
    assert (ring["done"][0][dead] == _lib.DONE_TIMEOUT).all() and (ring["chunks"][0][dead] < V).all()
    assert (ring["episode"][0] == 0).all() and np.array_equal(ring["trace_id"][0], tid)
    assert np.array_equal(ring["qoe"][0][dead], env.episode_qoe().cpu().numpy()[dead])
    first = led.blob.clone()
    env.step_random(V, 3)
    env.step_random(3, 4)
    cnt = led.count().cpu().numpy()
    assert (cnt[dead] == 1).all(), "a timed-out lane recorded again"
    assert (cnt[live] == 2).all()
    for k in FLOATS + INTS:                                                          # the dead lanes' record is untouched
        a = A.EpisodeLedger(N, 4, "cuda")
        a.blob.copy_(first)
        assert torch.equal(led.ring()[k][0][torch.from_numpy(dead).cuda()], a.ring()[k][0][torch.from_numpy(dead).cuda()]), k
    # the live lanes: their first episode equals the oracle's, as if the dead lanes were not there
    want = expected(oracle, out["actions"][:, live], lambda k: (tid[live], off[live]), n_ep=1, traces=traces)
    got = {k: ring[k][0][live].reshape(-1, 1) for k in FLOATS + INTS}
    check_records(got, want, f"{impl}/live lanes")


# ---- 8: per-lane speeds, a speed schedule, a speed rule ----
CTL = A.LatencySpeedController((2.0, 6.0), (1.0, 8.0), ((0.9, 1.0, 1.0), (0.9, 1.1, 1.25), (0.75, 1.5, 2.0)))


@pytest.mark.parametrize("impl", ["jump", "split3"])
@pytest.mark.parametrize("feature", ["lanes", "schedule", "rule"])
def test_speed_features(oracle, impl, feature):
    rng = np.random.default_rng(21)
    kw, okw = {}, {}
    if feature == "lanes":
        sp = rng.choice([0.75, 1.0, 1.25, 1.5], N)
        kw, okw = dict(speed=torch.from_numpy(sp)), dict(speeds=sp)
    elif feature == "schedule":
        sp = rng.choice([0.75, 1.0, 1.25, 1.5], (V + 2, N))
        kw, okw = dict(speed=torch.from_numpy(sp)), dict(speeds=np.ascontiguousarray(sp.T))
    else:
        kw, okw = dict(speed=CTL), dict(rule=rule_arrays(CTL))
    env = A.BatchedABREnv(A.MPD(V, L, MB, SU, A.Chunk(LADDER)), A.QOEMetric(*W), A.NetworkInfo(1.0, TRACES), N,
                          device="cuda", auto_reset=True, impl=impl, **kw)
    led = env.set_episode_ledger(4)
    tid, off = rng.integers(0, 7, N).astype(np.int32), rng.integers(0, 20, N).astype(np.int32)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    acts = env.step_random(2 * V + 2, 31)["actions"].cpu().numpy()
    assert (led.count().cpu().numpy() == 2).all()
    got = records(led, 2)
    want = expected(oracle, acts, lambda k: (tid, off), n_ep=2, **okw)
    check_records(got, want, f"{impl}/{feature}")
    check_totals(led, got, want)
    assert np.array_equal(got["qoe"][:, -1], env.episode_qoe().cpu().numpy())


# ---- 10: the ledger changes nothing else ----
@pytest.mark.parametrize("impl", ALL)
def test_outputs_and_workspace_are_identical_with_and_without_a_ledger(impl):
    a = armed(make(impl), SMP)
    b = make(impl)
    b.set_episode_sampler(SMP.seed)
    b.load_state_dict(a.state_dict())     # the same bytes to start from, also in the regions no kernel of this case writes
    assert torch.equal(a.workspace, b.workspace)
    b.set_episode_ledger(8)
    oa, ob = a.step_random(T, 77), b.step_random(T, 77)
    for k in ("obs", "reward", "done", "actions"):
        assert torch.equal(oa[k], ob[k]), k
    assert torch.equal(a.workspace, b.workspace)
    b.set_episode_ledger(None)                                    # off again: nothing more is appended
    assert b.episode_ledger is None
    a.step_random(V, 1), b.step_random(V, 1)
    assert torch.equal(a.workspace, b.workspace)


# ---- 11: shards and checkpoints ----
@pytest.mark.parametrize("impl", ["auto", "split3"])
def test_two_shards_reproduce_the_unsharded_ledger(impl):
    whole = run(impl, "random")[1]
    for base, n in ((0, 120), (120, 80)):
        sh = A.ShardedABREnv(A.MPD(V, L, MB, SU, A.Chunk(LADDER)), A.QOEMetric(*W), A.NetworkInfo(1.0, TRACES),
                             total_lanes=n, device="cuda", rank=0, world=1, gather=False, env=make(impl, n=n, base=base))
        sh.set_episode_sampler(SMP.seed)
        led = sh.set_episode_ledger(8)
        assert sh.episode_ledger is led and led.n_lanes == n
        sh.reset(sample=True)
        sh.env.step_random(T, 77)
        assert torch.equal(led.count(), whole.count()[base:base + n])
        for k in FLOATS:
            assert torch.equal(led.totals()[k], whole.totals()[k][base:base + n]), k
        for k in FLOATS + INTS:
            assert torch.equal(led.ring()[k], whole.ring()[k][:, base:base + n]), k


def test_checkpoint_mid_rollout_continues_to_the_same_blob():
    a = armed(make(), SMP)
    la = a.set_episode_ledger(2)
    a.step_random(V + 3, 11)
    sd, lsd = a.state_dict(), la.state_dict()
    a.step_random(T, 12)
    b = make()
    b.set_episode_sampler(SMP.seed)
    lb = b.set_episode_ledger(2)
    b.load_state_dict(sd)
    lb.load_state_dict(lsd)
    b.step_random(T, 12)
    assert (la.count() == 4).all() and torch.equal(la.blob, lb.blob)
    # clear() empties it; an installed EpisodeLedger can be handed over as it is
    lb.clear()
    assert not lb.blob.any()
    c = armed(make(), SMP)
    assert c.set_episode_ledger(lb) is lb
    c.step_random(V, 1)
    assert (lb.count() == 1).all()


# ---- 12: refusals ----
def test_refusals():
    env = armed(make(), SMP)
    with pytest.raises(ValueError):
        env.set_episode_ledger(0)
    with pytest.raises(ValueError):
        env.set_episode_ledger(A.EpisodeLedger(N + 1, 2, "cuda"))
    lib = env.lib
    led = A.EpisodeLedger(N, 2, "cuda")
    for st, word in ((_lib.EpisodeLedger(base_dev=led.blob.data_ptr(), rows=0), b"rows"),
                     (_lib.EpisodeLedger(base_dev=None, rows=2), b"NULL"),
                     (_lib.EpisodeLedger(base_dev=led.blob.data_ptr() + 64, rows=2), b"aligned")):
        assert lib.abr_env_set_episode_ledger(env._h, C.byref(st)) == -1 and word in lib.abr_last_error()
    env.step_random(V, 1)                                          # nothing was stored: nothing is appended
    assert not led.blob.any()
    assert env.episode_ledger is None
