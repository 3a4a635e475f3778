"""The trace generator on the device (include/abr_env.h: abr_trace_synth; csrc/abr_env.hip: trace_synth_kernel): every
sample bit for bit the numpy twin's (tests/trace_synth_twin.py) over ragged, non-adjacent, sentinel-padded rows; sub-ranges
and in-place output; and the environment on a regenerated corpus -- every kernel replayed episode by episode through the
oracle on the twin's traces, the learned policy's actions from the policy twin, and stream order."""
import numpy as np
import pytest
import torch

import trace_synth_twin as twin
from helpers import oracle_rewards
from sampler_twin import twin as sampler_twin
import abrsimulator_amd as A
from abrsimulator_amd import _lib

pytestmark = pytest.mark.gpu

BIG = 2 ** 32 + 5
SENT = -7.25                     # no sample is negative
LENGTH_SET = [1, 2, 63, 64, 65, 128, 129, 200, 1000]


def models():
    return {1: A.TraceModel([3.0], spread=0.5),
            3: A.TraceModel([0.4, 2.0, 5.0], spread=[0.0, 0.3, 1.0], stay=0.7, outage=[0.3, 0.0, 0.05], initial=[0.2, 0.5, 0.3]),
            8: A.TraceModel(np.linspace(0.2, 6.0, 8), spread=0.25, stay=0.6, outage=0.02)}


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def padded_layout(lengths, rng):
    """Offsets of rows laid out in a shuffled order with 1..5 untouched doubles before, between and after them (rows are
    8-byte aligned only and not adjacent); a row of length 0 still gets a slot, which must stay untouched."""
    n = len(lengths)
    off = np.zeros(n, np.int64)
    pos = int(rng.integers(1, 6))
    for t in rng.permutation(n):
        off[t] = pos
        pos += max(int(lengths[t]), 3) + int(rng.integers(1, 6))
    return off, pos


def run_padded(model, lengths, seed, gen, base, rng):
    off, total = padded_layout(lengths, rng)
    flat = torch.full((total,), SENT, dtype=torch.float64, device="cuda")
    out = (flat, torch.from_numpy(off).cuda(), torch.from_numpy(np.asarray(lengths, np.int32)).cuda())
    ptr = flat.data_ptr()
    got = A.synth_traces(model, None, seed, generation=gen, trace_id_base=base, out=out)
    assert got[0] is flat and flat.data_ptr() == ptr
    return flat.cpu().numpy(), off


def check_padded(model, lengths, seed, gen, base, rng):
    got, off = run_padded(model, lengths, seed, gen, base, rng)
    want = np.full(got.shape, SENT)
    for t, row in enumerate(twin.corpus(twin.from_package(model), seed, gen, lengths, base)):
        want[off[t]:off[t] + len(row)] = row
    assert np.array_equal(bits(got), bits(want)), (len(lengths), gen, base, np.flatnonzero(bits(got) != bits(want))[:8])


@pytest.mark.parametrize("n_traces", [1, 3, 4, 5, 9, 257])
def test_device_equals_the_twin(n_traces):
    rng = np.random.default_rng(100 + n_traces)
    ms = models()
    combos = [(0, 0), (1, BIG)] if n_traces == 257 else [(0, 0), (0, BIG), (1, 0), (2 ** 32 - 1, BIG)]
    for K in (1, 3, 8):
        lengths = rng.choice(LENGTH_SET, n_traces)
        if n_traces >= 9:
            lengths[:9] = rng.permutation(LENGTH_SET)            # every length of the set at least once
        if n_traces >= 3:
            lengths[1] = 0                                       # a trace of device length 0 is skipped
        for gen, base in combos:
            check_padded(ms[K], lengths, 0xC0FFEE + K, gen, base, rng)
    a, _ = run_padded(ms[3], [200], 5, 0, 0, np.random.default_rng(1))
    b, _ = run_padded(ms[3], [200], 5, 1, 0, np.random.default_rng(1))
    assert not np.array_equal(a, b)                              # another generation is another corpus


def test_more_traces_than_waves_in_the_grid_take_the_stride():
    """The launch is capped at 2 048 workgroups of four waves: with more than 8 192 traces every wave of the grid
    walks more than one trace (the stride).  (At 7 waves per SIMD 7 168 of those waves are resident at a time.)"""
    rng = np.random.default_rng(7)
    n = 8192 + 4 * 37 + 3
    lengths = rng.choice([1, 2, 3, 65], n, p=[0.4, 0.3, 0.25, 0.05])
    lengths[rng.integers(0, n, 20)] = 0
    check_padded(models()[3], lengths, 99, 3, BIG, rng)


def test_sub_range_equals_the_whole_and_out_fills_in_place():
    model = models()[8]
    lengths = np.random.default_rng(3).choice(LENGTH_SET, 40)
    flat, off, lens = A.synth_traces(model, lengths, 42, generation=6)
    assert flat.dtype == torch.float64 and off.dtype == torch.int64 and lens.dtype == torch.int32 and flat.is_cuda
    assert np.array_equal(lens.cpu().numpy(), lengths) and np.array_equal(off.cpu().numpy(), np.cumsum(lengths) - lengths)
    whole = flat.cpu().numpy()
    want = np.concatenate(twin.corpus(twin.from_package(model), 42, 6, lengths))
    assert np.array_equal(bits(whole), bits(want))
    a, b = 11, 29
    sub = A.synth_traces(model, lengths[a:b], 42, generation=6, trace_id_base=a)[0].cpu().numpy()
    o = np.cumsum(lengths) - lengths
    assert np.array_equal(bits(sub), bits(whole[o[a]:o[b]]))
    # out=: the same tensors, filled in place
    out = (torch.zeros_like(flat), off, lens)
    p = out[0].data_ptr()
    got = A.synth_traces(model, None, 42, generation=6, out=out)
    assert all(x is y for x, y in zip(got, out)) and out[0].data_ptr() == p and torch.equal(out[0], flat)
    with pytest.raises(ValueError):
        A.synth_traces(model, None, 42, out=(flat.cpu(), off, lens))
    with pytest.raises(ValueError):
        A.synth_traces(model, [5, 0, 3], 42)
    with pytest.raises(ValueError):
        A.synth_traces(model, [5], 42, trace_id_base=-1)


# ---------------------------------------------------------------------------------------------------------------------
# the environment reads what was generated

LADDER, V, L, MB, SU, W, N = twin.ENV_LADDER, twin.ENV_V, twin.ENV_L, twin.ENV_MB, twin.ENV_SU, twin.ENV_W, twin.ENV_N
T = 3 * V + 3
TL = np.asarray(twin.ENV_LENGTHS, np.int32)
OBS = _lib.OBS_ROWS
SMP_SEED = 0x5EED_0F_EB150DE5


def env_model():
    return A.TraceModel(**twin.ENV_MODEL)


_corpora = {}


def twin_traces(gen):
    if gen not in _corpora:
        _corpora[gen] = twin.corpus(twin.from_package(env_model()), twin.ENV_SEED, gen, twin.ENV_LENGTHS)
    return _corpora[gen]


def make(impl="auto", n=N):
    """The environment over a white-noise corpus of the right lengths: what synth_traces then overwrites."""
    rng = np.random.default_rng(0)
    traces = [rng.uniform(0.3, 6.0, int(k)) for k in twin.ENV_LENGTHS]
    return A.BatchedABREnv(A.MPD(V, L, MB, SU, A.Chunk(LADDER)), A.QOEMetric(*W), A.NetworkInfo(1.0, traces), n,
                           device="cuda", auto_reset=True, impl=impl)


def np_out(out):
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def replay_mismatches(oracle, out, traces, e0):
    """Names of the outputs that differ from the oracle's replay, episode by episode, of fused decisions that start at
    chunk 0 of episode e0 on `traces` and the sampler twin's pairs; also asserts that no episode of the replay comes near
    the tick bound."""
    acts, rew, done, obs = out["actions"], out["reward"], out["done"], out["obs"]
    n_steps, n = rew.shape
    g = np.arange(n, dtype=np.uint64)
    cfg = oracle.env_cfg(LADDER, L, V, MB, SU, 1.0, W, 1.0)
    n_ep = -(-n_steps // V)
    reps, bad = [], set()
    for k in range(n_ep + 1):
        tid, off = sampler_twin(SMP_SEED, g, np.full(n, e0 + k), TL)
        s0, m = k * V, max(0, min(V, n_steps - k * V))
        a = np.zeros((n, V), np.int32)
        a[:, :m] = np.clip(acts[s0:s0 + m].T, 0, len(LADDER) - 1)
        steps, _, fin, _ = oracle.env_batch(cfg, traces, tid, off, a)
        assert fin["ticks"].max() < twin.ENV_MAX_TICKS
        reps.append((s0, m, a, steps, fin))
    for k in range(n_ep):
        s0, m, a, steps, fin = reps[k]
        rw = oracle_rewards(steps, fin, a, W, ladder=LADDER)
        for s in range(m):
            t = s0 + s
            if not np.array_equal(rew[t], rw[:, s]):
                bad.add("reward")
            if not np.array_equal(done[t], np.full(n, 1 if s == V - 1 else 0, np.uint8)):
                bad.add("done")
            nxt, col = (reps[k][3], s + 1) if s < V - 1 else (reps[k + 1][3], 0)
            for r, key in enumerate(OBS):
                if not np.array_equal(obs[t, r], nxt[key][:, col].astype(np.float32)):
                    bad.add("obs." + key)
    return sorted(bad)


@pytest.mark.parametrize("impl", ["auto", "jump", "split", "split3", "tick"])
def test_env_rolls_out_on_the_generated_corpus(oracle, impl):
    env, model = make(impl), env_model()
    env.synth_traces(model, twin.ENV_SEED, 1)
    assert np.array_equal(bits(env.traces.cpu().numpy()), bits(np.concatenate(twin_traces(1))))
    env.set_episode_sampler(SMP_SEED)
    env.reset(sample=True)
    e0 = env.episodes()["episode"].cpu().numpy()
    assert (e0 == e0[0]).all()
    out = np_out(env.step_random(T, 77))
    assert (out["done"] & ~np.uint8(_lib.DONE_EPISODE) == 0).all(), "a lane timed out or was frozen"
    assert replay_mismatches(oracle, out, twin_traces(1), int(e0[0])) == []
    # the same handle on generation 2
    env.synth_traces(model, twin.ENV_SEED, 2)
    assert np.array_equal(bits(env.traces.cpu().numpy()), bits(np.concatenate(twin_traces(2))))
    env.reset(sample=True)
    e1 = env.episodes()["episode"].cpu().numpy()
    assert (e1 == e1[0]).all() and e1[0] > e0[0]
    out = np_out(env.step_random(T, 78))
    assert (out["done"] & ~np.uint8(_lib.DONE_EPISODE) == 0).all()
    assert replay_mismatches(oracle, out, twin_traces(2), int(e1[0])) == []
    assert "reward" in replay_mismatches(oracle, out, twin_traces(1), int(e1[0]))         # not the old corpus


def policy_case(gen):
    import closed_loop_check as K
    for s in range(10_000):
        case = K.make_episode_case(s, N)
        if (case["ctl"], case["feature"], case["mode"]) == ("policy", "config", "sampled"):
            break
    case["meta"].update(ladder=LADDER, chunk_length=L, video_length=V, max_buffer=MB, start_up_length=SU, interval=1.0,
                        weights=W, speed=1.0)
    case.update(traces=twin_traces(gen), br=None, vbr=False, impl="jump", auto_reset=True, lane_id_base=0,
                tid=np.zeros(N, np.int32), off=np.zeros(N, np.int32), sampler=dict(seed=SMP_SEED, pool=None, span=0),
                ops=[("reset", None, None, None), ("launch", V + 3), ("launch", T - V - 3)], n_steps=T,
                max_ticks=twin.ENV_MAX_TICKS)
    case["params"] = K.policy_params(np.random.default_rng(5), case, 4, [16], 0.25)
    return case


def test_step_policy_on_a_regenerated_corpus(oracle):
    """The lane engine's actions are the policy twin's, driven through the oracle on the twin's generation-2 traces
    (tests/closed_loop_check.py: check_episodes): the corpus was regenerated twice before the rollout."""
    import closed_loop_check as K
    case = policy_case(2)
    p = case["params"]
    env, model = make("jump"), env_model()
    env.synth_traces(model, twin.ENV_SEED, 1)
    env.synth_traces(model, twin.ENV_SEED, 2)
    env.set_episode_sampler(SMP_SEED)
    ctl = A.PolicyController(A.EnvPlayer(env), p["layers"], window=p["window"], norm=(p["norm"][0], p["norm"][1]),
                             explore=p["explore"], seed=p["seed"])
    parts, frames, episodes = [], [], []
    for op in case["ops"]:
        if op[0] == "reset":
            env.reset(sample=True)
        else:
            o = env.step_policy(ctl, op[1])
            parts.append({k: o[k].cpu().numpy() for k in ("actions", "reward", "done", "obs")})
        frames.append({k: v.cpu().numpy().copy() for k, v in env.observe_f64().items()})
        episodes.append({k: v.cpu().numpy().copy() for k, v in env.episodes().items()})
    out = {k: np.concatenate([q[k] for q in parts]) for k in ("actions", "reward", "done", "obs")}
    out.update(frames=frames, episodes=episodes, speed_logs=None, entries=None,
               history=tuple(x.cpu().numpy().copy() for x in env.history()), qoe=env.episode_qoe().cpu().numpy())
    stats = {}
    mm = K.check_episodes(case, out, stats)
    assert not mm, (len(mm), mm[:6])
    assert len(stats["answers"]["policy"]) >= 3
    assert K.check_episodes(policy_case(1), out, {})                                      # not generation 1's traces


def test_two_shards_regenerate_the_same_corpus_and_reproduce_the_unsharded_env():
    """ShardedABREnv.synth_traces: every shard generates the whole corpus itself (no collective), so two shards of one
    GPU reproduce their slices of the unsharded environment on the regenerated corpus."""
    model = env_model()
    whole = make("auto")
    whole.synth_traces(model, twin.ENV_SEED, 1)
    whole.set_episode_sampler(SMP_SEED)
    whole.reset(sample=True)
    want = np_out(whole.step_random(T, 4))
    for base, n in ((0, 120), (120, 80)):
        rng = np.random.default_rng(0)
        traces = [rng.uniform(0.3, 6.0, int(k)) for k in twin.ENV_LENGTHS]
        env = A.BatchedABREnv(A.MPD(V, L, MB, SU, A.Chunk(LADDER)), A.QOEMetric(*W), A.NetworkInfo(1.0, traces), n,
                              device="cuda", auto_reset=True, impl="auto", lane_id_base=base)
        sh = A.ShardedABREnv(A.MPD(V, L, MB, SU, A.Chunk(LADDER)), A.QOEMetric(*W), A.NetworkInfo(1.0, traces),
                             total_lanes=n, device="cuda", rank=0, world=1, gather=False, env=env)
        sh.synth_traces(model, twin.ENV_SEED, 1)
        assert np.array_equal(bits(sh.env.traces.cpu().numpy()), bits(np.concatenate(twin_traces(1))))
        sh.set_episode_sampler(SMP_SEED)
        sh.reset(sample=True)
        got = np_out(sh.env.step_random(T, 4))
        for k in ("reward", "done", "obs", "actions"):
            assert np.array_equal(got[k], want[k][..., base:base + n]), (base, k)


def test_stream_order_needs_no_host_synchronisation():
    model = env_model()
    want = None
    for sync in (True, False):
        env = make("auto")
        env.set_episode_sampler(SMP_SEED)
        out = env._rollout_out(T)
        torch.cuda.synchronize()
        for gen in (1, 2):
            env.synth_traces(model, twin.ENV_SEED, gen)
            if sync:
                torch.cuda.synchronize()
            env.reset(sample=True)
            if sync:
                torch.cuda.synchronize()
            env.step_random(T, 5 + gen, out=out)
            if sync:
                torch.cuda.synchronize()
        got = np_out(out)
        got["traces"] = env.traces.cpu().numpy()
        if want is None:
            want = got
    for k in want:
        assert np.array_equal(want[k], got[k]), k
    assert np.array_equal(bits(got["traces"]), bits(np.concatenate(twin_traces(2))))
