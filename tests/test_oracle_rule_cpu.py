"""The C oracle's speed-rule mode (oracle/abr_oracle.c: oracle_speed_rule; oracle.env_batch(rule=...)) against the tick-loop twin
(tests/speed_twin.py: RuleTickEnv, itself pinned to the reference through oracle/pyloop.py), bit for bit: every call-site
frame, the measured throughputs, the final state and every logged answer, on seeded cases with and without per-chunk
ladders.  The existing modes are unchanged (tests/test_oracle_golden.py)."""
import numpy as np
import pytest

from oracle import oracle as O
from helpers import oracle_env_cfg
from speed_twin import RuleTickEnv

STEP = ("global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level", "average_latency",
        "play_length", "play_id", "chunk_id", "last_bitrate", "last_bandwidth")
FINAL = ("global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level", "average_latency", "play_id",
         "chunk_id")


class _Row:
    """A per-chunk ladder as PyTickEnv reads it (ladder[action] at the downloading chunk)."""

    def __init__(self, env, table):
        self.env, self.table = env, table

    def __getitem__(self, a):
        return self.table[self.env.chunk][a]


def _case(seed):
    rng = np.random.default_rng(4100 + seed)
    L = float(rng.choice([1.0, 2.0, 4.0]))
    B = int(rng.integers(1, 7))
    ladder = np.sort(rng.uniform(0.2, 6.0, B)).round(3).tolist()
    V = int(rng.integers(2, 14))
    mb = float(rng.choice([L * 0.6, L * 1.5, L * 3, 20.0]))
    meta = dict(ladder=ladder, chunk_length=L, video_length=V, max_buffer=mb,
                start_up_length=float(min(mb, rng.choice([0.0, L, 1.7]))),
                interval=float(rng.choice([0.05, 0.3, 1.0, 3.7])), weights=[4.3, 1.0, 1.0, 0.1])
    br = None
    if seed % 2:
        br = np.sort(np.tile(ladder, (V, 1)) * rng.uniform(0.7, 1.3, (V, B)), axis=1)
    traces = [rng.uniform(0.5, 12.0, int(n)) for n in rng.integers(30, 400, 3)]
    N = 9
    tid = rng.integers(0, 3, N).astype(np.int32)
    off = np.array([rng.integers(0, len(traces[t])) for t in tid], np.int32)
    acts = rng.integers(0, B, (N, V)).astype(np.int32)
    nl, nb = int(rng.integers(0, 5)), int(rng.integers(0, 5))
    lat = np.sort(rng.choice(np.arange(0.25, 9.0, 0.25), nl, replace=False))
    buf = np.sort(rng.choice(np.arange(0.25, mb + 0.5, 0.25), min(nb, len(np.arange(0.25, mb + 0.5, 0.25))),
                             replace=False))
    sp = rng.choice([0.5, 0.75, 0.9, 1.0, 1.1, 1.25, 1.5, 2.0], (nl + 1, len(buf) + 1))
    return meta, br, traces, tid, off, acts, (lat, buf, sp)


def _twin(meta, br, trace, off, acts, rule):
    env = RuleTickEnv(meta["ladder"], meta["chunk_length"], meta["video_length"], meta["max_buffer"],
                      meta["start_up_length"], meta["interval"], meta["weights"], list(trace), int(off), rule=rule)
    if br is not None:
        env.ladder = _Row(env, br)
    frames = [dict(env.reset(), play_length=env.play_len)]
    for a in acts:
        o, over = env.step(int(a))
        if not over:
            frames.append(dict(o, play_length=env.play_len))
    return env, frames


@pytest.mark.parametrize("seed", range(16))
def test_rule_mode_equals_the_tick_loop_twin(seed):
    meta, br, traces, tid, off, acts, rule = _case(seed)
    N, V = acts.shape
    rows = V + 3
    log = np.full((N, rows), -7.0)
    calls = np.zeros(N, np.int32)
    steps, bw, fin, _ = O.env_batch(oracle_env_cfg(O, meta, br_table=br), traces, tid, off, acts, rule=rule,
                                    speed_log_out=log, speed_calls_out=calls, threads=3 if seed % 3 == 0 else 1)
    for i in range(N):
        env, frames = _twin(meta, br, traces[tid[i]], off[i], acts[i], rule)
        assert len(frames) == V
        for s, f in enumerate(frames):
            for k in STEP:
                assert steps[k][i, s] == f[k], (seed, i, s, k)
        fo = env._obs()
        for k in FINAL:
            assert fin[k][i] == fo[k], (seed, i, k)
        assert fin["ticks"][i] == env.ticks
        assert np.array_equal(bw[i], env.hist_bw)
        if br is None:
            assert fin["qoe"][i] == env.qoe()
        assert calls[i] == len(env.log)
        k = min(len(env.log), rows)
        assert np.array_equal(log[i, :k], env.log[:k]) and (log[i, k:] == -7.0).all(), (seed, i)


def test_rule_mode_plays_more_than_one_speed_and_logs_are_optional():
    seen = set()
    for seed in range(16):
        meta, br, traces, tid, off, acts, rule = _case(seed)
        log = np.zeros((len(tid), meta["video_length"] + 3))
        O.env_batch(oracle_env_cfg(O, meta, br_table=br), traces, tid, off, acts, rule=rule, speed_log_out=log)
        seen |= set(np.unique(log[log != 0]).tolist())
        a = O.env_batch(oracle_env_cfg(O, meta, br_table=br), traces, tid, off, acts, rule=rule)
        b = O.env_batch(oracle_env_cfg(O, meta, br_table=br), traces, tid, off, acts, rule=rule, speed_log_out=log)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert len(seen) >= 4


def test_a_constant_rule_is_the_constant_speed():
    """A rule with one cell is config.speed at that value: the rule mode changes nothing else."""
    meta, br, traces, tid, off, acts, _ = _case(3)
    for v in (0.75, 1.0, 1.25):
        cfg = oracle_env_cfg(O, dict(meta, speed=v), br_table=br)
        a = O.env_batch(cfg, traces, tid, off, acts)
        b = O.env_batch(cfg, traces, tid, off, acts, rule=((), (), ((v,),)))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
