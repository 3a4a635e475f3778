"""The closed-loop speed rule (include/abr_env.h: abr_speed_rule) without a GPU.

- The tick-loop twin (tests/speed_twin.py) is pinned to the C oracle: a constant table is the constant speed, and the
  twin's logged answers replayed as a speed schedule give the twin's frames.
- The event-driven lane step with the rule, compiled for the host from the kernels' own source
  (tests/native/speed_rule_harness.cpp), matches the twin bit for bit, log included.
- The ctypes mirror of the struct, and every refusal of abr_env_set_speed_rule that needs no handle."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers import native_harness
from speed_twin import rule_np, twin_batch

LADDER = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
ABR_E_INVALID = -1           # include/abr_env.h


@pytest.fixture(scope="module")
def H():
    lib = native_harness("speed_rule_harness")
    lib.sr_batch.restype = C.c_int64
    return lib


def _struct(lat_thr, buf_thr, speeds):
    from abrsimulator_amd import _lib
    r = _lib.SpeedRule()
    r.n_lat, r.n_buf = len(lat_thr), len(buf_thr)
    for q, t in enumerate(lat_thr):
        r.lat_thr[q] = t
    for q, t in enumerate(buf_thr):
        r.buf_thr[q] = t
    for i, row in enumerate(np.asarray(speeds)):
        for j, v in enumerate(row):
            r.speed[i][j] = float(v)
    return r


def _P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def harness_batch(H, meta, traces, trace_id, offset, actions, rule, log_rows):
    from oracle.oracle import pack_traces
    V = meta["video_length"]
    max_ticks = int(64 * V * np.ceil(meta["chunk_length"] / 0.01))
    flat, off, lens = pack_traces(traces)
    trace_id = np.ascontiguousarray(trace_id, np.int32)
    offset = np.ascontiguousarray(offset, np.int32)
    actions = np.ascontiguousarray(actions, np.int32)
    N = actions.shape[0]
    rec = np.zeros((N, V, 7)); bw = np.zeros((N, V)); fin = np.zeros((N, 7)); fin_n = np.zeros((N, 2), np.int64)
    log = np.full((N, log_rows), np.nan)
    ladder = np.asarray(meta["ladder"], np.float64)
    rc = H.sr_batch(C.byref(_struct(*rule)), C.c_double(meta["interval"]), C.c_double(meta["chunk_length"]),
                    C.c_int32(V), C.c_double(meta["max_buffer"]), C.c_double(meta["start_up_length"]),
                    C.c_int32(max_ticks), _P(ladder, C.c_double), _P(flat, C.c_double), _P(off, C.c_int64),
                    _P(lens, C.c_int32), _P(trace_id, C.c_int32), _P(offset, C.c_int32), _P(actions, C.c_int32),
                    C.c_int32(N), _P(rec, C.c_double), _P(bw, C.c_double), _P(fin, C.c_double),
                    _P(fin_n, C.c_int64), _P(log, C.c_double), C.c_int32(log_rows))
    assert rc == 0, rc
    return rec, bw, fin, fin_n, log


def workload(seed, N, V=10, L=4.0, interval=1.0, max_buffer=20.0, start_up=8.0, bw=(0.2, 6.0), n_traces=8,
             round_bw=False):
    rng = np.random.default_rng(seed)
    if round_bw:
        traces = [rng.choice([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], 600) for _ in range(n_traces)]
    else:
        traces = [rng.uniform(bw[0], bw[1], 600).astype(np.float32).astype(np.float64) for _ in range(n_traces)]
    meta = dict(ladder=LADDER, chunk_length=L, video_length=V, max_buffer=max_buffer, start_up_length=start_up,
                interval=interval, weights=[4.3, 1, 1, 0.1])
    trace_id = rng.integers(0, n_traces, N).astype(np.int32)
    offset = rng.integers(0, 600, N).astype(np.int32)
    actions = rng.integers(0, len(LADDER), (N, V)).astype(np.int32)
    return meta, traces, trace_id, offset, actions


def random_rule(rng, lat_grid=(0.0, 0.5, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0), buf_grid=(0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 12.0)):
    """Thresholds on a grid of round values (latencies and buffer levels land on them exactly: sums of 0.01 and of
    chunk lengths), speeds that change every chunk."""
    nl, nb = int(rng.integers(0, 5)), int(rng.integers(0, 5))
    lat = np.sort(rng.choice(lat_grid, nl, replace=False)).astype(np.float64)
    buf = np.sort(rng.choice(buf_grid, nb, replace=False)).astype(np.float64)
    sp = rng.choice([0.5, 0.75, 0.8, 0.9, 1.0, 1.1, 1.25, 1.5, 2.0, 0.9173], (nl + 1, nb + 1))
    return lat, buf, sp


def oracle_cfg(oracle, meta, speed=1.0):
    return oracle.env_cfg(meta["ladder"], meta["chunk_length"], meta["video_length"], meta["max_buffer"],
                          meta["start_up_length"], meta["interval"], meta["weights"], speed)


FRAME = ["global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level"]


def check_against_oracle(steps, final, bws, steps_o, bw_o, fin_o):
    for k in FRAME + ["play_id", "last_bandwidth"]:
        assert np.array_equal(steps[k], steps_o[k]), k
    assert np.array_equal(bws, bw_o)
    for k in FRAME + ["play_id"]:
        assert np.array_equal(final[k], fin_o[k]), k
    assert np.allclose(final["average_latency"], fin_o["average_latency"], rtol=1e-12)
    assert np.allclose(final["qoe"], fin_o["qoe"], rtol=1e-12)


# ---- the twin against the pinned oracle ----

@pytest.mark.parametrize("s", [1.0, 0.8, 1.25])
def test_twin_with_a_constant_table_is_the_constant_speed(oracle, s):
    meta, traces, trace_id, offset, actions = workload(3, 120)
    rule = (np.array([1.0, 4.0]), np.array([2.0]), np.full((3, 2), s))
    steps, final, bws, log, n_ans = twin_batch(meta, traces, trace_id, offset, actions, rule, 16)
    steps_o, bw_o, fin_o, _ = oracle.env_batch(oracle_cfg(oracle, meta, s), traces, trace_id, offset, actions)
    check_against_oracle(steps, final, bws, steps_o, bw_o, fin_o)
    assert np.all(log[~np.isnan(log)] == s)


@pytest.mark.parametrize("seed", [41, 42, 43])
def test_twin_log_replayed_as_a_schedule_through_the_oracle(oracle, seed):
    rng = np.random.default_rng(seed)
    meta, traces, trace_id, offset, actions = workload(seed, 150, V=12, max_buffer=float(rng.choice([20.0, 6.0])),
                                                       start_up=float(rng.choice([8.0, 2.0])))
    rows = meta["video_length"] + 4
    rule = random_rule(rng)
    steps, final, bws, log, n_ans = twin_batch(meta, traces, trace_id, offset, actions, rule, rows)
    assert n_ans.max() <= rows
    sched = np.where(np.isnan(log), 1.0, log)            # rows past the last answer are never asked for
    steps_o, bw_o, fin_o, _ = oracle.env_batch(oracle_cfg(oracle, meta), traces, trace_id, offset, actions,
                                               speeds=sched)
    check_against_oracle(steps, final, bws, steps_o, bw_o, fin_o)


# ---- the host build of the kernels' source against the twin ----

def test_rule_eval_host_build_matches_numpy(H):
    rng = np.random.default_rng(7)
    for _ in range(200):
        lat_thr, buf_thr, sp = random_rule(rng)
        n = 2000
        # half the inputs exactly on a threshold, the rest around them and far off
        pool_l = np.concatenate([lat_thr, np.nextafter(lat_thr, -np.inf), np.nextafter(lat_thr, np.inf),
                                 [-1.0, 0.0, 100.0]])
        pool_b = np.concatenate([buf_thr, np.nextafter(buf_thr, -np.inf), np.nextafter(buf_thr, np.inf),
                                 [0.0, 30.0]])
        lat = np.where(rng.random(n) < 0.5, rng.choice(pool_l, n), rng.uniform(-1, 10, n))
        buf = np.where(rng.random(n) < 0.5, rng.choice(pool_b, n), rng.uniform(0, 25, n))
        out = np.zeros(n)
        H.sr_eval(C.byref(_struct(lat_thr, buf_thr, sp)), _P(lat, C.c_double), _P(buf, C.c_double),
                  C.c_int64(n), _P(out, C.c_double))
        assert np.array_equal(out, rule_np(lat_thr, buf_thr, sp, lat, buf))


# workloads: thresholds hit exactly, speeds that change every chunk, start-up exit (start_up 0 / 2 / 8), rebuffering
# (starved traces), buffer_full gating (small max_buffer, fast traces), round bandwidths (knife edges)
HARNESS_CASES = [
    dict(seed=51, N=500, rule=(np.array([2.0, 4.0]), np.array([1.0, 8.0]), [[0.9, 1.0, 1.0], [0.9, 1.1, 1.25],
                                                                         [0.75, 1.5, 2.0]])),
    dict(seed=52, N=400, rule="random", max_buffer=6.0, start_up=2.0, bw=(2.0, 12.0)),
    dict(seed=53, N=400, rule="random", bw=(0.1, 1.5), interval=0.3),
    dict(seed=54, N=400, rule="random", L=2.0, max_buffer=4.0, start_up=0.0, round_bw=True),
    dict(seed=55, N=300, rule="random", L=1.0, start_up=1.0, V=20, interval=0.5),
    dict(seed=56, N=300, rule=(np.array([]), np.array([0.5, 1.0, 2.0, 4.0]), [[0.5, 0.8, 1.0, 1.25, 2.0]]),
         max_buffer=9.0, start_up=4.0, round_bw=True),
    dict(seed=57, N=300, rule=(np.array([0.5, 1.0, 2.0, 8.0]), np.array([]), [[0.5], [0.9173], [1.1], [1.5], [2.0]])),
]


@pytest.mark.parametrize("case", HARNESS_CASES, ids=lambda c: str(c["seed"]))
def test_host_lane_step_with_rule_matches_twin(H, case):
    case = dict(case)
    seed, N, rule = case.pop("seed"), case.pop("N"), case.pop("rule")
    rng = np.random.default_rng(seed)
    fixed = not isinstance(rule, str)
    if not fixed:
        rule = random_rule(rng)
    rule = (np.asarray(rule[0], np.float64), np.asarray(rule[1], np.float64), np.asarray(rule[2], np.float64))
    meta, traces, trace_id, offset, actions = workload(seed, N, **case)
    rows = meta["video_length"] + 4
    steps, final, bws, log, n_ans = twin_batch(meta, traces, trace_id, offset, actions, rule, rows)
    rec, bw, fin, fin_n, hlog = harness_batch(H, meta, traces, trace_id, offset, actions, rule, rows)
    for c, k in enumerate(FRAME):
        bad = np.argwhere(rec[:, :, c] != steps[k])
        assert bad.size == 0, (k, bad[:3])
        assert np.array_equal(fin[:, c], final[k]), k
    assert np.array_equal(rec[:, :, 5], steps["last_bandwidth"])
    assert np.array_equal(rec[:, :, 6], steps["play_id"])
    assert np.array_equal(fin[:, 6], final["play_id"])
    assert np.array_equal(bw, bws)
    assert np.array_equal(np.isnan(hlog), np.isnan(log)) and np.array_equal(hlog[~np.isnan(log)], log[~np.isnan(log)])
    # average_latency from the carried sums ((dt * sumk - pt_sum) / play_time)
    lat = (0.01 * fin_n[:, 1].astype(np.float64) - fin[:, 5]) / fin[:, 3]
    assert np.allclose(lat, final["average_latency"], rtol=1e-9)
    if fixed:                                             # the hand-made tables are reached in more than one cell
        assert len(np.unique(log[~np.isnan(log)])) >= 2


# ---- the C ABI without a GPU ----

def test_struct_layout_matches_header():
    from abrsimulator_amd import _lib
    S = _lib.SpeedRule
    assert C.sizeof(S) == 272
    assert S.n_lat.offset == 0 and S.n_buf.offset == 4 and S.lat_thr.offset == 8 and S.buf_thr.offset == 40
    assert S.speed.offset == 72
    hdr = open(os.path.join(ROOT, "include", "abr_env.h")).read()
    assert "#define ABR_SPEED_RULE_MAX_THR 4" in hdr
    assert "int abr_env_set_speed_rule(abr_env *env, const abr_speed_rule *rule, double *speed_log_dev, " \
           "int32_t log_rows);" in hdr


GOOD = ([1.0, 3.0], [2.0], [[1.0, 1.0], [0.9, 1.1], [0.9, 1.25]])
BAD = [
    dict(n_lat=5), dict(n_lat=-1), dict(n_buf=5), dict(n_buf=-1),
    dict(lat_thr=[3.0, 1.0]), dict(lat_thr=[1.0, 1.0]), dict(lat_thr=[1.0, float("inf")]),
    dict(lat_thr=[float("nan"), 1.0]), dict(buf_thr=[float("-inf")]), dict(buf_thr=[float("nan")]),
    dict(speed=(0, 0, 0.0)), dict(speed=(2, 1, -1.0)), dict(speed=(1, 0, float("nan"))),
    dict(speed=(0, 1, float("inf"))), dict(log_rows=-1), dict(log_rows=4),
]


def _bad_struct(bad):
    r = _struct(*GOOD)
    for k, v in bad.items():
        if k in ("n_lat", "n_buf"):
            setattr(r, k, v)
        elif k in ("lat_thr", "buf_thr"):
            for q, t in enumerate(v):
                getattr(r, k)[q] = t
        elif k == "speed":
            r.speed[v[0]][v[1]] = v[2]
    return r


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}" for k in b))
def test_refusals_before_the_handle(bad):
    """Every bad field answers ABR_E_INVALID with a message that names it, with a NULL handle: the struct is checked
    first, nothing is stored."""
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    rows = bad.get("log_rows", 0)
    assert lib.abr_env_set_speed_rule(None, C.byref(_bad_struct(bad)), None, rows) == ABR_E_INVALID
    msg = lib.abr_last_error().decode()
    assert "env is NULL" not in msg, msg


def test_good_rules_reach_the_handle_check():
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    # entries past n_lat / n_buf are ignored, whatever they hold
    r = _struct(*GOOD)
    r.lat_thr[3] = float("nan"); r.speed[4][4] = -1.0
    for rule in (r, _struct([], [], [[1.0]]), None):
        assert lib.abr_env_set_speed_rule(None, C.byref(rule) if rule is not None else None, None, 0) \
            == ABR_E_INVALID
        assert "env is NULL" in lib.abr_last_error().decode()
    assert lib.abr_env_set_speed_rule(None, C.byref(r), C.c_void_p(256), 8) == ABR_E_INVALID
    assert "env is NULL" in lib.abr_last_error().decode()


def test_python_controller_validation_and_struct():
    from abrsimulator_amd import LatencySpeedController as LSC
    c = LSC((1.0, 3.0), (2.0,), ((1.0, 1.0), (0.9, 1.1), (0.9, 1.25)))
    s = c.to_struct()
    assert (s.n_lat, s.n_buf) == (2, 1) and s.speed[2][1] == 1.25 and s.lat_thr[1] == 3.0
    assert c.speed_for(3.0, 2.0) == 1.25 and c.speed_for(2.999, 1.999) == 0.9
    assert LSC().speeds == ((1.0,),)
    k = LSC.catch_up(3.0)
    assert k.speed_for(3.0, 0.0) == 1.1 and k.speed_for(2.0, 0.0) == 1.0
    k = LSC.catch_up(3.0, fast=1.2, low_buffer=1.0, slow=0.8)
    assert k.speed_for(5.0, 0.5) == 0.8 and k.speed_for(5.0, 1.0) == 1.2 and k.speed_for(0.0, 4.0) == 1.0
    for bad in [dict(latency_thresholds=(1, 2, 3, 4, 5), speeds=[[1.0]] * 6),
                dict(latency_thresholds=(2.0, 1.0), speeds=[[1.0]] * 3),
                dict(buffer_thresholds=(float("nan"),), speeds=[[1.0, 1.0]]),
                dict(speeds=[[0.0]]), dict(speeds=[[1.0, 1.0]]), dict(latency_thresholds=(1.0,), speeds=[[1.0]]),
                dict(speeds=[[float("inf")]])]:
        with pytest.raises(ValueError):
            LSC(**bad)
    with pytest.raises(RuntimeError, match="device"):
        c.get_next_speed()
