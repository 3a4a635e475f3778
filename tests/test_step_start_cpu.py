"""The step start of a lane that knows its call site's trace interval (csrc/abr_lane_jump.h: lanej_begin_step_at) against the
search over six candidates that defines the result (lanej_begin_step), on the CPU.

tests/native/step_start_harness.cpp runs every lane twice, side by side: a general lane that only ever searches, and a fast
lane that is told its call site's interval the way the role-split kernels' download side is (role_d_pre / role_d_validate),
in launches whose first decision searches.  At every decision the fast path's StepStart (c, bw_next, ke, ke_next, tn,
avail_next) and cursor (j, tpos) are compared with the search on a copy of the cursor.

Conditions, for every configuration:
  * no field differs, and the one-thread kernels' classification agrees with the download side's;
  * the search takes EXACTLY the first decision of each launch plus the decisions whose call site buffer_full moved -- the
    second count is the general lane's alone, so a fast path that always falls back cannot pass;
  * avail_j holds its definition for the configuration's tables.
The bench shape must also show, on the general lane alone, that buffer_full moves fewer than 0.1 % of its call sites.

The same harness runs once more as a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer (no
sanitizer runs on code loaded into Python)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import native_harness

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
STATS = ["decisions", "mismatch", "searched", "first", "moved", "disagree", "avail_j_bad", "timed_out", "rearms", "case_a",
         "case_b", "far_behind", "wrap_mod"]


@pytest.fixture(scope="module")
def H():
    lib = native_harness("step_start_harness")
    lib.ss_run.restype = C.c_int64
    assert lib.ss_n_stats() == len(STATS)
    return lib


def run(H, *, interval, max_buffer, bw, tlens, V=8, L=4.0, start_up=4.0, lanes=200, launches=3, fuse=11, max_ticks=0,
        auto_reset=1, resample=1, proven=1, seed=0):
    rng = np.random.default_rng(seed)
    traces = [rng.uniform(bw[0], bw[1], int(n)).astype(np.float32).astype(np.float64) for n in tlens]
    flat = np.concatenate(traces)
    lens = np.array([len(t) for t in traces], np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    tid = rng.integers(0, len(traces), lanes).astype(np.int32)
    offset = rng.integers(0, 4000, lanes).astype(np.int32)
    n_steps = launches * fuse
    actions = rng.integers(0, len(LADDER), (lanes, n_steps)).astype(np.int32)
    if not max_ticks:
        max_ticks = int(32 * V * np.ceil(L / 0.01))
    ladder = np.array(LADDER)
    st = np.zeros(len(STATS), np.int64)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = H.ss_run(C.c_double(interval), C.c_double(L), C.c_double(1.0), C.c_int32(V), C.c_double(max_buffer),
                  C.c_double(start_up), C.c_int32(max_ticks), P(ladder, C.c_double), C.c_int32(len(LADDER)),
                  C.c_int32(auto_reset), C.c_int32(resample), P(flat, C.c_double), P(off, C.c_int64), P(lens, C.c_int32),
                  C.c_int32(len(traces)), P(tid, C.c_int32), P(offset, C.c_int32), P(actions, C.c_int32), C.c_int32(lanes),
                  C.c_int32(n_steps), C.c_int32(fuse), C.c_int32(proven), P(st, C.c_int64))
    assert rc == 0, rc
    s = dict(zip(STATS, (int(v) for v in st)))
    print(s)
    assert s["mismatch"] == 0 and s["disagree"] == 0 and s["avail_j_bad"] == 0, s
    assert s["decisions"] > 0 and s["searched"] == s["first"] + s["moved"], s
    return s


def test_bench_shape(H):
    """48 chunks of 4 s, max_buffer 20 s, interval 1 s, traces of 1000 samples in 0.2..6 Mbit/s, launches of 48 decisions
    under auto_reset: buffer_full moves fewer than 0.1 % of the call sites, so nearly every decision takes the fast path."""
    s = run(H, interval=1.0, max_buffer=20.0, bw=(0.2, 6.0), tlens=[1000] * 64, V=48, start_up=8.0, lanes=1024, launches=3,
            fuse=48, resample=0, seed=1)
    assert s["decisions"] == 1024 * 144 and s["timed_out"] == 0 and s["rearms"] == 1024 * 3
    assert s["moved"] < 0.001 * s["decisions"], s
    assert s["searched"] < 0.03 * s["decisions"], s
    assert s["case_a"] > 1000 and s["case_b"] > 1000, s


def test_starved_network_many_intervals_per_wait(H):
    """Interval 0.3 s on a network slower than the lowest rung: every wait for availability spans more intervals than the
    search's look-ahead covers (kCatch), which case B takes in one step."""
    for proven in (1, 0):
        s = run(H, interval=0.3, max_buffer=20.0, bw=(0.5, 6.0), tlens=[300, 157, 1000, 40], proven=proven, seed=2)
        assert s["case_b"] > 0.3 * s["decisions"] and s["far_behind"] > 0.3 * s["decisions"], s
    s = run(H, interval=0.3, max_buffer=20.0, bw=(0.02, 0.25), tlens=[300, 157, 1000, 40], seed=3)
    assert s["case_a"] > 0.5 * s["decisions"], s


@pytest.mark.parametrize("interval,L,max_buffer,start_up", [(0.5, 2.0, 3.0, 4.0), (0.7, 4.0, 5.0, 8.0)])
def test_buffer_full_gates_often(H, interval, L, max_buffer, start_up):
    """A max_buffer below the start-up length: playback begins with the buffer above it, and on a fast network it is still
    full when the next chunk becomes available (tests/golden/env_bufferfull_i05 is the first of these shapes)."""
    for proven in (1, 0):
        s = run(H, interval=interval, L=L, max_buffer=max_buffer, start_up=start_up, bw=(2.0, 12.0),
                tlens=[300, 157, 1000, 40], proven=proven, seed=4)
        assert 0.1 * s["decisions"] < s["moved"] and s["searched"] < 0.5 * s["decisions"], s


@pytest.mark.parametrize("tlen", [1, 2, 3])
def test_traces_shorter_than_the_look_ahead(H, tlen):
    """The `%` branch of trace_wrap: a wait of several intervals on a trace of one to three samples."""
    for interval, proven in ((0.3, 1), (1.0, 0)):
        s = run(H, interval=interval, max_buffer=20.0, bw=(0.3, 6.0), tlens=[tlen] * 3, proven=proven, seed=5 + tlen)
        assert s["wrap_mod"] > 100, s


def test_mixed_trace_lengths(H):
    s = run(H, interval=1.0, max_buffer=20.0, bw=(0.2, 6.0), tlens=[1, 2, 3, 5, 8, 90, 1000, 2999], seed=9)
    assert s["rearms"] > 200 and s["wrap_mod"] > 0, s


def test_lanes_time_out(H):
    """max_ticks of 1.5 x the shortest possible episode on a slow network: some episodes finish, most lanes end in one that
    does not."""
    s = run(H, interval=1.0, max_buffer=20.0, bw=(0.2, 1.5), tlens=[300, 157, 40], max_ticks=6000, seed=10)
    assert s["timed_out"] > 20 and s["decisions"] > 1000 and s["rearms"] > 20, s


def test_episodes_that_end_without_a_re_arm(H):
    s = run(H, interval=1.0, max_buffer=20.0, bw=(0.2, 6.0), tlens=[300, 157, 40], auto_reset=0, seed=11)
    assert s["rearms"] == 0 and s["decisions"] == 200 * 8, s


def test_re_arms_inside_and_across_launches(H):
    """Launches of 5 and of 8 decisions over episodes of 8 chunks: a re-arm in the middle of a launch, and one that coincides
    with a launch boundary (the re-armed lane's first call site is then a launch's first decision: it searches)."""
    for fuse in (5, 8):
        s = run(H, interval=0.5, max_buffer=20.0, bw=(0.2, 6.0), tlens=[300, 157, 40], fuse=fuse, launches=6, seed=12)
        assert s["rearms"] >= 200 * (6 * fuse // 8 - 1), s


def test_sanitized_program(tmp_path):
    """A built-in replay of the configurations above in small, through a stand-alone build of the harness with
    AddressSanitizer and UndefinedBehaviorSanitizer.  The runtimes are linked statically."""
    src = os.path.join(_ROOT, "tests", "native", "step_start_harness.cpp")
    exe = str(tmp_path / "step_start_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-DSTEP_START_MAIN", "-I", os.path.join(_ROOT, "abrsimulator_amd", "csrc"),
                           src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout.split()
    assert out[0] == "ok" and int(out[1]) > 10000 and 0 < int(out[2]) < int(out[1]), r.stdout[-3000:]
