"""The two builds of the lane functions (csrc/abr_lane_jump.h: TablesT<SPEEDS>), compiled for the HOST
(tests/native/speed_instances_harness.cpp): the build without the play-speed features equals the build that carries them
with none set, and both equal the oracle -- bit for bit, over the CPU episode configurations that have no speed feature
(tests/test_lane_jump_cpu.py: the reference's goldens, the seeded cases, the config-space fuzz).  Also what the change must
leave alone at the library's boundary: abr_env_has_impl, the ABI version, the struct layouts, the workspace size."""
import ctypes as C

import numpy as np
import pytest

from conftest import ENV_GOLDENS, load_golden
from helpers import c_abi_output, native_harness
from test_lane_jump_cpu import CASES, _case, _check, _random_config


@pytest.fixture(scope="module")
def H():
    lib = native_harness("speed_instances_harness")
    lib.si_create.restype = C.c_void_p
    lib.si_batch.restype = C.c_int64
    return lib


def run_build(H, speeds_flag, meta, traces, trace_id, offset, actions, max_ticks=0):
    """One batch of episodes through the lane functions of TablesT<speeds_flag>: (rec, bw, pred, fin, n_play)."""
    from oracle.oracle import pack_traces
    ladder = np.asarray(meta["ladder"], np.float64)
    V = meta["video_length"]
    if not max_ticks:
        max_ticks = int(32 * V * np.ceil(meta["chunk_length"] / 0.01))
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    h = H.si_create(C.c_double(meta["interval"]), C.c_double(meta["chunk_length"]), C.c_double(meta.get("speed", 1.0)),
                    C.c_int32(V), C.c_double(meta["max_buffer"]), C.c_double(meta["start_up_length"]),
                    C.c_int32(max_ticks), P(ladder, C.c_double), C.c_int32(len(ladder)))
    flat, off, lens = pack_traces(traces)
    trace_id = np.ascontiguousarray(trace_id, np.int32)
    offset = np.ascontiguousarray(offset, np.int32)
    actions = np.ascontiguousarray(actions, np.int32)
    N = actions.shape[0]
    rec, bw, pred = np.zeros((N, V, 8)), np.zeros((N, V)), np.zeros((N, V), np.int32)
    fin, fin_i = np.zeros((N, 6)), np.zeros((N, 2), np.int32)
    rc = H.si_batch(C.c_void_p(h), C.c_int32(speeds_flag), P(flat, C.c_double), P(off, C.c_int64), P(lens, C.c_int32),
                    P(trace_id, C.c_int32), P(offset, C.c_int32), P(actions, C.c_int32), C.c_int32(N), P(rec, C.c_double),
                    P(bw, C.c_double), P(pred, C.c_int32), P(fin, C.c_double), P(fin_i, C.c_int32))
    H.si_destroy(C.c_void_p(h))
    assert rc == 0, rc
    return rec, bw, pred, fin, fin_i[:, 0]


def both_builds(H, meta, traces, trace_id, offset, actions, steps, bwo, fino, max_ticks=0):
    """Flag off == flag on in every recorded value (the observation's clocks, buffer, flags, the latency integral, the
    download side's call-site predictions, the final state), and each equals the oracle."""
    on = run_build(H, 1, meta, traces, trace_id, offset, actions, max_ticks)
    off = run_build(H, 0, meta, traces, trace_id, offset, actions, max_ticks)
    for name, a, b in zip(("rec", "bw", "pred", "fin", "n_play"), on, off):
        assert np.array_equal(a, b), name
    for rec, bw, _, fin, _ in (on, off):
        _check(rec, bw, fin, steps, bwo, fino)
    return on


def test_the_harness_ran_two_different_builds(H):
    out = (C.c_int32 * 4)()
    H.si_sizes(out)
    assert out[2] == 1 and out[3] == 0
    assert out[1] < out[0]                 # the no-speeds table carries no speed fields


@pytest.mark.parametrize("name", ENV_GOLDENS)
def test_goldens_bit_exact_in_both_builds(H, name):
    m, g = load_golden(name)
    steps = {k: g[k] for k in ["global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level", "start_up",
                               "buffer_empty", "buffer_full"]}
    steps["last_bandwidth"] = g["arg_last_bandwidth"]
    fino = {k: g["final_" + k] for k in ["global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level"]}
    rec, bw, pred, fin, n_play = both_builds(H, m, list(g["traces"]), g["trace_id"], g["offset"], g["actions"], steps,
                                             g["final_bandwidths"], fino)
    sd = m.get("speed", 1.0) * 0.01
    n = n_play.astype(np.float64)
    lat = (0.01 * fin[:, 5] - sd * (n * (n - 1) / 2)) / fin[:, 3]
    assert np.allclose(lat, g["final_average_latency"], rtol=1e-9)


@pytest.mark.parametrize("case", CASES, ids=[str(c["seed"]) for c in CASES])
def test_seeded_cases_in_both_builds(H, oracle, case):
    meta, traces, trace_id, offset, actions = _case(**case)
    cfg = oracle.env_cfg(meta["ladder"], meta["chunk_length"], meta["video_length"], meta["max_buffer"],
                         meta["start_up_length"], meta["interval"], meta["weights"], meta["speed"])
    steps, bwo, fino, _ = oracle.env_batch(cfg, traces, trace_id, offset, actions)
    rec, bw, pred, fin, _ = both_builds(H, meta, traces, trace_id, offset, actions, steps, bwo, fino)
    if case["seed"] in (5, 6):             # the small-buffer cases: the gated call sites are predicted in both builds
        assert (pred >= 0).sum() > 0


@pytest.mark.parametrize("seed", range(60))
def test_random_configurations_in_both_builds(H, oracle, seed):
    rng = np.random.default_rng(1000 + seed)        # the configurations of test_random_configurations_against_oracle
    meta, (lo, hi) = _random_config(rng)
    n_traces, N = 6, 200
    lens = rng.integers(40, 3000, n_traces)
    traces = [rng.uniform(lo, hi, l).astype(np.float32).astype(np.float64) for l in lens]
    trace_id = rng.integers(0, n_traces, N).astype(np.int32)
    offset = np.array([rng.integers(0, lens[t]) for t in trace_id], np.int32)
    actions = rng.integers(0, len(meta["ladder"]), (N, meta["video_length"])).astype(np.int32)
    cfg = oracle.env_cfg(meta["ladder"], meta["chunk_length"], meta["video_length"], meta["max_buffer"],
                         meta["start_up_length"], meta["interval"], meta["weights"], meta["speed"])
    steps, bwo, fino, _ = oracle.env_batch(cfg, traces, trace_id, offset, actions, max_ticks=4_000_000)
    both_builds(H, meta, traces, trace_id, offset, actions, steps, bwo, fino, max_ticks=int(fino["ticks"].max()) + 1000)


def test_library_boundary_is_unchanged():
    """The instances are chosen inside the library: what a caller sees -- the implementations it may ask for, the ABI
    version, the public structs, the workspace's size per lane (the speed regions stay where they were) -- is as before."""
    from abrsimulator_amd import _lib as L
    L.build()
    lib = L.lib()
    assert [lib.abr_env_has_impl(i) for i in range(9)] == [1, 1, 1, 1, 0, 1, 0, 0, 0]
    assert lib.abr_abi_version() == 4 == L.ABI_VERSION
    out = c_abi_output(r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(abr_env_config), sizeof(abr_mpc_config), sizeof(abr_env_state_view),
         sizeof(abr_mpc_options), sizeof(abr_speed_rule), offsetof(abr_speed_rule, speed), offsetof(abr_env_state_view, bw_hist));
  return 0;
}''')
    got = list(map(int, out[0].split()))
    assert got[:4] == [C.sizeof(L.EnvConfig), C.sizeof(L.MpcConfig), C.sizeof(L.StateView), C.sizeof(L.MpcOptions)]
    assert got[4:6] == [8 + 2 * 4 * 8 + 25 * 8, 8 + 2 * 4 * 8]            # n_lat, n_buf; lat_thr[4], buf_thr[4]; speed[5][5]
    assert got[6] == L.StateView.bw_hist.offset
    cfg = L.EnvConfig()
    cfg.n_rates, cfg.video_length = 6, 48
    cfg.chunk_length, cfg.max_buffer, cfg.start_up_length, cfg.interval, cfg.speed = 4.0, 20.0, 8.0, 1.0, 1.0
    for i, b in enumerate([0.3, 0.75, 1.2, 1.85, 2.85, 4.3]):
        cfg.ladder[i] = b
    n1, n2 = C.c_size_t(), C.c_size_t()
    assert lib.abr_env_workspace_bytes(C.byref(cfg), 65536, C.byref(n1)) == 0
    assert lib.abr_env_workspace_bytes(C.byref(cfg), 131072, C.byref(n2)) == 0
    # per lane: 8 float64 rows (sd_lane, pt_lane, pt_sum among them), sumk, 15 int32 rows (pl_left, play_id among them), ...
    assert n2.value - n1.value == 65536 * (8 * 8 + 8 + 15 * 4 + 2 + 48 + 48 * 8 + 4 * 8 + 4 + 72)
