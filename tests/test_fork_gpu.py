"""The lane fork on the device (include/abr_env.h: abr_env_fork; BatchedABREnv.fork).

Shape: 200 lanes (three full 64-lane groups and a partial one), 5-chunk episodes over 3 rates.  Three single steps with
seeded actions, a state_dict(), then a fork whose mapping holds a 3-cycle, a source used four times, skipped lanes, a lane
copied onto itself and sixty seeded pairs.  Expectations: the workspace (every byte of it: the per-lane regions moved, the
rest untouched) and the quality blob equal the numpy twin (tests/fork_twin.py) applied to the saved bytes; obs, trace ids
and offsets follow; and in the two scripted decisions that end the episode every lane reports what its SOURCE lane reports
in a second environment that loaded the saved state and was fed the same actions -- pre-existing code, the reference.
Every index fed to the device is a lane or -1: out-of-range indices are tested on the host (tests/test_fork_cpu.py)."""
import numpy as np
import pytest
import torch

import abrsimulator_amd as A
from abrsimulator_amd import _lib
import fork_twin as T

pytestmark = pytest.mark.gpu

LADDER = [0.3, 1.2, 2.85]
V, L, MB, SU, W = 5, 4.0, 20.0, 4.0, [4.3, 1.0, 1.0, 0.1]
M, N, PRE = len(LADDER), 200, 3
IMPLS = ["jump", "split", "split3", "tick"]
RULE = A.LatencySpeedController((2.0, 6.0), (1.0, 8.0), ((0.9, 1.0, 1.0), (0.9, 1.1, 1.25), (0.75, 1.5, 2.0)))


def corpus():
    rng = np.random.default_rng(0)
    return [rng.uniform(0.5, 6.0, int(rng.integers(30, 200))) for _ in range(8)]


TRACES = corpus()
TID = (np.arange(N) % len(TRACES)).astype(np.int32)
OFF = ((np.arange(N) * 7) % 13).astype(np.int32)
ACTS = np.random.default_rng(5).integers(0, M, (V, N)).astype(np.int32)


def mapping():
    """(src, dst) pairs, shuffled: the cases of the module docstring.  dst values are distinct."""
    rng = np.random.default_rng(11)
    pairs = [(10, 11), (11, 12), (12, 10)] + [(20, d) for d in (21, 22, 23, 150)] + [(-1, 30), (-1, 31), (40, 40)]
    free = np.array([d for d in range(50, N) if d != 150])
    for d in rng.choice(free, 60, replace=False):
        pairs.append((int(rng.integers(0, N)), int(d)))
    order = rng.permutation(len(pairs))
    src = np.array([pairs[k][0] for k in order], np.int32)
    dst = np.array([pairs[k][1] for k in order], np.int32)
    assert len(set(dst.tolist())) == len(dst)
    return src, dst


SRC, DST = mapping()
ORIGIN = np.arange(N)                       # the lane whose state each lane holds after the fork
ORIGIN[DST[SRC >= 0]] = SRC[SRC >= 0]
SRC_FULL = np.full(N, -1, np.int32)         # the same mapping with dst = None
SRC_FULL[DST] = SRC


def make(impl, **kw):
    return A.BatchedABREnv(A.MPD(V, L, MB, SU, A.Chunk(LADDER)), A.QOEMetric(*W), A.NetworkInfo(1.0, TRACES), N,
                           device="cuda", impl=impl, **kw)


def dress(env, quality, ledger):
    if ledger:
        env.set_episode_ledger(2)
    if quality:
        env.set_quality(0.37, "log", rows=2)
    return env


def f64_offset(env):
    """Where the per-lane regions start in the workspace, and a check that the twin's layout is the library's."""
    v, base = env.state_view(), env.workspace.data_ptr()
    f64 = v.buffer_level - base
    o = T.workspace_offsets(V, N, f64)
    assert v.hist_n - base == o["f64"][0] + 2 * 8 * N and v.hist_sum_inv - base == o["f64"][0] + 3 * 8 * N
    assert v.chunk_id - base == o["i32"][0] + 4 * N and v.last_bitrate - base == o["i32"][0] + 9 * 4 * N
    assert v.done - base == o["u8"][0] + N
    assert v.action_hist - base == o["action_hist"][0] and v.bw_hist - base == o["bw_hist"][0]
    assert o["mpc_action"][0] + 4 * N <= env.workspace.numel() - 256
    return f64


def run_case(impl, quality=False, ledger=False, speed=1.0, form="pairs", cont_impl=None):
    e1 = dress(make(impl, speed=speed), quality, ledger)
    e1.reset(torch.from_numpy(TID), torch.from_numpy(OFF))
    for t in range(PRE):
        e1.step(torch.from_numpy(ACTS[t]).cuda())
    sd = e1.state_dict()
    obs0 = e1.obs.cpu().numpy().copy()
    ws0 = sd["workspace"].cpu().numpy()
    led0 = e1.episode_ledger.blob.cpu().numpy().copy() if ledger else None
    if form == "pairs":
        e1.fork(torch.from_numpy(SRC).cuda(), torch.from_numpy(DST).cuda())
    else:
        e1.fork(torch.from_numpy(SRC_FULL).cuda())
    # the bytes: every per-lane region moved as the twin moves it, every other byte of the workspace as it was
    f64 = f64_offset(e1)
    ws1 = e1.workspace.cpu().numpy()
    want = T.fork_workspace(ws0, V, N, f64, SRC, DST)
    assert np.array_equal(ws1, want), np.nonzero(ws1 != want)[0][:8]
    moved = T.lane_byte_mask(len(ws0), V, N, f64, DST[SRC >= 0])
    assert np.array_equal(ws1[~moved], ws0[~moved])
    assert (ws1 != ws0).any()
    assert np.array_equal(e1.obs.cpu().numpy().view(np.uint32), T.fork_columns(obs0.view(np.uint32), SRC, DST))
    assert np.array_equal(e1.trace_id.cpu().numpy(), TID[ORIGIN]) and np.array_equal(e1.start_offset.cpu().numpy(), OFF[ORIGIN])
    if quality:
        q0, q1 = sd["quality"]["blob"].cpu().numpy(), e1.quality.blob.cpu().numpy()
        lo = e1.quality.layout
        wantq = q0.copy()
        col = q0[lo["q_run"]:lo["q_run"] + 8 * N].view(np.uint64)[None]
        wantq[lo["q_run"]:lo["q_run"] + 8 * N] = T.fork_columns(col, SRC, DST).view(np.uint8).reshape(-1)
        assert np.array_equal(q1, wantq) and (q1 != q0).any()
    if ledger:
        assert np.array_equal(e1.episode_ledger.blob.cpu().numpy(), led0)
    # the continuation: lane d of the forked env against lane ORIGIN[d] of an env restored from the saved state
    e2 = dress(make(impl, speed=speed), quality, ledger)
    e2.load_state_dict(sd)
    if cont_impl is not None:
        e1._check(e1.lib.abr_env_set_impl(e1._h, cont_impl))
    a2 = ACTS[PRE:]
    a1 = np.ascontiguousarray(a2[:, ORIGIN])
    o1 = e1.step_script(torch.from_numpy(a1).cuda())
    o2 = e2.step_script(torch.from_numpy(a2).cuda())
    for k in ("obs", "reward", "done"):
        g, w = o1[k].cpu().numpy(), o2[k].cpu().numpy()[..., ORIGIN]
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                              w.view(np.uint32) if w.dtype == np.float32 else w), k
    assert (o1["done"][-1].cpu().numpy() == _lib.DONE_EPISODE).all()
    q1, q2 = e1.episode_qoe(quality=quality).cpu().numpy(), e2.episode_qoe(quality=quality).cpu().numpy()
    assert np.array_equal(q1, q2[ORIGIN])
    f1, f2 = e1.observe_f64(), e2.observe_f64()
    for k in f1:
        assert np.array_equal(f1[k].cpu().numpy(), f2[k].cpu().numpy()[ORIGIN]), k
    h1, h2 = e1.history(), e2.history()
    assert np.array_equal(h1[0].cpu().numpy(), h2[0].cpu().numpy()[:, ORIGIN])
    assert np.array_equal(h1[1].cpu().numpy(), h2[1].cpu().numpy()[:, ORIGIN])
    if quality:
        assert np.array_equal(e1.quality.last().cpu().numpy(), e2.quality.last().cpu().numpy()[ORIGIN])
        assert (e1.quality.count().cpu().numpy() == 1).all()          # the records stayed with the slots: one episode each
    if ledger:
        assert (e1.episode_ledger.count().cpu().numpy() == 1).all()


@pytest.mark.parametrize("impl", IMPLS)
def test_fork_moves_the_columns_and_the_copies_continue_as_their_sources(impl):
    run_case(impl, form="pairs" if impl in ("jump", "split3") else "full")


@pytest.mark.parametrize("impl", IMPLS)
def test_fork_with_a_ledger_and_a_quality_model(impl):
    run_case(impl, quality=True, ledger=True, form="full" if impl in ("jump", "split3") else "pairs")


@pytest.mark.parametrize("impl", ["jump", "split", "split3"])
def test_fork_under_a_speed_rule(impl):
    run_case(impl, speed=RULE, quality=True)


@pytest.mark.parametrize("impl,cont", [("jump", 5), ("split3", 0), ("split", 5), ("jump", 2)])
def test_fork_under_one_implementation_continue_under_another(impl, cont):
    run_case(impl, cont_impl=cont)


def test_refused_under_per_lane_speeds_and_schedules():
    src = torch.arange(N, dtype=torch.int32, device="cuda")
    for speed in (torch.full((N,), 1.1, dtype=torch.float64), torch.full((2, N), 1.05, dtype=torch.float64)):
        env = make("jump", speed=speed)
        env.reset(torch.from_numpy(TID), torch.from_numpy(OFF))
        with pytest.raises(_lib.AbrError, match="-4.*per-lane speeds"):
            env.fork(src)
    # pending ones refuse as well; taking them back lifts the refusal
    env = make("jump")
    env.reset(torch.from_numpy(TID), torch.from_numpy(OFF))
    sp = torch.full((N,), 1.1, dtype=torch.float64, device="cuda")
    env._check(env.lib.abr_env_set_lane_speeds(env._h, _lib.ptr(sp)))
    with pytest.raises(_lib.AbrError, match="-4.*pending"):
        env.fork(src)
    env._check(env.lib.abr_env_set_lane_speeds(env._h, None))
    env.fork(src)
    # a scratch that is too small is refused before anything is launched
    import ctypes as C
    need = C.c_size_t()
    env._check(env.lib.abr_env_fork_scratch_bytes(env._h, N, C.byref(need)))
    assert need.value == T.scratch_layout(V, N)[1]
    small = torch.empty(need.value - 256, dtype=torch.uint8, device="cuda")
    rc = env.lib.abr_env_fork(env._h, _lib.ptr(src), None, N, _lib.ptr(small), small.numel(), None, env._stream())
    assert rc == -1 and b"scratch has" in env.lib.abr_last_error()
    torch.cuda.synchronize()
