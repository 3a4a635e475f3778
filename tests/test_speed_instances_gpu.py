"""The no-speeds instances of the environment kernels (SPEEDS == false: csrc/abr_env.hip make_tables, launch_env) on the
device, at the smallest shapes where the dispatch or the slimmer state can go wrong: 130 lanes (three workgroups, the last
with two live lanes), video_length 6, eight traces of 7-40 samples, max_ticks = the oracle's longest episode + 1000, fused
rollouts in pieces of 4 + 5 + 3 decisions that cross an episode end with auto_reset and without it.

  * the no-speeds instance of every implementation against the oracle (closed_loop_check.check: == on every float32
    observation row, reward and done flag, == on the float64 frame of abr_env_observe_f64, 1e-9 / 1e-10 on
    average_latency / the episode QoE: DESIGN section 5), random and scripted;
  * the two instances against each other: a handle without speeds and one whose per-lane speeds all equal the config
    speed give identical outputs and identical workspaces outside the speed regions, which the no-speeds handle leaves
    as the test filled them;
  * one handle toggled: no speeds, then per-lane speeds / a schedule / the speed rule, then none again, every phase
    against the oracle of its configuration -- a stale dispatch is a mismatch;
  * a no-speeds workspace handed from each implementation to each other one in the middle of an episode;
  * one decision per launch of abr_env_step_mpc and of a policy rollout at 65 lanes, against their twins (K1 MODE 1).

No test here can see WHICH instance a launch ran: outputs and workspaces are the same by design.  That the no-speeds
instance is the one on the hot path is on record in profiles/speed_instances_sq_counters.json (the profiler names
env_split3_kernel<2, false, false, false>).

The oracle side of every case is computed once per module, before the first launch that uses it."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

import closed_loop_check as K  # noqa: E402

pytestmark = pytest.mark.gpu

N, V, PIECES = 130, 6, [4, 5, 3]
T = sum(PIECES)
META = dict(ladder=[0.3, 0.75, 1.2, 1.85, 2.85, 4.3], chunk_length=2.0, video_length=V, max_buffer=3.0,
            start_up_length=2.0, interval=0.5, weights=[4.3, 1.0, 1.0, 0.1], speed=1.0)
RULE = ((1.5, 4.0), (1.0, 3.0), ((0.9, 1.0, 1.1), (1.0, 1.25, 1.5), (1.1, 1.5, 2.0)))
PHILOX = 0x5EED5EED1234
KERNELS = ("split3", "split", "jump", "tick")            # tick: where the feature "no speeds" is all it accepts
TICK_ORACLE_BOUND = 40_000_000


@functools.lru_cache(maxsize=None)
def make_case(feature, launch, auto_reset, episode0=0):
    """One open-loop case in closed_loop_check's layout (controller "script"); the oracle's replays fix max_ticks.
    episode0: the episode number the lanes are at when the run starts -- the counter-based random policy draws its action
    from (lane, chunk, episode number), and a full reset of an armed handle starts episode number + 1, not 0."""
    from oracle import oracle as O
    rng = np.random.default_rng(20261018)                # the same traces, lanes and script whatever the variant
    # slow traces (rebuffering) and fast ones (the 1.5-chunk buffer fills: call sites gated by buffer_full)
    traces = [rng.uniform(*((0.4, 4.0) if j % 2 else (3.0, 14.0)), int(n)).astype(np.float32).astype(np.float64)
              for j, n in enumerate(rng.integers(7, 41, 8))]
    tl = np.array([len(t) for t in traces])
    tid = rng.integers(0, len(traces), N).astype(np.int32)
    off = (rng.integers(0, 1 << 20, N) % tl[tid]).astype(np.int32)
    B = len(META["ladder"])
    n_ep = T // V if auto_reset else 1
    scripted = rng.integers(0, B, (2 * V, N)).astype(np.int32)
    lane_speeds = rng.choice([0.6, 0.8, 1.0, 1.25, 1.7, 0.9173], N)
    schedule = rng.choice([0.5, 0.75, 1.0, 1.1, 1.25, 1.5, 2.0], (N, 4))
    if launch == "random":
        script = np.stack([O.philox_action(PHILOX, np.arange(N), t % V, episode0 + t // V, B) for t in range(2 * V)])
    else:
        script = scripted
    case = dict(seed=0, ctl="script", feature=feature, impl=None, vbr=False, auto_reset=auto_reset, n_lanes=N,
                meta=dict(META), traces=traces, tid=tid, off=off, br=None, params={}, pieces=list(PIECES), n_steps=T,
                script=script[:n_ep * V], launch=launch, philox=PHILOX)
    kw = {}
    if feature == "lanes":
        case["lane_speeds"] = kw["speeds"] = lane_speeds
    elif feature == "ones":                              # per-lane speeds that all equal the config speed
        case["feature"], case["lane_speeds"] = "lanes", np.full(N, META["speed"])
        kw["speeds"] = case["lane_speeds"]
    elif feature == "schedule":
        case["schedule"] = kw["speeds"] = schedule
    elif feature == "rule":
        case["rule"] = RULE
        kw["rule"] = K.rule_arrays(case)
    ticks = 0
    for e in range(n_ep):
        a = np.ascontiguousarray(case["script"][e * V:(e + 1) * V].T)
        fin = O.env_batch(K.env_cfg(case), traces, tid, off, a, max_ticks=TICK_ORACLE_BOUND, **kw)[2]
        ticks = max(ticks, int(fin["ticks"].max()))
    case["max_ticks"] = ticks + 1000
    return case


def common_max_ticks(*cases):
    return max(c["max_ticks"] for c in cases)


def build_env(case, impl, max_ticks=None, speeds=True):
    import abrsimulator_amd as A
    m = case["meta"]
    speed = m["speed"]
    if speeds and case["feature"] == "lanes":
        speed = torch.from_numpy(np.asarray(case["lane_speeds"], np.float64))
    elif speeds and case["feature"] == "schedule":
        speed = torch.from_numpy(np.ascontiguousarray(np.asarray(case["schedule"], np.float64).T))
    env = A.BatchedABREnv(A.MPD(V, m["chunk_length"], m["max_buffer"], m["start_up_length"], A.Chunk(m["ladder"])),
                          A.QOEMetric(*m["weights"]), A.NetworkInfo(m["interval"], case["traces"]), case["n_lanes"],
                          speed=speed, impl=impl, auto_reset=case["auto_reset"], max_ticks=max_ticks or case["max_ticks"])
    if speeds and case["feature"] == "rule":
        env.set_speed_controller(A.LatencySpeedController(*case["rule"]), log_rows=V + 4)
    return env


def script_rows(case):
    """(the rows step_script is given, the actions the run reports): a finished lane ignores its row and reports -1."""
    rows = np.stack([case["script"][t if case["auto_reset"] else t % V] for t in range(T)])
    given = np.where((np.arange(T) < V)[:, None] | case["auto_reset"], rows, -1).astype(np.int32)
    return rows, given


def run_pieces(env, case, pieces=None, start=0, reset=True):
    """reset (optional), then the case's launches from decision `start` on: closed_loop_check.check's `out`."""
    if reset:
        env.reset(torch.from_numpy(case["tid"]), torch.from_numpy(case["off"]))
    rows, given = script_rows(case)
    dev = torch.from_numpy(rows).cuda()
    parts, frames, t = [], [], start
    for n in (pieces or case["pieces"]):
        o = env.step_script(dev[t:t + n]) if case["launch"] == "script" else env.step_random(n, case["philox"])
        p = {k: o[k].cpu().numpy().copy() for k in ("obs", "reward", "done")}
        p["actions"] = o["actions"].cpu().numpy().copy() if case["launch"] == "random" else given[t:t + n]
        parts.append(p)
        t += n
        frames.append((t, {k: v.cpu().numpy().copy() for k, v in env.observe_f64().items()}))
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("actions", "reward", "done", "obs")}
    out["frames"] = frames
    out["history"] = tuple(x.cpu().numpy().copy() for x in env.history())
    out["qoe"] = env.episode_qoe().cpu().numpy()
    log = env.speed_log()
    out["speed_log"] = log.cpu().numpy().copy() if (log is not None and case["feature"] == "rule") else None
    out["entries"] = None
    torch.cuda.synchronize()
    return out


def check(case, out):
    """closed_loop_check.check; under auto_reset the frame a piece leaves exactly on an episode boundary -- call site 0 of
    an episode the oracle's replays do not reach -- is compared here instead: a fresh lane's counters."""
    frames = out["frames"]
    if case["auto_reset"]:
        for t, f in frames:
            if t % V == 0:
                assert (f["chunk_id"] == 0).all() and (f["rebuffer_time"] == 0).all() and (f["play_time"] == 0).all()
                assert (f["buffer_level"] == 0).all() and (f["hist_n"] == 0).all()
        frames = [(t, f) for t, f in frames if t % V]
    return K.check(case, dict(out, frames=frames))


def same_out(a, b, what):
    for k in ("actions", "reward", "done", "obs", "qoe"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    for (ta, fa), (tb, fb) in zip(a["frames"], b["frames"]):
        assert ta == tb
        for k in fa:
            assert np.array_equal(fa[k], fb[k], equal_nan=True), (what, "frame", ta, k)
    for x, y in zip(a["history"], b["history"]):
        assert np.array_equal(x, y), (what, "history")


# ---------------------------------------------------------------------------------------------------------------------
# the no-speeds instance against the oracle

@pytest.mark.parametrize("impl", KERNELS)
def test_no_speeds_instance_matches_the_oracle(impl):
    for launch in ("random", "script"):
        for auto_reset in (True, False):
            case = make_case("config", launch, auto_reset)
            env = build_env(case, impl)
            out = run_pieces(env, case)
            env.close()
            mm = check(case, out)
            assert not mm, (impl, launch, auto_reset, len(mm), mm[:6])
            if auto_reset:                           # the pieces really cross an episode end, on every lane
                assert (out["done"][V - 1] == 1).all() and (out["done"][V] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the two instances against each other

def speed_regions(env):
    """Byte ranges of the workspace's speed state: sd_lane, pt_lane, pt_sum (float64 rows 4-6 of the lane state that starts
    at buffer_level) and pl_left, play_id (int32 rows 13-14 of the block whose row 1 is chunk_id)."""
    v = env.state_view()
    base, n = env.workspace.data_ptr(), env.n_lanes
    f = v.buffer_level - base
    q = v.chunk_id - 4 * n - base
    return [(f + 4 * n * 8, f + 7 * n * 8), (q + 13 * n * 4, q + 15 * n * 4)]


@pytest.mark.parametrize("impl", ("split3", "split", "jump"))
def test_both_instances_agree_and_the_no_speeds_one_leaves_the_speed_state_alone(impl):
    for launch in ("random", "script"):
        plain, ones = make_case("config", launch, True), make_case("ones", launch, True)
        mt = common_max_ticks(plain, ones)
        a, b = build_env(plain, impl, mt), build_env(ones, impl, mt)
        regions = speed_regions(a)
        assert regions == speed_regions(b) and a.workspace.numel() == b.workspace.numel()
        for lo, hi in regions:
            a.workspace[lo:hi] = 0xA5
        b.workspace.copy_(a.workspace)               # never reset, same configuration: the same tables and tag, and now
        torch.cuda.synchronize()                     # the same bytes wherever neither instance writes
        oa, ob = run_pieces(a, plain), run_pieces(b, ones)
        same_out(oa, ob, (impl, launch))
        wa, wb = a.workspace.cpu().numpy(), b.workspace.cpu().numpy()
        keep = np.ones(wa.size, bool)
        for lo, hi in regions:
            assert (wa[lo:hi] == 0xA5).all(), (impl, launch, "the no-speeds instance wrote speed state", lo)
            keep[lo:hi] = False
        assert np.array_equal(wa[keep], wb[keep]), (impl, launch, np.flatnonzero((wa != wb) & keep)[:8])
        sd = wb[regions[0][0]:regions[0][0] + 8 * N].view(np.float64)
        assert (sd == 0.01 * META["speed"]).all()    # ... while the speeds instance keeps its per-lane speed*dt there
        a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------------
# one handle, toggled

def _install(env, case, keep):
    """What BatchedABREnv's constructor does for a speed feature, on a handle that is already running: latched by the next
    full reset."""
    import abrsimulator_amd as A
    from abrsimulator_amd import _lib
    if case["feature"] == "rule":
        env.set_speed_controller(A.LatencySpeedController(*case["rule"]), log_rows=V + 4)
    elif case["feature"] == "config":
        env.set_speed_controller(None)               # also drops per-lane speeds and schedules
    elif case["feature"] == "lanes":
        ls = torch.from_numpy(np.ascontiguousarray(case["lane_speeds"], np.float64)).cuda()
        keep.append(ls)
        env._check(env.lib.abr_env_set_lane_speeds(env._h, _lib.ptr(ls)))
    else:
        ls = torch.from_numpy(np.ascontiguousarray(np.asarray(case["schedule"], np.float64).T)).cuda()
        keep.append(ls)
        env._check(env.lib.abr_env_set_speed_schedule(env._h, _lib.ptr(ls), int(ls.shape[0])))


@pytest.mark.parametrize("feature", ("lanes", "schedule", "rule"))
@pytest.mark.parametrize("impl", ("split3", "split", "jump"))
def test_toggling_speeds_on_one_handle_selects_the_right_instance(impl, feature):
    auto_reset = feature != "rule"                   # (the rule's log is compared per episode: one episode)
    launch = "script" if feature == "schedule" else "random"
    # The handle's episode numbers go on across the phases (the random policy's counter): under auto_reset a phase runs
    # T / V whole episodes and its last re-arm leaves the lanes at first + T / V, without it they stay at first; the next
    # phase's full reset of the armed handle then starts the number after that.
    per_phase = T // V + 1 if auto_reset else 1
    cases = [make_case(f, launch, auto_reset, phase * per_phase) for phase, f in enumerate(("config", feature, "config"))]
    env = build_env(cases[0], impl, common_max_ticks(*cases))
    keep = []
    for phase, case in enumerate(cases):
        if phase:
            _install(env, case, keep)
        out = run_pieces(env, case)
        assert (env.episodes()["episode"].cpu().numpy() == (phase + 1) * per_phase - 1).all(), (impl, feature, phase)
        mm = check(case, out)
        assert not mm, (impl, feature, phase, len(mm), mm[:6])
    env.close()


def test_the_tick_kernel_still_refuses_speeds():
    from abrsimulator_amd import _lib
    case = make_case("config", "script", True)
    env = build_env(case, "tick")
    ls = torch.ones(1, N, dtype=torch.float64, device="cuda")
    assert env.lib.abr_env_set_speed_schedule(env._h, _lib.ptr(ls), 1) == -4
    out = run_pieces(env, case)                      # ... and goes on as the no-speeds instance it is
    assert not check(case, out)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
# hand-over in the middle of an episode

def test_no_speeds_workspace_is_handed_between_implementations_mid_episode():
    case = make_case("config", "script", True)
    envs = {k: build_env(case, k) for k in KERNELS}
    whole = run_pieces(envs["jump"], case)
    assert not check(case, whole)
    for src in KERNELS:
        first = run_pieces(envs[src], case, pieces=PIECES[:1])
        sd = envs[src].state_dict()
        for dst in KERNELS:
            if dst == src:
                continue
            envs[dst].load_state_dict(sd)
            rest = run_pieces(envs[dst], case, pieces=PIECES[1:], start=PIECES[0], reset=False)
            for k in ("reward", "done", "obs"):
                assert np.array_equal(np.concatenate([first[k], rest[k]]), whole[k], equal_nan=True), (src, dst, k)
            for (ta, fa), (tb, fb) in zip(rest["frames"], whole["frames"][1:]):
                assert ta == tb and all(np.array_equal(fa[k], fb[k], equal_nan=True) for k in fa), (src, dst, ta)
            assert np.array_equal(rest["qoe"], whole["qoe"]), (src, dst)
            for x, y in zip(rest["history"], whole["history"]):
                assert np.array_equal(x, y), (src, dst)
    for e in envs.values():
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# one decision per launch under MPC and under the learned policy: K1 MODE 1's no-speeds instance

def _first_case(ctl, lanes):
    for seed in range(10_000):
        case = K.make_case(seed, lanes)
        if case["ctl"] == ctl and case["feature"] == "config" and not case["auto_reset"]:
            return case
    raise AssertionError(ctl)


def test_one_step_launches_of_step_mpc_match_the_twin_at_65_lanes():
    import gpu_fuzz_closed
    case = _first_case("mpc", 65)
    case = dict(case, impl="auto", pieces=[1] * case["n_steps"])
    mm = K.check(case, gpu_fuzz_closed.run_case(case))
    assert not mm, (K.describe(case), len(mm), mm[:6])


def test_one_step_launches_of_a_policy_rollout_match_the_twin_at_65_lanes():
    import test_policy_gpu as P
    for seed in range(100):
        case = P._policy_case(seed, 8, [16, 16], 0.25, False, "auto", n_lanes=65)
        if case["feature"] == "config":
            break
    assert case["feature"] == "config" and case["n_lanes"] == 65
    case["pieces"] = [1] * case["n_steps"]
    mm = K.check(case, P.run_policy_case(case))
    assert not mm, (K.describe(case), len(mm), mm[:6])
