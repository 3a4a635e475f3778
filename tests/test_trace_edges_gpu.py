"""Outages, bursts and short traces on the device (tests/trace_families.py; the CPU side is tests/test_trace_edges_cpu.py).

Open loop: every product implementation (jump, split, split3, tick, auto) on every trace family, scripted and counter-based
random actions, step by step and fused in pieces that do not divide the video length, with and without auto_reset, under
the config speed, per-lane speeds and speed schedules, at lane counts off the workgroup sizes, and one large launch per
role-split kernel with sampled lanes compared in full.  Closed loop: a slice of family-swapped cases of both families of
tests/closed_loop_check.py through tools/gpu_fuzz_closed.py.  The episode sampler over pools of one-, two- and
three-sample traces.  The reference-generated fixture with zero runs (tests/golden/env_outage).  A dead (all-zero)
trace among live ones under a small max_ticks.

Everything is compared with the oracle by closed_loop_check's checkers: bitwise for every obs row (float32 of the
reference value: inf for a 1e300 sample), reward, done flag, frame field, history row and final state; average_latency
to 1e-9 and the episode QoE to 1e-10.  The oracle side of every comparison -- the replays, and each
case's max_ticks = the oracle's longest episode + 1000 -- is computed before the first launch of the case; every case is
built and run once.

Measured once on an MI355X with the whole GPU suite (profiles/trace_edges_fuzz.json): 350 runs in 345 cells, 4 515 982
lane-steps, 0 mismatches, no time-out on a live trace; 34.8 s wall, 27.6 s of it the closed-loop slice, most of that the
reference closed loop on the host that measures each case's max_ticks (the two older closed-loop slices: 5.8 s + 7.5 s).
The device agreed with the oracle everywhere: no kernel was changed."""
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from helpers import golden_rewards

sys.path.insert(0, os.path.join(ROOT, "tools"))

import closed_loop_check as K  # noqa: E402
import trace_families as TF  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = "env_outage"
REPORT = dict(lane_steps=0, cells={}, mismatches=0, cases=0, seconds={})


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The run's record (lane-steps, cells, mismatches, wall time per part), written as JSON where
    ABR_TRACE_EDGES_REPORT points when that is set (how profiles/trace_edges_fuzz.json is made)."""
    t0 = time.time()
    yield
    REPORT["seconds"] = {k: round(v, 2) for k, v in REPORT["seconds"].items()}
    REPORT["seconds"]["total"] = round(time.time() - t0, 1)             # the oracle side of every case included
    path = os.environ.get("ABR_TRACE_EDGES_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _count(key, lane_steps, mm, seconds):
    REPORT["lane_steps"] += int(lane_steps)
    REPORT["cells"][key] = REPORT["cells"].get(key, 0) + 1
    REPORT["mismatches"] += len(mm)
    REPORT["cases"] += 1
    part = key.split(":")[0]
    REPORT["seconds"][part] = REPORT["seconds"].get(part, 0.0) + seconds


def _check(case, out, stats=None):
    with np.errstate(over="ignore"):               # float32(1e300) = inf, compared as such
        return K.check(case, out, stats)


# ---------------------------------------------------------------------------------------------------------------------
# open loop

def run_open_case(case, impl):
    """One open-loop case (trace_families.open_loop_case) on implementation `impl`: closed_loop_check.check's `out`,
    the frames holding every observe_f64 row."""
    import abrsimulator_amd as A
    m = case["meta"]
    V, N, T = m["video_length"], case["n_lanes"], case["n_steps"]
    speed = m["speed"]
    if case["feature"] == "lanes":
        speed = torch.from_numpy(np.asarray(case["lane_speeds"], np.float64))
    elif case["feature"] == "schedule":
        speed = torch.from_numpy(np.ascontiguousarray(np.asarray(case["schedule"], np.float64).T))
    env = A.BatchedABREnv(A.MPD(V, m["chunk_length"], m["max_buffer"], m["start_up_length"], A.Chunk(m["ladder"])),
                          A.QOEMetric(*m["weights"]), A.NetworkInfo(m["interval"], case["traces"]), N, speed=speed,
                          impl=impl, auto_reset=case["auto_reset"], max_ticks=case["max_ticks"])
    env.reset(torch.from_numpy(case["tid"]), torch.from_numpy(case["off"]))
    script = case["script"]
    rows = np.stack([script[t if case["auto_reset"] else t % V] for t in range(T)])       # a finished lane ignores its row
    given = np.where((np.arange(T) < V)[:, None] | case["auto_reset"], rows, -1).astype(np.int32)
    dev = torch.from_numpy(rows).cuda()
    parts, frames, t = [], [], 0
    for n in case["pieces"]:
        if case["launch"] == "step":
            o, r, d = env.step(dev[t].contiguous())
            o = dict(obs=o[None], reward=r[None], done=d[None])
        elif case["launch"] == "script":
            o = env.step_script(dev[t:t + n])
        else:
            o = env.step_random(n, case["philox"])
        p = {k: o[k].cpu().numpy().copy() for k in ("obs", "reward", "done")}
        p["actions"] = o["actions"].cpu().numpy().copy() if case["launch"] == "random" else given[t:t + n]
        parts.append(p)
        t += n
        frames.append((t, {k: v.cpu().numpy().copy() for k, v in env.observe_f64().items()}))
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("actions", "reward", "done", "obs")}
    out["frames"] = frames
    out["history"] = tuple(x.cpu().numpy().copy() for x in env.history())
    out["qoe"] = env.episode_qoe().cpu().numpy()
    out["speed_log"] = out["entries"] = None
    torch.cuda.synchronize()
    env.close()
    return out


def frame_extras(case, frames, lanes=None):
    """What closed_loop_check.check leaves out of a frame: play_length, last_bandwidth (float64), last_bitrate and the
    three flags at every call site a piece ended on, against the oracle's records."""
    V = case["meta"]["video_length"]
    lanes = slice(None) if lanes is None else lanes
    bad = []
    for t, f in frames:
        e, s = (t // V, t % V) if case["auto_reset"] else (0, min(t, V))
        if s == V:
            continue                                               # the final state: check compares it
        steps = case["replays"][e][0]
        fl = f["flags"].astype(np.int32)
        for name, got, want in (("play_length", f["play_length"], steps["play_length"][lanes, s]),
                                ("last_bandwidth", f["last_bandwidth"], steps["last_bandwidth"][lanes, s]),
                                ("last_bitrate", f["last_bitrate"].astype(np.int32), steps["last_bitrate"][lanes, s]),
                                ("start_up", fl & 1, steps["start_up"][lanes, s]),
                                ("buffer_empty", (fl >> 1) & 1, steps["buffer_empty"][lanes, s]),
                                ("buffer_full", (fl >> 2) & 1, steps["buffer_full"][lanes, s])):
            if not np.array_equal(got, want):
                i = int(np.flatnonzero(got != want)[0])
                bad.append(dict(name="frame." + name, step=t, lane=i, value=got[i].item(), expected=want[i].item()))
    return bad


@pytest.mark.parametrize("family,k", TF.OPEN_SLICE, ids=[f"{f}-{k}" for f, k in TF.OPEN_SLICE])
def test_open_loop_every_implementation(family, k):
    case = TF.open_loop_case(family, k)                            # the oracle's replays: before any launch
    for impl in TF.open_impls(case["feature"]):
        t0 = time.time()
        out = run_open_case(dict(case, impl=impl), impl)
        mm = _check(case, out) + frame_extras(case, out["frames"])
        _count(f"open:{family}/{case['launch']}/{case['feature']}/{impl}", case["n_lanes"] * case["n_steps"], mm,
               time.time() - t0)
        assert not mm, (family, k, impl, case["launch"], case["feature"], case["auto_reset"], case["n_lanes"],
                        case["meta"], len(mm), mm[:6])


def subset_case(case, out, pick):
    """The lanes `pick` of an open-loop case and its run, as a case and `out` of their own."""
    sub = dict(case, n_lanes=len(pick), tid=case["tid"][pick], off=case["off"][pick], script=case["script"][:, pick],
               replays=[(s[pick], b[pick], f[pick], a[pick]) for s, b, f, a in case["replays"]])
    for key in ("lane_speeds", "schedule"):
        if key in case:
            sub[key] = np.asarray(case[key])[pick]
    o = dict(out)
    for key in ("actions", "reward", "done"):
        o[key] = out[key][:, pick]
    o["obs"] = out["obs"][:, :, pick]
    o["frames"] = [(t, {q: v[pick] for q, v in f.items()}) for t, f in out["frames"]]
    o["history"] = tuple(h[:, pick] for h in out["history"])
    o["qoe"] = out["qoe"][pick]
    return sub, o


@pytest.mark.parametrize("impl,lanes,family,k", TF.BIG_LAUNCHES, ids=[b[0] for b in TF.BIG_LAUNCHES])
def test_open_loop_large_launch_sampled_lanes(impl, lanes, family, k):
    """One large fused launch per role-split kernel; 512 lanes sampled across the index range are compared in full, and
    no lane anywhere times out (max_ticks is the oracle's longest episode over ALL lanes + 1000)."""
    case = TF.open_loop_case(family, k, n_lanes=lanes, config=TF.BIG_CONFIG)
    assert case["launch"] != "step" and case["auto_reset"]
    t0 = time.time()
    out = run_open_case(dict(case, impl=impl), impl)
    assert ((out["done"] & K.DONE_TIMEOUT) == 0).all()
    V = case["meta"]["video_length"]
    want_done = (np.arange(case["n_steps"]) % V == V - 1).astype(np.uint8)
    assert (out["done"] == want_done[:, None]).all()
    pick = np.sort(np.random.default_rng(5).choice(lanes, 512, replace=False))
    pick[:2], pick[-2:] = (0, 1), (lanes - 2, lanes - 1)
    sub, o = subset_case(case, out, pick)
    mm = _check(sub, o) + frame_extras(sub, o["frames"])
    _count(f"open_large:{family}/{case['launch']}/{case['feature']}/{impl}", lanes * case["n_steps"], mm, time.time() - t0)
    assert not mm, (impl, lanes, len(mm), mm[:6])


# ---------------------------------------------------------------------------------------------------------------------
# closed loop

def test_closed_loop_slice_on_every_family():
    """Every (controller, family) pair at least twice -- seven controllers, four speed features, four episode modes --
    through gpu_fuzz_closed.run_seed / run_episode_seed with traces=family; the slice's edges, counted on the reference's
    own runs (never on the device's), are the non-vacuity conditions of tests/test_trace_edges_cpu.py."""
    import gpu_fuzz_closed
    pairs, total, short, impls = {}, {}, {}, set()
    for kind, seed, fam in TF.closed_slice():
        t0 = time.time()
        if kind == "episodes":
            mm, ls, key, case = gpu_fuzz_closed.run_episode_seed(seed, TF.CLOSED_EPISODE_LANES, None, traces=fam)
        else:
            mm, ls, key, case = gpu_fuzz_closed.run_seed(seed, None, None, traces=fam)
        _count(f"closed:{fam}/{key}/{case['impl']}", ls, mm, time.time() - t0)
        assert not mm, (fam, (K.describe_ep if kind == "episodes" else K.describe)(case), len(mm), mm[:6])
        pairs[(case["ctl"], fam)] = pairs.get((case["ctl"], fam), 0) + 1
        impls.add(case["impl"])
        TF.add_stats(total, case["edge_stats"])
        if fam == "short":
            TF.add_stats(short, case["edge_stats"])
    assert set(pairs) == {(c, f) for c in K.EP_CONTROLLERS for f in TF.FAMILIES} and min(pairs.values()) >= 2
    assert impls == set(TF.OPEN_IMPLS)
    assert total["zero_start"] >= 0.05 * total["decisions"] and total["hist_burst"] >= 0.03 * total["hist"], total
    assert short["wrapped2"] >= 0.25 * short["lanes"] > 0, short
    REPORT["closed_edge_stats"] = total


# ---------------------------------------------------------------------------------------------------------------------
# the episode sampler over pools of very short traces

SAMPLER_CASES = [  # (episode-family seed of mode "sampled", impl, pool, offset_span)
    (12, "tick", None, 0),              # buffer / config
    (12 + 112, "jump", [0, 2, 2, 1], 1),
    (0, "split3", None, 5),             # mpc / config
    (0 + 112, "split", [1], 0),
    (24, "auto", [4, 0, 3], 1000),      # policy / config
    (17, "jump", None, 2),              # rate / lanes
]


@pytest.mark.parametrize("seed,impl,pool,span", SAMPLER_CASES, ids=[f"{s}-{i}" for s, i, _, _ in SAMPLER_CASES])
def test_episode_sampler_over_one_two_and_three_sample_traces(seed, impl, pool, span):
    """episodes() after every operation against the sampler's twin, and every episode replayed through the oracle from
    the twin's (trace, offset): traces of 1, 2, 3, 1 and 2 samples, offset_span 0, 1, 2, 5 and above every length."""
    import gpu_fuzz_closed
    base = K.make_episode_case(seed, TF.CLOSED_EPISODE_LANES)
    assert base["mode"] == "sampled" and impl in K.accepted_impls_ep(base["ctl"], base["feature"])
    base = dict(base, impl=impl, sampler=dict(seed=base["sampler"]["seed"], pool=pool, span=span))
    case = TF.with_traces(base, "short", seed, lengths=(1, 2, 3, 1, 2))
    t0 = time.time()
    stats = {}
    out = gpu_fuzz_closed.run_episode_case(case)
    mm = K.check_episodes(case, out, stats)
    _count(f"sampler:{case['ctl']}/{impl}/span{span}", case["n_lanes"] * case["n_steps"], mm, time.time() - t0)
    assert not mm, (K.describe_ep(case), len(mm), mm[:6])
    last = out["episodes"][-1]                       # every lane has been re-armed twice by now: the sampler's pairs
    assert last["episode"].min() >= 2
    assert {int(t) for t in last["trace_id"]} == (set(pool) if pool else set(range(5)))
    tl = np.array([len(t) for t in case["traces"]])[last["trace_id"]]
    assert (last["start_offset"] < (np.minimum(span, tl) if span else tl)).all()
    assert stats.get("wrapped", 0) > 0


# ---------------------------------------------------------------------------------------------------------------------
# the fixture: the reference itself over zero runs

@pytest.mark.parametrize("impl", TF.OPEN_IMPLS)
def test_fixture_step_by_step(impl):
    import test_env_gpu
    test_env_gpu.test_step_matches_reference_goldens(FIXTURE, impl)


@pytest.mark.parametrize("impl", TF.OPEN_IMPLS)
def test_fixture_fused(impl):
    """One scripted launch of the whole episode: every obs row, reward and done flag against the reference's frames."""
    from helpers import make_env
    m, g = load_golden(FIXTURE)
    N, V = g["actions"].shape
    env = make_env(m, g["traces"], N, impl=impl)
    env.reset(torch.from_numpy(g["trace_id"]), torch.from_numpy(g["offset"]))
    out = {k: v.cpu().numpy() for k, v in env.step_script(torch.from_numpy(g["actions"].T.copy()).cuda()).items()
           if v is not None}
    assert np.array_equal(out["reward"].T, golden_rewards(m, g))
    assert (out["done"][:-1] == 0).all() and (out["done"][-1] == 1).all()
    rows = dict(chunk_id="chunk_id", last_bitrate="arg_last_bitrate", last_bandwidth="arg_last_bandwidth",
                buffer_level="buffer_level", global_time="global_time", play_time="play_time",
                rebuffer_time="rebuffer_time", start_up_time="start_up_time")
    for r, key in enumerate(K.OBS):
        for s in range(V - 1):
            assert np.array_equal(out["obs"][s, r], g[rows[key]][:, s + 1].astype(np.float32)), (impl, key, s)
    f = env.observe_f64()
    for key in ("global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level"):
        assert np.array_equal(f[key].cpu().numpy(), g["final_" + key]), (impl, key)
    assert np.array_equal(env.history()[1].cpu().numpy().T, g["final_bandwidths"])
    assert np.allclose(env.episode_qoe().cpu().numpy(), g["final_qoe"], rtol=1e-10, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# a dead trace among live ones

def dead_trace_case(auto_reset):
    """192 lanes, every third one on an all-zero trace, so that every wave mixes dead and live lanes; max_ticks =
    (V + 2) * chunk_ticks + 1000.  The live lanes' expected run is the oracle's, under the same bound."""
    V, L, N = 6, 2.0, 192
    mt = (V + 2) * 200 + 1000
    rng = np.random.default_rng(2026)
    live = []
    for _ in range(3):
        t = rng.uniform(3.0, 9.0, 120).astype(np.float32).astype(np.float64)
        t[rng.random(120) < 0.08] = 0.0                            # outages of one sample on the live traces too
        live.append(t)
    traces = [np.zeros(50)] + live
    tid = np.where(np.arange(N) % 3 == 0, 0, 1 + np.arange(N) % 3).astype(np.int32)
    tid[64:70] = 0                                                  # and six dead lanes in a row
    off = rng.integers(0, 50, N).astype(np.int32)
    meta = dict(ladder=[0.3, 0.75, 1.2, 1.85, 2.85, 4.3], chunk_length=L, video_length=V, max_buffer=8.0,
                start_up_length=2.0, interval=0.5, weights=[4.3, 1.0, 1.0, 0.1], speed=1.0)
    T = 2 * V + 3 if auto_reset else V + 2
    n_ep = -(-T // V) if auto_reset else 1
    script = rng.integers(0, 6, (n_ep * V, N)).astype(np.int32)
    case = dict(seed=0, ctl="script", feature="config", impl=None, vbr=False, auto_reset=auto_reset, n_lanes=N,
                meta=meta, traces=traces, tid=tid, off=off, br=None, params={}, n_steps=T, script=script,
                launch="script", philox=0, trace_family="dead", max_ticks=mt,
                pieces=[4, 5, T - 9] if auto_reset else [3, T - 3])
    from oracle import oracle as O
    alive = np.flatnonzero(tid != 0)
    case["replays"] = []
    for e in range(n_ep):
        a = np.ascontiguousarray(script[e * V:(e + 1) * V].T)
        steps = np.zeros((N, V), O.STEP_DTYPE)
        bw, fin = np.zeros((N, V)), np.zeros(N, O.FINAL_DTYPE)
        steps[alive], bw[alive], fin[alive], _ = O.env_batch(K.env_cfg(case), traces, tid[alive], off[alive], a[alive],
                                                             max_ticks=mt)          # raises if a live lane ran out
        case["replays"].append((steps, bw, fin, a))
    # the oracle on a dead lane: out of ticks (rc -2) at tick max_ticks, before its first chunk is down
    with pytest.raises(RuntimeError, match="-2"):
        O.env_batch(K.env_cfg(case), traces, tid[:1], off[:1], script[:V, :1].T.copy(), max_ticks=mt)
    return case, alive, np.flatnonzero(tid == 0)


@pytest.mark.parametrize("auto_reset", [False, True], ids=["plain", "auto_reset"])
def test_dead_trace_times_out_at_the_oracles_tick_and_leaves_live_lanes_alone(auto_reset):
    """Lanes on the all-zero trace report ABR_DONE_TIMEOUT at their first decision (the oracle runs out of ticks there,
    at tick max_ticks), identically on every implementation, fused and step by step; they are not re-armed.  The live
    lanes of the same waves equal the oracle's run in full."""
    case, alive, dead = dead_trace_case(auto_reset)
    mt = case["max_ticks"]
    g = 0.0
    for _ in range(mt):
        g += 0.01                                                   # global_time after max_ticks ticks (Simulator.py:205)
    ref = None
    for impl in TF.OPEN_IMPLS:
        for launch in (("script",) if auto_reset else ("script", "step")):
            t0 = time.time()
            c = dict(case, impl=impl, launch=launch, pieces=case["pieces"] if launch == "script" else [1] * case["n_steps"])
            out = run_open_case(c, impl)
            sub, o = subset_case(c, out, alive)
            mm = _check(sub, o) + frame_extras(sub, o["frames"])
            _count(f"dead:{launch}/{impl}", case["n_lanes"] * case["n_steps"], mm, time.time() - t0)
            assert not mm, (impl, launch, len(mm), mm[:6])
            d = out["done"][:, dead]
            assert ((d & K.DONE_TIMEOUT) != 0).all() and (d == d[0]).all(), (impl, launch, np.unique(d))
            assert (out["reward"][1:, dead] == 0).all()
            fin = out["frames"][-1][1]
            assert (fin["chunk_id"][dead] == 0).all()
            if impl != "tick":                  # the tick kernel freezes a timed-out lane at a block boundary
                assert (fin["tick"][dead] == mt).all() and (fin["global_time"][dead] == g).all(), (impl, launch)
                key = (out["obs"][:, :, dead], out["reward"][:, dead], {q: v[dead] for q, v in fin.items()})
                if ref is None:
                    ref = key
                assert np.array_equal(key[0], ref[0]) and np.array_equal(key[1], ref[1]), (impl, launch)
                for q in ref[2]:
                    assert np.array_equal(key[2][q], ref[2][q], equal_nan=True), (impl, launch, q)
