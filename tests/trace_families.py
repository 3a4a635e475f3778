"""Bandwidth-trace families at the edges of the accepted domain (finite, >= 0, length >= 1) -- TEST INFRASTRUCTURE.

Every other generator of the suite draws comfortable positive samples from long traces.  The families here hold what
real throughput logs hold and what changes the character of the event-driven download: zeros and multi-sample outages
(c = 0: no progress, no jump), samples so small that an interval adds less than an ulp of downloaded_size, samples so
large that a chunk finishes on its first tick, and traces of one, two or three samples that wrap at every interval.
Seeded, pure numpy; every value is float32-representable float64 (the `extreme` family excepted: subnormals and 1e300
exist in float64 only) and every trace keeps at least one sample above MIN_LIVE, so the reference finishes.

make(family, rng, length)         one trace
with_traces(case, family, seed)   a closed_loop_check case (either family) on traces of one family, max_ticks measured
                                  on the reference's own closed loop
edge_stats(case, steps, bw, fin)  how often an oracle replay met each edge (non-vacuity counters)"""
import numpy as np

FAMILIES = ("outage", "sparse_zero", "tiny", "burst", "mixed", "short", "constant")    # closed and open loop
OPEN_LOOP_FAMILIES = FAMILIES + ("extreme",)
SHORT_LENGTHS = (1, 2, 3, 7)
MIN_LIVE = 0.05
TINY = (1e-3, 1e-6, 1e-12)
BURST = (1e3, 1e4, 1e6)
EXTREME = (5e-324, 1e-310, 1e300)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _base(rng, length):
    """A playable trace: uniform samples between lo and 3..10 lo, lo in {0.3, 1, 2}."""
    lo = float(rng.choice([0.3, 1.0, 2.0]))
    return _f32(rng.uniform(lo, lo * float(rng.choice([3.0, 10.0])), length))


def _keep_live(rng, t, base):
    """At least one sample above MIN_LIVE (position drawn from rng)."""
    if not (t > MIN_LIVE).any():
        i = int(rng.integers(0, len(t)))
        t[i] = base[i]
    return t


def _mix(rng, length, values, share):
    base = _base(rng, length)
    t = np.where(rng.random(length) < share, rng.choice(np.asarray(values, np.float64), length), base)
    return _keep_live(rng, t, base)


def _outage(rng, length):
    base = _base(rng, length)
    t = base.copy()
    starts = np.flatnonzero(rng.random(length) < 0.12)
    for s, n in zip(starts, rng.integers(1, 12, len(starts))):
        t[s:s + n] = 0.0
    return _keep_live(rng, t, base)


def _constant(rng, length):
    v = float(rng.choice([0.06, 0.3, 1.0, 2.5, 7.0, 1e3]))
    return np.full(length, float(_f32(v)))


_MAKERS = {
    "outage": _outage,
    "sparse_zero": lambda rng, n: _mix(rng, n, (0.0,), 0.3),
    "tiny": lambda rng, n: _mix(rng, n, _f32(TINY), 0.3),
    "burst": lambda rng, n: _mix(rng, n, BURST, 0.3),
    "mixed": lambda rng, n: _mix(rng, n, (0.0, float(_f32(1e-6)), 1e6), 0.45),
    "constant": _constant,
    "extreme": lambda rng, n: _mix(rng, n, EXTREME, 0.3),
}
_CUT = ("outage", "sparse_zero", "tiny", "burst", "mixed")


def make(family, rng, length):
    """One trace of `family`, float64 [length].  `short` draws one of the first five families at 16 samples and cuts it
    to `length` when that is one of SHORT_LENGTHS, else to a length drawn from them."""
    if family == "short":
        n = int(length) if int(length) in SHORT_LENGTHS else int(rng.choice(SHORT_LENGTHS))
        full = _MAKERS[str(rng.choice(_CUT))](rng, 16)
        return _keep_live(rng, full[:n].copy(), _base(rng, n))
    t = np.ascontiguousarray(_MAKERS[family](rng, int(length)), np.float64)
    assert len(t) == length and np.isfinite(t).all() and (t >= 0).all() and (t > MIN_LIVE).any()
    return t


def make_pool(family, rng, lengths):
    """One trace per entry of `lengths` (`short`: lengths from SHORT_LENGTHS; `constant`: the first one has length 1)."""
    out = []
    for j, n in enumerate(lengths):
        if family == "constant" and j == 0:
            n = 1
        out.append(make(family, rng, n))
    return out


def with_traces(case, family, seed, lengths=None):
    """The closed_loop_check case `case` (make_case or make_episode_case) on traces of `family`: the same number of
    traces, every start offset folded into the new lengths, and max_ticks = the largest tick count of an episode of the
    reference's own closed loop + 1000 (measured on the oracle, never on the device); that run and its edge_stats stay on
    the case ("reference", "edge_stats").  The case given is not modified."""
    rng = np.random.default_rng([int(seed), OPEN_LOOP_FAMILIES.index(family), 4242])
    old = [len(t) for t in case["traces"]]
    lens = [min(n, 600) for n in old]                   # outages stretch an episode over many samples already
    traces = make_pool(family, rng, lens) if lengths is None else [make(family, rng, n) for n in lengths]
    assert len(traces) == len(old)
    tl = np.array([len(t) for t in traces], np.int64)
    out = dict(case, traces=traces, trace_family=family)
    out["off"] = (case["off"] % tl[case["tid"]]).astype(np.int32)
    if "ops" in case:
        out["ops"] = [op if op[0] != "reset" or op[2] is None else
                      ("reset", op[1], op[2], (op[3] % tl[op[2]]).astype(np.int32)) for op in case["ops"]]
    ticks, out["edge_stats"], out["reference"] = reference_run(out)
    out["max_ticks"] = ticks + 1000
    return out


def reference_run(case):
    """The reference closed loop of `case` (either family) replayed through the oracle: (the largest tick count of one
    episode, edge_stats over every replayed episode, the run in the layout closed_loop_check's checkers take)."""
    import closed_loop_check as K
    ent = K.OracleEntries(case) if case["ctl"] == "fastmpc" else None
    V, N, B = case["meta"]["video_length"], case["n_lanes"], len(case["meta"]["ladder"])
    top, st = 0, None
    if "ops" in case:
        out = K.oracle_run_episodes(case, ent)
        segs, _ = K.episode_plan(case)
        for k in range(max(len(s) for s in segs)):
            segs_k = [s[k] for s in segs if len(s) > k]
            steps, bw, fin = K._run_batch(case, segs_k, K._padded_actions(case, segs_k, out["actions"]))[:3]
            top = max(top, int(fin["ticks"].max()))
            st = edge_stats(case, steps, bw, fin, tid=[s.trace for s in segs_k], off=[s.offset for s in segs_k],
                            n=[s.n for s in segs_k], into=st)
        return top, st, out
    out = K.oracle_run(case, ent)
    T = case["n_steps"]
    speeds = K.lane_speeds_for(case, out.get("speed_log"))
    for e in range(-(-T // V) if case["auto_reset"] else 1):
        n = min(V, T - e * V)
        a = np.zeros((N, V), np.int32)
        a[:, :n] = np.clip(out["actions"][e * V:e * V + n].T, 0, B - 1)
        steps, bw, fin = K.replay(case, a, speeds)
        top = max(top, int(fin["ticks"].max()))
        st = edge_stats(case, steps, bw, fin, n=np.full(N, n), into=st)
    return top, st, out


EDGE_KEYS = ("decisions", "zero_start", "hist", "hist_burst", "hist_starved", "lanes", "wrapped2", "rebuffered")


def edge_stats(case, steps, bw, fin, tid=None, off=None, n=None, into=None):
    """Counters of the edges an oracle replay met, from the replay alone (steps / bw [N, V], fin [N] of
    oracle.env_batch on the case's traces; tid / off: the lanes' pairs when they are not the case's own; n: the
    decisions each lane took of its episode when not all V).  Added into `into` when given.  Keys: decisions,
    zero_start (decisions whose download starts in a zero interval), hist, hist_burst (history entries >= 1e3: the
    chunk came down on its first ticks), hist_starved (entries below the lowest rung / 4: the download sat through an
    outage), lanes (whole episodes), wrapped2 (of those, episodes that wrap their trace twice or more), rebuffered (of
    those, lanes that stalled after start-up)."""
    m = case["meta"]
    tid = case["tid"] if tid is None else np.asarray(tid)
    off = case["off"] if off is None else np.asarray(off)
    N, V = bw.shape
    n = np.full(N, V) if n is None else np.asarray(n)
    s = dict.fromkeys(EDGE_KEYS, 0) if into is None else into
    lowest = float(np.min(case["br"])) if case.get("br") is not None else float(min(m["ladder"]))
    took = np.arange(V)[None, :] < n[:, None]
    for i in range(N):
        t = case["traces"][int(tid[i])]
        idx = (steps["global_time"][i] / m["interval"]).astype(np.int64)
        s["zero_start"] += int(((t[(int(off[i]) + idx) % len(t)] == 0.0) & took[i]).sum())
        if n[i] == V:
            last = int(fin["global_time"][i] / m["interval"])
            s["wrapped2"] += int((int(off[i]) + last) // len(t) >= 2)
    whole = n == V
    s["decisions"] += int(took.sum())
    s["hist"] += int(took.sum())
    s["hist_burst"] += int(((bw >= 1e3) & took).sum())
    s["hist_starved"] += int(((bw < lowest / 4) & took).sum())
    s["lanes"] += int(whole.sum())
    s["rebuffered"] += int((fin["rebuffer_time"][whole] > 0).sum())
    return s


def add_stats(total, st):
    for k in EDGE_KEYS:
        total[k] = total.get(k, 0) + st[k]
    return total


# ---------------------------------------------------------------------------------------------------------------------
# the committed slices (tests/test_trace_edges_cpu.py checks their coverage on the oracle, tests/test_trace_edges_gpu.py
# runs them on the device)

OPEN_IMPLS = ("jump", "split", "split3", "tick", "auto")
OPEN_LANES = (64, 100, 127, 130, 192)
OPEN_LAUNCHES = ("step", "script", "random")      # env.step per decision; step_script / step_random in pieces
OPEN_SPEEDS = ("config", "lanes", "schedule")
TICK_ORACLE_BOUND = 40_000_000                     # the oracle's own bound while the case's max_ticks is measured


def open_impls(feature):
    """The impls an open-loop case runs on: the tick kernel serves neither per-lane speeds nor schedules
    (tests/test_env_gpu.py: CAPABILITY)."""
    return [k for k in OPEN_IMPLS if k != "tick" or feature == "config"]


def open_loop_case(family, k, n_lanes=None, config=None):
    """Open-loop case k of `family` in closed_loop_check's config-family layout with the controller "script": a
    configuration of test_lane_jump_cpu._random_config, five traces of the family, a speed feature, a launch kind, with
    or without auto_reset, pieces that do not divide V, and the actions of every decision known before the launch.
    case["replays"]: the oracle's (steps, bw, fin, actions) per episode, computed here."""
    import closed_loop_check as K
    from oracle import oracle as O
    from test_lane_jump_cpu import _random_config
    fi = OPEN_LOOP_FAMILIES.index(family)
    rng = np.random.default_rng([int(k), fi, 777])
    meta, _ = _random_config(rng)
    if config:
        meta.update(config)
    V, B = meta["video_length"], len(meta["ladder"])
    feature = OPEN_SPEEDS[(k + fi) % 3]
    launch = OPEN_LAUNCHES[(k // 2 + fi) % 3]
    auto_reset = launch != "step" and (k + fi // 3) % 2 == 1
    N = int(n_lanes or OPEN_LANES[(k + fi) % len(OPEN_LANES)])
    traces = make_pool(family, rng, rng.integers(8, 400, 5))
    tl = np.array([len(t) for t in traces])
    tid = rng.integers(0, len(traces), N).astype(np.int32)
    off = (rng.integers(0, 1 << 20, N) % tl[tid]).astype(np.int32)
    T = (2 * V + 1 + int(rng.integers(0, max(1, V - 1)))) if auto_reset else (V + 2 if launch != "random" else V)
    if launch == "step":
        pieces = [1] * T
    else:
        cuts = sorted({int(x) for x in rng.integers(1, T, max(1, T // 4))} - {j * V for j in range(1, T // V + 1)})
        pieces = np.diff([0] + cuts + [T]).tolist()
    n_ep = -(-T // V) if auto_reset else 1
    philox = int(rng.integers(1, 1 << 62))
    if launch == "random":
        script = np.stack([O.philox_action(philox, np.arange(N), t % V, t // V, B) for t in range(n_ep * V)])
    else:
        script = rng.integers(0, B, (n_ep * V, N)).astype(np.int32)
    if feature != "config":
        meta["speed"] = 1.0
    case = dict(seed=k, ctl="script", feature=feature, impl=None, vbr=False, auto_reset=auto_reset, n_lanes=N,
                meta=meta, traces=traces, tid=tid, off=off, br=None, params={}, pieces=pieces, n_steps=T,
                script=script, launch=launch, philox=philox, trace_family=family)
    if feature == "lanes":
        case["lane_speeds"] = rng.choice([0.6, 0.8, 1.0, 1.25, 1.7, 0.9173], N)
    elif feature == "schedule":
        case["schedule"] = rng.choice([0.5, 0.75, 1.0, 1.1, 1.25, 1.5, 2.0], (N, int(rng.integers(2, 7))))
    speeds = K.lane_speeds_for(case, None)
    case["replays"] = []
    for e in range(n_ep):
        a = np.ascontiguousarray(script[e * V:(e + 1) * V].T)
        steps, bw, fin, _ = O.env_batch(K.env_cfg(case), traces, tid, off, a, speeds=speeds,
                                        max_ticks=TICK_ORACLE_BOUND, threads=_threads())
        case["replays"].append((steps, bw, fin, a))
    case["max_ticks"] = max(int(r[2]["ticks"].max()) for r in case["replays"]) + 1000
    case["edge_stats"] = None
    for steps, bw, fin, _ in case["replays"]:
        case["edge_stats"] = edge_stats(case, steps, bw, fin, into=case["edge_stats"])
    return case


def open_loop_expected(case):
    """The oracle's replays of an open-loop case laid out as a device run (closed_loop_check.check's `out`)."""
    import closed_loop_check as K
    from helpers import oracle_rewards
    m = case["meta"]
    V, N, T = m["video_length"], case["n_lanes"], case["n_steps"]
    out = dict(actions=np.full((T, N), -1, np.int32), reward=np.zeros((T, N), np.float32),
               done=np.ones((T, N), np.uint8), obs=np.zeros((T, len(K.OBS), N), np.float32), frames=[])
    for e, (steps, bw, fin, acts) in enumerate(case["replays"]):
        rw = oracle_rewards(steps, fin, acts, m["weights"], ladder=m["ladder"])
        for s in range(min(V, T - e * V)):
            t = e * V + s
            out["actions"][t], out["reward"][t], out["done"][t] = acts[:, s], rw[:, s], 1 if s == V - 1 else 0
            if s < V - 1 or case["auto_reset"]:
                out["obs"][t] = _to_f32(np.stack([steps[k][:, s + 1 if s < V - 1 else 0] for k in K.OBS]))
            else:
                term = [fin["chunk_id"], acts[:, V - 1], bw[:, V - 1], fin["buffer_level"], fin["global_time"],
                        fin["play_time"], fin["rebuffer_time"], fin["start_up_time"]]
                out["obs"][t:] = _to_f32(np.stack(term))[None]
    keys = K.FRAME + ("play_id", "chunk_id", "average_latency")
    for t in np.cumsum(case["pieces"]):
        e, s = (t // V, t % V) if case["auto_reset"] else (0, min(t, V))
        steps, bw, fin, acts = case["replays"][e]
        f = {k: np.asarray(fin[k] if s == V else steps[k][:, s]).copy() for k in keys}
        f["hist_n"], f["hist_sum_inv"] = K._hist_summary(case, bw, s)
        out["frames"].append((int(t), f))
    steps, bw, fin, acts = case["replays"][-1]
    prev = case["replays"][-2] if len(case["replays"]) > 1 else case["replays"][-1]
    ha, hb = prev[3].T.astype(np.uint8).copy(), prev[1].T.copy()
    c = T - (len(case["replays"]) - 1) * V if case["auto_reset"] else V
    ha[:c], hb[:c] = acts.T[:c], bw.T[:c]
    out["history"] = (ha, hb)
    done = [r for j, r in enumerate(case["replays"]) if (j + 1) * V <= T]
    out["qoe"] = done[-1][2]["qoe"].copy()
    out["speed_log"] = out["entries"] = None
    return out


def _to_f32(x):
    """float32(x); a 1e300 sample of the `extreme` family reads inf there, as on the device."""
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float32)


def _threads():
    from helpers import threads
    return threads()


OPEN_PER_FAMILY = 6        # the launch kind changes every second k, auto_reset and the speed feature with every k
OPEN_SLICE = [(f, k) for f in OPEN_LOOP_FAMILIES for k in range(OPEN_PER_FAMILY)]
# one large launch per role-split kernel, on a configuration whose episodes stay short
BIG_CONFIG = dict(ladder=[0.3, 0.75, 1.2, 1.85, 2.85, 4.3], chunk_length=2.0, video_length=8, max_buffer=6.0,
                  start_up_length=2.0, interval=0.5, speed=1.0)
BIG_LAUNCHES = (("split3", 65_536, "outage", 3), ("split", 131_072, "mixed", 2))    # impl, lanes, family, case k


CLOSED_EPISODE_LANES = 64     # one full wave: the reference closed loop runs lane by lane in Python, on the GPU box too


def closed_slice():
    """The closed-loop slice: (kind, seed, family) with kind "config" (make_case) or "episodes" (make_episode_case).
    The episode family covers every (controller, family) pair twice -- the learned policy included -- while the speed
    feature and the episode mode rotate through all four of each per controller, at CLOSED_EPISODE_LANES lanes; the
    config family adds three cases per family at its own lane counts (off the workgroup sizes), its six controllers
    rotating, with and without auto_reset and per-chunk ladders."""
    import closed_loop_check as K
    out = []
    for rep in range(2):
        for fi, fam in enumerate(FAMILIES):
            for ci in range(len(K.EP_CONTROLLERS)):
                j = rep * len(FAMILIES) + fi
                feature, mode = (j + ci) % 4, (j // 4 + ci + rep) % 4
                out.append(("episodes", ci * 4 + feature + len(K.EP_CELLS) * (mode + 4 * ((j + ci) % 3)), fam))
    for fi, fam in enumerate(FAMILIES):
        for r in range(3):
            ci = (fi * 3 + r) % len(K.CONTROLLERS)
            feature = (fi + r) % 4
            out.append(("config", ci * 4 + feature + len(K.CELLS) * ((fi + 2 * r) % 6), fam))
    return out


def closed_case(kind, seed, family):
    import closed_loop_check as K
    base = K.make_episode_case(seed, CLOSED_EPISODE_LANES) if kind == "episodes" else K.make_case(seed)
    return with_traces(base, family, seed)
