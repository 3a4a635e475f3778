"""Config-space fuzz of the closed-loop rollouts: case generators and checkers (host only; the GPU runner is
tools/gpu_fuzz_closed.py, the slices tests/test_closed_loop_fuzz_gpu.py and tests/test_closed_loop_episodes_gpu.py).

Two case families.  The config family (make_case / check) is one random configuration (ladder, chunk length, video
length, buffer limit, start-up length, trace interval, ragged traces with wrap-around), one controller evaluated on the
device (harmonic MPC, RobustMPC, FastMPC, BBA-0, RATE, BOLA), one speed feature (the config speed, per-lane speeds, a
speed schedule, a LatencySpeedController), a per-chunk ladder or not, a lane count, a kernel implementation the
combination is accepted by, and a launch split into pieces; every lane runs episode e over decisions [eV, (e+1)V).  The
episode family (make_episode_case / check_episodes, further below) adds the learned policy as a seventh controller, an
episode sampler, lane_id_base, and masked resets that stagger the lanes: each lane's run is a list of segments of its own.

Why checking (a) and (b) together proves the closed loop.  Let F_i(s) be lane i's frame at its s-th call site of an
episode.  (a) replays the device's actions A_i through the C oracle (with the speeds the lane played) and compares every
frame, reward, done flag, the history and the final state: the device's frames equal F_i(s | A_i).  (b) asks the
reference controller (the oracle's brute-force MPC search with the harmonic (n, S) carried as in oracle_mpc_policy,
tests/robust_twin.py, tests/fastmpc_twin.py on the device-built table, tests/rules_twin.py, tests/policy_twin.py) for its
answer at every one of those replayed frames and requires A_i(s) to equal it.  By induction over s: frame 0 depends on
nothing the controller did; if the device's first s actions are the reference's answers, the frame at call site s is the
reference closed loop's frame at s (by (a)), so the reference's answer there is A_i(s) (by (b)).  Hence the whole run is
the reference closed loop, whatever the speed feature.  A replay alone (a) would accept any action sequence, e.g. one
computed from a stale buffer level.  Under the speed rule the speeds themselves are device outputs (the log): (c) checks
every lane's log against the oracle's rule mode (abr_oracle.c: oracle_speed_rule, pinned to the tick-loop twin
tests/speed_twin.py), which closes the same loop for the speeds.
(d) Without auto_reset a finished lane answers -1, reports its terminal record again and its state does not move.

The controller "script" (ScriptReference) is the open loop in the same layout: the action of every decision is known
before the launch (a scripted rollout, or the counter-based random policy's draw), so (b) pins the actions the device
reports and (a), (d) and the frames check everything else (tests/trace_families.py: open_loop_case).

Edges (build-defined, include/abr_env.h): an empty history answers bitrate 0 (D13); near the video end every MPC search
runs at the clipped horizon V - c (D12).  Under auto_reset a lane restarts from its own trace and offset, or the
sampler's pair for its next episode number: the harmonic (n, S) restarts, RobustMPC's state empties itself at chunk 0
(carried across episodes here, as on the device), RATE and FastMPC read the current episode's history only.  A speed
rule's log holds the lane's current episode only, so the config family pairs the speed rule with auto_reset off; the
episode family runs the rule under auto_reset and masked resets, and checks the log after every operation (rows the
current episode wrote, rows it has not reached as the earlier episodes left them)."""
import numpy as np

from oracle import oracle as O
from oracle.pyloop import PyTickEnv
from helpers import oracle_env_cfg, oracle_rewards, threads
import fastmpc_twin
import robust_twin
import rules_twin
from speed_twin import rule_np

CONTROLLERS = ("mpc", "robust", "fastmpc", "buffer", "rate", "bola")
SPEEDS = ("config", "lanes", "schedule", "rule")
CELLS = [(c, f) for c in CONTROLLERS for f in SPEEDS]          # cell = seed % 24
LANES = (64, 100, 128, 130, 127, 192)
GRID_CAP = 4096                                                 # n_rates ** horizon: the oracle's brute force stays cheap
RULE_KIND = {"buffer": rules_twin.BUFFER, "rate": rules_twin.RATE, "bola": rules_twin.BOLA}
FRAME = ("global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level")
OBS = ("chunk_id", "last_bitrate", "last_bandwidth", "buffer_level", "global_time", "play_time", "rebuffer_time",
       "start_up_time")                                         # abrsimulator_amd._lib.OBS_ROWS
DONE_TIMEOUT = 2                                                # include/abr_env.h: ABR_DONE_TIMEOUT


def accepted_impls(ctl, feature):
    """The product impls that accept this combination (abr_env.hip: kFeatures; tests/test_env_gpu.py's table)."""
    if ctl in ("mpc", "robust"):
        return ["jump", "split", "split3", "auto"]              # the fused MPC rollout: every event-driven kernel
    return ["jump", "auto"] if feature != "config" else ["jump", "tick", "auto"]   # rule rollouts: one thread per lane


# ---------------------------------------------------------------------------------------------------------------------
# the generator

def make_case(seed, n_lanes=None):
    """A deterministic case description (plain Python / numpy values)."""
    rng = np.random.default_rng(70_000 + seed)
    ctl, feature = CELLS[seed % len(CELLS)]
    rnd = seed // len(CELLS)
    impls = accepted_impls(ctl, feature)
    impl = impls[rnd % len(impls)]
    vbr = rnd % 2 == 1
    auto_reset = (rnd // 2) % 2 == 1 and feature != "rule"
    L = float(rng.choice([1.0, 2.0, 2.5, 3.0, 4.0, 6.0]))
    interval = float(rng.choice([0.05, 0.25, 0.3, 0.5, 0.7, 1.0, 2.0, 3.7]))
    B = int(rng.integers(1, 9)) if rng.random() < 0.8 else int(rng.integers(9, 17))
    ladder = np.sort(rng.uniform(0.2, 8.0, B)).round(3)
    ladder = np.maximum.accumulate(np.maximum(ladder, 0.2)).tolist()
    if B >= 2 and rng.random() < 0.2:
        ladder[1] = ladder[0]                                   # a tie at the bottom: "highest rate <= x" picks 1
    max_buffer = float(rng.choice([L * 0.6, L * 1.2, L * 1.5, L * 1.9, L * 3, 7.3, 20.0]))
    start_up = float(min(max_buffer, rng.choice([0.0, L, 1.7])))
    speed = float(rng.choice([0.8, 1.0, 1.25]))
    V = int(rng.integers(2, 25))
    bw_lo = float(rng.choice([0.1, 0.5, 2.0] if feature != "rule" else [0.5, 2.0]))
    bw_hi = bw_lo * float(rng.choice([3.0, 10.0, 40.0]))
    N = int(n_lanes if n_lanes is not None else LANES[rnd % len(LANES)])
    n_traces = 5
    lens = rng.integers(40, 3000, n_traces)
    traces = [rng.uniform(bw_lo, bw_hi, int(n)).astype(np.float32).astype(np.float64) for n in lens]
    tid = rng.integers(0, n_traces, N).astype(np.int32)
    off = np.array([rng.integers(0, lens[t]) for t in tid], np.int32)
    br = np.tile(np.asarray(ladder, np.float64), (V, 1))
    if vbr:
        br = np.sort(br * rng.uniform(0.7, 1.3, (V, 1)) * rng.uniform(0.9, 1.1, (V, B)), axis=1)
    case = dict(seed=seed, ctl=ctl, feature=feature, impl=impl, vbr=vbr, auto_reset=auto_reset, n_lanes=N,
                meta=dict(ladder=ladder, chunk_length=L, video_length=V, max_buffer=max_buffer, start_up_length=start_up,
                          interval=interval, weights=[4.3, 1.0, 1.0, 0.1], speed=speed if feature == "config" else 1.0),
                traces=traces, tid=tid, off=off, br=br if vbr else None)
    # the controller
    p = dict()
    if ctl in ("mpc", "robust", "fastmpc"):
        hmax = 2
        while hmax < 6 and B ** (hmax + 1) <= GRID_CAP:
            hmax += 1
        p["horizon"] = int(rng.integers(2, hmax + 1)) if B > 1 else int(rng.integers(2, 7))
        p["qoe"] = [float(rng.choice([4.3, 1.0, 0.3])), float(rng.choice([0.0, -0.0, 0.5, 1.0])), 0.0]
        sz = br * L
        if rng.random() < 0.35:
            sz = sz * rng.uniform(0.7, 1.3, (1 if not vbr and rng.random() < 0.5 else V, B))
            sz = np.broadcast_to(sz, (V, B)).copy()
        p["sizes"] = sz
        if ctl != "mpc":
            p["window"] = int(rng.integers(1, 9))
        if ctl == "fastmpc":
            same = bool((br == br[:1]).all() and (sz == sz[:1]).all()) and p["horizon"] < V
            p["layout"] = "uniform" if same and rng.random() < 0.6 else "per_chunk"
            p["utility"] = str(rng.choice(["identity", "log"]))
            p["clip"] = bool(rng.random() < 0.7)
            nb, nq = int(rng.integers(2, 24)), int(rng.integers(2, 24))
            p["buffer_points"] = np.sort(rng.uniform(0.0, max_buffer + L, nb))
            p["buffer_points"][0] = 0.0
            p["tput_points"] = np.geomspace(br.min() / rng.uniform(2, 6), br.max() * rng.uniform(1.5, 6), nq)
    elif ctl == "buffer":
        p["reservoir"] = 0.0 if rng.random() < 0.3 else float(rng.uniform(0.0, 0.5 * max_buffer))  # 0: B == r at c = 0
        p["cushion"] = float(rng.uniform(0.3, 2.0) * max_buffer)           # reservoir + cushion > max_buffer in some
    elif ctl == "rate":
        p["window"] = int(rng.integers(1, V + 4))                          # window > V in some
        p["safety"] = float(rng.choice([0.6, 0.8, 1.0, 1.25]))
    else:
        p["gp"] = float(rng.choice([0.5, 1.0, 5.0]))
        p["v"] = float(rng.uniform(0.3, 3.0) * max_buffer)
    case["params"] = p
    # the speed feature
    if feature == "lanes":
        case["lane_speeds"] = rng.choice([0.6, 0.8, 1.0, 1.25, 1.7, 0.9173], N)
    elif feature == "schedule":
        case["schedule"] = rng.choice([0.5, 0.75, 1.0, 1.1, 1.25, 1.5, 2.0], (N, int(rng.integers(2, 7))))
    elif feature == "rule":
        nl, nb = int(rng.integers(1, 3)), int(rng.integers(0, 3))
        lat = np.sort(rng.choice(np.arange(0.5, 9.0, 0.5), nl, replace=False))
        buf = np.sort(rng.choice(np.arange(0.25, max(max_buffer, 0.5) + 0.25, 0.25), min(nb, 2), replace=False))
        sp = rng.choice([0.75, 0.9, 1.0, 1.1, 1.25, 1.5, 2.0], (nl + 1, len(buf) + 1))
        case["rule"] = (tuple(float(x) for x in lat), tuple(float(x) for x in buf),
                        tuple(tuple(float(x) for x in r) for r in sp))
    # the launch: pieces whose ends never fall on an episode boundary
    T = (2 * V + 1 + int(rng.integers(0, max(1, V - 1)))) if auto_reset else V + 2 + int(rng.integers(0, 3))
    cuts = sorted({int(x) for x in rng.integers(1, T, max(1, T // 4))} - {k * V for k in range(1, T // V + 1)})
    case["pieces"] = np.diff([0] + cuts + [T]).tolist()
    case["n_steps"] = T
    # a generous per-episode tick bound (the tick tables are sized by it): every download at the slowest sample, every
    # availability wait, every drain of a full buffer at speed 0.5; a lane that still runs out is a failed case
    slow = min(float(t.min()) for t in traces)
    per_chunk = float(br.max()) * L / slow + L + (max_buffer + L) / 0.5
    case["max_ticks"] = int(min(2 ** 31 - 1, 2 * V * per_chunk / 0.01 + 10_000))
    return case


def describe(case):
    m = case["meta"]
    return (f"seed={case['seed']} {case['ctl']}/{case['feature']}/{case['impl']} vbr={int(case['vbr'])} "
            f"auto_reset={int(case['auto_reset'])} N={case['n_lanes']} V={m['video_length']} B={len(m['ladder'])} "
            f"L={m['chunk_length']} mb={m['max_buffer']} su={m['start_up_length']} it={m['interval']}")


def br_table(case):
    m = case["meta"]
    return case["br"] if case["br"] is not None else np.tile(np.asarray(m["ladder"], np.float64), (m["video_length"], 1))


def env_cfg(case):
    return oracle_env_cfg(O, case["meta"], br_table=case["br"])


def mpc_cfg(case, horizon=None):
    m, p = case["meta"], case["params"]
    wr, wv, ws = p["qoe"]
    return O.mpc_cfg(len(m["ladder"]), p["horizon"] if horizon is None else horizon, m["video_length"],
                     m["chunk_length"], m["max_buffer"], wv, wr, ws)


def rule_params(case):
    p = case["params"]
    return dict(kind=RULE_KIND[case["ctl"]], window=p.get("window", 0), reservoir=p.get("reservoir", 0.0),
                cushion=p.get("cushion", 0.0), safety=p.get("safety", 0.0), v=p.get("v", 0.0), gp=p.get("gp", 0.0))


def bola_utility(table):
    return np.log(table / table[:, :1])


def fastmpc_edges(case):
    p = case["params"]
    bp, tp = np.asarray(p["buffer_points"], np.float64), np.asarray(p["tput_points"], np.float64)
    return (bp[:-1] + bp[1:]) / 2.0, np.sqrt(tp[:-1] * tp[1:])


# ---------------------------------------------------------------------------------------------------------------------
# the reference controllers at one call site

class Reference:
    """The reference controller of one case, one lane at a time, its state carried in call order."""

    def __init__(self, case, entries=None):
        self.case, self.entries = case, entries
        m, p = case["meta"], case["params"]
        self.V, self.B = m["video_length"], len(m["ladder"])
        self.table = br_table(case)
        self.kind = case["ctl"]
        N = case["n_lanes"]
        if self.kind == "mpc":
            self.n, self.S = np.zeros(N), np.zeros(N)
        if self.kind == "robust":
            self.st = robust_twin.empty_state(N, p["window"])
        if self.kind == "fastmpc":
            self.be, self.te = fastmpc_edges(case)
            self.uniform = p["layout"] == "uniform"
        if self.kind == "bola":
            self.u = bola_utility(self.table)
        self.clipped = 0
        self.used = set()              # FastMPC: the table entries the decisions read

    def new_episode(self, i):
        if self.kind == "mpc":
            self.n[i], self.S[i] = 0.0, 0.0

    def fold(self, i, x):
        """A measured throughput enters the harmonic history (Simulator.py:164)."""
        if self.kind == "mpc":
            self.S[i] = self.S[i] + 1.0 / x
            self.n[i] = self.n[i] + 1.0

    def answer(self, i, c, prev, buf, h):
        """The action at chunk c, previous bitrate prev, buffer buf, history h[0..c)."""
        p, V, B = self.case["params"], self.V, self.B
        br, sz = self.table, p.get("sizes")
        if self.kind == "mpc":
            if not self.n[i] > 0:
                return 0                                                 # D13
            H = p["horizon"]
            pred, self.n[i], self.S[i] = O.mpc_predict_ns(H, self.n[i], self.S[i])   # D9
            he = min(H, V - c)                                           # D12
            self.clipped += he < H
            f, _, _ = O.mpc_brute(mpc_cfg(self.case, he), br, sz, c, prev, buf, pred[:he], want_J=False)
            return f // B ** (he - 1)
        if self.kind == "robust":
            self.clipped += c + p["horizon"] > V
            a, _, _ = robust_twin.select_scalar(O, mpc_cfg(self.case), br, sz, p["window"], c, prev, buf, h, self.st, i)
            return max(a, 0)
        if self.kind == "fastmpc":
            self.clipped += c + p["horizon"] > V
            n = min(p["window"], c)
            if n > 0 and -B <= prev < B:
                P = fastmpc_twin.harmonic_tail(h, c, n)
                self.used.add((fastmpc_twin.row_of(c, V, p["horizon"], self.uniform), prev % B,
                               fastmpc_twin.cell(self.be, buf), fastmpc_twin.cell(self.te, P)))
            return fastmpc_twin.lookup(self.entries, self.be, self.te, p["window"], V, p["horizon"], self.uniform, c,
                                       prev, buf, h)
        return rules_twin.rule_scalar(rule_params(self.case), c, buf, h, br[c], self.u[c] if self.kind == "bola" else None)


# ---------------------------------------------------------------------------------------------------------------------
# replay

def lane_speeds_for(case, speed_log):
    """The speeds the lanes played, as env_batch's `speeds`: None (config speed), [N] or [N, rows]."""
    if case["feature"] == "lanes":
        return np.asarray(case["lane_speeds"], np.float64)
    if case["feature"] == "schedule":
        return np.asarray(case["schedule"], np.float64)
    if case["feature"] == "rule":
        log = np.asarray(speed_log, np.float64)                          # [rows, N]; rows never reached hold 0
        return np.ascontiguousarray(np.where(log == 0.0, 1.0, log).T)
    return None


def replay(case, actions, speeds):
    """The device's actions replayed through the oracle on a thread pool: (steps, bw, fin)."""
    return O.env_batch(env_cfg(case), case["traces"], case["tid"], case["off"], actions, speeds=speeds,
                       threads=threads())[:3]


class _Row:
    def __init__(self, env, table):
        self.env, self.table = env, table

    def __getitem__(self, a):
        return self.table[self.env.chunk][a]


class RuleTwin(PyTickEnv):
    """The tick loop with a speed rule at every played chunk's first playing tick (tests/speed_twin.py: RuleTickEnv),
    on a per-chunk bitrate table."""

    def __init__(self, case, i, rule):
        m = case["meta"]
        super().__init__(m["ladder"], m["chunk_length"], m["video_length"], m["max_buffer"], m["start_up_length"],
                         m["interval"], m["weights"], case["traces"][case["tid"][i]], int(case["off"][i]))
        self.ladder = _Row(self, br_table(case))
        self.rule, self.log, self._sp = rule, [], 1.0

    @property
    def speed(self):
        if self.play_len == 0:
            self._sp = float(rule_np(*self.rule, self.t - self.play_time, self.buf))
            self.log.append(self._sp)
        return self._sp

    @speed.setter
    def speed(self, _):
        pass


def rule_arrays(case):
    lat, buf, sp = case["rule"]
    return np.asarray(lat, np.float64), np.asarray(buf, np.float64), np.asarray(sp, np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the checker

def _mm(out, name, step, lane, got, want):
    out.append(dict(name=name, step=int(step), lane=int(lane), value=got, expected=want))


def _cmp(out, name, step, got, want, lanes=None, rtol=None):
    got, want = np.asarray(got), np.asarray(want)
    if rtol is None:
        bad = ~((got == want) | (np.isnan(got.astype(np.float64)) & np.isnan(want.astype(np.float64))))
    else:
        bad = ~np.isclose(got, want, rtol=rtol, atol=1e-12)
    for j in np.flatnonzero(bad)[:8]:
        _mm(out, name, step, j if lanes is None else lanes[j], got.flat[j].item(), want.flat[j].item())
    return int(bad.sum())


def check(case, out, stats=None):
    """Compare one run's outputs with the reference closed loop.  `out` (numpy): actions / reward / done [T, N],
    obs [T, 8, N], frames: list of (decisions so far, {F64_ROWS key: [N]}) after each piece, history: (actions u8
    [V, N], bandwidths f64 [V, N]), qoe [N], speed_log [rows, N] or None, entries (FastMPC) or None.  Returns the list
    of mismatches (dicts: name, step, lane, value, expected); `stats` (dict) collects the non-vacuity counters."""
    mm = []
    m = case["meta"]
    V, N, T = m["video_length"], case["n_lanes"], case["n_steps"]
    B = len(m["ladder"])
    acts, rew, done, obs = out["actions"], out["reward"], out["done"], out["obs"]
    stats = {} if stats is None else stats
    if ((done & DONE_TIMEOUT) != 0).any():
        for t, i in np.argwhere((done & DONE_TIMEOUT) != 0)[:4]:
            _mm(mm, "timeout", t, i, int(done[t, i]), 0)
        return mm
    n_ep = -(-T // V) if case["auto_reset"] else 1
    speeds = lane_speeds_for(case, out.get("speed_log"))
    table = br_table(case)
    ref = make_reference(case, out.get("entries"))
    ep = []
    for e in range(n_ep):
        s0, n = e * V, min(V, T - e * V)
        a = np.zeros((N, V), np.int32)
        a[:, :n] = np.clip(acts[s0:s0 + n].T, 0, B - 1)
        steps, bw, fin = replay(case, a, speeds)
        ep.append((s0, n, a, steps, bw, fin))
        if isinstance(ref, PolicyReference):                    # every lane at episode e of the run
            ref.prepare(np.arange(N), np.full(N, e), steps, bw, np.full(N, n))
        # (b) decisions at every replayed call site, the controller state carried in call order
        want = np.zeros((n, N), np.int32)
        for i in range(N):
            ref.new_episode(i)
            for s in range(n):
                if s:
                    ref.fold(i, bw[i, s - 1])
                want[s, i] = ref.answer(i, s, int(steps["last_bitrate"][i, s]), float(steps["buffer_level"][i, s]),
                                        bw[i, :s])
        for s in range(n):
            _cmp(mm, "action", s0 + s, acts[s0 + s], want[s])
        # (a) the replay: rewards, obs, done
        rw = oracle_rewards(steps, fin, a, m["weights"], ladder=m["ladder"], br_table=case["br"])
        for s in range(n):
            t = s0 + s
            _cmp(mm, "reward", t, rew[t], rw[:, s])
            _cmp(mm, "done", t, done[t], np.full(N, 1 if s == V - 1 else 0, np.uint8))
            if s < V - 1:
                nxt = {k: steps[k][:, s + 1] for k in OBS}
            elif case["auto_reset"]:
                nxt = {k: steps[k][:, 0] for k in OBS}
            else:
                nxt = dict(chunk_id=fin["chunk_id"], last_bitrate=a[:, V - 1], last_bandwidth=bw[:, V - 1],
                           **{k: fin[k] for k in ("buffer_level", "global_time", "play_time", "rebuffer_time",
                                                  "start_up_time")})
            for r, k in enumerate(OBS):
                _cmp(mm, "obs." + k, t, obs[t, r], np.asarray(nxt[k]).astype(np.float32))
        if n == V:
            stats["rebuffer"] = stats.get("rebuffer", 0) + int((fin["rebuffer_time"] > 0).sum())
        # a call site just below max_buffer: the download waited for the buffer to drain (one tick drains <= 0.02 s)
        b, mb = steps["buffer_level"][:, 1:n], m["max_buffer"]
        stats["buffer_full"] = stats.get("buffer_full", 0) + int(((b < mb) & (b >= mb - 0.05)).sum())
    # (d) finished lanes, without auto_reset
    if not case["auto_reset"]:
        fin, a, bw = ep[0][5], ep[0][2], ep[0][4]
        for t in range(V, T):
            _cmp(mm, "action", t, acts[t], np.full(N, -1, np.int32))
            _cmp(mm, "done", t, done[t], np.ones(N, np.uint8))
            _cmp(mm, "reward", t, rew[t], np.zeros(N, np.float32))
            for r, k in enumerate(OBS):
                _cmp(mm, "obs." + k, t, obs[t, r], obs[V - 1, r])
    # frames after each piece: the call-site frame (or the final state); hist_n / hist_sum_inv with MPC's D9 appends
    for t, f in out["frames"]:
        e, s = (t // V, t % V) if case["auto_reset"] else (0, min(t, V))
        s0, n, a, steps, bw, fin = ep[e]
        if s == V:
            want = {k: fin[k] for k in FRAME + ("play_id", "chunk_id", "average_latency")}
        else:
            want = {k: steps[k][:, s] for k in FRAME + ("play_id", "chunk_id", "average_latency")}
        for k in FRAME + ("play_id", "chunk_id"):
            _cmp(mm, "frame." + k, t, f[k], want[k])
        _cmp(mm, "frame.average_latency", t, f["average_latency"], want["average_latency"], rtol=1e-9)
        hn, hs = _hist_summary(case, bw, s)
        _cmp(mm, "frame.hist_n", t, f["hist_n"], hn)
        _cmp(mm, "frame.hist_sum_inv", t, f["hist_sum_inv"], hs)
    # history (rows the current episode has written) and QoE of the last finished episode
    s0, n, a, steps, bw, fin = ep[-1]
    c = (T - s0) if case["auto_reset"] else V
    ha, hb = out["history"]
    for r in range(c):
        _cmp(mm, "history.bitrate", r, ha[r], a[:, r].astype(np.uint8))
        _cmp(mm, "history.bandwidth", r, hb[r], bw[:, r])
    done_eps = [x for x in ep if x[1] == V]
    if done_eps:
        fin = done_eps[-1][5]
        _cmp(mm, "qoe", -1, out["qoe"], fin["qoe"], rtol=1e-10)
        stats["qoe"] = True
    # (c) the speed rule's answers against the oracle's rule mode (pinned to the tick-loop twin, tests/speed_twin.py), on
    # every lane; rows past a lane's last answer hold the log's initial zeros
    if case["feature"] == "rule":
        a = ep[0][2]
        log = np.asarray(out["speed_log"])
        w = np.zeros((N, log.shape[0]))
        O.env_batch(env_cfg(case), case["traces"], case["tid"], case["off"], a, rule=rule_arrays(case),
                    speed_log_out=w, threads=threads())
        for r, i in np.argwhere(log != w.T)[:8]:
            _mm(mm, "speed_log", r, i, float(log[r, i]), float(w[i, r]))
        stats.setdefault("speeds", set()).update(np.unique(log[log != 0]).tolist())
    # FastMPC: a sample of the device-built entries against the oracle's search (identity utility)
    if case["ctl"] == "fastmpc" and out.get("entries") is not None:
        _check_entries(case, out["entries"], mm, ref.used)
    # non-vacuity counters
    ans = stats.setdefault("answers", {}).setdefault(case["ctl"], set())
    ans.update(np.unique(acts[acts >= 0]).tolist())
    stats["clipped"] = stats.get("clipped", 0) + ref.clipped
    if case["auto_reset"]:
        ends = np.cumsum(case["pieces"])
        starts = ends - np.asarray(case["pieces"])
        mid = all(any(st_ < k * V < en for st_, en in zip(starts, ends)) for k in range(1, (T - 1) // V + 1))
        stats.setdefault("mid_piece", []).append(bool(mid and T > V))
    return mm


def _hist_summary(case, bw, s):
    """(hist_n, hist_sum_inv) at call site s of an episode: the measured throughputs in list order, and for the
    harmonic MPC the H predictions it appended (D9) at each decision that had a history."""
    N = bw.shape[0]
    n, S = np.zeros(N), np.zeros(N)
    H = case["params"].get("horizon", 0)
    s = min(s, case["meta"]["video_length"])
    for i in range(N):
        ni, Si = 0.0, 0.0
        for j in range(s):
            if case["ctl"] == "mpc" and ni > 0:
                _, ni, Si = O.mpc_predict_ns(H, ni, Si)
            Si = Si + 1.0 / bw[i, j]
            ni = ni + 1.0
        n[i], S[i] = ni, Si
    return n, S


def entry_want(case, idx):
    """The oracle's table entry at idx = (row, previous bitrate, buffer cell, throughput cell): the first action of the
    brute-force search at the grid point (utility log: the utility table in place of the bitrates)."""
    p, m = case["params"], case["meta"]
    r, pv, bi, qi = idx
    c = fastmpc_twin.chunk_of_row(r, m["video_length"], p["layout"] == "uniform")
    u = br_table(case) if p["utility"] == "identity" else np.log(br_table(case) / br_table(case)[:, -1:])
    return fastmpc_twin.entry_oracle(O, mpc_cfg(case), u, p["sizes"], c, pv, p["buffer_points"][bi],
                                     p["tput_points"][qi], p["clip"])


class OracleEntries:
    """A FastMPC table whose entries are computed by the oracle when read (for the host-only checks)."""

    def __init__(self, case):
        p, m = case["params"], case["meta"]
        R = p["horizon"] if p["layout"] == "uniform" else m["video_length"]
        self.shape = (R, len(m["ladder"]), len(p["buffer_points"]), len(p["tput_points"]))
        self.case, self.cache = case, {}

    def __getitem__(self, idx):
        idx = tuple(int(x) for x in idx)
        if idx not in self.cache:
            self.cache[idx] = entry_want(self.case, idx)
        return self.cache[idx]


def _check_entries(case, entries, mm, used, n=24):
    """Every entry a decision read, and n more at random, against the oracle's search (identity utility: a log computed
    on the host may differ from the device's in the last ulp, which can move a tie)."""
    if case["params"]["utility"] != "identity":
        return
    R, M, Nb, Nq = entries.shape
    rng = np.random.default_rng(case["seed"])
    idx = sorted(used | {tuple(int(x) for x in rng.integers(0, [R, M, Nb, Nq])) for _ in range(n)})
    for k in idx:
        want = entry_want(case, k)
        if entries[k] != want:
            _mm(mm, "entries", k[0], -1, dict(idx=k, value=int(entries[k])), int(want))


def assert_non_vacuous(stats, cases):
    """The slice's aggregate: each check guards against something that could have happened."""
    problems = []
    for ctl, a in stats.get("answers", {}).items():
        if len(a) < 3:
            problems.append(f"{ctl} answered only {sorted(a)}")
    if not stats.get("rebuffer"):
        problems.append("no lane rebuffered")
    if not stats.get("buffer_full"):
        problems.append("no lane waited on a full buffer")
    if any(c["feature"] == "rule" for c in cases) and len(stats.get("speeds", ())) < 2:
        problems.append(f"the speed rule played {sorted(stats.get('speeds', ()))}")
    if not all(stats.get("mid_piece", [True])):
        problems.append("an auto_reset case has an episode boundary on a piece end")
    if any(c["ctl"] in ("mpc", "robust") for c in cases) and not stats.get("clipped"):
        problems.append("no MPC decision had a clipped horizon")
    return problems


# ---------------------------------------------------------------------------------------------------------------------
# the reference closed loop in the device's output layout (what the checker's own tests feed it)

def _cfg_for_lane(case, i):
    cfg = env_cfg(case)
    if case["feature"] == "lanes":
        cfg.speed = float(case["lane_speeds"][i])
    elif case["feature"] == "schedule":
        row = np.ascontiguousarray(case["schedule"][i], np.float64)
        cfg._sched_keep = row
        cfg.speed_sched, cfg.speed_rows, cfg.speed_stride = row.ctypes.data, len(row), 1
    return cfg


def oracle_run(case, entries=None, log_rows=None):
    """The reference closed loop of a case, episode by episode through the oracle (oracle.env_batch_mpc for the harmonic
    MPC at one speed; oracle.env_episode_policy driven by the reference controllers otherwise; the tick-loop twin under
    a speed rule), laid out as a device run: the `out` dict check() takes."""
    m = case["meta"]
    V, N, T, B = m["video_length"], case["n_lanes"], case["n_steps"], len(m["ladder"])
    n_ep = -(-T // V) if case["auto_reset"] else 1
    rows = V + 4 if log_rows is None else log_rows
    ref = Reference(case, entries)
    eps = []                                     # per episode: (steps, bw, acts [N, V], fin)
    log = np.zeros((rows, N))
    if case["ctl"] == "mpc" and case["feature"] == "config":
        steps, bw, acts, fin = O.env_batch_mpc(env_cfg(case), mpc_cfg(case), br_table(case), case["params"]["sizes"],
                                               case["traces"], case["tid"], case["off"])
        eps = [(steps, bw, acts, fin)] * n_ep
    else:
        for e in range(n_ep):
            acts = np.zeros((N, V), np.int32)
            for i in range(N):
                ref.new_episode(i)
                seen = [0]

                def pol(c, prev, buf, h, i=i, seen=seen):
                    for x in h[seen[0]:c]:
                        ref.fold(i, x)
                    seen[0] = c
                    return ref.answer(i, c, prev, buf, h)
                if case["feature"] == "rule":
                    env = RuleTwin(case, i, rule_arrays(case))
                    env.reset()
                    for s in range(V):
                        a = pol(env.chunk, env.hist_rates[-1] if env.hist_rates else -1, env.buf, np.asarray(env.hist_bw))
                        acts[i, s] = a
                        env.step(a)
                    k = min(len(env.log), rows)
                    log[:, i] = 0.0
                    log[:k, i] = env.log[:k]
                else:
                    _, _, a, _ = O.env_episode_policy(
                        _cfg_for_lane(case, i), case["traces"][case["tid"][i]], case["off"][i],
                        lambda o, h: pol(int(o["chunk_id"]), int(o["last_bitrate"]), float(o["buffer_level"]), h))
                    acts[i] = a
            steps, bw, fin = replay(case, acts, lane_speeds_for(case, log))
            eps.append((steps, bw, acts, fin))
    out = dict(actions=np.full((T, N), -1, np.int32), reward=np.zeros((T, N), np.float32),
               done=np.ones((T, N), np.uint8), obs=np.zeros((T, len(OBS), N), np.float32), frames=[])
    for e, (steps, bw, acts, fin) in enumerate(eps):
        rw = oracle_rewards(steps, fin, acts, m["weights"], ladder=m["ladder"], br_table=case["br"])
        for s in range(min(V, T - e * V)):
            t = e * V + s
            out["actions"][t], out["reward"][t] = acts[:, s], rw[:, s]
            out["done"][t] = 1 if s == V - 1 else 0
            if s < V - 1 or case["auto_reset"]:
                ss = s + 1 if s < V - 1 else 0
                out["obs"][t] = np.stack([steps[k][:, ss] for k in OBS]).astype(np.float32)
            else:
                term = [fin["chunk_id"], acts[:, V - 1], bw[:, V - 1], fin["buffer_level"], fin["global_time"],
                        fin["play_time"], fin["rebuffer_time"], fin["start_up_time"]]
                out["obs"][t:] = np.stack(term).astype(np.float32)[None]
    for t in np.cumsum(case["pieces"]):
        e, s = (t // V, t % V) if case["auto_reset"] else (0, min(t, V))
        steps, bw, acts, fin = eps[e]
        src = fin if s == V else {k: steps[k][:, s] for k in FRAME + ("play_id", "chunk_id", "average_latency")}
        f = {k: np.asarray(src[k]).copy() for k in FRAME + ("play_id", "chunk_id", "average_latency")}
        f["hist_n"], f["hist_sum_inv"] = _hist_summary(case, bw, s)
        out["frames"].append((int(t), f))
    e_last = len(eps) - 1
    steps, bw, acts, fin = eps[e_last]
    prev = eps[e_last - 1] if e_last else None
    ha = (prev[2] if prev else acts).T.astype(np.uint8).copy()
    hb = (prev[1] if prev else bw).T.copy()
    c = T - e_last * V if case["auto_reset"] else V
    ha[:c], hb[:c] = acts.T[:c], bw.T[:c]
    out["history"] = (ha, hb)
    done_eps = [x for j, x in enumerate(eps) if (j + 1) * V <= T]
    out["qoe"] = done_eps[-1][3]["qoe"].copy()
    out["speed_log"] = log if case["feature"] == "rule" else None
    out["entries"] = entries
    return out


# =====================================================================================================================
# The episode family: sampled, staggered and policy-driven episodes (make_episode_case / check_episodes)
#
# A case of this family is a make_case-style configuration plus an episode mode (EP_MODES), a list of operations --
# launches of n decisions and masked resets between them -- an episode sampler or none, a lane_id_base, and a
# controller among EP_CONTROLLERS (the learned policy included).  Each lane's run is a list of segments: a segment
# starts at a reset or a re-arm (always at chunk 0), has an episode number and a (trace, offset) pair, and ends with
# `done`, is cut by a masked reset, or is still running.  The checker replays the device's actions segment by segment
# through the oracle (batched by segment index; the speed rule in the oracle's rule mode on every lane) and asks the
# reference controller for its answer at every replayed call site, its state carried per lane in call order.

EP_CONTROLLERS = CONTROLLERS + ("policy",)
EP_MODES = ("sampled", "sampled_staggered", "staggered", "masked")
EP_CELLS = [(c, f) for c in EP_CONTROLLERS for f in SPEEDS]    # cell = seed % 28, mode = (seed // 28) % 4
EP_SLICE = len(EP_CELLS) * len(EP_MODES)                        # every (controller, speed feature, mode) once


def accepted_impls_ep(ctl, feature):
    if ctl == "policy":
        return ["jump", "split", "split3", "auto"]             # abr_env_step_policy: every event-driven kernel
    return accepted_impls(ctl, feature)


def _policy_layers(rng, F, widths, M):
    out, fan = [], F
    for w in list(widths) + [M]:
        out.append((rng.normal(0, 1.5 / np.sqrt(fan), (w, fan)).astype(np.float32),
                    rng.normal(0, 0.2, w).astype(np.float32)))
        fan = w
    return out


def policy_params(rng, case, W, widths, explore):
    """The policy of a case (tests/test_policy_gpu.py: _policy_case): layers, a normalisation, the seed and threshold."""
    m = case["meta"]
    V, M = m["video_length"], len(m["ladder"])
    F = 4 + W + M
    thr = (1 << 32) if explore >= 1.0 else int(np.floor(explore * 2.0 ** 32))
    top = float(br_table(case).max())
    norm = np.stack([np.zeros(F), np.r_[1 / m["max_buffer"], 1 / top, 1 / V, 0.1, np.full(W + M, 1 / top)]])
    return dict(window=W, layers=_policy_layers(rng, F, widths, M), seed=int(rng.integers(1 << 62)), thr=thr,
                explore=explore, norm=norm)


def _wave_mask(rng, N, live_hint=None):
    """A mask mixing a whole wave, part of another and scattered lanes (never empty)."""
    m = np.zeros(N, bool)
    waves = -(-N // 64)
    kind = int(rng.integers(0, 3))
    if kind == 0 or waves == 1:
        w = int(rng.integers(0, waves))
        m[w * 64:(w + 1) * 64] = True                          # one whole wave (the last one may be partial)
    if kind >= 1:
        w = int(rng.integers(0, waves))
        lo = w * 64 + int(rng.integers(0, 32))
        m[lo:min(N, lo + int(rng.integers(1, 32)))] = True     # part of a wave
    m |= rng.random(N) < float(rng.choice([0.05, 0.2, 0.5]))
    if live_hint is not None:
        m |= live_hint & (rng.random(N) < 0.5)
    if not m.any():
        m[int(rng.integers(0, N))] = True
    return m


def make_episode_case(seed, n_lanes=None):
    """A deterministic case of the episode family (plain Python / numpy values)."""
    rng = np.random.default_rng(90_000 + seed)
    ctl, feature = EP_CELLS[seed % len(EP_CELLS)]
    mode = EP_MODES[(seed // len(EP_CELLS)) % len(EP_MODES)]
    rnd = seed // len(EP_CELLS)
    impls = accepted_impls_ep(ctl, feature)
    impl = impls[(rnd + seed // EP_SLICE) % len(impls)]
    vbr = rng.random() < 0.5
    auto_reset = mode != "masked"
    L = float(rng.choice([1.0, 2.0, 2.5, 3.0, 4.0, 6.0]))
    interval = float(rng.choice([0.05, 0.25, 0.3, 0.5, 0.7, 1.0, 2.0, 3.7]))
    B = int(rng.integers(1, 9)) if rng.random() < 0.8 else int(rng.integers(9, 17))
    ladder = np.sort(rng.uniform(0.2, 8.0, B)).round(3)
    ladder = np.maximum.accumulate(np.maximum(ladder, 0.2)).tolist()
    if B >= 2 and rng.random() < 0.2:
        ladder[1] = ladder[0]
    max_buffer = float(rng.choice([L * 0.6, L * 1.2, L * 1.5, L * 1.9, L * 3, 7.3, 20.0]))
    start_up = float(min(max_buffer, rng.choice([0.0, L, 1.7])))
    speed = float(rng.choice([0.8, 1.0, 1.25]))
    V = int(rng.integers(3, 19))
    bw_lo = float(rng.choice([0.1, 0.5, 2.0] if feature != "rule" else [0.5, 2.0]))
    bw_hi = bw_lo * float(rng.choice([3.0, 10.0, 40.0]))
    N = int(n_lanes if n_lanes is not None else LANES[rnd % len(LANES)])
    n_traces = 5
    lens = rng.integers(40, 3000, n_traces)
    lens[int(rng.integers(0, n_traces))] = int(rng.integers(8, 40))      # a short trace: offsets that wrap
    traces = [rng.uniform(bw_lo, bw_hi, int(n)).astype(np.float32).astype(np.float64) for n in lens]
    tid = rng.integers(0, n_traces, N).astype(np.int32)
    off = np.array([rng.integers(0, lens[t]) for t in tid], np.int32)
    br = np.tile(np.asarray(ladder, np.float64), (V, 1))
    if vbr:
        br = np.sort(br * rng.uniform(0.7, 1.3, (V, 1)) * rng.uniform(0.9, 1.1, (V, B)), axis=1)
    case = dict(seed=seed, family="episodes", mode=mode, ctl=ctl, feature=feature, impl=impl, vbr=vbr,
                auto_reset=auto_reset, n_lanes=N,
                meta=dict(ladder=ladder, chunk_length=L, video_length=V, max_buffer=max_buffer, start_up_length=start_up,
                          interval=interval, weights=[4.3, 1.0, 1.0, 0.1], speed=speed if feature == "config" else 1.0),
                traces=traces, tid=tid, off=off, br=br if vbr else None)
    # the controller
    p = dict()
    if ctl in ("mpc", "robust", "fastmpc"):
        hmax = 2
        while hmax < 6 and B ** (hmax + 1) <= GRID_CAP:
            hmax += 1
        p["horizon"] = int(rng.integers(2, hmax + 1)) if B > 1 else int(rng.integers(2, 7))
        p["qoe"] = [float(rng.choice([4.3, 1.0, 0.3])), float(rng.choice([0.0, 0.5, 1.0])), 0.0]
        sz = br * L
        if rng.random() < 0.35:
            sz = np.broadcast_to(sz * rng.uniform(0.7, 1.3, (V, B)), (V, B)).copy()
        p["sizes"] = sz
        if ctl != "mpc":
            p["window"] = int(rng.integers(1, 9))
        if ctl == "fastmpc":
            same = bool((br == br[:1]).all() and (sz == sz[:1]).all()) and p["horizon"] < V
            p["layout"] = "uniform" if same and rng.random() < 0.6 else "per_chunk"
            p["utility"] = str(rng.choice(["identity", "log"]))
            p["clip"] = bool(rng.random() < 0.7)
            nb, nq = int(rng.integers(2, 24)), int(rng.integers(2, 24))
            p["buffer_points"] = np.sort(rng.uniform(0.0, max_buffer + L, nb))
            p["buffer_points"][0] = 0.0
            p["tput_points"] = np.geomspace(br.min() / rng.uniform(2, 6), br.max() * rng.uniform(1.5, 6), nq)
    elif ctl == "buffer":
        p["reservoir"] = 0.0 if rng.random() < 0.3 else float(rng.uniform(0.0, 0.5 * max_buffer))
        p["cushion"] = float(rng.uniform(0.3, 2.0) * max_buffer)
    elif ctl == "rate":
        p["window"] = int(rng.integers(1, V + 4))
        p["safety"] = float(rng.choice([0.6, 0.8, 1.0, 1.25]))
    elif ctl == "bola":
        p["gp"] = float(rng.choice([0.5, 1.0, 5.0]))
        p["v"] = float(rng.uniform(0.3, 3.0) * max_buffer)
    case["params"] = p
    if ctl == "policy":
        W = int(rng.integers(0, 17))
        widths = [int(rng.integers(1, 65)) for _ in range(int(rng.integers(0, 3)))]
        explore = float(rng.choice([0.0, 0.0, 0.3, 0.6, 1.0]))
        case["params"] = policy_params(rng, case, W, widths, explore)
    # the speed feature
    if feature == "lanes":
        case["lane_speeds"] = rng.choice([0.6, 0.8, 1.0, 1.25, 1.7, 0.9173], N)
    elif feature == "schedule":
        case["schedule"] = rng.choice([0.5, 0.75, 1.0, 1.1, 1.25, 1.5, 2.0], (N, int(rng.integers(2, 7))))
    elif feature == "rule":
        nl, nb = int(rng.integers(1, 3)), int(rng.integers(0, 3))
        lat = np.sort(rng.choice(np.arange(0.5, 9.0, 0.5), nl, replace=False))
        buf = np.sort(rng.choice(np.arange(0.25, max(max_buffer, 0.5) + 0.25, 0.25), min(nb, 2), replace=False))
        sp = rng.choice([0.75, 0.9, 1.0, 1.1, 1.25, 1.5, 2.0], (nl + 1, len(buf) + 1))
        case["rule"] = (tuple(float(x) for x in lat), tuple(float(x) for x in buf),
                        tuple(tuple(float(x) for x in r) for r in sp))
        case["log_rows"] = int(V + 4 if rng.random() < 0.7 else max(1, V // 2))
    # the sampler and the global lane ids
    sampler = None
    if mode in ("sampled", "sampled_staggered") or (mode == "masked" and rng.random() < 0.5):
        k = int(rng.integers(0, 3))
        pool = None if k == 0 else ([int(rng.integers(0, n_traces))] if k == 1 else
                                    rng.integers(0, n_traces, int(rng.integers(2, 9))).tolist())
        span = int(rng.choice([0, 1, int(rng.integers(2, 40)), int(lens.max()) + int(rng.integers(1, 500))]))
        sampler = dict(seed=int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)), pool=pool, span=span)
    case["sampler"] = sampler
    base = int(rng.choice(3))
    case["lane_id_base"] = (0 if base == 0 else
                            int(rng.integers(1, 2 ** 20)) * 64 + int(rng.integers(1, 64)) if base == 1 else
                            2 ** 32 + int(rng.integers(0, 2 ** 40)))
    # the operations: an initial reset, then launches with masked resets between them
    ops = [("reset", None, "sample" if sampler is not None and rng.random() < 0.5 else "given")]
    T = 2 * V + 1 + int(rng.integers(0, V + 1)) if auto_reset else 2 * V + 2 + int(rng.integers(0, V))
    n_resets = 0 if mode == "sampled" else int(rng.integers(1, 4))
    if mode == "masked":                 # one reset while every lane runs, one after the first lanes finished
        at = sorted({int(rng.integers(1, V)), int(rng.integers(V, T - 1))} |
                    {int(x) for x in rng.integers(1, T - 1, n_resets - 1)})
    else:
        at = sorted({int(x) for x in rng.integers(1, T - 1, n_resets)})
    cuts = sorted(set(at) | {int(x) for x in rng.integers(1, T, max(1, T // 5))})
    t = 0
    for c in cuts + [T]:
        if c <= t:
            continue
        ops.append(("launch", c - t))
        t = c
        if t in at:
            ops.append(("reset", _wave_mask(rng, N), "sample" if sampler is not None and rng.random() < 0.6
                        else "given"))
    # explicit pairs for the resets that take them
    out_ops = []
    for op in ops:
        if op[0] == "reset" and op[2] == "given":
            t_ = rng.integers(0, n_traces, N).astype(np.int32)
            o_ = np.array([rng.integers(0, lens[x]) for x in t_], np.int32)
            if op[1] is None:
                t_, o_ = tid, off
            out_ops.append(("reset", op[1], t_, o_))
        elif op[0] == "reset":
            out_ops.append(("reset", op[1], None, None))
        else:
            out_ops.append(op)
    case["ops"] = out_ops
    case["n_steps"] = T
    slow = min(float(x.min()) for x in traces)
    per_chunk = float(br.max()) * L / slow + L + (max_buffer + L) / 0.5
    case["max_ticks"] = int(min(2 ** 31 - 1, 2 * V * per_chunk / 0.01 + 10_000))
    return case


def describe_ep(case):
    s = case["sampler"]
    smp = "none" if s is None else f"pool={s['pool']} span={s['span']}"
    return (f"episodes seed={case['seed']} {case['ctl']}/{case['feature']}/{case['mode']}/{case['impl']} "
            f"vbr={int(case['vbr'])} N={case['n_lanes']} V={case['meta']['video_length']} "
            f"B={len(case['meta']['ladder'])} it={case['meta']['interval']} base={case['lane_id_base']} sampler: {smp} "
            f"ops={[_op_str(op) for op in case['ops']]}")


def _op_str(op):
    if op[0] == "launch":
        return op[1]
    return "R" + ("" if op[1] is None else str(int(op[1].sum())))


def global_lanes(case):
    if "lane_ids" in case:
        return np.asarray(case["lane_ids"], np.uint64)
    return np.uint64(case.get("lane_id_base", 0)) + np.arange(case["n_lanes"], dtype=np.uint64)


def sampled_pairs(case, lanes, eps):
    """The sampler's pairs of episodes `eps` of lanes `lanes` (local ids), from the independent twin."""
    from sampler_twin import twin
    s = case["sampler"]
    tl = [len(t) for t in case["traces"]]
    return twin(s["seed"], global_lanes(case)[np.asarray(lanes)], np.asarray(eps, np.int64) & 0xFFFFFFFF, tl,
                s["pool"], s["span"])


class Segment:
    __slots__ = ("lane", "k", "t0", "n", "episode", "trace", "offset", "end", "reset_start", "wave_mixed")

    def __init__(self, lane, k, t0, episode, trace, offset, reset_start, wave_mixed):
        self.lane, self.k, self.t0, self.n, self.episode = lane, k, t0, 0, episode
        self.trace, self.offset, self.end = int(trace), int(offset), None        # end: None, "done" or "cut"
        self.reset_start, self.wave_mixed = reset_start, wave_mixed


def episode_plan(case, pair_fn=None):
    """Each lane's segments and what every operation leaves behind, from the operations alone (no lane times out).
    Returns (segs: per lane a list of Segment, after: per op a list of (segment index per lane, finished [N]),
    launch_starts: per launch op the decision index it starts at)."""
    V, N = case["meta"]["video_length"], case["n_lanes"]
    pair_fn = pair_fn or sampled_pairs
    segs = [[] for _ in range(N)]
    fin = np.zeros(N, bool)
    after, t = [], 0
    for op in case["ops"]:
        if op[0] == "reset":
            lanes = np.arange(N) if op[1] is None else np.flatnonzero(op[1])
            eps = np.array([segs[i][-1].episode + 1 if segs[i] else 0 for i in lanes], np.int64)
            if op[2] is None:
                tr, of = pair_fn(case, lanes, eps)
            else:
                tr, of = op[2][lanes], op[3][lanes]
            mixed = op[1] is not None and any(not op[1][w * 64:(w + 1) * 64].all() for w in set((lanes // 64).tolist()))
            for j, i in enumerate(lanes):
                if segs[i] and segs[i][-1].end is None:
                    segs[i][-1].end = "cut"
                segs[i].append(Segment(i, len(segs[i]), t, int(eps[j]), tr[j], of[j], op[1] is not None, mixed))
                fin[i] = False
        else:
            for _ in range(op[1]):
                ended = []
                for i in range(N):
                    if fin[i]:
                        continue
                    sg = segs[i][-1]
                    sg.n += 1
                    if sg.n == V:
                        sg.end = "done"
                        ended.append(i)
                t += 1
                if case["auto_reset"] and ended:
                    eps = np.array([segs[i][-1].episode + 1 for i in ended], np.int64)
                    if case.get("sampler") is not None:
                        tr, of = pair_fn(case, ended, eps)
                    else:
                        tr = [segs[i][-1].trace for i in ended]
                        of = [segs[i][-1].offset for i in ended]
                    for j, i in enumerate(ended):
                        segs[i].append(Segment(i, len(segs[i]), t, int(eps[j]), tr[j], of[j], False, False))
                else:
                    for i in ended:
                        fin[i] = True
        after.append(([len(s) - 1 for s in segs], fin.copy()))
    return segs, after


def segment_speeds(case, lanes):
    if case["feature"] == "lanes":
        return np.asarray(case["lane_speeds"], np.float64)[lanes]
    if case["feature"] == "schedule":
        return np.ascontiguousarray(np.asarray(case["schedule"], np.float64)[lanes])
    return None


class PolicyReference:
    """The learned policy's twin (tests/policy_twin.py) as a reference controller: stateless, so the answers of a batch
    of segments are computed at once from their replayed frames (prepare), keyed by each lane's own episode number and
    global lane id."""

    def __init__(self, case, entries=None):
        self.case, self.clipped, self.used = case, 0, set()
        self.ans, self.coins = {}, []

    def new_episode(self, i):
        pass

    def fold(self, i, x):
        pass

    def prepare(self, lanes, eps, steps, bw, n=None):
        import policy_twin as T
        p, m = self.case["params"], self.case["meta"]
        V, M = m["video_length"], len(m["ladder"])
        lanes = np.asarray(lanes)
        K_ = len(lanes)
        table = br_table(self.case)
        c = np.tile(np.arange(V), K_)
        rows = np.repeat(np.arange(K_), V)
        hist = np.repeat(bw, V, axis=0).T
        x = T.features(p["window"], M, V, c, steps["last_bitrate"].reshape(-1), steps["buffer_level"].reshape(-1),
                       steps["global_time"].reshape(-1), steps["play_time"].reshape(-1), hist, lambda r: table[r],
                       p["norm"])
        eps = np.asarray(eps, np.uint64)                       # [K], or [K, V]: one episode number per call site
        a, _, coin = T.decide(p["layers"], x, p["seed"], p["thr"], global_lanes(self.case)[lanes[rows]], c,
                              eps[rows] if eps.ndim == 1 else eps.reshape(-1), M)
        a, coin = a.reshape(K_, V), coin.reshape(K_, V)
        for j, i in enumerate(lanes):
            self.ans[int(i)] = a[j]
            if n is not None:
                self.coins.extend(coin[j, :n[j]].tolist())

    def answer(self, i, c, prev, buf, h):
        return int(self.ans[int(i)][c])


class ScriptReference:
    """Open loop as a controller (the config family only): case["script"][t, i] is the action of lane i at decision t
    of the run, known before the launch (scripted actions, or the counter-based random policy's draw)."""

    def __init__(self, case, entries=None):
        self.case, self.clipped, self.used = case, 0, set()
        self.episode = np.full(case["n_lanes"], -1)

    def new_episode(self, i):
        self.episode[i] += 1

    def fold(self, i, x):
        pass

    def answer(self, i, c, prev, buf, h):
        return int(self.case["script"][self.episode[i] * self.case["meta"]["video_length"] + c, i])


def make_reference(case, entries=None):
    if case["ctl"] == "script":
        return ScriptReference(case, entries)
    return PolicyReference(case, entries) if case["ctl"] == "policy" else Reference(case, entries)


def _robust_snapshot(ref, i):
    return {k: v[..., i].copy() for k, v in ref.st.items()} if ref.kind == "robust" else None


def _robust_restore(ref, i, snap):
    if snap is not None:
        for k, v in snap.items():
            ref.st[k][..., i] = v


def _run_batch(case, segs_k, acts, speeds_fn=segment_speeds, log_rows=None):
    """Replay the segments `segs_k` (one per lane) with actions [K, V]: (steps, bw, fin, log [K, rows] or None,
    calls [K] or None)."""
    lanes = np.array([s.lane for s in segs_k])
    tr = np.array([s.trace for s in segs_k], np.int32)
    of = np.array([s.offset for s in segs_k], np.int32)
    if case["feature"] == "rule":
        rows = case["log_rows"] if log_rows is None else log_rows
        log = np.zeros((len(segs_k), rows))
        calls = np.zeros(len(segs_k), np.int32)
        steps, bw, fin, _ = O.env_batch(env_cfg(case), case["traces"], tr, of, acts, rule=rule_arrays(case),
                                        speed_log_out=log, speed_calls_out=calls, threads=threads())
        return steps, bw, fin, log, calls
    steps, bw, fin, _ = O.env_batch(env_cfg(case), case["traces"], tr, of, acts, speeds=speeds_fn(case, lanes),
                                    threads=threads())
    return steps, bw, fin, None, None


def _written(steps_row, fin_row, calls, seg):
    """How many speed-log rows a segment has written where it stands: every answer of an ended episode, else the
    chunks whose first playing tick lies before its current call site."""
    if seg.end == "done":
        return int(calls)
    c = seg.n
    return int(steps_row["play_id"][c]) + int(steps_row["play_length"][c] > 0)


def expected_layout(case, segs, after, res):
    """The device's outputs implied by per-segment results res[(lane, k)] = (steps row [V], bw [V], fin, acts [V], log
    row or None, calls): the `out` dict check_episodes compares (actions / reward / done / obs [T, ...], per op
    frames, episodes and speed logs, history, qoe with the lanes it is meaningful for)."""
    m = case["meta"]
    V, N, T = m["video_length"], case["n_lanes"], case["n_steps"]
    ex = dict(actions=np.full((T, N), -1, np.int32), reward=np.zeros((T, N), np.float32),
              done=np.ones((T, N), np.uint8), obs=np.zeros((T, len(OBS), N), np.float32))
    for i in range(N):
        for sg in segs[i]:
            steps, bw, fin, acts, _, _ = res[(i, sg.k)]
            if sg.n == 0:
                continue
            rw = oracle_rewards({k: steps[k][None] for k in ("rebuffer_time", "start_up_time")},
                                {k: np.asarray([fin[k]]) for k in ("rebuffer_time", "start_up_time")}, acts[None],
                                m["weights"], ladder=m["ladder"], br_table=case["br"])[0]
            for s in range(sg.n):
                t = sg.t0 + s
                ex["actions"][t, i], ex["reward"][t, i] = acts[s], rw[s]
                ex["done"][t, i] = 1 if s == V - 1 else 0
                if s < V - 1:
                    ex["obs"][t, :, i] = [steps[k][s + 1] for k in OBS]
                elif case["auto_reset"]:
                    nx = res[(i, sg.k + 1)][0]
                    ex["obs"][t, :, i] = [nx[k][0] for k in OBS]
                else:
                    term = [fin["chunk_id"], acts[V - 1], bw[V - 1], fin["buffer_level"], fin["global_time"],
                            fin["play_time"], fin["rebuffer_time"], fin["start_up_time"]]
                    ex["obs"][t:sg.t0 + V + _idle_len(case, segs[i], sg), :, i] = np.asarray(term, np.float32)
    frames, episodes, logs = [], [], []
    rows = case.get("log_rows", 0)
    cur_log = np.zeros((rows, N)) if case["feature"] == "rule" else None
    done_upto = [0] * N                       # segments whose log rows are already laid into cur_log
    for oi, (ks, finished) in enumerate(after):
        f = {k: np.zeros(N) for k in FRAME + ("play_id", "chunk_id", "average_latency", "hist_n", "hist_sum_inv")}
        e = {k: np.zeros(N, np.int32) for k in ("trace_id", "start_offset", "episode")}
        for i in range(N):
            sg = segs[i][ks[i]]
            steps, bw, fin, acts, log, calls = res[(i, sg.k)]
            c = _n_at(case, sg, oi)
            src = {k: fin[k] for k in FRAME + ("play_id", "chunk_id", "average_latency")} if c == V else \
                {k: steps[k][c] for k in FRAME + ("play_id", "chunk_id", "average_latency")}
            for k, v in src.items():
                f[k][i] = v
            f["hist_n"][i], f["hist_sum_inv"][i] = _hist_lane(case, bw, c)
            e["trace_id"][i], e["start_offset"][i], e["episode"][i] = sg.trace, sg.offset, sg.episode
            if cur_log is not None:
                for k in range(done_upto[i], sg.k):            # earlier segments: every row they wrote
                    p_ = segs[i][k]
                    st_, _, fn_, _, lg_, cl_ = res[(i, k)]
                    w = _written(st_, fn_, cl_, _Seg(p_, p_.n, p_.end))
                    cur_log[:min(w, rows), i] = lg_[:min(w, rows)]
                done_upto[i] = sg.k
        if cur_log is not None:
            lg = cur_log.copy()
            for i in range(N):
                sg = segs[i][ks[i]]
                st_, _, fn_, _, lg_, cl_ = res[(i, sg.k)]
                c = _n_at(case, sg, oi)
                w = _written(st_, fn_, cl_, _Seg(sg, c, "done" if c == V else None))
                lg[:min(w, rows), i] = lg_[:min(w, rows)]
            logs.append(lg)
        frames.append(f)
        episodes.append(e)
    ex["frames"], ex["episodes"], ex["speed_logs"] = frames, episodes, logs if cur_log is not None else None
    # history rows of each lane's current segment, QoE of its last finished episode where it is meaningful
    ks, finished = after[-1]
    ha, hb = np.zeros((V, N), np.uint8), np.zeros((V, N))
    hist_rows = np.zeros(N, np.int32)
    qoe, qoe_ok = np.zeros(N), np.zeros(N, bool)
    for i in range(N):
        sg = segs[i][ks[i]]
        steps, bw, fin, acts, _, _ = res[(i, sg.k)]
        c = V if sg.end == "done" else sg.n
        ha[:c, i], hb[:c, i], hist_rows[i] = acts[:c], bw[:c], c
        dn = [s for s in segs[i] if s.end == "done"]
        if dn and (case["auto_reset"] or sg.end == "done"):
            qoe[i], qoe_ok[i] = res[(i, dn[-1].k)][2]["qoe"], True
    ex["history"], ex["hist_rows"], ex["qoe"], ex["qoe_ok"] = (ha, hb), hist_rows, qoe, qoe_ok
    return ex


class _Seg:
    """A segment seen at an earlier operation: n decisions taken, ended or not."""

    def __init__(self, sg, n, end):
        self.n, self.end = n, end


def _idle_len(case, lane_segs, sg):
    """Decisions a finished lane (auto_reset off) idles after segment sg: up to its next segment or the end."""
    nxt = [s for s in lane_segs if s.k == sg.k + 1]
    end = nxt[0].t0 if nxt else case["n_steps"]
    return end - (sg.t0 + case["meta"]["video_length"])


def _n_at(case, sg, oi):
    """Decisions segment sg had taken after operation oi (it is the lane's current segment then)."""
    t = sum(op[1] for op in case["ops"][:oi + 1] if op[0] == "launch")
    return min(t - sg.t0, case["meta"]["video_length"]) if t >= sg.t0 else 0


def _hist_lane(case, bw, s):
    ni, Si = 0.0, 0.0
    H = case["params"].get("horizon", 0)
    for j in range(min(s, case["meta"]["video_length"])):
        if case["ctl"] == "mpc" and ni > 0:
            _, ni, Si = O.mpc_predict_ns(H, ni, Si)
        Si = Si + 1.0 / bw[j]
        ni = ni + 1.0
    return ni, Si


def _padded_actions(case, segs_k, acts_dev):
    V, B = case["meta"]["video_length"], len(case["meta"]["ladder"])
    a = np.zeros((len(segs_k), V), np.int32)
    for j, sg in enumerate(segs_k):
        if sg.n:
            a[j, :sg.n] = np.clip(acts_dev[sg.t0:sg.t0 + sg.n, sg.lane], 0, B - 1)
    return a


def check_episodes(case, out, stats=None, pair_fn=None, run_batch=None):
    """Compare one run of the episode family with the reference closed loop.  `out` (numpy): actions / reward / done
    [T, N], obs [T, 8, N]; per operation: frames (observe_f64 dicts), episodes (episodes() dicts) and speed_logs
    ([rows, N] or None); history (u8 [V, N], f64 [V, N]), qoe [N], entries (FastMPC) or None.  Returns the list of
    mismatches; `stats` collects the non-vacuity counters (assert_non_vacuous_ep).  pair_fn and run_batch replace the
    sampler twin and the oracle replay (the checker's own tests)."""
    mm = []
    m = case["meta"]
    V, N, T = m["video_length"], case["n_lanes"], case["n_steps"]
    stats = {} if stats is None else stats
    done = out["done"]
    if ((done & DONE_TIMEOUT) != 0).any():
        for t, i in np.argwhere((done & DONE_TIMEOUT) != 0)[:4]:
            _mm(mm, "timeout", t, i, int(done[t, i]), 0)
        return mm
    segs, after = episode_plan(case, pair_fn)
    ref = make_reference(case, out.get("entries"))
    res, prev_logs = {}, {}
    K_ = max(len(s) for s in segs)
    acts = out["actions"]
    for k in range(K_):
        segs_k = [s[k] for s in segs if len(s) > k]
        a = _padded_actions(case, segs_k, acts)
        steps, bw, fin, log, calls = (run_batch or _run_batch)(case, segs_k, a)
        if isinstance(ref, PolicyReference):
            ref.prepare([s.lane for s in segs_k], [s.episode for s in segs_k], steps, bw, [s.n for s in segs_k])
        for j, sg in enumerate(segs_k):
            i = sg.lane
            res[(i, k)] = (steps[j], bw[j], fin[j], a[j], None if log is None else log[j],
                           None if calls is None else calls[j])
            # (b) the reference's answer at every replayed call site, its state carried in call order
            ref.new_episode(i)
            for s in range(sg.n):
                if s:
                    ref.fold(i, bw[j, s - 1])
                want = ref.answer(i, s, int(steps["last_bitrate"][j, s]), float(steps["buffer_level"][j, s]),
                                  bw[j, :s])
                if acts[sg.t0 + s, i] != want:
                    _mm(mm, "action", sg.t0 + s, i, int(acts[sg.t0 + s, i]), int(want))
        _ep_stats(case, stats, segs_k, steps, fin, log, calls, prev_logs)
    ex = expected_layout(case, segs, after, res)
    # (a) the replay, (d) finished lanes idle until they are revived
    for t in range(T):
        _cmp(mm, "reward", t, out["reward"][t], ex["reward"][t])
        _cmp(mm, "done", t, done[t], ex["done"][t])
        idle = ex["actions"][t] < 0
        _cmp(mm, "action", t, acts[t][idle], ex["actions"][t][idle], lanes=np.flatnonzero(idle))
        for r, k in enumerate(OBS):
            _cmp(mm, "obs." + k, t, out["obs"][t, r], ex["obs"][t, r])
    # the frame, episodes() and the speed log after every operation
    for oi, f in enumerate(out["frames"]):
        want = ex["frames"][oi]
        for k in FRAME + ("play_id", "chunk_id", "hist_n", "hist_sum_inv"):
            _cmp(mm, "frame." + k, oi, f[k], want[k])
        _cmp(mm, "frame.average_latency", oi, f["average_latency"], want["average_latency"], rtol=1e-9)
        for k in ("trace_id", "start_offset", "episode"):
            _cmp(mm, "episodes." + k, oi, out["episodes"][oi][k], ex["episodes"][oi][k])
        if ex["speed_logs"] is not None:
            got, w = np.asarray(out["speed_logs"][oi]), ex["speed_logs"][oi]
            for r, i in np.argwhere(got != w)[:8]:
                _mm(mm, "speed_log", oi * 10_000 + r, i, float(got[r, i]), float(w[r, i]))
    # history rows of each lane's current segment, the QoE of its last finished episode
    ha, hb = out["history"]
    for i in range(N):
        c = ex["hist_rows"][i]
        for r in np.flatnonzero(ha[:c, i] != ex["history"][0][:c, i])[:4]:
            _mm(mm, "history.bitrate", r, i, int(ha[r, i]), int(ex["history"][0][r, i]))
        for r in np.flatnonzero(hb[:c, i] != ex["history"][1][:c, i])[:4]:
            _mm(mm, "history.bandwidth", r, i, float(hb[r, i]), float(ex["history"][1][r, i]))
    ok = ex["qoe_ok"]
    if ok.any():
        _cmp(mm, "qoe", -1, out["qoe"][ok], ex["qoe"][ok], lanes=np.flatnonzero(ok), rtol=1e-10)
        stats["qoe"] = True
    if case["ctl"] == "fastmpc" and out.get("entries") is not None:
        _check_entries(case, out["entries"], mm, ref.used)
    _case_stats(case, stats, segs, after, acts, ref)
    return mm


def _ep_stats(case, stats, segs_k, steps, fin, log, calls, prev_logs):
    """Per segment batch: offsets that wrap, restarted histories read mid-wave, rule answers across re-arms (prev_logs:
    the case's previous segment log per lane)."""
    m = case["meta"]
    V, mb = m["video_length"], m["max_buffer"]
    for j, sg in enumerate(segs_k):
        if sg.n == 0:
            continue
        if sg.n == V:
            stats["rebuffer"] = stats.get("rebuffer", 0) + int(fin["rebuffer_time"][j] > 0)
        b = steps["buffer_level"][j, 1:sg.n]                  # a call site just below max_buffer: a full-buffer wait
        stats["buffer_full"] = stats.get("buffer_full", 0) + int(((b < mb) & (b >= mb - 0.05)).sum())
        last = min(sg.n, V - 1)
        reach = sg.offset + int(steps["global_time"][j, last] / m["interval"])
        if case.get("sampler") is not None and reach >= len(case["traces"][sg.trace]):
            stats["wrapped"] = stats.get("wrapped", 0) + 1
        if sg.reset_start and sg.wave_mixed and sg.n >= 2 and case["ctl"] in ("robust", "rate", "fastmpc"):
            h = stats.setdefault("restarted_history", {})
            h[case["ctl"]] = h.get(case["ctl"], 0) + sg.n - 1
    if log is not None:
        for j, sg in enumerate(segs_k):
            played = log[j][:min(int(calls[j]), len(log[j]))]
            stats.setdefault("speeds", set()).update(np.unique(played).tolist())
            p = prev_logs.get(sg.lane)
            if p is not None and not sg.reset_start and sg.n and not np.array_equal(p[:2], log[j][:2]):
                stats["rule_differs"] = stats.get("rule_differs", 0) + 1
            prev_logs[sg.lane] = log[j]


def _case_stats(case, stats, segs, after, acts, ref):
    m = case["meta"]
    V, N = m["video_length"], case["n_lanes"]
    ans = stats.setdefault("answers", {}).setdefault(case["ctl"], set())
    ans.update(np.unique(acts[acts >= 0]).tolist())
    stats["clipped"] = stats.get("clipped", 0) + ref.clipped
    stats.setdefault("cells", set()).add((case["ctl"], case["feature"], case["mode"]))
    if case["impl"] in ("split", "split3", "auto"):
        starts = set()
        t = 0
        for op in case["ops"]:
            if op[0] == "launch":
                starts |= set(range(t + 1, t + op[1]))
                t += op[1]
        if any(sg.t0 in starts and not sg.reset_start and sg.k > 0 for s in segs for sg in s):
            stats["mid_launch_rearm"] = stats.get("mid_launch_rearm", 0) + 1
    # lanes of one wave at different episode numbers when a launch starts
    for oi, op in enumerate(case["ops"]):
        if op[0] == "launch" and oi > 0:
            ks = after[oi - 1][0]
            ep = np.array([segs[i][ks[i]].episode for i in range(N)])
            if any(len(set(ep[w:w + 64].tolist())) > 1 for w in range(0, N, 64)):
                stats["wave_mixed_episodes"] = stats.get("wave_mixed_episodes", 0) + 1
                break
    s = case.get("sampler")
    if s is not None and s["pool"] is not None and len(set(s["pool"])) >= 2:
        drawn = {sg.trace for x in segs for sg in x}
        stats["pool_all_drawn"] = stats.get("pool_all_drawn", 0) + int(set(s["pool"]) <= drawn)
    if case.get("lane_id_base", 0) >= 2 ** 32:
        stats["high_lane_ids"] = stats.get("high_lane_ids", 0) + 1
    if isinstance(ref, PolicyReference) and case["params"]["thr"] > 0:
        stats.setdefault("explore", set()).update(bool(x) for x in ref.coins)


def assert_non_vacuous_ep(stats, cases):
    """The episode family's aggregate: what the fuzz is meant to reach, it reached."""
    problems = assert_non_vacuous({k: v for k, v in stats.items() if k != "mid_piece"}, cases)
    if any(c["impl"] in ("split", "split3", "auto") for c in cases) and not stats.get("mid_launch_rearm"):
        problems.append("no re-arm in the middle of a launch on a role-split impl")
    if not stats.get("wave_mixed_episodes"):
        problems.append("no launch had lanes of one wave at different episode numbers")
    if any(c["sampler"] and c["sampler"]["pool"] and len(set(c["sampler"]["pool"])) >= 2 for c in cases) \
            and not stats.get("pool_all_drawn"):
        problems.append("no case drew every entry of its pool")
    if any(c["sampler"] for c in cases) and not stats.get("wrapped"):
        problems.append("no sampled offset wrapped within its episode")
    if not stats.get("high_lane_ids"):
        problems.append("no lane_id_base >= 2^32")
    if any(c["ctl"] == "policy" and c["params"]["thr"] > 0 for c in cases) and stats.get("explore") != {True, False}:
        problems.append(f"policy exploration taken / not taken: {sorted(stats.get('explore', ()))}")
    if any(c["feature"] == "rule" and c["auto_reset"] for c in cases) and not stats.get("rule_differs"):
        problems.append("no speed-rule answers differed across a re-arm")
    for ctl in ("robust", "rate", "fastmpc"):
        if any(c["ctl"] == ctl and c["mode"] != "sampled" for c in cases) and \
                not stats.get("restarted_history", {}).get(ctl):
            problems.append(f"{ctl} never read a history that restarted mid-wave")
    return problems


def _policy_closed_loop(case, segs_k, res, episode_fn=None):
    """The policy's closed loop on a batch of segments: the policy is stateless and its answer at call site s depends on
    the actions before s only, so replaying and taking the answers up to the first disagreement converges in at most V
    rounds.  Call sites past a segment's cut keep action 0 (no controller call happens there on the device)."""
    V = case["meta"]["video_length"]
    ref = PolicyReference(case)
    a = np.zeros((len(segs_k), V), np.int32)
    n = np.array([sg.n for sg in segs_k])
    while True:
        steps, bw, fin, log, calls = _run_batch(case, segs_k, a)
        eps = [sg.episode for sg in segs_k] if episode_fn is None else episode_fn(segs_k)
        ref.prepare([sg.lane for sg in segs_k], eps, steps, bw)
        want = np.stack([ref.ans[sg.lane] for sg in segs_k])
        bad = (want != a) & (np.arange(V)[None, :] < n[:, None])
        if not bad.any():
            break
        for j in np.flatnonzero(bad.any(1)):
            s = int(np.argmax(bad[j]))
            a[j, s] = want[j, s]
    for j, sg in enumerate(segs_k):
        res[(sg.lane, sg.k)] = (steps[j], bw[j], fin[j], a[j], None if log is None else log[j],
                                None if calls is None else int(calls[j]))


def oracle_run_episodes(case, entries=None, pair_fn=None, ref_factory=Reference, policy_episode_fn=None):
    """The reference closed loop of an episode-family case, segment by segment through the oracle (every call site's
    action the reference controller's answer, its state carried per lane in call order; the speed rule in the oracle's
    rule mode), laid out as a device run: the `out` dict check_episodes takes.  pair_fn, ref_factory and
    policy_episode_fn (segments, batch -> episode numbers [K, V]) replace the sampler's pairs, the reference controller
    and the policy's episode numbers: the checker's own tests build wrong runs with them."""
    m = case["meta"]
    V, N = m["video_length"], case["n_lanes"]
    segs, after = episode_plan(case, pair_fn)
    ref = ref_factory(case, entries) if case["ctl"] != "policy" else None
    rows = case.get("log_rows", 1)
    res = {}
    for k in range(max(len(s) for s in segs)):
        if ref is None:
            _policy_closed_loop(case, [s[k] for s in segs if len(s) > k], res,
                                None if policy_episode_fn is None else (lambda b: policy_episode_fn(segs, b)))
            continue
        for i in range(N):
            if len(segs[i]) <= k:
                continue
            sg = segs[i][k]
            log, calls = np.zeros(rows), np.zeros(1, np.int32)
            rule = dict(rule=rule_arrays(case), speed_log_out=log, speed_calls_out=calls) if case["feature"] == "rule" \
                else {}
            trace = case["traces"][sg.trace]
            ref.new_episode(i)
            seen, box = [0], {}

            def pol(o, h, i=i, sg=sg, seen=seen, box=box):
                c = int(o["chunk_id"])
                if c >= sg.n:                                   # past the cut: no controller call on the device
                    return 0
                for x in h[seen[0]:c]:
                    ref.fold(i, x)
                seen[0] = c
                a = ref.answer(i, c, int(o["last_bitrate"]), float(o["buffer_level"]), h)
                if c == sg.n - 1:
                    box["snap"] = _robust_snapshot(ref, i)
                return a
            steps, bw, acts, fin = O.env_episode_policy(_cfg_for_lane(case, i), trace, sg.offset, pol, **rule)
            if "snap" in box:
                _robust_restore(ref, i, box["snap"])
            res[(i, k)] = (steps, bw, fin, acts, log if case["feature"] == "rule" else None, int(calls[0]))
    ex = expected_layout(case, segs, after, res)
    out = {k: ex[k] for k in ("actions", "reward", "done", "obs")}
    out["frames"], out["episodes"], out["speed_logs"] = ex["frames"], ex["episodes"], ex["speed_logs"]
    out["history"], out["qoe"], out["entries"] = ex["history"], ex["qoe"], entries
    return out


def subset_episode_case(case, out, pick):
    """The lanes `pick` of an episode-family case and its device run, as a case and `out` of their own (global lane ids
    kept), for checking sampled lanes of a large run."""
    pick = np.asarray(pick)
    sub = dict(case, n_lanes=len(pick), tid=case["tid"][pick], off=case["off"][pick], lane_ids=global_lanes(case)[pick])
    for k in ("lane_speeds", "schedule"):
        if k in case:
            sub[k] = np.asarray(case[k])[pick]
    sub["ops"] = [op if op[0] == "launch" else
                  ("reset", None if op[1] is None else op[1][pick], None if op[2] is None else op[2][pick],
                   None if op[3] is None else op[3][pick]) for op in case["ops"]]
    o = dict(out)
    for k in ("actions", "reward", "done"):
        o[k] = out[k][:, pick]
    o["obs"] = out["obs"][:, :, pick]
    o["frames"] = [{k: v[pick] for k, v in f.items()} for f in out["frames"]]
    o["episodes"] = [{k: v[pick] for k, v in e.items()} for e in out["episodes"]]
    o["speed_logs"] = None if out["speed_logs"] is None else [x[:, pick] for x in out["speed_logs"]]
    o["history"] = tuple(h[:, pick] for h in out["history"])
    o["qoe"] = out["qoe"][pick]
    return sub, o
