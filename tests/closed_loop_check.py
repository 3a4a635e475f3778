"""Config-space fuzz of the closed-loop rollouts: case generator and checker (host only; the GPU runner is
tools/gpu_fuzz_closed.py, the slice tests/test_closed_loop_fuzz_gpu.py).

A case is one random configuration (ladder, chunk length, video length, buffer limit, start-up length, trace interval,
ragged traces with wrap-around), one controller evaluated on the device (harmonic MPC, RobustMPC, FastMPC, BBA-0, RATE,
BOLA), one speed feature (the config speed, per-lane speeds, a speed schedule, a LatencySpeedController), a per-chunk
ladder or not, a lane count, a kernel implementation the combination is accepted by, and a launch split into pieces.

Why checking (a) and (b) together proves the closed loop.  Let F_i(s) be lane i's frame at its s-th call site of an
episode.  (a) replays the device's actions A_i through the C oracle (with the speeds the lane played) and compares every
frame, reward, done flag, the history and the final state: the device's frames equal F_i(s | A_i).  (b) asks the
reference controller (the oracle's brute-force MPC search with the harmonic (n, S) carried as in oracle_mpc_policy,
tests/robust_twin.py, tests/fastmpc_twin.py on the device-built table, tests/rules_twin.py) for its answer at every one
of those replayed frames and requires A_i(s) to equal it.  By induction over s: frame 0 depends on nothing the
controller did; if the device's first s actions are the reference's answers, the frame at call site s is the
reference closed loop's frame at s (by (a)), so the reference's answer there is A_i(s) (by (b)).  Hence the whole run is
the reference closed loop, whatever the speed feature.  A replay alone (a) would accept any action sequence, e.g. one
computed from a stale buffer level.  Under the speed rule the speeds themselves are device outputs (the log): (c) checks
them against the tick-loop twin (tests/speed_twin.py) on a subset of lanes, which closes the same loop for the speeds.
(d) Without auto_reset a finished lane answers -1, reports its terminal record again and its state does not move.

Edges (build-defined, include/abr_env.h): an empty history answers bitrate 0 (D13); near the video end every MPC search
runs at the clipped horizon V - c (D12).  Under auto_reset a lane restarts from its own trace and offset: the harmonic
(n, S) restarts, RobustMPC's state empties itself at chunk 0 (carried across episodes here, as on the device), RATE and
FastMPC read the current episode's history only.  A speed rule's log holds the lane's current episode only, so the
generator pairs the speed rule with auto_reset off (tests/test_speed_rule_gpu.py covers a rule under auto_reset)."""
import numpy as np

from oracle import oracle as O
from oracle.pyloop import PyTickEnv
from helpers import oracle_env_cfg, oracle_rewards, thread_map, threads
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
TWIN_LANES = 16
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


def twin_log(case, i, actions):
    env = RuleTwin(case, i, rule_arrays(case))
    env.reset()
    for a in actions:
        _, over = env.step(int(a))
        if over:
            break
    return env.log


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
    ref = Reference(case, out.get("entries"))
    ep = []
    for e in range(n_ep):
        s0, n = e * V, min(V, T - e * V)
        a = np.zeros((N, V), np.int32)
        a[:, :n] = np.clip(acts[s0:s0 + n].T, 0, B - 1)
        steps, bw, fin = replay(case, a, speeds)
        ep.append((s0, n, a, steps, bw, fin))
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
    # (c) the speed rule's answers against the tick-loop twin, on the lanes with the fewest ticks
    if case["feature"] == "rule":
        fin, a = ep[0][5], ep[0][2]
        log = np.asarray(out["speed_log"])
        sub = np.sort(np.argsort(fin["ticks"], kind="stable")[:TWIN_LANES])
        logs = thread_map(lambda i: twin_log(case, i, a[i]), sub)
        for i, tl in zip(sub, logs):
            w = np.zeros(log.shape[0])
            k = min(len(tl), log.shape[0])
            w[:k] = tl[:k]
            for r in np.flatnonzero(log[:, i] != w)[:8]:
                _mm(mm, "speed_log", r, i, float(log[r, i]), float(w[r]))
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
