"""Config-space fuzz of the closed-loop rollouts: case generators and checkers (host only; the GPU runner is
tools/gpu_fuzz_closed.py, the slices tests/test_closed_loop_fuzz_gpu.py and tests/test_closed_loop_episodes_gpu.py).

Two case families.  The config family (make_case / check) is one random configuration (ladder, chunk length, video
length, buffer limit, start-up length, trace interval, ragged traces with wrap-around), one controller evaluated on the
device (harmonic MPC, RobustMPC, FastMPC, BBA-0, RATE, BOLA), one speed feature (the config speed, per-lane speeds, a
speed schedule, a LatencySpeedController), a per-chunk ladder or not, a lane count, a kernel implementation the
combination is accepted by, and a launch split into pieces; every lane runs episode e over decisions [eV, (e+1)V).  The
episode family (make_episode_case / check_episodes, further below) adds the learned policy as a seventh controller, an
episode sampler, lane_id_base, and masked resets that stagger the lanes: each lane's run is a list of segments of its own.
The learned family (make_learned_case / check_learned, at the end) runs the episode family's cases under the learned-policy
engines -- MLP and GRU cell, lane and matrix engine, populations, softmax sampling, the value head and GAE -- with an
episode ledger and a quality model, and checks every slab and record they produce (tests/test_closed_loop_learned_gpu.py).

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


def expected_layout(case, segs, after, res, reward_fn=None):
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
            if reward_fn is not None:                          # the learned family: the reward with a quality term
                rw = reward_fn(case, steps, fin, acts)
            else:
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


def check_episodes(case, out, stats=None, pair_fn=None, run_batch=None, ref=None, reward_fn=None,
                   collect=None):
    """Compare one run of the episode family with the reference closed loop.  `out` (numpy): actions / reward / done
    [T, N], obs [T, 8, N]; per operation: frames (observe_f64 dicts), episodes (episodes() dicts) and speed_logs
    ([rows, N] or None); history (u8 [V, N], f64 [V, N]), qoe [N], entries (FastMPC) or None.  Returns the list of
    mismatches; `stats` collects the non-vacuity counters (assert_non_vacuous_ep).  pair_fn and run_batch replace the
    sampler twin and the oracle replay (the checker's own tests).  ref, reward_fn and collect are the learned family's
    hooks (check_learned): another reference controller, the reward under a quality model, and a dict that receives the
    plan, the replay and the reference for the comparisons that family adds; the defaults are this family's behaviour."""
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
    ref = make_reference(case, out.get("entries")) if ref is None else ref
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
    ex = expected_layout(case, segs, after, res, reward_fn)
    if collect is not None:
        collect.update(segs=segs, after=after, res=res, ex=ex, ref=ref)
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


def _policy_closed_loop(case, segs_k, res, episode_fn=None, ref=None):
    """The policy's closed loop on a batch of segments: the policy is stateless and its answer at call site s depends on
    the actions before s only, so replaying and taking the answers up to the first disagreement converges in at most V
    rounds.  Call sites past a segment's cut keep action 0 (no controller call happens there on the device).  `ref`: the
    learned family's reference (LearnedReference), which is told the actions of the round so that it evaluates no call
    site whose frame is not final yet; the recurrent policy's answer at s depends on frames 0..s, so on the actions before
    s only, and the same argument holds."""
    V = case["meta"]["video_length"]
    lazy = ref is not None
    ref = PolicyReference(case) if ref is None else ref
    a = np.zeros((len(segs_k), V), np.int32)
    n = np.array([sg.n for sg in segs_k])
    while True:
        steps, bw, fin, log, calls = _run_batch(case, segs_k, a)
        eps = [sg.episode for sg in segs_k] if episode_fn is None else episode_fn(segs_k)
        if lazy:
            ref.prepare([sg.lane for sg in segs_k], eps, steps, bw, n, k=segs_k[0].k, acts=a)
        else:
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


# =====================================================================================================================
# The learned family: the learned-policy engines and the per-episode ledgers (make_learned_case / check_learned)
#
# A case of this family is an episode-family case (environment, speed feature, episode mode, sampler, lane_id_base,
# operations, max_ticks: unchanged in kind) whose controller is one of eight learned policies (NETS): an MLP or a GRU
# cell, on the lane engine or the matrix engine, alone or as a population with one weight set per lane group; with
# arg-max or softmax sampling, an exploration coin, a value head or none, an episode ledger or none, a quality model or
# none, and (`single`) launches of one decision taken through select(commit=True) + step instead of step_policy.
#
# check_learned is check_episodes with LearnedReference as the reference controller, plus the outputs this family adds.
# The induction of the module docstring holds unchanged for the recurrent policy: its answer at call site s is a function
# of the frames at call sites 0..s of the lane's segment (h = 0 at s = 0, then h = hp), which by (a) are the reference
# closed loop's frames if the actions before s are the reference's answers.  The member of a population lane is
# local lane // group -- abr_lane_jump.h: pop_member(block_first_lane, group) with block_first_lane = blockIdx.x * the
# block size, an index into the environment's own lanes, and group a multiple of the block size -- never the global id.

NETS = ("mlp", "mlp_mx", "gru", "gru_mx", "pop", "pop_mx", "gru_pop", "gru_pop_mx")
LEARNED_CELLS = [(n, f) for n in NETS for f in SPEEDS]         # cell = seed % 32, mode = (seed // 32) % 4
LEARNED_SLICE = len(LEARNED_CELLS) * len(EP_MODES)              # every (net, speed feature, mode) once
POP_LANES = (300, 512, 600)                                     # 2 or 3 members of 256 lanes, the last partial in two
POP_GROUP = 256
GRU_H = dict(gru=(1, 7, 31, 32, 33, 64), gru_mx=(1, 31, 32, 33, 64, 65, 96, 127, 128))
MX_WIDTHS = (1, 16, 32, 33, 64, 65, 96, 97, 128)
LEDGER_FLOATS = ("rebuffer_time", "start_up_time", "average_latency", "variance", "qoe")
LEDGER_INTS = ("episode", "trace_id", "start_offset", "chunks", "done")
LEDGER_RTOL = dict(rebuffer_time=None, start_up_time=None, average_latency=1e-9, variance=None, qoe=1e-10)
DONE_EPISODE = 1                                                # include/abr_env.h: ABR_DONE_EPISODE


def net_is(case, what):
    net = case["net"]
    return dict(gru=net.startswith("gru"), pop="pop" in net, matrix=net.endswith("_mx"))[what]


def _gru_parts(rng, F, H, M):
    """GRUCell's four tensors and the head's two, scaled by fan-in as _policy_layers scales an MLP."""
    n = lambda sd, *sh: rng.normal(0, sd, sh).astype(np.float32)
    return (n(1.5 / np.sqrt(F), 3 * H, F), n(1.5 / np.sqrt(H), 3 * H, H), n(0.2, 3 * H), n(0.2, 3 * H),
            n(1.5 / np.sqrt(H), M, H), n(0.2, M))


def make_learned_case(seed, n_lanes=None, group=None):
    """A deterministic case of the learned family.  n_lanes / group: smaller lane counts and lane groups for the host-only
    tests (the device takes groups that are multiples of 256)."""
    rng = np.random.default_rng(110_000 + seed)
    net, feature = LEARNED_CELLS[seed % len(LEARNED_CELLS)]
    mode = EP_MODES[(seed // len(LEARNED_CELLS)) % len(EP_MODES)]
    rnd = seed // len(LEARNED_CELLS)
    impls = accepted_impls_ep("policy", feature)
    impl = impls[(rnd + seed // LEARNED_SLICE) % len(impls)]
    pop = "pop" in net
    vbr = rng.random() < 0.5
    auto_reset = mode != "masked"
    # the environment, as make_episode_case draws it
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
    own = POP_LANES[rnd % len(POP_LANES)] if pop else LANES[rnd % len(LANES)]
    N = int(n_lanes if n_lanes is not None else own)
    group = int(group if group is not None else POP_GROUP)
    n_traces = 5
    lens = rng.integers(40, 3000, n_traces)
    lens[int(rng.integers(0, n_traces))] = int(rng.integers(8, 40))
    traces = [rng.uniform(bw_lo, bw_hi, int(n)).astype(np.float32).astype(np.float64) for n in lens]
    tid = rng.integers(0, n_traces, N).astype(np.int32)
    off = np.array([rng.integers(0, lens[t]) for t in tid], np.int32)
    br = np.tile(np.asarray(ladder, np.float64), (V, 1))
    if vbr:
        br = np.sort(br * rng.uniform(0.7, 1.3, (V, 1)) * rng.uniform(0.9, 1.1, (V, B)), axis=1)
    case = dict(seed=seed, family="learned", mode=mode, ctl="policy", net=net, feature=feature, impl=impl, vbr=vbr,
                auto_reset=auto_reset, n_lanes=N,
                meta=dict(ladder=ladder, chunk_length=L, video_length=V, max_buffer=max_buffer, start_up_length=start_up,
                          interval=interval, weights=[4.3, 1.0, 1.0, 0.1], speed=speed if feature == "config" else 1.0),
                traces=traces, tid=tid, off=off, br=br if vbr else None)
    # the policy
    W = int(rng.integers(0, 17))
    F = 4 + W + B
    P = -(-N // group) if pop else 1
    explore = float(rng.choice([0.0, 0.0, 0.3, 1.0]))
    if net_is(case, "gru"):
        H = int(rng.choice(GRU_H["gru_mx" if net_is(case, "matrix") else "gru"]))
        p = policy_params(rng, case, W, [], explore)
        del p["layers"]
        p["hidden"] = H
        members = [dict(parts=_gru_parts(rng, F, H, B)) for _ in range(P)]
        vin = H
    else:
        if net_is(case, "matrix"):
            widths = [int(x) for x in rng.choice(MX_WIDTHS, int(rng.integers(0, 4)))]
            if rng.random() < 0.5:                              # at least one width past the lane engine's 64
                widths = widths or [0]
                widths[int(rng.integers(0, len(widths)))] = int(rng.choice([65, 96, 97, 128]))
        else:
            widths = [int(rng.integers(1, 65)) for _ in range(int(rng.integers(0, 3)))]
        p = policy_params(rng, case, W, widths, explore)
        members = [dict(layers=p.pop("layers"))] + [dict(layers=_policy_layers(rng, F, widths, B)) for _ in range(P - 1)]
        p["widths"] = widths
        vin = widths[-1] if widths else F
    has_head = rng.random() < 2.0 / 3.0
    for mb in members:
        mb["head"] = ((rng.normal(0, 1.0 / np.sqrt(vin), vin).astype(np.float32),
                       rng.normal(0, 0.2, 1).astype(np.float32)) if has_head else None)
    p["sample"] = "softmax" if rng.random() < 0.6 else "argmax"
    p["temperature"] = float(rng.choice([0.5, 0.7, 1.0, 2.0]))
    p["members"], p["group"], p["value"] = members, group, has_head
    case["params"] = p
    # the ledgers
    case["ledger"] = dict(rows=int(rng.choice([1, 2, 3]))) if rng.random() < 0.5 else None
    case["quality"] = None
    if rng.random() < 0.5:
        k = int(rng.integers(0, 4))
        util = ("identity", "log", "log_top")[k] if k < 3 else rng.uniform(-1.0, 3.0, (V, B)).round(3)
        case["quality"] = dict(weight=float(rng.choice([0.37, 1.0, 3.0])), utility=util,
                               rows=case["ledger"]["rows"] if case["ledger"] else 1)
    case["single"] = bool(rng.random() < 0.25)
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
    if mode == "masked":
        at = sorted({int(rng.integers(1, V)), int(rng.integers(V, T - 1))} |
                    {int(x) for x in rng.integers(1, T - 1, n_resets - 1)})
    else:
        at = sorted({int(x) for x in rng.integers(1, T - 1, n_resets)})
    cuts = sorted(set(at) | {int(x) for x in rng.integers(1, T, max(1, T // 5))})
    if case["single"]:                                          # a launch of one decision, split off a longer one
        ends = [0] + cuts + [T]
        if not any(b - a == 1 for a, b in zip(ends, ends[1:])):
            a = max(zip(ends, ends[1:]), key=lambda x: x[1] - x[0])[0]
            cuts = sorted(set(cuts) | {a + 1})
    t = 0
    for c in cuts + [T]:
        if c <= t:
            continue
        ops.append(("launch", c - t))
        t = c
        if t in at:
            ops.append(("reset", _wave_mask(rng, N), "sample" if sampler is not None and rng.random() < 0.6
                        else "given"))
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


def describe_learned(case):
    p = case["params"]
    shape = f"H={p['hidden']}" if net_is(case, "gru") else f"widths={p['widths']}"
    q = case["quality"]
    qs = "none" if q is None else f"{q['weight']}*{q['utility'] if isinstance(q['utility'], str) else 'table'}"
    led = "none" if case["ledger"] is None else case["ledger"]["rows"]
    return (f"learned seed={case['seed']} {case['net']}/{case['feature']}/{case['mode']}/{case['impl']} {shape} "
            f"W={p['window']} {p['sample']} T={p['temperature']} explore={p['explore']} value={int(p['value'])} "
            f"members={len(p['members'])} group={p['group']} ledger={led} quality={qs} single={int(case['single'])} "
            + describe_ep(case))


def quality_table(case):
    """u float64 [V][M] of a case's quality model, from the definitions (README): identity u = br[c][m];
    log u = ln(br[c][m] / br[c][0]); log_top u = ln(br[c][m] / br[c][M - 1]); or the array as it is."""
    import math
    util, br = case["quality"]["utility"], br_table(case)
    if not isinstance(util, str):
        return np.asarray(util, np.float64)
    if util == "identity":
        return np.array(br, np.float64)
    ref = br[:, 0] if util == "log" else br[:, -1]
    return np.array([[math.log(br[c, m] / ref[c]) for m in range(br.shape[1])] for c in range(br.shape[0])])


def launch_spans(case):
    """[(operation index, first decision, decisions)] of the launches."""
    out, t = [], 0
    for oi, op in enumerate(case["ops"]):
        if op[0] == "launch":
            out.append((oi, t, op[1]))
            t += op[1]
    return out


class LearnedReference(PolicyReference):
    """The twins of the learned-policy engines as a reference controller.  MLP nets: policy_sample_twin.decide_sampled's
    decision (the first arg-max, the softmax draw by word 2, the exploration coin by words 0 and 1 of the philox block
    keyed by (seed, global lane id, chunk, the lane's own episode number)) on scores computed once with policy_twin.layer,
    actor_critic_twin's value over the same hidden output.  GRU nets: policy_gru_twin.decide in a loop over the call site
    s = 0..n, vectorised over the batch's segments, h = 0 at s = 0 and h = hp after.  Populations: each member's
    segments with that member's weights, member = local lane // group.  Besides the answers it keeps every call site's
    slabs (features, scores, probs, value, the state the decision started from and the one it left), for check_learned.
    Call site n of a segment -- the frame its last decision left -- is evaluated too: last_value reads it.
    mut: the perturbations of the checker's own tests (tests/test_closed_loop_learned_cpu.py)."""

    def __init__(self, case, entries=None, mut=None):
        super().__init__(case, entries)
        self.mut = mut or {}
        self.slabs, self.seen, self.col, self.segs = {}, {}, {}, None
        self._k, self._P = None, None
        p = case["params"]
        self.gru = net_is(case, "gru")
        self.iT = np.float32(1.0 / p["temperature"])
        self.mode = 1 if p["sample"] == "softmax" else 0
        t, self.launch_starts = 0, set()
        for op in case["ops"]:
            if op[0] == "launch":
                self.launch_starts.add(t)
                t += op[1]

    def member_of(self, lanes):
        p, N = self.case["params"], self.case["n_lanes"]
        g, P = p["group"], len(p["members"])
        lanes = np.asarray(lanes)
        if P == 1:
            return np.zeros(len(lanes), np.int64)
        if self.mut.get("member") == "global":
            return ((global_lanes(self.case)[lanes] // np.uint64(g)) % np.uint64(P)).astype(np.int64)
        mb = lanes // g
        if self.mut.get("member") == "partial_off_by_one" and N % g:
            mb = np.where(mb == P - 1, P - 2, mb)
        return mb

    def _decide(self, mb, x, h, lane, c, ep):
        """One member's decision on columns x [F, n] (h [H, n] for a GRU): dict(actions, scores, probs, value, hp, g,
        coin)."""
        import actor_critic_twin as AC
        import policy_gru_twin as G
        import policy_sample_twin as ST
        import policy_twin as T
        p = self.case["params"]
        M = len(self.case["meta"]["ladder"])
        if self.gru:
            head = None if mb["head"] is None else np.concatenate([mb["head"][0], mb["head"][1]])
            o = G.decide(mb["parts"], x, h, p["seed"], p["thr"], lane, c, ep, M, self.mode, self.iT, head)
            o["g"] = T.argmax_first(o["scores"])
            _, w1, _, _ = T.philox4(p["seed"], lane, c, ep)
            o["coin"] = (w1 < np.uint64(p["thr"])) if p["thr"] < (1 << 32) else np.ones(len(c), bool)
            return o
        y = AC.hidden(mb["layers"], x)
        s = T.layer(mb["layers"][-1][0], mb["layers"][-1][1], y)
        g = T.argmax_first(s)
        if self.mode == ST.ARGMAX:
            pick, probs = g, (np.arange(M)[:, None] == g[None, :]).astype(np.float32)
        else:
            _, _, w2, _ = T.philox4(p["seed"], lane, c, ep)
            pick, probs, _, _ = ST.softmax_sample(s, g, self.iT, w2)
        a, coin = T.explore(p["seed"], p["thr"], lane, c, ep, M, pick)
        v = None
        if mb["head"] is not None:
            v = T.layer(mb["head"][0].reshape(1, -1), mb["head"][1].reshape(1), y)[0]
        return dict(actions=a, scores=s, probs=probs, value=v, hp=None, g=g, coin=coin)

    def _eval(self, rows, sites, lanes, ks, feat, eps2, hcur):
        """Evaluate call site sites[r] of batch rows `rows` and store the slabs; returns the actions."""
        p = self.case["params"]
        x = np.ascontiguousarray(feat[rows, sites].T)                      # [F, n]
        ll = lanes[rows]
        gl = global_lanes(self.case)[ll]
        if self.mut.get("lane") == "mod_2_32":
            gl = gl & np.uint64(0xFFFFFFFF)
        ep = eps2[rows, sites].astype(np.int64)
        if self.mut.get("episode") == "previous":
            ep = np.maximum(ep - (ks[rows] > 0), 0)
        h = None
        if self.gru:
            h = hcur[:, rows].copy()
            for r, (j, s) in enumerate(zip(rows, sites)):
                sg = self.segs[ll[r]][ks[j]] if self.segs is not None else None
                if s == 0:
                    stale = self.mut.get("gru") == "no_restart_at_masked_reset" and sg is not None and sg.reset_start \
                        and sg.k > 0 and ll[r] in self.col
                    h[:, r] = self.col[ll[r]] if stale else 0.0
                elif self.mut.get("gru") == "restart_at_launch" and sg is not None and sg.t0 + s in self.launch_starts:
                    h[:, r] = 0.0
        mbs = self.member_of(ll)
        acts = np.zeros(len(rows), np.int32)
        for m in np.unique(mbs):
            q = np.flatnonzero(mbs == m)
            o = self._decide(p["members"][int(m)], x[:, q], None if h is None else h[:, q], gl[q], sites[q],
                             ep[q].astype(np.uint64))
            acts[q] = o["actions"]
            for r_, a_ in zip(q, range(len(q))):
                j, s = rows[r_], sites[r_]
                sl = self.slabs[(int(ll[r_]), int(ks[j]))]
                sl["features"][s], sl["scores"][s], sl["probs"][s] = x[:, r_], o["scores"][:, a_], o["probs"][:, a_]
                sl["actions"][s], sl["g"][s], sl["coin"][s] = o["actions"][a_], o["g"][a_], o["coin"][a_]
                if o["value"] is not None:
                    sl["value"][s] = o["value"][a_]
                if self.gru:
                    sl["hin"][s], sl["hp"][s] = h[:, r_], o["hp"][:, a_]
                    hcur[:, j] = o["hp"][:, a_]
                sl["sites"] = max(sl["sites"], s + 1)
        return acts

    def prepare(self, lanes, eps, steps, bw, n=None, k=None, acts=None):
        """As PolicyReference.prepare.  k: the batch's segment index (default: counted per lane).  acts [K, V]: the closed
        loop's actions of this round (_policy_closed_loop): a segment is then evaluated only up to the first call site
        whose answer differs from acts -- the frames behind it are not final -- and goes on from there in the next round."""
        import policy_twin as T
        p, m = self.case["params"], self.case["meta"]
        V, M = m["video_length"], len(m["ladder"])
        lanes = np.asarray(lanes)
        K_ = len(lanes)
        n = np.full(K_, V) if n is None else np.asarray(n)
        if k is None:
            ks = np.array([self.seen.get(int(i), 0) for i in lanes])
            for i in lanes:
                self.seen[int(i)] = self.seen.get(int(i), 0) + 1
        else:
            ks = np.full(K_, int(k))
        table = br_table(self.case)
        c = np.tile(np.arange(V), K_)
        hist = np.repeat(bw, V, axis=0).T
        feat = T.features(p["window"], M, V, c, steps["last_bitrate"].reshape(-1), steps["buffer_level"].reshape(-1),
                          steps["global_time"].reshape(-1), steps["play_time"].reshape(-1), hist, lambda r: table[r],
                          p["norm"]).T.reshape(K_, V, -1)
        eps = np.asarray(eps, np.int64)
        eps2 = np.repeat(eps[:, None], V, axis=1) if eps.ndim == 1 else eps
        last = np.minimum(n, V - 1)                                        # call site n: the frame last_value reads
        fresh = acts is None or self._k != (int(ks[0]), K_)
        if fresh:
            self._k = (int(ks[0]), K_)
            self._P = np.zeros(K_, np.int64)
            self._h = np.zeros((p.get("hidden", 1), K_), np.float32)
            F, H = feat.shape[2], p.get("hidden", 0)
            for j, i in enumerate(lanes):
                self.slabs[(int(i), int(ks[j]))] = dict(
                    features=np.zeros((V, F), np.float32), scores=np.zeros((V, M), np.float32),
                    probs=np.zeros((V, M), np.float32), value=np.zeros(V, np.float32), hin=np.zeros((V, H), np.float32),
                    hp=np.zeros((V, H), np.float32), actions=np.full(V, -9, np.int32), g=np.zeros(V, np.int64),
                    coin=np.zeros(V, bool), sites=0)
        P = self._P
        if acts is None and not self.gru:                                  # stateless: every call site at once
            rows = np.repeat(np.arange(K_), last + 1)
            sites = np.concatenate([np.arange(x + 1) for x in last])
            self._eval(rows, sites, lanes, ks, feat, eps2, self._h)
            P[:] = last + 1
        else:
            stopped = np.zeros(K_, bool)
            while ((P <= last) & ~stopped).any():
                rows = np.flatnonzero((P <= last) & ~stopped)
                sites = P[rows].copy()
                a = self._eval(rows, sites, lanes, ks, feat, eps2, self._h)
                P[rows] += 1
                if acts is not None:                                       # a wrong guess: what follows is not final
                    wrong = (sites < n[rows]) & (a != acts[rows, sites])
                    stopped[rows[wrong]] = True
        for j, i in enumerate(lanes):
            sl = self.slabs[(int(i), int(ks[j]))]
            ans = sl["actions"].copy()
            if acts is not None:
                ans[P[j]:] = acts[j, P[j]:]
            self.ans[int(i)] = ans
            done_all = P[j] > last[j]
            if done_all:
                if acts is None:
                    self.coins.extend(sl["coin"][:n[j]].tolist())
                if self.gru and n[j] > 0:
                    self.col[int(i)] = sl["hp"][n[j] - 1].copy()           # the lane's state column after this segment


def _site_index(case, segs):
    """(segment index, call site) of every (decision, lane) of the run; -1 where the lane is idle."""
    T, N = case["n_steps"], case["n_lanes"]
    kk, ss = np.full((T, N), -1, np.int64), np.full((T, N), -1, np.int64)
    for i in range(N):
        for sg in segs[i]:
            kk[sg.t0:sg.t0 + sg.n, i] = sg.k
            ss[sg.t0:sg.t0 + sg.n, i] = np.arange(sg.n)
    return kk, ss


def _variance_in_order(case, acts):
    """The sum over the episode of |br[c][a_c] - br[c + 1][a_(c + 1)]|, added in chunk order (the ledger's variance)."""
    br = br_table(case)
    v = 0.0
    for c in range(len(acts) - 1):
        v = v + abs(br[c][acts[c]] - br[c + 1][acts[c + 1]])
    return v


def learned_reward_fn(case, mut=None):
    """expected_layout's reward of a segment under the case's quality model: float32(r64 - weight * u[c][a]) at every step
    that completed a download -- every live step of a run without time-outs -- r64 the oracle's float64 reward."""
    if case["quality"] is None:
        return None
    u, w = quality_table(case), np.float64(case["quality"]["weight"])
    shift = 1 if (mut or {}).get("quality") == "next_chunk" else 0

    def fn(case, steps, fin, acts):
        m = case["meta"]
        V = m["video_length"]
        r64 = O.step_rewards(steps["rebuffer_time"][None], steps["start_up_time"][None],
                             np.asarray([fin["rebuffer_time"]]), np.asarray([fin["start_up_time"]]), acts[None],
                             m["weights"], ladder=m["ladder"], br_table=case["br"], dtype=np.float64)[0]
        return (r64 - w * u[np.minimum(np.arange(V) + shift, V - 1), acts]).astype(np.float32)
    return fn


def learned_expected(case, segs, after, res, ref, mut=None):
    """What the learned family adds to expected_layout, from the plan, the replay res and the reference's slabs:
    launches (per launch: features / scores / probs / values / hidden [n, ., N], last_value [N]), hidden_after (per
    operation: the controller's state slab [H, N], GRU nets), ledger and quality (the blobs' regions and records after
    the last operation)."""
    import ledger_twin
    mut = mut or {}
    p, m = case["params"], case["meta"]
    V, N, M = m["video_length"], case["n_lanes"], len(m["ladder"])
    F, H = 4 + p["window"] + M, p.get("hidden", 0)
    gru = net_is(case, "gru")
    kk, ss = _site_index(case, segs)
    ex = dict(launches=[], hidden_after=[])
    for oi, t0, n in launch_spans(case):
        L = dict(features=np.zeros((n, F, N), np.float32), scores=np.zeros((n, M, N), np.float32),
                 probs=np.zeros((n, M, N), np.float32), values=np.zeros((n, N), np.float32) if p["value"] else None,
                 hidden=np.zeros((n, H, N), np.float32) if gru else None,
                 last_value=np.zeros(N, np.float32) if p["value"] else None)
        for t in range(t0, t0 + n):
            for i in np.flatnonzero(kk[t] >= 0):                           # an idle (lane, step) keeps the zeros
                sl, s = ref.slabs[(int(i), int(kk[t, i]))], ss[t, i]
                L["features"][t - t0, :, i], L["scores"][t - t0, :, i] = sl["features"][s], sl["scores"][s]
                L["probs"][t - t0, :, i] = sl["probs"][s]
                if p["value"]:
                    L["values"][t - t0, i] = sl["value"][s]
                if gru:
                    L["hidden"][t - t0, :, i] = sl["hp" if mut.get("hidden_out") == "hp" else "hin"][s]
            if mut.get("idle_probs"):
                L["probs"][t - t0, 0, kk[t] < 0] = 1.0
        if p["value"]:
            # last_value: V of the frame the launch leaves behind -- one more forward pass on it that stores no
            # decision: call site c of the lane's current segment (c = 0 after a re-arm or a reset: the recurrent state
            # restarts, so h_in = 0; else h_in is the hp of the decision before); 0.0 for a lane whose done bits are set
            # (policy_gru_twin.select / the header's done-lane rule), which has no next decision.
            ks, finished = after[oi]
            for i in range(N):
                if finished[i]:
                    continue
                sg = segs[i][ks[i]]
                c = _n_at(case, sg, oi)
                if mut.get("last_value") == "before_last_step" and kk[t0 + n - 1, i] >= 0:
                    L["last_value"][i] = L["values"][n - 1, i]
                else:
                    L["last_value"][i] = ref.slabs[(i, sg.k)]["value"][c]
        ex["launches"].append(L)
    # the state slab after every operation: the hp of each lane's last live decision in the run so far; a reset does not
    # touch it; a lane that has not decided yet holds the zeros the controller allocated
    if gru:
        t, cur = 0, np.zeros((H, N), np.float32)
        for op in case["ops"]:
            if op[0] == "launch":
                for tt in range(t, t + op[1]):
                    for i in np.flatnonzero(kk[tt] >= 0):
                        cur[:, i] = ref.slabs[(int(i), int(kk[tt, i]))]["hp"][ss[tt, i]]
                t += op[1]
            ex["hidden_after"].append(cur.copy())
    # the ledger and the quality records: one per finished episode and lane, in order; none for a segment a reset cut
    rows = case["ledger"]["rows"] if case["ledger"] else (case["quality"]["rows"] if case["quality"] else None)
    ex["ledger"] = ex["quality"] = None
    if rows is None:
        return ex
    led = mut.get("ledger_cls", ledger_twin.TwinLedger)(N, rows)
    u = quality_table(case) if case["quality"] else None
    qrec, qtot, qlast = np.zeros((rows, N)), np.zeros(N), np.zeros(N)
    recs = []
    for i in range(N):
        for sg in segs[i]:
            if sg.end != "done" and not (mut.get("ledger") == "abandoned" and sg.end == "cut" and sg.n):
                continue
            steps, bw, fin, acts, _, _ = res[(i, sg.k)]
            slot = int(led.count[i]) % rows
            led.append(i, m["weights"], fin["rebuffer_time"], fin["start_up_time"], fin["average_latency"],
                       _variance_in_order(case, acts), (sg.episode, sg.trace, sg.offset, V, DONE_EPISODE))
            q = 0.0
            if u is not None:
                for c in range(V):                                         # the completed downloads, in call order
                    q = q + u[c, acts[c]]
                qrec[slot, i], qlast[i] = q, q
                qtot[i] = qtot[i] + q
            recs.append((i, sg.k, q))
    count = led.count.copy()
    keep = [r for r in recs if sum(1 for x in recs if x[0] == r[0] and x[1] > r[1]) < rows]      # the last `rows` per lane
    rec = dict(lane=np.array([r[0] for r in keep], np.int64))
    for f, k in enumerate(LEDGER_FLOATS):
        rec[k] = np.array([_slot_of(led, segs, r, rows)[0][f] for r in keep], np.float64)
    for f, k in enumerate(LEDGER_INTS):
        rec[k] = np.array([_slot_of(led, segs, r, rows)[1][f] for r in keep], np.int64)
    rec["quality"] = np.array([r[2] for r in keep], np.float64)
    if case["ledger"]:
        ex["ledger"] = dict(count=count, total=led.total.copy(), rf=led.rf.copy(), ri=led.ri.copy(), records=rec)
    if case["quality"]:
        ex["quality"] = dict(count=count, rec=qrec, total=qtot, last=qlast, records=rec)
    return ex


def _slot_of(led, segs, r, rows):
    """(float fields, int fields) of record r = (lane, segment, quality) in the twin ledger's ring."""
    i, k, _ = r
    no = sum(1 for sg in segs[i] if sg.k < k and sg.end == "done")
    return led.rf[no % rows, :, i], led.ri[no % rows, :, i]


def _cmp_bits(out, name, step, got, want):
    """Float32 arrays on the bit pattern."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        _mm(out, name + ".shape", step, -1, list(got.shape), list(want.shape))
        return
    bad = got.view(np.uint32) != want.view(np.uint32)
    for idx in np.argwhere(bad)[:8]:
        _mm(out, name, step, idx[-1], dict(at=[int(x) for x in idx], value=float(got[tuple(idx)])),
            float(want[tuple(idx)]))


def check_learned(case, out, stats=None, pair_fn=None):
    """Compare one run of the learned family with the reference closed loop: everything check_episodes compares, and
    (float32 on the bit pattern) every slab the launches asked for, last_value, the controller's state slab after every
    operation, the GAE kernel on each launch's own slabs, the quality term of every reward, and the ledger and quality
    records after the last operation.  `out`: check_episodes' dict plus launches (per launch: features, scores, probs,
    values, last_value, hidden, adv, ret), hidden_after (per operation), ledger and quality (dicts of numpy arrays:
    count, total, rf, ri / rec, last; records, per_trace, per_member as the API returns them)."""
    import actor_critic_twin as AC
    stats = {} if stats is None else stats
    ref = LearnedReference(case)
    got = {}
    ref.segs = episode_plan(case, pair_fn)[0]
    mm = check_episodes(case, out, stats, pair_fn=pair_fn, ref=ref, reward_fn=learned_reward_fn(case), collect=got)
    if not got:                                                           # a time-out: nothing to compare against
        return mm
    segs, after, res = got["segs"], got["after"], got["res"]
    ex = learned_expected(case, segs, after, res, ref)
    p = case["params"]
    for li, ((oi, t0, n), L, E) in enumerate(zip(launch_spans(case), out["launches"], ex["launches"])):
        for k in ("features", "scores", "probs", "values", "hidden", "last_value"):
            if E[k] is not None:
                _cmp_bits(mm, k, t0 if k != "last_value" else oi, L[k], E[k])
        if p["value"]:
            sl = slice(t0, t0 + n)
            adv, ret = AC.gae(out["reward"][sl], L["values"], L["last_value"], out["done"][sl], out["actions"][sl],
                              gamma=0.99, lam=0.95)
            _cmp_bits(mm, "gae.adv", t0, L["adv"], adv)
            _cmp_bits(mm, "gae.ret", t0, L["ret"], ret)
    for oi, E in enumerate(ex["hidden_after"]):
        _cmp_bits(mm, "ctl.hidden", oi, out["hidden_after"][oi], E)
    N = case["n_lanes"]
    P, g = len(p["members"]), p["group"]
    if ex["ledger"] is not None:
        G_, E = out["ledger"], ex["ledger"]
        _cmp(mm, "ledger.count", -1, G_["count"], E["count"])
        for f, k in enumerate(LEDGER_FLOATS):
            _cmp(mm, "ledger.total." + k, -1, G_["total"][f], E["total"][f], rtol=1e-10)
            _cmp(mm, "ledger.ring." + k, -1, G_["rf"][:, f].reshape(-1), E["rf"][:, f].reshape(-1),
                 lanes=np.tile(np.arange(N), E["rf"].shape[0]), rtol=LEDGER_RTOL[k])
        for f, k in enumerate(LEDGER_INTS):
            _cmp(mm, "ledger.ring." + k, -1, G_["ri"][:, f].reshape(-1), E["ri"][:, f].reshape(-1),
                 lanes=np.tile(np.arange(N), E["ri"].shape[0]))
        _cmp_records(mm, "ledger.records", G_["records"], E["records"], LEDGER_INTS + LEDGER_FLOATS)
        _cmp_groups(mm, "ledger.per_trace", G_["per_trace"], E["records"], E["records"]["trace_id"], len(case["traces"]),
                    LEDGER_FLOATS)
        if P > 1:
            tot = {k: E["total"][f] for f, k in enumerate(LEDGER_FLOATS)}
            _cmp_members(mm, "ledger.per_member", G_["per_member"], E["count"], tot, g, P)
    if ex["quality"] is not None:
        G_, E = out["quality"], ex["quality"]
        _cmp(mm, "quality.count", -1, G_["count"], E["count"])
        _cmp(mm, "quality.ring", -1, G_["rec"].reshape(-1), E["rec"].reshape(-1),
             lanes=np.tile(np.arange(N), E["rec"].shape[0]))
        _cmp(mm, "quality.last", -1, G_["last"], E["last"])
        _cmp(mm, "quality.total", -1, G_["total"], E["total"], rtol=1e-10)
        keys = ("quality",) + ((LEDGER_INTS + LEDGER_FLOATS) if case["ledger"] else ())
        _cmp_records(mm, "quality.records", G_["records"], E["records"], keys)
        if case["ledger"] and len(G_["records"]["qoe_q"]) == len(E["records"]["lane"]):
            # qoe_q is qoe - weight * quality of the SAME record (tests/test_quality_gpu.py): `==` on the record's own
            # fields, which are compared above (qoe at 1e-10, quality exactly).  Against the oracle's qoe the difference
            # cancels -- the two terms are of one size -- so a relative bound on it would bound nothing.
            want = G_["records"]["qoe"] - np.float64(case["quality"]["weight"]) * G_["records"]["quality"]
            _cmp(mm, "quality.records.qoe_q", -1, G_["records"]["qoe_q"], want, lanes=E["records"]["lane"])
    _learned_stats(case, stats, segs, after, ref, ex, out)
    return mm


def _cmp_records(mm, name, got, want, keys):
    if not np.array_equal(np.asarray(got["lane"]), want["lane"]):
        _mm(mm, name + ".lane", -1, -1, np.asarray(got["lane"]).tolist()[:8], want["lane"].tolist()[:8])
        return
    for k in keys:
        _cmp(mm, f"{name}.{k}", -1, got[k], want[k], lanes=want["lane"], rtol=LEDGER_RTOL.get(k))


def _cmp_groups(mm, name, got, rec, key, n, fields):
    key = np.asarray(key, np.int64)
    cnt = np.bincount(key, minlength=n)
    _cmp(mm, name + ".count", -1, got["count"], cnt)
    has = cnt > 0
    for k in fields:
        s = np.zeros(n)
        np.add.at(s, key, rec[k])
        _cmp(mm, f"{name}.{k}", -1, np.asarray(got[k])[has], (s[has] / cnt[has]), lanes=np.flatnonzero(has),
             rtol=LEDGER_RTOL[k] or 1e-10)


def _cmp_members(mm, name, got, count, totals, group, P):
    mb = np.arange(len(count)) // group
    cnt = np.bincount(mb, weights=count, minlength=P).astype(np.int64)
    _cmp(mm, name + ".count", -1, got["count"], cnt)
    for k, v in totals.items():
        s = np.bincount(mb, weights=v, minlength=P)
        _cmp(mm, f"{name}.{k}", -1, got[k], s / np.maximum(cnt, 1), rtol=LEDGER_RTOL[k] or 1e-10)


def _learned_stats(case, stats, segs, after, ref, ex, out):
    """The non-vacuity counters of one checked case (assert_non_vacuous_learned)."""
    p, m = case["params"], case["meta"]
    V, N, M = m["video_length"], case["n_lanes"], len(m["ladder"])
    inc = lambda k, v=1: stats.__setitem__(k, stats.get(k, 0) + int(v))
    stats.setdefault("net_impls", {}).setdefault(case["net"], set()).add(case["impl"])
    kk, ss = _site_index(case, segs)
    acts = out["actions"]
    for (i, k), sl in ref.slabs.items():
        n = segs[i][k].n
        if p["sample"] == "softmax" and n:
            own = ~sl["coin"][:n]
            inc("soft_differs", (own & (sl["actions"][:n] != sl["g"][:n])).sum())
            inc("soft_equals", (own & (sl["actions"][:n] == sl["g"][:n])).sum())
    if M >= 6 and set(np.unique(acts[acts >= 0]).tolist()) == set(range(M)):
        inc("all_actions")
    gru = net_is(case, "gru")
    if gru:
        for i in range(N):
            for sg in segs[i][1:]:
                pv = segs[i][sg.k - 1]
                if sg.reset_start and pv.end == "cut" and pv.n and sg.n and \
                        ref.slabs[(i, pv.k)]["hp"][pv.n - 1].any():
                    inc("gru_masked_rearm")
        if case["impl"] in ("split", "split3", "auto"):
            inner = set()
            for _, t0, n in launch_spans(case):
                inner |= set(range(t0 + 1, t0 + n))
            inc("gru_mid_launch_rearm", any(sg.t0 in inner and not sg.reset_start and sg.k > 0 and sg.n
                                            for s in segs for sg in s))
    for t in range(kk.shape[0]):
        for w in range(0, N, 64):
            s = ss[t, w:w + 64]
            if (s == 0).any() and (s > 0).any():
                inc("wave_mixed_chunks")
                break
        else:
            continue
        break
    P, g = len(p["members"]), p["group"]
    if P > 1:
        if N % g and (acts[:, (P - 1) * g:] >= 0).any():
            inc("partial_group_decided")
        mb = np.arange(N) // g
        for c in range(V):
            sets = [set(acts[(ss == c) & (mb[None, :] == q)].tolist()) for q in range(P)]
            if sum(1 for x in sets if x) >= 2 and len(set().union(*sets)) > 1:
                inc("members_differ")
                break
    cut_and_done = any({sg.end for sg in s if sg.n} >= {"cut", "done"} for s in segs)
    if case["ledger"]:
        inc("ledger_wrapped", (ex["ledger"]["count"] > case["ledger"]["rows"]).any())
        inc("ledger_cut_and_done", cut_and_done)
    if case["quality"]:
        inc("quality_cut_and_done", cut_and_done)
    if case["single"]:
        inc("single_decisions", any(n == 1 and (kk[t0] >= 0).any() for _, t0, n in launch_spans(case)))
    if case["lane_id_base"] >= 2 ** 32 and p["sample"] == "softmax":
        inc("high_lane_ids_softmax")


def assert_non_vacuous_learned(stats, cases):
    """The learned family's aggregate over a slice: what the fuzz is meant to reach, it reached."""
    problems = []
    for net in NETS:
        got = stats.get("net_impls", {}).get(net, set())
        if got != set(accepted_impls_ep("policy", "config")):
            problems.append(f"{net} ran on {sorted(got)} only")
    for k, what in (("soft_differs", "no softmax pick differed from the arg-max"),
                    ("soft_equals", "no softmax pick equalled the arg-max"),
                    ("all_actions", "no case with M >= 6 answered every action"),
                    ("gru_masked_rearm", "no running GRU lane with a nonzero state was re-armed by a masked reset and "
                                         "decided afterwards"),
                    ("gru_mid_launch_rearm", "no GRU lane was re-armed in the middle of a launch on a role-split impl"),
                    ("wave_mixed_chunks", "no wave decided with lanes at chunk 0 and lanes past it"),
                    ("partial_group_decided", "no population's partial last group took decisions"),
                    ("members_differ", "no two members answered differently at call sites of one chunk index"),
                    ("ledger_wrapped", "no ledger ring wrapped"),
                    ("ledger_cut_and_done", "no ledger case had an abandoned and a finished episode on one lane"),
                    ("quality_cut_and_done", "no quality case had an abandoned and a finished episode on one lane"),
                    ("single_decisions", "no decision went through select + step"),
                    ("high_lane_ids_softmax", "no lane_id_base >= 2^32 under softmax")):
        if not stats.get(k):
            problems.append(what)
    if stats.get("explore") != {True, False}:
        problems.append(f"the exploration coin fell {sorted(stats.get('explore', ()))}")
    mx = [c["params"] for c in cases if net_is(c, "matrix")]
    sizes = [w for q in mx for w in (q.get("widths") or []) + ([q["hidden"]] if "hidden" in q else [])]
    if not any(w > 64 for w in sizes) or not any(w % 32 for w in sizes):
        problems.append("no matrix-engine case past 64 units, or none off the 32-row tile")
    return problems


def oracle_run_learned(case, pair_fn=None, mut=None):
    """The reference closed loop of a learned-family case on the host, laid out as a device run: the `out` dict
    check_learned takes.  _policy_closed_loop's fixed-point iteration with LearnedReference (the recurrent policy's
    answer at s depends on the actions before s only, so it converges in at most V rounds as well).  pair_fn and mut
    (LearnedReference, learned_expected, learned_reward_fn) build the wrong runs of the checker's own tests."""
    import actor_critic_twin as AC
    mut = mut or {}
    segs, after = episode_plan(case, pair_fn)
    ref = LearnedReference(case, mut=mut)
    ref.segs = segs
    res = {}
    for k in range(max(len(s) for s in segs)):
        _policy_closed_loop(case, [s[k] for s in segs if len(s) > k], res, ref=ref)
    ex = expected_layout(case, segs, after, res, learned_reward_fn(case, mut))
    out = {k: ex[k] for k in ("actions", "reward", "done", "obs")}
    out["frames"], out["episodes"], out["speed_logs"] = ex["frames"], ex["episodes"], ex["speed_logs"]
    out["history"], out["qoe"], out["entries"] = ex["history"], ex["qoe"], None
    if mut.get("quality") == "on_idle" and case["quality"]:             # the term applied where nothing was downloaded
        u, w = quality_table(case), case["quality"]["weight"]
        idle = out["actions"] < 0
        out["reward"] = np.where(idle, np.float32(-w * u[-1, 0]), out["reward"]).astype(np.float32)
    le = learned_expected(case, segs, after, res, ref, mut)
    for (oi, t0, n), L in zip(launch_spans(case), le["launches"]):
        if case["params"]["value"]:
            sl = slice(t0, t0 + n)
            L["adv"], L["ret"] = AC.gae(out["reward"][sl], L["values"], L["last_value"], out["done"][sl],
                                        out["actions"][sl], gamma=0.99, lam=0.95)
    out["launches"], out["hidden_after"] = le["launches"], le["hidden_after"]
    N, p = case["n_lanes"], case["params"]
    P, g = len(p["members"]), p["group"]
    rec = le["ledger"]["records"] if le["ledger"] else (le["quality"]["records"] if le["quality"] else None)
    out["ledger"] = out["quality"] = None
    if le["ledger"]:
        E = le["ledger"]
        nt = len(case["traces"])
        cnt = np.bincount(rec["trace_id"], minlength=nt)
        per_trace = dict(count=cnt)
        for k in LEDGER_FLOATS:
            s = np.zeros(nt)
            np.add.at(s, rec["trace_id"], rec[k])
            with np.errstate(all="ignore"):
                per_trace[k] = s / cnt
        mb = np.arange(N) // g
        mc = np.bincount(mb, weights=E["count"], minlength=P).astype(np.int64)
        per_member = dict(count=mc)
        for f, k in enumerate(LEDGER_FLOATS):
            per_member[k] = np.bincount(mb, weights=E["total"][f], minlength=P) / np.maximum(mc, 1)
        out["ledger"] = dict(E, per_trace=per_trace, per_member=per_member if P > 1 else None)
    if le["quality"]:
        E = le["quality"]
        r = dict(rec)
        if le["ledger"]:
            r["qoe_q"] = rec["qoe"] - np.float64(case["quality"]["weight"]) * rec["quality"]
        out["quality"] = dict(E, records=r)
    return out
