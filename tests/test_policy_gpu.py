"""The learned policy on the device: abr_env_policy_select against the numpy twin bit for bit on states reached by random
rollouts, the fused rollout closed against the oracle (tests/closed_loop_check.py's (a) + (b) argument with the policy's
twin as the reference controller: closed_loop_check.PolicyReference), the fused rollout against select + step, the
exploration draw against step_random, finished lanes, refusals and load_weights."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_check as K
import policy_twin as T

pytestmark = pytest.mark.gpu

LADDER = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]


def _layers(rng, F, widths, M):
    out, fan = [], F
    for w in widths + [M]:
        out.append((rng.normal(0, 1.5 / np.sqrt(fan), (w, fan)).astype(np.float32),
                    rng.normal(0, 0.2, w).astype(np.float32)))
        fan = w
    return out


def _env(A, V, N, rng, br=None, speeds=None, auto_reset=False, impl="auto", traces=None):
    L = 4.0
    chunks = A.Chunk(LADDER) if br is None else [A.Chunk(list(r)) for r in br]
    mpd = A.MPD(V, L, 12.0, 4.0, chunks)
    traces = traces or [rng.uniform(0.3, 7.0, int(n)).astype(np.float32).astype(np.float64) for n in (500, 901, 333)]
    env = A.BatchedABREnv(mpd, A.QOEMetric(4.3, 1.0, 1.0, 0.1), A.NetworkInfo(1.0, traces), N,
                          speed=1.0 if speeds is None else torch.from_numpy(speeds), impl=impl, auto_reset=auto_reset)
    tid = rng.integers(0, len(traces), N).astype(np.int32)
    off = rng.integers(0, 333, N).astype(np.int32)
    env.reset(torch.from_numpy(tid), torch.from_numpy(off))
    return env


def _twin_select(env, ctl, layers, br_table, episode=0):
    """The twin's (features [F, N], scores [M, N], actions [N]) on the environment's current state."""
    f = {k: v.cpu().numpy() for k, v in env.observe_f64().items()}
    hist = env.history()[1].cpu().numpy()
    N, V, M = env.n_lanes, env.video_length, env.n_rates
    c = f["chunk_id"].astype(np.int64)
    dn = env.mpc_inputs()[5].cpu().numpy()
    cc = np.clip(c, 0, V - 1)
    norm = ctl.norm.cpu().numpy() if ctl.norm is not None else None
    x = T.features(ctl.window, M, V, cc, f["last_bitrate"].astype(np.int64), f["buffer_level"], f["global_time"],
                   f["play_time"], hist, lambda r: br_table[r], norm)
    a, s, _ = T.decide(layers, x, ctl.seed, ctl.explore_threshold, np.arange(N), cc, episode, M)
    live = (dn == 0) & (c < V)
    x[:, ~live] = 0.0
    s[:, ~live] = 0.0
    a = np.where(live, a, -1)
    return x, s, a


def test_select_matches_twin_on_random_rollout_states():
    import abrsimulator_amd as A
    rng = np.random.default_rng(11)
    V, N = 20, 4096
    br = np.sort(np.tile(LADDER, (V, 1)) * rng.uniform(0.8, 1.2, (V, 6)), axis=1)
    speeds = rng.choice([0.75, 1.0, 1.25, 1.5], N)
    env = _env(A, V, N, rng, br=br, speeds=speeds)
    for ep, (W, widths, explore) in enumerate(((8, [64, 64], 0.0), (16, [5], 0.25), (0, [], 0.0), (1, [64, 1], 1.0))):
        env.reset()                                                        # the lanes' episode number is now ep + 1
        F = 4 + W + 6
        layers = _layers(rng, F, widths, 6)
        ctl = A.PolicyController(A.EnvPlayer(env), layers, window=W, explore=explore, seed=int(rng.integers(1 << 62)))
        seen = set()
        for s in range(0, V + 2, 3):
            out = ctl.select()
            x, sc, a = _twin_select(env, ctl, layers, br, episode=ep + 1)
            got_x = out["features"].cpu().numpy()
            got_s = out["scores"].cpu().numpy()
            eq = lambda u, v: ((u.view(np.uint32) == v.view(np.uint32)) | (np.isnan(u) & np.isnan(v))).all()
            assert eq(got_x, x), (W, widths, s)
            assert eq(got_s, sc), (W, widths, s)
            assert np.array_equal(out["actions"].cpu().numpy(), a), (W, widths, s)
            seen.update(np.unique(a).tolist())
            env.step_random(3, seed=int(rng.integers(1 << 62)), want_actions=False)
        assert -1 in seen and len(seen) >= 3, seen


# ---------------------------------------------------------------------------------------------------------------------
# closed loop against the oracle

def _policy_case(seed, W, widths, explore, auto_reset, impl, n_lanes=None):
    rng = np.random.default_rng(900 + seed)
    for s in range(seed, seed + 10_000):                                   # a case whose speed feature the policy takes
        case = K.make_case(s, n_lanes)
        if case["feature"] in ("config", "lanes", "schedule"):
            break
    V = case["meta"]["video_length"]
    M = len(case["meta"]["ladder"])
    T_ = (2 * V + 1 + int(rng.integers(0, max(1, V - 1)))) if auto_reset else V + 2 + int(rng.integers(0, 3))
    cuts = sorted({int(x) for x in rng.integers(1, T_, max(1, T_ // 4))} - {k * V for k in range(1, T_ // V + 1)})
    F = 4 + W + M
    thr = (1 << 32) if explore >= 1.0 else int(np.floor(explore * 2.0 ** 32))
    top = float(K.br_table(case).max())
    norm = np.stack([np.zeros(F), np.r_[1 / case["meta"]["max_buffer"], 1 / top, 1 / V, 0.1, np.full(W + M, 1 / top)]])
    case.update(ctl="policy", impl=impl, auto_reset=auto_reset, n_steps=T_, pieces=np.diff([0] + cuts + [T_]).tolist(),
                lane_ids=np.arange(case["n_lanes"]),
                params=dict(window=W, layers=_layers(rng, F, widths, M), seed=int(rng.integers(1 << 62)), thr=thr,
                            explore=explore, norm=norm))
    return case


def run_policy_case(case, want_scores=False):
    import abrsimulator_amd as A
    m, p = case["meta"], case["params"]
    V, N = m["video_length"], case["n_lanes"]
    chunks = A.Chunk(m["ladder"]) if case["br"] is None else [A.Chunk(list(r)) for r in case["br"]]
    mpd = A.MPD(V, m["chunk_length"], m["max_buffer"], m["start_up_length"], chunks)
    speed = m["speed"]
    if case["feature"] == "lanes":
        speed = torch.from_numpy(np.asarray(case["lane_speeds"], np.float64))
    elif case["feature"] == "schedule":
        speed = torch.from_numpy(np.ascontiguousarray(np.asarray(case["schedule"], np.float64).T))
    env = A.BatchedABREnv(mpd, A.QOEMetric(*m["weights"]), A.NetworkInfo(m["interval"], case["traces"]), N,
                          speed=speed, impl=case["impl"], auto_reset=case["auto_reset"], max_ticks=case["max_ticks"])
    env.reset(torch.from_numpy(case["tid"]), torch.from_numpy(case["off"]))
    ctl = A.PolicyController(A.EnvPlayer(env), p["layers"], window=p["window"], norm=(p["norm"][0], p["norm"][1]),
                             explore=p["explore"], seed=p["seed"])
    assert ctl.explore_threshold == p["thr"]
    parts, frames, t = [], [], 0
    for n in case["pieces"]:
        o = env.step_policy(ctl, n, want_features=True, want_scores=want_scores)
        parts.append({k: v.cpu().numpy() for k, v in o.items() if v is not None})
        t += n
        frames.append((t, {k: v.cpu().numpy().copy() for k, v in env.observe_f64().items()}))
    out = {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}
    out["frames"] = frames
    out["history"] = tuple(x.cpu().numpy().copy() for x in env.history())
    out["qoe"] = env.episode_qoe().cpu().numpy()
    out["speed_log"] = None
    out["entries"] = None
    torch.cuda.synchronize()
    env.close()
    return out


CLOSED = [  # (seed, W, widths, explore, auto_reset, impl)
    (0, 8, [16, 16], 0.0, False, "auto"), (1, 0, [8], 0.25, True, "jump"), (2, 16, [], 0.0, True, "split"),
    (3, 1, [12, 7], 0.25, False, "split3"), (4, 8, [64, 64], 0.25, True, "auto"), (5, 16, [3], 0.0, False, "jump"),
    (6, 1, [], 0.25, True, "split3"), (7, 0, [64, 1], 0.0, True, "split"),
]


def test_closed_loop_against_the_oracle():
    answers, explored = set(), 0
    for (seed, W, widths, explore, auto_reset, impl) in CLOSED:
        case = _policy_case(seed, W, widths, explore, auto_reset, impl)
        out = run_policy_case(case)
        stats = {}
        mm = K.check(case, out, stats)
        assert not mm, (K.describe(case), W, widths, len(mm), mm[:6])
        answers |= stats["answers"]["policy"]
        explored += explore > 0
    assert len(answers) >= 3 and explored >= 3


def test_closed_loop_sampled_lanes_at_65536():
    case = _policy_case(10, 8, [64, 64], 0.5, False, "auto", n_lanes=65536)
    out = run_policy_case(case)
    rng = np.random.default_rng(3)
    pick = np.sort(rng.choice(case["n_lanes"], 256, replace=False))
    sub = dict(case, n_lanes=len(pick), tid=case["tid"][pick], off=case["off"][pick], lane_ids=pick)
    for k in ("lane_speeds", "schedule"):
        if k in case:
            sub[k] = np.asarray(case[k])[pick]
    o = dict(out)
    for k in ("actions", "reward", "done"):
        o[k] = out[k][:, pick]
    o["obs"] = out["obs"][:, :, pick]
    o["frames"] = [(t, {k: v[pick] for k, v in f.items()}) for t, f in out["frames"]]
    o["history"] = tuple(h[:, pick] for h in out["history"])
    o["qoe"] = out["qoe"][pick]
    stats = {}
    mm = K.check(sub, o, stats)
    assert not mm, mm[:6]
    assert len(stats["answers"]["policy"]) >= min(2, len(case["meta"]["ladder"]))


# ---------------------------------------------------------------------------------------------------------------------
# the fused rollout, the exploration wiring, finished lanes, refusals, load_weights

def test_fused_equals_select_plus_step():
    import abrsimulator_amd as A
    rng = np.random.default_rng(21)
    V, N, n = 10, 1000, 13
    for impl in ("auto", "jump", "split"):
        envs = [_env(A, V, N, np.random.default_rng(5), impl=impl, auto_reset=True) for _ in range(2)]
        layers = _layers(rng, 4 + 4 + 6, [32], 6)
        ctls = [A.PolicyController(A.EnvPlayer(e), layers, window=4, explore=0.3, seed=99) for e in envs]
        fused = envs[0].step_policy(ctls[0], n, want_features=True, want_scores=True)
        for s in range(n):
            sel = ctls[1].select()
            obs, rew, dn = envs[1].step(sel["actions"])
            assert torch.equal(fused["actions"][s], sel["actions"]), (impl, s)
            assert torch.equal(fused["features"][s], sel["features"]), (impl, s)
            assert torch.equal(fused["scores"][s], sel["scores"]), (impl, s)
            assert torch.equal(fused["obs"][s], obs), (impl, s)
            assert torch.equal(fused["reward"][s], rew), (impl, s)
            assert torch.equal(fused["done"][s], dn), (impl, s)
        for e in envs:
            e.close()


def test_always_explore_equals_step_random():
    import abrsimulator_amd as A
    V, N = 12, 3000
    for auto_reset in (False, True):
        envs = [_env(A, V, N, np.random.default_rng(8), auto_reset=auto_reset) for _ in range(2)]
        for e in envs:
            e.reset()                                                      # episode number 1 after a re-reset
        ctl = A.PolicyController(A.EnvPlayer(envs[0]), _layers(np.random.default_rng(1), 4 + 2 + 6, [], 6), window=2,
                                 explore=1.0, seed=123456789123)
        assert ctl.explore_threshold == 1 << 32
        a = envs[0].step_policy(ctl, 2 * V + 3)
        b = envs[1].step_random(2 * V + 3, seed=123456789123)
        for k in ("actions", "obs", "reward", "done"):
            assert torch.equal(a[k], b[k]), (auto_reset, k)
        for e in envs:
            e.close()


def test_done_lanes_tick_refusal_and_weight_size():
    import abrsimulator_amd as A
    from abrsimulator_amd import _lib
    V, N = 6, 500
    env = _env(A, V, N, np.random.default_rng(2))
    ctl = A.PolicyController(A.EnvPlayer(env), _layers(np.random.default_rng(3), 4 + 3 + 6, [8], 6), window=3)
    out = env.step_policy(ctl, V + 2, want_features=True, want_scores=True)
    assert (out["actions"][:V] >= 0).all() and (out["actions"][V:] == -1).all()
    assert (out["features"][V:] == 0).all() and (out["scores"][V:] == 0).all()
    assert (out["features"][V:].view(torch.int32) == 0).all()              # +0.0f
    sel = ctl.select()
    assert (sel["actions"] == -1).all() and (sel["features"] == 0).all()
    env.close()
    tick = _env(A, V, N, np.random.default_rng(2), impl="tick")
    ctl = A.PolicyController(A.EnvPlayer(tick), _layers(np.random.default_rng(3), 4 + 3 + 6, [8], 6), window=3)
    with pytest.raises(_lib.AbrError, match=r"-4"):
        tick.step_policy(ctl, 2)
    assert (ctl.next_bitrate() >= 0).all()                                 # select runs on every impl
    pol = ctl.bound(tick)
    pol.weights_bytes -= 4
    act = torch.empty(N, dtype=torch.int32, device=tick.device)
    rc = tick.lib.abr_env_policy_select(tick._h, C.byref(pol), _lib.ptr(act), None, None, None)
    assert rc == -1 and b"weights_bytes" in tick.lib.abr_last_error()
    rc = tick.lib.abr_env_step_policy(tick._h, C.byref(pol), 1, None, None, None, None, None, None, None)
    assert rc == -1 and b"weights_bytes" in tick.lib.abr_last_error()
    tick.close()


def test_load_weights_between_rollouts():
    import abrsimulator_amd as A
    rng = np.random.default_rng(31)
    V, N = 16, 2048
    env = _env(A, V, N, np.random.default_rng(6))
    net = torch.nn.Sequential(torch.nn.Linear(4 + 8 + 6, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64),
                              torch.nn.ReLU(), torch.nn.Linear(64, 6)).cuda()
    ctl = A.PolicyController.from_module(A.EnvPlayer(env), net, window=8)
    layers = [(W.detach().cpu().numpy(), b.detach().cpu().numpy()) for W, b in A.PolicyController.module_layers(net)]
    assert np.array_equal(ctl.weights.cpu().numpy(), A.policy.pack_layers(layers))
    env.step_policy(ctl, 3)
    first = ctl.select()
    x, s, a = _twin_select(env, ctl, layers, np.tile(LADDER, (V, 1)))
    assert np.array_equal(first["actions"].cpu().numpy(), a)
    with torch.no_grad():
        for prm in net.parameters():
            prm.add_(torch.randn_like(prm))
    ctl.load_weights(net)                                                  # in place, on the stream
    layers2 = [(W.detach().cpu().numpy(), b.detach().cpu().numpy()) for W, b in A.PolicyController.module_layers(net)]
    second = ctl.select()
    x2, s2, a2 = _twin_select(env, ctl, layers2, np.tile(LADDER, (V, 1)))
    assert np.array_equal(second["actions"].cpu().numpy(), a2)
    assert torch.equal(first["features"], second["features"]) and not torch.equal(first["scores"], second["scores"])
    eq = lambda u, v: ((u.view(np.uint32) == v.view(np.uint32)) | (np.isnan(u) & np.isnan(v))).all()
    assert eq(second["scores"].cpu().numpy(), s2)
    env.close()
