"""The learned policy's sampled decisions on the device: abr_env_policy_select_sampled against the numpy twin
(tests/policy_sample_twin.py) bit for bit on states reached by random rollouts; mode 0 against the argmax entries; the
fused sampled rollout against select + step; the closed loop against the oracle (tests/closed_loop_check.py's argument
with the sampled twin as the reference, patched in with monkeypatch); the draw's frequencies on one replicated state;
the zero-temperature limit; resume from a state_dict and shards by lane_id_base."""
import functools

import numpy as np
import pytest
import torch

import closed_loop_check as K
import policy_sample_twin as ST
import policy_twin as T
from test_policy_gpu import LADDER, _env, _layers, _policy_case, run_policy_case

pytestmark = pytest.mark.gpu

f32 = np.float32


def _bits_eq(u, v):
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    return ((u.view(np.uint32) == v.view(np.uint32)) | (np.isnan(u) & np.isnan(v))).all()


def _twin_select(env, ctl, layers, br_table, episode):
    """The sampled twin's (features [F, N], scores [M, N], actions [N], probs [M, N]) on the environment's state."""
    f = {k: v.cpu().numpy() for k, v in env.observe_f64().items()}
    hist = env.history()[1].cpu().numpy()
    N, V, M = env.n_lanes, env.video_length, env.n_rates
    c = f["chunk_id"].astype(np.int64)
    dn = env.mpc_inputs()[5].cpu().numpy()
    cc = np.clip(c, 0, V - 1)
    norm = ctl.norm.cpu().numpy() if ctl.norm is not None else None
    x = T.features(ctl.window, M, V, cc, f["last_bitrate"].astype(np.int64), f["buffer_level"], f["global_time"],
                   f["play_time"], hist, lambda r: br_table[r], norm)
    mode = ST.SOFTMAX if ctl.sample == "softmax" else ST.ARGMAX
    a, s, _, p = ST.decide_sampled(layers, x, ctl.seed, ctl.explore_threshold, np.arange(N), cc, episode, M,
                                   ctl.inv_temperature, mode)
    live = (dn == 0) & (c < V)
    x[:, ~live] = 0.0
    s[:, ~live] = 0.0
    p[:, ~live] = 0.0
    return x, s, np.where(live, a, -1), p


def test_select_sampled_matches_twin_on_random_rollout_states():
    import abrsimulator_amd as A
    rng = np.random.default_rng(71)
    V, N = 20, 4096
    br = np.sort(np.tile(LADDER, (V, 1)) * rng.uniform(0.8, 1.2, (V, 6)), axis=1)
    speeds = rng.choice([0.75, 1.0, 1.25, 1.5], N)
    env = _env(A, V, N, rng, br=br, speeds=speeds)
    shapes = ((8, [64, 64], 0.0, 1.0), (16, [5], 0.25, 0.3), (0, [], 0.0, 2.0), (1, [64, 1], 1.0, 1.0),
              (4, [16, 16], 0.25, 0.05))
    for ep, (W, widths, explore, temp) in enumerate(shapes):
        env.reset()                                                        # the lanes' episode number is now ep + 1
        layers = _layers(rng, 4 + W + 6, widths, 6)
        ctl = A.PolicyController(A.EnvPlayer(env), layers, window=W, explore=explore, seed=int(rng.integers(1 << 62)),
                                 sample="softmax", temperature=temp)
        seen, spread = set(), 0
        for s in range(0, V + 2, 3):
            out = ctl.select(want_probs=True)
            x, sc, a, p = _twin_select(env, ctl, layers, br, episode=ep + 1)
            assert _bits_eq(out["features"].cpu().numpy(), x), (W, widths, s)
            assert _bits_eq(out["scores"].cpu().numpy(), sc), (W, widths, s)
            assert _bits_eq(out["probs"].cpu().numpy(), p), (W, widths, s)
            assert np.array_equal(out["actions"].cpu().numpy(), a), (W, widths, s)
            seen.update(np.unique(a).tolist())
            spread += int(((p > 0.05) & (p < 0.95)).any(0).sum())
            env.step_random(3, seed=int(rng.integers(1 << 62)), want_actions=False)
        assert -1 in seen and len(seen) >= 3 and spread > 0, (seen, spread)
    env.close()


def test_argmax_mode_equals_the_argmax_entries():
    import abrsimulator_amd as A
    rng = np.random.default_rng(72)
    V, N, n = 12, 3000, 2 * 12 + 3
    envs = [_env(A, V, N, np.random.default_rng(9), auto_reset=True) for _ in range(2)]
    layers = _layers(rng, 4 + 4 + 6, [32, 8], 6)
    ctls = [A.PolicyController(A.EnvPlayer(e), layers, window=4, explore=0.3, seed=77) for e in envs]
    assert not ctls[0].uses_sampled_entries(False)
    old = ctls[0].select()
    new = ctls[1].select(want_probs=True)                                 # abr_env_policy_select_sampled, mode 0
    for k in ("actions", "features", "scores"):
        assert torch.equal(old[k], new[k]), k
    g = torch.from_numpy(T.argmax_first(old["scores"].cpu().numpy())).to(new["probs"].device)
    assert torch.equal(new["probs"], torch.nn.functional.one_hot(g, 6).T.float())
    a = envs[0].step_policy(ctls[0], n, want_features=True, want_scores=True)
    b = envs[1].step_policy(ctls[1], n, want_features=True, want_scores=True, want_probs=True)
    for k in ("actions", "features", "scores", "obs", "reward", "done"):
        assert torch.equal(a[k], b[k]), k
    live = b["actions"] >= 0
    assert torch.equal(b["probs"].sum(1)[live], torch.ones_like(b["probs"].sum(1)[live]))
    for e in envs:
        e.close()


def test_fused_sampled_equals_select_plus_step():
    import abrsimulator_amd as A
    rng = np.random.default_rng(73)
    V, N, n = 10, 1000, 23
    for impl in ("auto", "jump", "split", "split3"):
        envs = [_env(A, V, N, np.random.default_rng(5), impl=impl, auto_reset=True) for _ in range(2)]
        layers = _layers(rng, 4 + 4 + 6, [32], 6)
        ctls = [A.PolicyController(A.EnvPlayer(e), layers, window=4, explore=0.2, seed=99, sample="softmax",
                                   temperature=0.8) for e in envs]
        fused = envs[0].step_policy(ctls[0], n, want_features=True, want_scores=True, want_probs=True)
        for s in range(n):
            sel = ctls[1].select(want_probs=True)
            obs, rew, dn = envs[1].step(sel["actions"])
            for k in ("actions", "features", "scores", "probs"):
                assert torch.equal(fused[k][s], sel[k]), (impl, s, k)
            assert torch.equal(fused["obs"][s], obs), (impl, s)
            assert torch.equal(fused["reward"][s], rew), (impl, s)
            assert torch.equal(fused["done"][s], dn), (impl, s)
        for e in envs:
            e.close()


# ---------------------------------------------------------------------------------------------------------------------
# closed loop against the oracle: closed_loop_check's policy argument, with the sampled twin as the reference

TEMP = 0.7


def _sampled_reference(monkeypatch, temp=TEMP):
    """Every PolicyController the runners build samples at `temp`, and closed_loop_check's PolicyReference decides with
    the sampled twin."""
    import abrsimulator_amd as A
    iT = f32(1.0 / temp)
    monkeypatch.setattr(A, "PolicyController", functools.partial(A.policy.PolicyController, sample="softmax",
                                                                 temperature=temp))
    monkeypatch.setattr(T, "decide", lambda layers, x, seed, thr, lane, c, episode, M:
                        ST.decide_sampled(layers, x, seed, thr, lane, c, episode, M, iT)[:3])


SAMPLED_CLOSED = [  # (seed, W, widths, explore, auto_reset, impl)
    (0, 8, [16, 16], 0.0, False, "auto"), (1, 0, [8], 0.25, True, "jump"), (2, 16, [], 0.0, True, "split"),
    (3, 1, [12, 7], 0.25, False, "split3"), (4, 8, [64, 64], 0.0, True, "auto"),
]


def test_closed_loop_sampled_against_the_oracle(monkeypatch):
    _sampled_reference(monkeypatch)
    answers = set()
    for (seed, W, widths, explore, auto_reset, impl) in SAMPLED_CLOSED:
        case = _policy_case(seed, W, widths, explore, auto_reset, impl)
        out = run_policy_case(case)
        stats = {}
        mm = K.check(case, out, stats)
        assert not mm, (K.describe(case), W, widths, len(mm), mm[:6])
        answers |= stats["answers"]["policy"]
    assert len(answers) >= 3


def test_closed_loop_sampled_with_the_episode_sampler(monkeypatch):
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gpu_fuzz_closed
    _sampled_reference(monkeypatch)
    for seed in (26, 53):                                                  # policy / sampled, sampled_staggered
        case = K.make_episode_case(seed)
        assert case["ctl"] == "policy" and case["sampler"] is not None
        out = gpu_fuzz_closed.run_episode_case(case)
        stats = {}
        mm = K.check_episodes(case, out, stats)
        assert not mm, (K.describe_ep(case), len(mm), mm[:6])
        assert len(stats["answers"]["policy"]) >= 2


def test_closed_loop_sampled_lanes_at_65536(monkeypatch):
    _sampled_reference(monkeypatch)
    case = _policy_case(10, 8, [64, 64], 0.25, False, "auto", n_lanes=65536)
    out = run_policy_case(case)
    pick = np.sort(np.random.default_rng(3).choice(case["n_lanes"], 256, replace=False))
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
# the draw's statistics, the temperature limit, resume and shards

def test_frequencies_on_one_replicated_state():
    """2^20 lanes in one state (same trace, offset and speed: they differ only in lane id); each action's frequency lies
    within 5 sigma of its probability, at temperatures 1 and 0.3 (seed 2024, fixed in advance)."""
    import abrsimulator_amd as A
    N, V = 1 << 20, 8
    rng = np.random.default_rng(2024)
    trace = rng.uniform(0.3, 7.0, 400).astype(np.float32).astype(np.float64)
    mpd = A.MPD(V, 4.0, 12.0, 4.0, A.Chunk(LADDER))
    env = A.BatchedABREnv(mpd, A.QOEMetric(4.3, 1.0, 1.0, 0.1), A.NetworkInfo(1.0, [trace]), N)
    env.reset(torch.zeros(N, dtype=torch.int32), torch.full((N,), 17, dtype=torch.int32))
    env.step(torch.full((N,), 2, dtype=torch.int32, device=env.device))
    layers = [(rng.normal(0, 0.3, (6, 4 + 2 + 6)).astype(np.float32), rng.normal(0, 0.5, 6).astype(np.float32))]
    ctl = A.PolicyController(A.EnvPlayer(env), layers, window=2, seed=2024, sample="softmax")
    for temp in (1.0, 0.3):
        ctl.temperature = temp
        out = ctl.select(want_probs=True)
        p = out["probs"].cpu().numpy()
        assert (p == p[:, :1]).all()                                       # one state: one distribution
        s = out["scores"][:, 0].cpu().numpy()[:, None]
        want = ST.softmax_sample(s, T.argmax_first(s), ctl.inv_temperature, np.zeros(1, np.uint64))[1][:, 0]
        assert _bits_eq(p[:, 0], want)
        p = p[:, 0].astype(np.float64)
        assert (p > 0.02).sum() >= 3, p                                    # a distribution worth testing
        freq = torch.bincount(out["actions"].long(), minlength=6).cpu().numpy() / N
        sigma = np.sqrt(p * (1 - p) / N)
        assert (np.abs(freq - p) <= 5 * sigma + 1e-12).all(), (temp, freq, p, sigma)
    env.close()


def test_high_inverse_temperature_takes_the_argmax():
    import abrsimulator_amd as A
    rng = np.random.default_rng(74)
    V, N = 16, 8192
    env = _env(A, V, N, rng)
    layers = _layers(rng, 4 + 8 + 6, [64, 64], 6)
    ctl = A.PolicyController(A.EnvPlayer(env), layers, window=8, seed=5, sample="softmax", temperature=2.0 ** -100)
    assert ctl.inv_temperature == f32(2.0 ** 100)
    checked = 0
    for _ in range(4):
        out = ctl.select(want_probs=True)
        s = out["scores"].cpu().numpy().astype(np.float64)
        top = np.sort(s, 0)
        ok = (out["actions"].cpu().numpy() >= 0) & ((top[-1] - top[-2]) * 2.0 ** 100 >= 80)
        g = T.argmax_first(out["scores"].cpu().numpy())
        assert np.array_equal(out["actions"].cpu().numpy()[ok], g[ok])
        checked += int(ok.sum())
        env.step_random(3, seed=int(rng.integers(1 << 62)), want_actions=False)
    assert checked >= N
    env.close()


def test_resume_and_shards_draw_the_same():
    import abrsimulator_amd as A
    rng = np.random.default_rng(75)
    V, N, k, n = 10, 2048, 7, 19
    layers = _layers(rng, 4 + 4 + 6, [16], 6)
    mk = lambda e: A.PolicyController(A.EnvPlayer(e), layers, window=4, explore=0.1, seed=31, sample="softmax",
                                      temperature=0.5)
    whole = _env(A, V, N, np.random.default_rng(4), auto_reset=True)
    ref = whole.step_policy(mk(whole), k + n, want_probs=True)
    # resume: k decisions, a state_dict, a fresh env continues
    a = _env(A, V, N, np.random.default_rng(4), auto_reset=True)
    a.step_policy(mk(a), k)
    sd = a.state_dict()
    b = _env(A, V, N, np.random.default_rng(4), auto_reset=True)
    b.load_state_dict(sd)
    cont = b.step_policy(mk(b), n, want_probs=True)
    for key in ("actions", "probs", "reward", "done", "obs"):
        assert torch.equal(cont[key], ref[key][k:]), key
    # two shards with lane_id_base reproduce the unsharded lanes
    tid, off = whole.trace_id.cpu(), whole.start_offset.cpu()
    h = N // 2
    for lo in (0, h):
        sh = A.BatchedABREnv(whole.mpd, whole.qoe_metric, whole.network_info, h, auto_reset=True, lane_id_base=lo)
        sh.reset(tid[lo:lo + h].clone(), off[lo:lo + h].clone())
        o = sh.step_policy(mk(sh), k + n, want_probs=True)
        for key in ("actions", "probs", "reward", "done"):
            assert torch.equal(o[key], ref[key][..., lo:lo + h]), (lo, key)
        sh.close()
    for e in (whole, a, b):
        e.close()
