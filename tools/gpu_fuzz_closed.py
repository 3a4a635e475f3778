#!/usr/bin/env python3
"""Config-space fuzz of the closed-loop rollouts on the GPU box: each seed is one case of tests/closed_loop_check.py
(random configuration x controller {harmonic MPC, RobustMPC, FastMPC, BBA-0, RATE, BOLA} x speed feature {config speed,
per-lane speeds, schedule, LatencySpeedController} x per-chunk ladder x lane count x accepted impl x auto_reset), run
through the public API (BatchedABREnv, step_mpc / step_rule, set_speed_controller, speed_log) in pieces, then checked
against the C oracle and the controller twins: every action, obs row, reward, done flag, the frame after every piece,
the history, QoE, the speed log and the FastMPC entries the decisions read.
With --episodes each seed is a case of the episode family (closed_loop_check.make_episode_case: the policy as a seventh
controller, an episode sampler, staggered lanes through masked resets, lane_id_base up to 2^40 + 2^32), run through
step_mpc / step_rule / step_policy and reset(mask=...), and checked after every operation (check_episodes).
With --traces FAMILY every case runs on traces of one family of tests/trace_families.py (outages, isolated zeros, tiny and
huge samples, traces of one to seven samples, constants) with max_ticks measured on the reference's own closed loop.
With --learned each seed is a case of the learned family (closed_loop_check.make_learned_case: an MLP or a GRU cell, on the
lane or the matrix engine, alone or as a population, arg-max or softmax, a value head, an episode ledger and a quality
model), run through step_policy -- or select(commit=True) + step for launches of one decision -- with every slab
requested, A.gae on every launch, and checked by check_learned.
    usage: python tools/gpu_fuzz_closed.py [--episodes | --learned] [--traces FAMILY] [n_seeds]
           [lanes (default: the case's own)] [first_seed]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import abrsimulator_amd as A  # noqa: E402
import closed_loop_check as K  # noqa: E402


def _controller(case, env):
    m, p, ctl = case["meta"], case["params"], case["ctl"]
    V, L = m["video_length"], m["chunk_length"]
    if ctl in ("mpc", "robust", "fastmpc"):
        br = K.br_table(case)
        mpd = A.MPD(V, L, m["max_buffer"], m["start_up_length"],
                    [A.Chunk(list(b), list(s)) for b, s in zip(br, p["sizes"])])
        player = A.EnvPlayer(env, mpd=mpd, qoe=A.QOEMetric(*p["qoe"]))
        if ctl == "mpc":
            return A.BatchedMPCController(player, horizon=p["horizon"], clip_horizon=True)
        if ctl == "robust":
            return A.BatchedMPCController(player, horizon=p["horizon"], clip_horizon=True, method="robust",
                                          window=p["window"])
        return A.FastMPCController(player, horizon=p["horizon"], window=p["window"], utility=p["utility"],
                                   clip_horizon=p["clip"], buffer_points=p["buffer_points"],
                                   tput_points=p["tput_points"], layout=p["layout"])
    player = A.EnvPlayer(env)
    if ctl == "buffer":
        return A.BufferBasedController(player, reservoir=p["reservoir"], cushion=p["cushion"])
    if ctl == "rate":
        return A.RateBasedController(player, window=p["window"], safety=p["safety"])
    return A.BolaController(player, gamma_p=p["gp"], v=p["v"])


def run_case(case):
    """Run one case on the device; returns the `out` dict closed_loop_check.check takes."""
    m = case["meta"]
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
    if case["feature"] == "rule":
        env.set_speed_controller(A.LatencySpeedController(*case["rule"]), log_rows=V + 4)
    env.reset(torch.from_numpy(case["tid"]), torch.from_numpy(case["off"]))
    ctl = _controller(case, env)
    mpc = case["ctl"] in ("mpc", "robust")
    parts, frames, t = [], [], 0
    for n in case["pieces"]:
        o = env.step_mpc(ctl, n) if mpc else env.step_rule(ctl, n)
        parts.append({k: v.cpu().numpy() for k, v in o.items()})
        t += n
        frames.append((t, {k: v.cpu().numpy().copy() for k, v in env.observe_f64().items()}))
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("actions", "reward", "done", "obs")}
    out["frames"] = frames
    out["history"] = tuple(x.cpu().numpy().copy() for x in env.history())
    out["qoe"] = env.episode_qoe().cpu().numpy()
    out["speed_log"] = env.speed_log().cpu().numpy().copy() if case["feature"] == "rule" else None
    out["entries"] = ctl.entries().cpu().numpy() if case["ctl"] == "fastmpc" else None
    torch.cuda.synchronize()
    env.close()
    return out


def _policy(case, env):
    p = case["params"]
    ctl = A.PolicyController(A.EnvPlayer(env), p["layers"], window=p["window"], norm=(p["norm"][0], p["norm"][1]),
                             explore=p["explore"], seed=p["seed"])
    assert ctl.explore_threshold == p["thr"]
    return ctl


def run_episode_case(case):
    """Run one case of the episode family on the device; returns the `out` dict closed_loop_check.check_episodes
    takes (frames, episodes() and the speed log after every operation)."""
    m = case["meta"]
    V, N = m["video_length"], case["n_lanes"]
    chunks = A.Chunk(m["ladder"]) if case["br"] is None else [A.Chunk(list(r)) for r in case["br"]]
    mpd = A.MPD(V, m["chunk_length"], m["max_buffer"], m["start_up_length"], chunks)
    speed = m["speed"]
    if case["feature"] == "lanes":
        speed = torch.from_numpy(np.asarray(case["lane_speeds"], np.float64))
    elif case["feature"] == "schedule":
        speed = torch.from_numpy(np.ascontiguousarray(np.asarray(case["schedule"], np.float64).T))
    env = A.BatchedABREnv(mpd, A.QOEMetric(*m["weights"]), A.NetworkInfo(m["interval"], case["traces"]), N,
                          speed=speed, impl=case["impl"], auto_reset=case["auto_reset"], max_ticks=case["max_ticks"],
                          lane_id_base=case["lane_id_base"])
    if case["feature"] == "rule":
        env.set_speed_controller(A.LatencySpeedController(*case["rule"]), log_rows=case["log_rows"])
    s = case["sampler"]
    if s is not None:
        env.set_episode_sampler(s["seed"], s["pool"], s["span"])
    ctl = None
    kind = "mpc" if case["ctl"] in ("mpc", "robust") else ("policy" if case["ctl"] == "policy" else "rule")
    parts, frames, episodes, logs = [], [], [], []
    for op in case["ops"]:
        if op[0] == "reset":
            mask = None if op[1] is None else torch.from_numpy(op[1].astype(np.uint8))
            if op[2] is None:
                env.reset(mask=mask, sample=True)
            else:
                env.reset(torch.from_numpy(op[2]), torch.from_numpy(op[3]), mask=mask)
            if ctl is None:
                ctl = _policy(case, env) if kind == "policy" else _controller(case, env)
        else:
            n = op[1]
            o = (env.step_mpc(ctl, n) if kind == "mpc" else env.step_policy(ctl, n) if kind == "policy"
                 else env.step_rule(ctl, n))
            parts.append({k: o[k].cpu().numpy() for k in ("actions", "reward", "done", "obs")})
        frames.append({k: v.cpu().numpy().copy() for k, v in env.observe_f64().items()})
        episodes.append({k: v.cpu().numpy().copy() for k, v in env.episodes().items()})
        logs.append(env.speed_log().cpu().numpy().copy() if case["feature"] == "rule" else None)
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("actions", "reward", "done", "obs")}
    out["frames"], out["episodes"], out["speed_logs"] = frames, episodes, logs if case["feature"] == "rule" else None
    out["history"] = tuple(x.cpu().numpy().copy() for x in env.history())
    out["qoe"] = env.episode_qoe().cpu().numpy()
    out["entries"] = ctl.entries().cpu().numpy() if case["ctl"] == "fastmpc" else None
    torch.cuda.synchronize()
    env.close()
    return out


def _learned_controller(case, env):
    p = case["params"]
    net = case["net"]
    kw = dict(window=p["window"], norm=(p["norm"][0], p["norm"][1]), explore=p["explore"], seed=p["seed"],
              sample=p["sample"], temperature=p["temperature"], engine="matrix" if net.endswith("_mx") else "lane")
    mbs, player = p["members"], A.EnvPlayer(env)
    heads = [m["head"] for m in mbs] if p["value"] else None
    if net in ("mlp", "mlp_mx"):
        ctl = A.PolicyController(player, mbs[0]["layers"], value_head=heads[0] if heads else None, **kw)
    elif net in ("gru", "gru_mx"):
        ctl = A.RecurrentPolicyController(player, mbs[0]["parts"][:4], mbs[0]["parts"][4:],
                                          value_head=heads[0] if heads else None, **kw)
    elif net in ("pop", "pop_mx"):
        ctl = A.PolicyPopulation(player, [m["layers"] for m in mbs], p["group"], value_heads=heads, **kw)
    else:
        ctl = A.RecurrentPolicyPopulation(player, [(m["parts"][:4], m["parts"][4:]) for m in mbs], p["group"],
                                          value_heads=heads, **kw)
    assert ctl.explore_threshold == p["thr"] and float(ctl.inv_temperature) == float(np.float32(1.0 / p["temperature"]))
    return ctl


def run_learned_case(case):
    """Run one case of the learned family on the device; returns the `out` dict closed_loop_check.check_learned takes."""
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
                          speed=speed, impl=case["impl"], auto_reset=case["auto_reset"], max_ticks=case["max_ticks"],
                          lane_id_base=case["lane_id_base"])
    if case["feature"] == "rule":
        env.set_speed_controller(A.LatencySpeedController(*case["rule"]), log_rows=case["log_rows"])
    s = case["sampler"]
    if s is not None:
        env.set_episode_sampler(s["seed"], s["pool"], s["span"])
    led = env.set_episode_ledger(case["ledger"]["rows"]) if case["ledger"] else None
    ql = None
    if case["quality"]:
        q = case["quality"]
        ql = env.set_quality(q["weight"], q["utility"])                  # rows: the ledger's, else 1 (the default)
        assert ql.rows == q["rows"]
    gru = case["net"].startswith("gru")
    ctl = None
    np_ = lambda t: t.cpu().numpy().copy()
    parts, launches, frames, episodes, logs, hidden_after = [], [], [], [], [], []
    for op in case["ops"]:
        if op[0] == "reset":
            mask = None if op[1] is None else torch.from_numpy(op[1].astype(np.uint8))
            if op[2] is None:
                env.reset(mask=mask, sample=True)
            else:
                env.reset(torch.from_numpy(op[2]), torch.from_numpy(op[3]), mask=mask)
            if ctl is None:
                ctl = _learned_controller(case, env)
        else:
            n = op[1]
            if case["single"] and n == 1:                                 # the select + step pair of entries
                kw = dict(want_hidden=True, commit=True) if gru else {}
                o = ctl.select(True, True, True, p["value"], **kw)
                obs, rew, done = env.step(o["actions"])
                L = {k: np_(o[k])[None] for k in ("features", "scores", "probs")}
                L["values"] = np_(o["value"])[None] if p["value"] else None
                L["hidden"] = np_(o["hidden"])[None] if gru else None
                dev = dict(actions=o["actions"][None], reward=rew[None].clone(), done=done[None].clone(),
                           values=o["value"][None] if p["value"] else None)
                if p["value"]:                          # V of the frame the step left: a select that commits nothing
                    kw = dict(commit=False) if gru else {}
                    dev["last_value"] = ctl.select(False, False, False, True, **kw)["value"]
                parts.append(dict(actions=np_(o["actions"])[None], reward=np_(rew)[None], done=np_(done)[None],
                                  obs=np_(obs)[None]))
            else:
                dev = env.step_policy(ctl, n, want_features=True, want_scores=True, want_probs=True,
                                      want_values=p["value"], want_hidden=gru)
                L = {k: np_(dev[k]) for k in ("features", "scores", "probs")}
                L["values"] = np_(dev["values"]) if p["value"] else None
                L["hidden"] = np_(dev["hidden"]) if gru else None
                parts.append({k: np_(dev[k]) for k in ("actions", "reward", "done", "obs")})
            L["last_value"] = None
            if p["value"]:
                L["last_value"] = np_(dev["last_value"])
                adv, ret = A.gae(dev["reward"].contiguous(), dev["values"].contiguous(), dev["last_value"],
                                 dev["done"].contiguous(), dev["actions"].contiguous(), gamma=0.99, lam=0.95)
                L["adv"], L["ret"] = np_(adv), np_(ret)
            launches.append(L)
        frames.append({k: np_(v) for k, v in env.observe_f64().items()})
        episodes.append({k: np_(v) for k, v in env.episodes().items()})
        logs.append(np_(env.speed_log()) if case["feature"] == "rule" else None)
        hidden_after.append(np_(ctl.hidden) if gru else None)
    out = {k: np.concatenate([x[k] for x in parts]) for k in ("actions", "reward", "done", "obs")}
    out["frames"], out["episodes"], out["speed_logs"] = frames, episodes, logs if case["feature"] == "rule" else None
    out["history"] = tuple(np_(x) for x in env.history())
    out["qoe"] = env.episode_qoe().cpu().numpy()
    out["entries"] = None
    out["launches"], out["hidden_after"] = launches, hidden_after if gru else []
    P, g = len(p["members"]), p["group"]
    dn = lambda d: {k: np_(v) for k, v in d.items()}
    out["ledger"] = out["quality"] = None
    if led is not None:
        ring = led.ring()
        out["ledger"] = dict(count=np_(led.count()), total=np.stack([np_(led.totals()[k]) for k in K.LEDGER_FLOATS]),
                             rf=np.stack([np_(ring[k]) for k in K.LEDGER_FLOATS], axis=1),
                             ri=np.stack([np_(ring[k]) for k in K.LEDGER_INTS], axis=1), records=dn(led.records()),
                             per_trace=dn(led.per_trace(len(case["traces"]))),
                             per_member=dn(led.per_member(g, P)) if P > 1 else None)
    if ql is not None:
        out["quality"] = dict(count=np_(ql.count()), rec=np_(ql.ring()), total=np_(ql.totals()), last=np_(ql.last()),
                              records=dn(ql.records(led)))
    torch.cuda.synchronize()
    env.close()
    return out


def run_learned_seed(seed, N=None, stats=None, traces=None):
    """One case of the learned family against the reference.  Returns (mismatches, lane-steps, cell key, case)."""
    case = K.make_learned_case(seed, N)
    mm = K.check_learned(case, run_learned_case(case), stats)
    return mm, case["n_lanes"] * case["n_steps"], f"{case['net']}/{case['feature']}/{case['mode']}", case


def _swap(case, traces, seed):
    if traces is None:
        return case
    import trace_families
    return trace_families.with_traces(case, traces, seed)       # the reference side, before anything is launched


def run_episode_seed(seed, N=None, stats=None, traces=None):
    """One case of the episode family against the reference (traces: a family of tests/trace_families.py, or the
    case's own).  Returns (mismatches, lane-steps, cell key, case)."""
    case = _swap(K.make_episode_case(seed, N), traces, seed)
    mm = K.check_episodes(case, run_episode_case(case), stats)
    return mm, case["n_lanes"] * case["n_steps"], f"{case['ctl']}/{case['feature']}/{case['mode']}", case


def run_seed(seed, N=None, stats=None, traces=None):
    """One case against the reference (traces: as run_episode_seed).  Returns (mismatches, lane-steps, cell key, case)."""
    case = _swap(K.make_case(seed, N), traces, seed)
    mm = K.check(case, run_case(case), stats)
    return mm, case["n_lanes"] * case["n_steps"], f"{case['ctl']}/{case['feature']}", case


def main():
    argv = [a for a in sys.argv[1:] if a not in ("--episodes", "--learned")]
    episodes, learned = "--episodes" in sys.argv[1:], "--learned" in sys.argv[1:]
    traces = None
    if "--traces" in argv:
        i = argv.index("--traces")
        traces = argv[i + 1]
        del argv[i:i + 2]
    n_seeds = int(argv[0]) if len(argv) > 0 else 240
    N = int(argv[1]) if len(argv) > 1 and int(argv[1]) > 0 else None
    first = int(argv[2]) if len(argv) > 2 else 0
    t0 = time.time()
    bad, lane_steps, cells, impls, stats, cases = 0, 0, {}, {}, {}, []
    for seed in range(first, first + n_seeds):
        run = run_learned_seed if learned else run_episode_seed if episodes else run_seed
        mm, ls, key, case = run(seed, N, stats, traces)
        if mm:
            describe = K.describe_learned if learned else K.describe_ep if episodes else K.describe
            print("MISMATCH", describe(case), len(mm), mm[:4], flush=True)
        bad += len(mm)
        lane_steps += ls
        cells[key] = cells.get(key, 0) + 1
        impls[case["impl"]] = impls.get(case["impl"], 0) + 1
        cases.append(case)
    vac = (K.assert_non_vacuous_learned if learned else K.assert_non_vacuous_ep if episodes else
           K.assert_non_vacuous)(stats, cases)
    print(json.dumps(dict(family="learned" if learned else "episodes" if episodes else "configs",
                          traces=traces or "case", seeds=n_seeds,
                          first_seed=first,
                          lanes_per_seed=N or "case", lane_steps=lane_steps,
                          mismatches=bad, non_vacuity_problems=vac, cases=cells, impls=impls,
                          clipped_mpc_decisions=stats.get("clipped", 0), seconds=round(time.time() - t0, 1))))
    sys.exit(1 if bad or vac else 0)


if __name__ == "__main__":
    main()
