"""The step start of a lane that knows its call site's trace interval (csrc/abr_lane_jump.h: lanej_begin_step_at) on the
DEVICE, where a wave mixes lanes that know it with lanes that search.

200 lanes (three full waves and a partial one), a video of 8 chunks, three launches of 11 fused decisions under auto_reset:
the launches cross four episode ends and put their boundaries inside episodes, so every launch starts with a search and
every re-arm takes the availability table from a fresh cursor.  Four configurations of tests/test_step_start_cpu.py --
bench-like, interval 0.3 s on a starved network, a max_buffer that gates often, traces of one to three samples -- on the
three-wave, two-wave and one-thread kernels, the random policy's launches (MODE 2) and scripted ones (MODE 3) in turn,
against the oracle's replay with `==`: observations, rewards, done bytes, and the workspace read back after every launch.
One case hands the workspace from the three-wave kernel to the one-thread kernel and on to the two-wave kernel between
launches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, V, FUSE, LAUNCHES = 200, 8, 11, 3
IMPLS = ("split3", "split", "jump")
IMPL_CODE = {"jump": 0, "split": 2, "split3": 5}
LADDER = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
CONFIGS = {
    "bench_like": dict(interval=1.0, L=4.0, max_buffer=20.0, start_up=8.0, bw=(0.2, 6.0), tlens=(1000, 1000, 1000, 1000),
                       launch="random"),
    "starved_i03": dict(interval=0.3, L=4.0, max_buffer=20.0, start_up=4.0, bw=(0.1, 1.5), tlens=(300, 157, 1000, 40),
                        launch="script"),
    "gated_i05": dict(interval=0.5, L=2.0, max_buffer=3.0, start_up=4.0, bw=(2.0, 12.0), tlens=(300, 157, 1000, 40),
                      launch="random"),
    "short_traces": dict(interval=0.3, L=4.0, max_buffer=20.0, start_up=4.0, bw=(0.3, 6.0), tlens=(1, 2, 3, 2),
                         launch="script"),
}
_cases = {}


def _case(name):
    """closed_loop_check's open-loop case layout (as trace_families.open_loop_case builds it); the oracle's replays are
    computed once per configuration, before any launch, and shared by the implementations."""
    if name in _cases:
        return _cases[name]
    import closed_loop_check as K
    import trace_families as TF
    from oracle import oracle as O
    c = CONFIGS[name]
    rng = np.random.default_rng([41, sorted(CONFIGS).index(name)])
    traces = [rng.uniform(c["bw"][0], c["bw"][1], n).astype(np.float32).astype(np.float64) for n in c["tlens"]]
    tl = np.array([len(t) for t in traces])
    tid = rng.integers(0, len(traces), N).astype(np.int32)
    off = (rng.integers(0, 1 << 20, N) % tl[tid]).astype(np.int32)
    meta = dict(ladder=LADDER, chunk_length=c["L"], video_length=V, max_buffer=c["max_buffer"], start_up_length=c["start_up"],
                interval=c["interval"], weights=[4.3, 1.0, 1.0, 0.1], speed=1.0)
    T = FUSE * LAUNCHES
    n_ep = -(-T // V)
    philox = 20240 + len(name)
    if c["launch"] == "random":
        script = np.stack([O.philox_action(philox, np.arange(N), t % V, t // V, len(LADDER)) for t in range(n_ep * V)])
    else:
        script = rng.integers(0, len(LADDER), (n_ep * V, N)).astype(np.int32)
    case = dict(seed=0, ctl="script", feature="config", impl=None, vbr=False, auto_reset=True, n_lanes=N, meta=meta,
                traces=traces, tid=tid, off=off, br=None, params={}, n_steps=T, script=script, launch=c["launch"],
                philox=philox, trace_family="step_start", pieces=[FUSE] * LAUNCHES)
    case["replays"] = []
    for e in range(n_ep):
        a = np.ascontiguousarray(script[e * V:(e + 1) * V].T)
        steps, bw, fin, _ = O.env_batch(K.env_cfg(case), traces, tid, off, a, max_ticks=TF.TICK_ORACLE_BOUND)
        case["replays"].append((steps, bw, fin, a))
    case["max_ticks"] = max(int(r[2]["ticks"].max()) for r in case["replays"]) + 1000
    assert case["max_ticks"] <= 1 << 20                     # the no-speeds instances: the headline's
    _cases[name] = case
    return case


def _run(case, impls):
    """test_trace_edges_gpu.run_open_case with an implementation per launch: the same handle and workspace throughout."""
    import abrsimulator_amd as A
    m = case["meta"]
    T = case["n_steps"]
    env = A.BatchedABREnv(A.MPD(V, m["chunk_length"], m["max_buffer"], m["start_up_length"], A.Chunk(m["ladder"])),
                          A.QOEMetric(*m["weights"]), A.NetworkInfo(m["interval"], case["traces"]), N, speed=1.0,
                          impl=impls[0], auto_reset=True, max_ticks=case["max_ticks"])
    assert env.general_instance(fused=True) is False
    env.reset(torch.from_numpy(case["tid"]), torch.from_numpy(case["off"]))
    rows = np.stack([case["script"][t] for t in range(T)]).astype(np.int32)
    dev = torch.from_numpy(rows).cuda()
    parts, frames, t = [], [], 0
    for n, impl in zip(case["pieces"], impls):
        env._check(env.lib.abr_env_set_impl(env._h, IMPL_CODE[impl]))
        assert env.effective_impl(fused=True) == impl
        if case["launch"] == "script":
            o = env.step_script(dev[t:t + n])
        else:
            o = env.step_random(n, case["philox"])
        p = {k: o[k].cpu().numpy().copy() for k in ("obs", "reward", "done")}
        p["actions"] = o["actions"].cpu().numpy().copy() if case["launch"] == "random" else rows[t:t + n]
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


def _check(case, out, what):
    import closed_loop_check as K
    from test_trace_edges_gpu import frame_extras
    assert ((out["done"] & K.DONE_TIMEOUT) == 0).all()
    assert np.array_equal(out["actions"], case["script"][:case["n_steps"]])
    with np.errstate(over="ignore"):
        mm = K.check(case, out) + frame_extras(case, out["frames"])
    assert not mm, (what, len(mm), mm[:6])


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_three_launches_of_eleven_decisions(name, impl):
    case = _case(name)
    _check(case, _run(case, [impl] * LAUNCHES), (name, impl))


def test_the_workspace_goes_from_one_kernel_to_the_next():
    """The call site's interval is not stored: whichever kernel takes the workspace over searches at its first decision."""
    case = _case("gated_i05")
    _check(case, _run(case, ["split3", "jump", "split"]), "handover")
