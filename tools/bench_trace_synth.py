#!/usr/bin/env python3
"""What regenerating the corpus on the device costs (include/abr_env.h: abr_trace_synth), and what a synthesised corpus
does to the controllers' choices.

Timing, per corpus shape (1 024 x 1 000, the bench corpus, and 16 384 x 1 000) and K in {4, 8}, the kinds alternating,
--repeats rounds, medians reported:
  (a) synth        abr_trace_synth, R launches between two HIP events after warm-ups: the bare C call through ctypes on
                   a struct built once, so that what the host does per launch stays well below the kernel's time (the
                   Python wrapper A.synth_traces rebuilds the struct and checks its tensors at every call)
  (b) rollout      one step_random(48) launch at 65 536 lanes on the bench workload, the same way, in the same process:
                   the yardstick for whether regeneration can sit inside a training iteration
  (c) host         the path it replaces: TraceModel.draw in numpy, then torch.as_tensor(...).to(device), wall clock with
                   a device synchronisation (about two seconds per run at 16 384 traces; --no-host-large skips those)
Study: mean episode_qoe and action histogram of MPC (horizon 5), RATE and BBA-0 over one episode of 65 536 lanes on the
white-noise bench corpus and on one synthesised corpus whose model is fixed here (STUDY_MODEL), every controller from the
same reset.  Writes OUT/trace_synth_bench.json and prints it.

    python tools/bench_trace_synth.py OUT [--launches 20] [--warmup 3] [--repeats 3] [--no-study] [--no-host-large]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import abrsimulator_amd as A  # noqa: E402
from abrsimulator_amd import _lib  # noqa: E402

LADDER = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
V, L, MAX_BUFFER, START_UP, INTERVAL, WEIGHTS = 48, 4.0, 20.0, 8.0, 1.0, [4.3, 1.0, 1.0, 0.1]
LANES, FUSE, SEED = 65536, 48, 20240
SHAPES = [(1024, 1000), (16384, 1000)]
MODELS = {4: dict(levels=[0.4, 1.0, 2.0, 4.0], spread=0.3, stay=0.9, outage=0.02),
          8: dict(levels=[0.2, 0.4, 0.8, 1.2, 2.0, 3.0, 4.5, 6.0], spread=0.3, stay=0.9, outage=0.02)}
STUDY_MODEL = MODELS[4]          # fixed before the first run: four regimes across the ladder, 10-sample mean dwell, 2 % outages


def make_env(traces, n=LANES):
    mpd = A.MPD(V, L, MAX_BUFFER, START_UP, A.Chunk(LADDER))
    return A.BatchedABREnv(mpd, A.QOEMetric(*WEIGHTS), A.NetworkInfo(INTERVAL, traces), n, device="cuda", auto_reset=True)


def reset(env):
    rng = np.random.default_rng(7)
    env.reset(torch.from_numpy((np.arange(env.n_lanes) % env.n_traces).astype(np.int32)),
              torch.from_numpy(rng.integers(0, 1000, env.n_lanes).astype(np.int32)))


def timed(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(launches):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / launches          # microseconds per launch


def bare_synth(model, bufs):
    """A closure that enqueues one abr_trace_synth on the current stream; generation is its argument."""
    import ctypes as C
    L, st = _lib.lib(), model.struct()
    flat, off, lens = bufs
    args = (C.byref(st), C.c_uint64(SEED))
    tail = (0, _lib.ptr(flat), _lib.ptr(off), _lib.ptr(lens), int(lens.numel()), _lib.current_stream(flat.device))

    def launch(generation=0):
        _lib.check(L.abr_trace_synth(*args, C.c_uint32(generation), *tail), L)
    launch.keep = (st, bufs)
    return launch


def host_path(model, n, length, gen):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = model.draw(SEED, gen, np.arange(n), length)
    t1 = time.perf_counter()
    d = torch.as_tensor(x.reshape(-1)).to("cuda")
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    del d
    return (t2 - t0) * 1e6, (t1 - t0) * 1e6, (t2 - t1) * 1e6


def study(traces_white):
    rows = []
    for corpus in ("white_noise", "synthesised"):
        for name in ("mpc", "rate", "bba0"):
            env = make_env(traces_white)
            if corpus == "synthesised":
                env.synth_traces(A.TraceModel(**STUDY_MODEL), SEED, 0)
            reset(env)
            if name == "mpc":
                player = A.EnvPlayer(env, mpd=A.MPD(V, L, MAX_BUFFER, START_UP, [A.Chunk(LADDER, [b * L for b in LADDER])] * V),
                                     qoe=A.QOEMetric(4.3, 1.0, 0.0))
                out = env.step_mpc(A.BatchedMPCController(player, horizon=5, clip_horizon=True, device="cuda"), V)
            else:
                ctl = (A.RateBasedController if name == "rate" else A.BufferBasedController)(A.EnvPlayer(env))
                out = env.step_rule(ctl, V)
            acts, done = out["actions"].cpu().numpy(), out["done"].cpu().numpy()
            qoe = env.episode_qoe().cpu().numpy()
            rows.append(dict(corpus=corpus, controller=name, lanes=LANES, mean_episode_qoe=float(qoe.mean()),
                             action_histogram=np.bincount(acts[acts >= 0], minlength=len(LADDER)).tolist(),
                             lanes_timed_out=int(((done & 2) != 0).any(0).sum()),
                             mean_bandwidth=float(env.traces.mean().item()),
                             zero_samples=float((env.traces == 0).double().mean().item())))
            print(json.dumps(rows[-1]), flush=True)
            env.close()
            del env, out
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-study", action="store_true")
    ap.add_argument("--no-host-large", action="store_true", help="skip the host path at 16 384 traces")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    white = [rng.uniform(0.2, 6.0, 1000).astype(np.float32).astype(np.float64) for _ in range(1024)]
    env = make_env(white)
    reset(env)
    out = env.bind_out(env._rollout_out(FUSE, want_actions=False))
    models = {K: A.TraceModel(**kw) for K, kw in MODELS.items()}
    bufs = {(n, length): A.synth_traces(models[4], [length] * n, SEED) for n, length in SHAPES}
    synth = {(n, length, K): bare_synth(models[K], bufs[(n, length)]) for n, length in SHAPES for K in MODELS}
    runs = {}
    for r in range(a.repeats):
        runs.setdefault(("rollout", 0, 0), []).append(timed(lambda: env.step_random(FUSE, 99, out=out), a.launches, a.warmup))
        for (n, length) in SHAPES:
            for K in MODELS:
                runs.setdefault(("synth", n, K), []).append(
                    timed(lambda: synth[(n, length, K)](r), a.launches, a.warmup))
                if n <= 1024 or not a.no_host_large:
                    runs.setdefault(("host", n, K), []).append(host_path(models[K], n, length, r))
    rollout = float(np.median(runs[("rollout", 0, 0)]))
    rows = [dict(kind="rollout", lanes=LANES, fuse=FUSE, impl=env.effective_impl(fused=True), us_per_launch=rollout,
                 runs=runs[("rollout", 0, 0)])]
    for (n, length) in SHAPES:
        for K in MODELS:
            s = float(np.median(runs[("synth", n, K)]))
            row = dict(kind="synth", traces=n, samples=length, K=K, us_per_launch=s, runs=runs[("synth", n, K)],
                       samples_per_s=n * length / (s * 1e-6), write_GB_per_s=8.0 * n * length / (s * 1e-6) / 1e9,
                       synth_over_rollout=s / rollout)
            h = runs.get(("host", n, K))
            if h:
                tot = float(np.median([x[0] for x in h]))
                row.update(host_us=tot, host_numpy_us=float(np.median([x[1] for x in h])),
                           host_copy_us=float(np.median([x[2] for x in h])), host_runs=len(h), host_over_synth=tot / s)
            rows.append(row)
    res = dict(device=torch.cuda.get_device_name(0), launches=a.launches, warmup=a.warmup, repeats=a.repeats, seed=SEED,
               models={str(k): v for k, v in MODELS.items()}, rows=rows)
    env.close()
    del env, out, bufs, synth
    torch.cuda.empty_cache()
    if not a.no_study:
        res["study"] = dict(model=STUDY_MODEL, seed=SEED, generation=0, video_length=V, weights=WEIGHTS, rows=study(white))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "trace_synth_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
