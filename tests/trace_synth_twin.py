"""numpy twin of the trace generator (include/abr_env.h: abr_trace_synth), written from the contract and independent of the
package's mirror (abrsimulator_amd/tracesynth.py: TraceModel.draw): one sequential chain per trace, plain Python integers
for the states, numpy float64 for the samples (one rounding per operation).

A model here is a dict of the contract's fields: K, level [K], spread [K], outage_thr [K], init_cum [K], cum [K][K]
(Python / numpy integers 0..2^32; only [0, K - 1) of a cumulative row is read)."""
import numpy as np

from policy_twin import philox4

TRACE_KEY = 0x5452414345535953
INIT_STEP = 0xFFFFFFFF
IDENTITY = sum(s << (3 * s) for s in range(8))


def model_dict(levels, spread, outage_thr, init_cum, cum):
    K = len(levels)
    sp = [float(spread)] * K if np.ndim(spread) == 0 else [float(x) for x in spread]
    return dict(K=K, level=[float(x) for x in levels], spread=sp, outage_thr=[int(x) for x in outage_thr],
                init_cum=[int(x) for x in init_cum], cum=[[int(x) for x in r] for r in cum])


def from_package(model):
    """The twin's dict of an abrsimulator_amd.TraceModel: its integers are the contract."""
    th = model.thresholds
    return model_dict(model.levels, model.spread, th["outage"], th["initial"], th["transition"])


def pick(row, K, w0):
    return sum(1 for j in range(K - 1) if w0 >= row[j])


def trace(m, seed, generation, g, length):
    """Trace g (a global id), `length` samples: (float64 [length], states [length])."""
    key = (int(seed) ^ TRACE_KEY) & (2 ** 64 - 1)
    gen = int(generation) & 0xFFFFFFFF
    K = m["K"]
    lane = np.full(length, int(g), np.uint64)
    w0, w1, w2, _ = philox4(key, lane, np.arange(length, dtype=np.uint64), gen)
    v0 = int(philox4(key, np.array([int(g)], np.uint64), INIT_STEP, gen)[0][0])
    s = pick(m["init_cum"], K, v0)
    states = np.empty(length, np.int64)
    for i in range(length):
        s = pick(m["cum"][s], K, int(w0[i]))
        states[i] = s
    level, spread = np.asarray(m["level"], np.float64)[states], np.asarray(m["spread"], np.float64)[states]
    thr = np.asarray(m["outage_thr"], np.uint64)[states]
    u = (w1 >> np.uint64(8)).astype(np.float64) * np.float64(2.0 ** -24)
    r = np.float64(2.0) * u - np.float64(1.0)
    t = spread * r
    x = level * (np.float64(1.0) + t)
    return np.where(w2 < thr, np.float64(0.0), x), states


def corpus(m, seed, generation, lengths, trace_id_base=0):
    """The rows of a corpus, a list of float64 arrays: trace t has global id trace_id_base + t; a length < 1 gives an empty
    row (the device skips it)."""
    return [trace(m, seed, generation, trace_id_base + t, int(n))[0] if n >= 1 else np.empty(0, np.float64)
            for t, n in enumerate(lengths)]


# The small environment of tests/test_trace_synth_gpu.py (the one of tests/test_episode_sampler_gpu.py) and the model its
# corpus is regenerated from; tests/test_trace_synth_cpu.py checks once, on the oracle alone, that no episode of it can
# run into the tick bound.
ENV_LADDER = [0.3, 0.75, 1.2, 1.85, 2.85, 4.3]
ENV_V, ENV_L, ENV_MB, ENV_SU, ENV_W = 8, 4.0, 20.0, 4.0, [4.3, 1.0, 1.0, 0.1]
ENV_N = 200
ENV_LENGTHS = [int(x) for x in np.random.default_rng(0).integers(20, 300, 7)]
ENV_MODEL = dict(levels=[0.3, 1.2, 2.85, 6.0], spread=0.3, stay=0.8, outage=0.05)
ENV_SEED = 0x7ACE5EED
ENV_MAX_TICKS = 32 * ENV_V * 400          # the library's default bound for V = 8, L = 4 s
