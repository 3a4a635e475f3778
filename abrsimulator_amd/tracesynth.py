"""Bandwidth corpora synthesised on the device (include/abr_env.h: abr_trace_synth; csrc/abr_env.hip: trace_synth_kernel).

A TraceModel is a Markov chain over K <= 8 bandwidth regimes: each regime has a level, a relative half-width of uniform
noise around it and an outage probability; a transition matrix moves the chain once per sample.  The corpus is a pure
function of (model, seed, generation, global trace id, sample index), so a trainer regenerates it in place between two
launches -- no host loop, no copy, no synchronisation:

    model = TraceModel([0.4, 1.2, 2.5, 5.0], spread=0.3, stay=0.9, outage=0.02)
    for it in range(iterations):
        env.synth_traces(model, seed, generation=it)
        env.reset(sample=True)
        out = env.step_policy(ctl, 48)

Probabilities become integer thresholds on 32-bit philox words (TraceModel.thresholds): the integers are the contract, and
TraceModel.draw computes the same samples in numpy, bit for bit.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .episodes import _philox4

MAX_STATES = _lib.TRACE_MAX_STATES
ONE = 1 << 32                       # probability 1 as a threshold
TRACE_KEY = 0x5452414345535953      # xor-ed into the seed
INIT_STEP = 0xFFFFFFFF              # the philox step word of the initial-state block: never a sample index


def threshold(p):
    """The threshold of a (cumulative) probability: min(2^32, int(round(p * 2^32)))."""
    return min(ONE, int(round(float(p) * ONE)))


def _per_state(x, K, name):
    a = np.asarray(x, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(K, float(a))
    if a.shape != (K,):
        raise ValueError(f"{name} must be a scalar or one value per state ({K}), got shape {a.shape}")
    return a


def _stochastic(p, name):
    """A probability row: finite, >= 0, sums to 1 (to rounding)."""
    if not np.isfinite(p).all() or (p < 0).any():
        raise ValueError(f"{name} must hold finite probabilities >= 0")
    if abs(float(p.sum()) - 1.0) > 1e-9:
        raise ValueError(f"{name} must sum to 1, sums to {float(p.sum())!r}")


def _cumulative(p):
    """Thresholds of the float64 cumulative sums of a probability row; the last one is 2^32 by definition."""
    c = [threshold(x) for x in np.cumsum(np.asarray(p, dtype=np.float64))]
    c[-1] = ONE
    return c


class TraceModel:
    """levels: the K regimes' bandwidths (same unit as the ladder), finite and >= 0; spread, outage: a scalar or one value
    per state, in [0, 1]; transition: a K x K row-stochastic matrix, default: `stay` on the diagonal and the rest of each
    row uniform; initial: the distribution of the state before sample 0, default uniform.  At least one state must have a
    positive level and an outage probability that does not round to 1.  ValueError on anything abr_trace_synth would
    refuse, before any device call."""

    def __init__(self, levels, spread=0.25, transition=None, stay=0.9, outage=0.0, initial=None):
        lv = np.asarray(levels, dtype=np.float64).reshape(-1)
        K = int(lv.size)
        if not 1 <= K <= MAX_STATES:
            raise ValueError(f"a trace model has 1..{MAX_STATES} states, got {K}")
        sp, out = _per_state(spread, K, "spread"), _per_state(outage, K, "outage")
        if not ((out >= 0.0) & (out <= 1.0)).all():
            raise ValueError("outage must be a probability in [0, 1]")
        if transition is None:
            if not 0.0 <= float(stay) <= 1.0:
                raise ValueError("stay must be a probability in [0, 1]")
            if K == 1:
                P = np.ones((1, 1))
            else:
                P = np.full((K, K), (1.0 - float(stay)) / (K - 1))
                np.fill_diagonal(P, float(stay))
        else:
            P = np.asarray(transition, dtype=np.float64)
            if P.shape != (K, K):
                raise ValueError(f"transition must be a {K} x {K} matrix, got shape {P.shape}")
        for s in range(K):
            _stochastic(P[s], f"transition[{s}]")
        p0 = np.full(K, 1.0 / K) if initial is None else np.asarray(initial, dtype=np.float64).reshape(-1)
        if p0.shape != (K,):
            raise ValueError(f"initial must hold {K} probabilities")
        _stochastic(p0, "initial")
        self._set(lv, sp, [threshold(x) for x in out], _cumulative(p0), [_cumulative(P[s]) for s in range(K)])

    @classmethod
    def from_thresholds(cls, levels, spread, outage_thr, init_cum, cum):
        """A model given by the contract's integers themselves (include/abr_env.h: abr_trace_model): K entries per row,
        checked as the C entry checks them.  Of a cumulative row (init_cum, cum[s]) only the first K - 1 entries are read
        and checked; the last one is 2^32 whatever is passed, and is stored as 2^32."""
        self = cls.__new__(cls)
        lv = np.asarray(levels, dtype=np.float64).reshape(-1)
        if not 1 <= lv.size <= MAX_STATES:
            raise ValueError(f"a trace model has 1..{MAX_STATES} states, got {lv.size}")
        K = int(lv.size)
        cum = [list(r) for r in cum]
        if len(outage_thr) != K or len(init_cum) != K or len(cum) != K or any(len(r) != K for r in cum):
            raise ValueError(f"outage_thr, init_cum and the rows of cum must hold {K} entries each")
        init_cum = list(init_cum)
        for r in [init_cum] + cum:
            r[-1] = ONE
        self._set(lv, _per_state(spread, K, "spread"), list(outage_thr), init_cum, cum)
        return self

    def _set(self, lv, sp, outage_thr, init_cum, cum):
        K = int(lv.size)
        if not np.isfinite(lv).all() or (lv < 0).any():
            raise ValueError("levels must be finite and >= 0")
        if not ((sp >= 0.0) & (sp <= 1.0)).all():                      # a NaN fails both comparisons
            raise ValueError("spread must be in [0, 1]")
        rows = [outage_thr, init_cum] + cum
        if any(int(v) != v or not 0 <= int(v) <= ONE for r in rows for v in r):
            raise ValueError("thresholds must be integers in [0, 2^32]")
        if any(r[j] < r[j - 1] for r in [init_cum] + cum for j in range(1, K)):
            raise ValueError("a cumulative row must not decrease")
        if not any(lv[s] > 0 and int(outage_thr[s]) < ONE for s in range(K)):
            raise ValueError("a trace model needs a state with level > 0 and an outage probability below 1")
        self.n_states = K
        self.levels, self.spread = lv.copy(), sp.copy()
        self.thresholds = dict(outage=np.array(outage_thr, dtype=np.uint64), initial=np.array(init_cum, dtype=np.uint64),
                               transition=np.array(cum, dtype=np.uint64).reshape(K, K))

    def struct(self):
        """The ctypes mirror of abr_trace_model."""
        st, K, th = _lib.TraceModel(), self.n_states, self.thresholds
        st.n_states, st.reserved_ = K, 0
        for s in range(K):
            st.level[s], st.spread[s] = float(self.levels[s]), float(self.spread[s])
            st.outage_thr[s], st.init_cum[s] = int(th["outage"][s]), int(th["initial"][s])
            for j in range(K):
                st.cum[s][j] = int(th["transition"][s, j])
        return st

    def draw(self, seed, generation, trace_ids, length):
        """The samples abr_trace_synth writes, float64 [len(trace_ids), length]: trace_ids are GLOBAL ids (trace_id_base +
        row), every row `length` samples long (a shorter trace of the corpus is a prefix of its row)."""
        g = np.asarray(trace_ids, dtype=np.uint64).reshape(-1)
        n, length, K, th = g.size, int(length), self.n_states, self.thresholds
        key = (int(seed) ^ TRACE_KEY) & (2 ** 64 - 1)
        gen = int(generation) & 0xFFFFFFFF
        steps = np.arange(length, dtype=np.uint64)
        w0, w1, w2, _ = _philox4(key, np.repeat(g, length), np.tile(steps, n), np.full(n * length, gen, dtype=np.uint64))
        w0, w1, w2 = (w.reshape(n, length) for w in (w0, w1, w2))
        v0 = _philox4(key, g, INIT_STEP, np.full(n, gen, dtype=np.uint64))[0]
        s = (v0[:, None] >= th["initial"][None, :K - 1]).sum(1)
        cum, state = th["transition"][:, :K - 1], np.empty((n, length), dtype=np.int64)
        for i in range(length):
            s = (w0[:, i, None] >= cum[s]).sum(1)
            state[:, i] = s
        u = (w1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = 2.0 * u - 1.0
        x = self.levels[state] * (1.0 + self.spread[state] * r)
        return np.where(w2 < th["outage"][state], 0.0, x)


def _launch(model, seed, generation, trace_id_base, flat, off, lens):
    if not isinstance(model, TraceModel):
        raise TypeError("synth_traces takes a TraceModel")
    if int(trace_id_base) < 0:
        raise ValueError("trace_id_base must be >= 0")
    L, st = _lib.lib(), model.struct()
    _lib.check(L.abr_trace_synth(C.byref(st), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint32(int(generation) & 0xFFFFFFFF),
                                 int(trace_id_base), _lib.ptr(flat), _lib.ptr(off), _lib.ptr(lens), int(lens.numel()),
                                 _lib.current_stream(flat.device)), L)


def synth_traces(model, lengths, seed, generation=0, trace_id_base=0, device="cuda", out=None):
    """A corpus of len(lengths) traces, trace t (global id trace_id_base + t) of lengths[t] samples, generated on the
    device: (flat float64, offsets int64, lengths int32), the layout of env.pack_traces.  out: such a triple of device
    tensors to fill in place instead (lengths is then ignored and nothing is allocated): row t is out[0][out[1][t] :
    + out[2][t]]; the rows need not be adjacent, a row of length < 1 is skipped, and nothing outside the rows is written.
    The caller guarantees that every row lies inside out[0], as the C contract has it: offsets and lengths live on the
    device and are not read back, so a wrong pair is an out-of-bounds device write that nothing here can catch.
    Runs on the current stream of the device without synchronising."""
    if out is not None:
        flat, off, lens = out
        for t, dt, name in ((flat, torch.float64, "out[0]"), (off, torch.int64, "out[1]"), (lens, torch.int32, "out[2]")):
            if not torch.is_tensor(t) or t.dtype != dt or t.device.type != "cuda" or not t.is_contiguous() or t.dim() != 1:
                raise ValueError(f"{name} must be a contiguous 1-D {dt} device tensor")
        if off.numel() != lens.numel() or lens.numel() < 1 or flat.device != off.device or flat.device != lens.device:
            raise ValueError("out must be (flat, offsets, lengths) on one device with one offset per length")
    else:
        ln = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if ln.size < 1 or (ln < 1).any() or int(ln.max()) > np.iinfo(np.int32).max:
            raise ValueError("lengths must hold at least one trace and every trace at least one sample")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("synth_traces runs on the device")
        o = np.zeros(ln.size, dtype=np.int64)
        o[1:] = np.cumsum(ln[:-1])
        with torch.cuda.device(dev):
            flat = torch.empty(int(ln.sum()), dtype=torch.float64, device=dev)
            off, lens = torch.from_numpy(o).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev)
    with torch.cuda.device(flat.device):
        _launch(model, seed, generation, trace_id_base, flat, off, lens)
    return flat, off, lens
