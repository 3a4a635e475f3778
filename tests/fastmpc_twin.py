"""numpy twin of FastMPC's lookup (include/abr_env.h: abr_fastmpc; csrc/abr_lane_jump.h: fastmpc_lookup) and the oracle's
answer for one table entry.

The lookup is RATE's harmonic mean (float64, same operations, same order) followed by comparisons only, so the twin
reproduces the device's answers bit for bit.  entries: uint8 [rows, M, Nb, Nq]; be / te: the edges (float64)."""
import numpy as np


def row_of(c, V, H, uniform):
    """The table row chunk c reads: c (per chunk) or min(V - c, H) - 1 (uniform)."""
    return (min(V - c, H) - 1) if uniform else c


def chunk_of_row(r, V, uniform):
    """The chunk row r is built at: r (per chunk) or V - 1 - r (uniform)."""
    return V - 1 - r if uniform else r


def harmonic_tail(h, c, n):
    """RATE's arithmetic in IEEE float64 (1/0 = inf, n/0 = inf, NaN propagates)."""
    with np.errstate(all="ignore"):
        S = np.float64(0.0)
        for j in range(c - n, c):
            S = S + np.float64(1.0) / np.float64(h[j])
        return np.float64(n) / S


def cell(edges, x):
    """Number of edges <= x (NaN: 0)."""
    return int(np.count_nonzero(np.asarray(edges, np.float64) <= x))


def lookup(entries, be, te, W, V, H, uniform, c, prev, B, h):
    """One lane: chunk c, previous bitrate prev (Python's -M..-1 wrap), buffer B, history h[0..c).  -1 for a chunk or a
    previous bitrate out of range."""
    M = entries.shape[1]
    c, prev = int(c), int(prev)
    if c < 0 or c >= V or prev < -M or prev >= M:
        return -1
    n = min(int(W), c)
    if n <= 0:
        return 0
    P = harmonic_tail(h, c, n)
    if prev < 0:
        prev += M
    return int(entries[row_of(c, V, H, uniform), prev, cell(be, B), cell(te, P)])


def lookup_lanes(entries, be, te, W, V, H, uniform, chunk, prev, buf, hist):
    """Every lane of (chunk[N], prev[N], buf[N], hist[T, N])."""
    return np.array([lookup(entries, be, te, W, V, H, uniform, chunk[i], prev[i], buf[i], hist[:, i])
                     for i in range(len(chunk))], np.int32)


def entry_oracle(O, ocfg, br, sz, c, p, buf, tput, clip=True):
    """The table entry at chunk c, previous bitrate p, buffer buf, estimate tput: the first action of the oracle's
    brute-force search at H_eff (no decision: 0).  ocfg: oracle.mpc_cfg at the full horizon; br / sz [V][M]."""
    H, V, M = ocfg.horizon, ocfg.video_length, ocfg.n_rates
    he = H
    if c + H > V:
        he = (V - c) if clip else 0
    if he <= 0:
        return 0
    cfg = O.mpc_cfg(M, he, V, ocfg.chunk_length, ocfg.max_buffer, ocfg.variance_weight, ocfg.rebuffer_weight,
                    ocfg.startup_weight)
    f, _, _ = O.mpc_brute(cfg, br, sz, c, p, buf, np.full(he, float(tput)), want_J=False)
    return f // M ** (he - 1)
