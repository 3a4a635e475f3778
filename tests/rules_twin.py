"""numpy twin of the bitrate rules (include/abr_env.h: abr_rule_config; csrc/abr_lane_jump.h: rule_select), float64 in
the contract's operation order, so that it reproduces the device's answers bit for bit.  Sums are sequential loops (never
np.sum, which is pairwise beyond 8 terms).

Scalar form: rule_scalar(p, c, B, h, br, u_row) for one call site (the oracle's policy callback).  Vectorised form:
rule_vec(p, c[N], B[N], hist[V, N], br_rows[N, M], u_rows[N, M]) over lanes.  `p` is a dict: kind (1 BUFFER, 2 RATE,
3 BOLA), window, reservoir, cushion, safety, v, gp."""
import numpy as np

BUFFER, RATE, BOLA = 1, 2, 3


def _hi(br, X):
    a = 0
    for m in range(1, len(br)):
        if br[m] <= X:
            a = m
    return a


def rule_scalar(p, c, B, h, br, u_row=None):
    """c = chunk_id, B = buffer_level, h = previous_bandwidths (oldest first, len >= c), br = chunk c's bitrates,
    u_row = chunk c's utilities (BOLA)."""
    br = [float(x) for x in br]
    M, B, c = len(br), float(B), int(c)
    if p["kind"] == BUFFER:
        r, k = float(p["reservoir"]), float(p["cushion"])
        if B <= r:
            return 0
        if B >= r + k:
            return M - 1
        return _hi(br, br[0] + ((B - r) / k) * (br[M - 1] - br[0]))
    if p["kind"] == RATE:
        n = min(int(p["window"]), c)
        if n == 0:
            return 0
        S = 0.0
        for j in range(c - n, c):
            S = S + 1.0 / float(h[j])
        return _hi(br, float(p["safety"]) * (float(n) / S))
    V, gp = float(p["v"]), float(p["gp"])
    best, a = (V * (float(u_row[0]) + gp) - B) / br[0], 0
    for m in range(1, M):
        sc = (V * (float(u_row[m]) + gp) - B) / br[m]
        if sc > best:
            best, a = sc, m
    return a


def _hi_vec(br, X):
    a = np.zeros(len(X), np.int32)
    for m in range(1, br.shape[1]):
        a = np.where(br[:, m] <= X, m, a).astype(np.int32)
    return a


def rule_vec(p, c, B, hist, br_rows, u_rows=None):
    """c int [N], B f64 [N], hist f64 [V, N] (row j = previous_bandwidths[j]), br_rows f64 [N, M] = each lane's chunk-c
    bitrates, u_rows f64 [N, M] (BOLA).  Returns int32 [N]."""
    c = np.asarray(c, np.int64)
    B = np.asarray(B, np.float64)
    br = np.asarray(br_rows, np.float64)
    N, M = br.shape
    if p["kind"] == BUFFER:
        r, k = float(p["reservoir"]), float(p["cushion"])
        X = br[:, 0] + ((B - r) / k) * (br[:, M - 1] - br[:, 0])
        a = _hi_vec(br, X)
        a = np.where(B >= r + k, M - 1, a)
        return np.where(B <= r, 0, a).astype(np.int32)
    if p["kind"] == RATE:
        W = int(p["window"])
        n = np.minimum(W, c)
        S = np.zeros(N)
        lanes = np.arange(N)
        for t in range(W):
            j = c - n + t
            ok = t < n
            x = hist[np.where(ok, j, 0), lanes]
            with np.errstate(divide="ignore"):
                S = np.where(ok, S + 1.0 / np.where(ok, x, 1.0), S)
        with np.errstate(divide="ignore", invalid="ignore"):
            X = float(p["safety"]) * (n.astype(np.float64) / S)
        return np.where(n == 0, 0, _hi_vec(br, X)).astype(np.int32)
    V, gp = float(p["v"]), float(p["gp"])
    u = np.asarray(u_rows, np.float64)
    best = (V * (u[:, 0] + gp) - B) / br[:, 0]
    a = np.zeros(N, np.int32)
    for m in range(1, M):
        sc = (V * (u[:, m] + gp) - B) / br[:, m]
        a = np.where(sc > best, m, a).astype(np.int32)
        best = np.where(sc > best, sc, best)
    return a


def params_of(ctl):
    """The twin's parameter dict of a controller (abrsimulator_amd.rules)."""
    c = ctl.config()
    return dict(kind=c.kind, window=c.window, reservoir=c.reservoir, cushion=c.cushion, safety=c.safety,
                v=c.bola_v, gp=c.bola_gp)
