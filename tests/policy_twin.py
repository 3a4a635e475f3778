"""numpy twin of the learned policy (include/abr_env.h: abr_policy; csrc/abr_lane_jump.h: policy_features,
policy_forward, policy_explore).

fmaf is emulated exactly: for float32 a, b, c the product p = a*b is exact in float64; TwoSum gives s = fl(p + c) and its
error e exactly; rounding s to odd (one ulp toward e when e != 0 and s has an even last bit) and then to float32 is the
correctly rounded fmaf (53 >= 2 * 24 + 2 bits)."""
import numpy as np

MASK32 = 0xFFFFFFFF


F32_TINY = float(np.finfo(np.float32).tiny)


def fmaf(a, b, c):
    """Correctly rounded float32 fma, elementwise (numpy arrays or scalars of float32).  s = fl64(a*b + c) rounded to
    float32 is already the correct result unless s lies exactly half way between two float32 values (for a normal float32
    result: the low 29 bits of its significand are 1 followed by zeros) or in float32's subnormal range, where the
    half-way points lie elsewhere; only those elements take fmaf_odd's rounding to odd."""
    with np.errstate(all="ignore"):
        a64, b64, c64 = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
        s = np.asarray(a64 * b64 + c64)
        r = s.astype(np.float32)
        risky = ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000) | ((np.abs(s) < F32_TINY) & (s != 0))
        if risky.any():
            a64, b64, c64 = (np.broadcast_to(x, s.shape)[risky] for x in (a64, b64, c64))
            r = np.array(r)
            r[risky] = fmaf_odd(a64, b64, c64)
        return r


def fmaf_odd(a, b, c):
    """fmaf by rounding to odd, on every element (the definition fmaf is checked against)."""
    with np.errstate(all="ignore"):
        a64, b64, c64 = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
        p = a64 * b64
        s = p + c64
        bp = s - p
        e = (p - (s - bp)) + (c64 - bp)
        bits = np.asarray(s).view(np.int64)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((bits & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def relu(v):
    v = np.asarray(v, np.float32)
    return np.where(v > np.float32(0), v, np.float32(0)).astype(np.float32)


def philox4(seed, lane, step, episode):
    """philox4x32-10, all four words (uint64 arrays holding 32-bit values); the rounds of oracle.philox_action."""
    lane = np.asarray(lane, np.uint64)
    M = np.uint64(MASK32)
    c0, c1 = lane & M, lane >> np.uint64(32)
    c2 = np.broadcast_to(np.asarray(step, np.uint64), c0.shape).copy()
    c3 = np.broadcast_to(np.asarray(episode, np.uint64), c0.shape).copy()
    k0, k1 = np.uint64(seed & MASK32), np.uint64((seed >> 32) & MASK32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M
        n1 = p1 & M
        n2 = ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M
        n3 = p0 & M
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return c0, c1, c2, c3


def feature_dim(W, M):
    return 4 + W + M


def features(W, M, V, c, a, B, G, P, hist, br, norm=None):
    """float32 [F, N] features of N lanes: c, a int [N]; B, G, P float64 [N]; hist float64 [T, N] (row j = h[j]);
    br(r) -> float64 [N, M] (chunk r's bitrates per lane, r an int array [N]); norm float64 [2, F] or None."""
    c = np.asarray(c, np.int64)
    a = np.asarray(a, np.int64)
    N = c.size
    F = feature_dim(W, M)
    lanes = np.arange(N)
    raw = np.zeros((F, N), np.float64)
    raw[0] = B
    ok = (a >= 0) & (a < M) & (c >= 1)
    prev = br(np.maximum(c - 1, 0))
    raw[1] = np.where(ok, prev[lanes, np.clip(a, 0, M - 1)], 0.0)
    raw[2] = (V - c).astype(np.float64)
    with np.errstate(all="ignore"):
        raw[3] = np.asarray(G, np.float64) - np.asarray(P, np.float64)
    for k in range(W):
        j = c - W + k
        raw[4 + k] = np.where(j >= 0, hist[np.maximum(j, 0), lanes], 0.0)
    raw[4 + W:] = br(c).T
    sh = np.zeros((F, 1)) if norm is None else np.asarray(norm, np.float64)[0][:, None]
    sc = np.ones((F, 1)) if norm is None else np.asarray(norm, np.float64)[1][:, None]
    with np.errstate(all="ignore"):
        return ((raw - sh) * sc).astype(np.float32)


def layer(W, b, x):
    """One layer in the contract's order: acc = b[j], then fmaf(W[j][k], x[k], acc) for k in order.  x [in, N]."""
    W = np.asarray(W, np.float32)
    x = np.asarray(x, np.float32)
    acc = np.repeat(np.asarray(b, np.float32).reshape(-1, 1), x.shape[1], axis=1)
    for k in range(W.shape[1]):                       # every row's chain at once: the same fmaf per element, in k order
        acc = fmaf(W[:, k:k + 1], x[k][None, :], acc)
    return acc


def forward(layers, x):
    """Scores [M, N] of features x [F, N]; layers [(W, b)], ReLU after every layer but the last."""
    h = x
    for li, (W, b) in enumerate(layers):
        h = layer(W, b, h)
        if li < len(layers) - 1:
            h = relu(h)
    return h


def argmax_first(scores):
    """g = 0, then g = m if score[m] > score[g] (NaN never wins).  scores [M, N]."""
    g = np.zeros(scores.shape[1], np.int64)
    best = scores[0].copy()
    for m in range(1, scores.shape[0]):
        take = scores[m] > best
        g = np.where(take, m, g)
        best = np.where(take, scores[m], best)
    return g


def explore(seed, thr, lane, c, episode, M, g):
    """The decision after the exploration draw: the random policy's action where word 1 < thr, else g."""
    w0, w1, _, _ = philox4(seed, lane, c, episode)
    rnd = ((w0 * np.uint64(M)) >> np.uint64(32)).astype(np.int64)
    coin = w1 < np.uint64(thr) if thr < (1 << 32) else np.ones(np.shape(w1), bool)
    return np.where(coin, rnd, g).astype(np.int32), coin


def decide(layers, x, seed, thr, lane, c, episode, M):
    """(actions [N], scores [M, N], coin [N])."""
    s = forward(layers, x)
    g = argmax_first(s)
    a, coin = explore(seed, thr, lane, c, episode, M, g)
    return a, s, coin
