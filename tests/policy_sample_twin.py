"""numpy twin of the learned policy's sampled decision (include/abr_env.h: abr_policy_sampling; csrc/abr_lane_jump.h:
exp_c, policy_softmax_sample, policy_decide), written in the contract's order: float32 products and differences with one
rounding each, numpy's rint (round half to even), policy_twin.fmaf for every fmaf, the correctly rounded float32
division."""
import numpy as np

import policy_twin as T

LOG2E = np.float32(float.fromhex("0x1.715476p+0"))
LN2_HI = np.float32(float.fromhex("0x1.63p-1"))
LN2_LO = np.float32(float.fromhex("-0x1.bd0106p-13"))
C = [np.float32(1.0), np.float32(1.0), np.float32(0.5), np.float32(float.fromhex("0x1.55549cp-3")),
     np.float32(float.fromhex("0x1.555694p-5")), np.float32(float.fromhex("0x1.1234fcp-7")),
     np.float32(float.fromhex("0x1.6b69e0p-10"))]
X_MIN = np.float32(-80.0)
ARGMAX, SOFTMAX = 0, 1


def exp_c(x):
    """The contract's exp for float32 x <= 0 (elementwise): +0 below -80 (and for -inf and NaN)."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        live = x >= X_MIN
        xs = np.where(live, x, np.float32(0))
        k = np.rint(xs * LOG2E).astype(np.float32)
        r = T.fmaf(-k, LN2_HI, xs)
        r = T.fmaf(-k, LN2_LO, r)
        p = np.full(r.shape, C[6], np.float32)
        for j in range(5, -1, -1):
            p = T.fmaf(p, r, C[j])
        e = np.ldexp(p, k.astype(np.int32)).astype(np.float32)
    return np.where(live, e, np.float32(0)).astype(np.float32)


def uniform_q(w2):
    """q = (w2 >> 8) * 2^-24, exact in float32."""
    return ((np.asarray(w2, np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def softmax_sample(s, g, iT, w2):
    """(sample [N], probs [M, N], e [M, N], S [N]) of scores s float32 [M, N], first argmax g [N], inv_temperature iT
    (float32 scalar or [N]) and philox word 2 w2 [N]."""
    s = np.asarray(s, np.float32)
    M, N = s.shape
    g = np.asarray(g, np.int64)
    lanes = np.arange(N)
    iT = np.broadcast_to(np.asarray(iT, np.float32), (N,))
    sg = s[g, lanes]
    fin = np.isfinite(sg)
    with np.errstate(all="ignore"):
        e = np.empty((M, N), np.float32)
        for m in range(M):
            d = (s[m] - sg).astype(np.float32)
            e[m] = exp_c((d * iT).astype(np.float32))
        S = np.zeros(N, np.float32)
        cum = np.empty((M, N), np.float32)
        for m in range(M):
            S = (S + e[m]).astype(np.float32)
            cum[m] = S
        t = (uniform_q(w2) * S).astype(np.float32)
        probs = (e / S).astype(np.float32)
    hit = cum > t
    sample = np.where(hit.any(0), np.argmax(hit, 0), g)
    onehot = (np.arange(M)[:, None] == g[None, :]).astype(np.float32)
    sample = np.where(fin, sample, g)
    probs = np.where(fin[None, :], probs, onehot).astype(np.float32)
    return sample.astype(np.int64), probs, e, S


def decide_sampled(layers, x, seed, thr, lane, c, episode, M, iT, mode=SOFTMAX):
    """(actions [N], scores [M, N], coin [N], probs [M, N]): policy_twin.decide with the policy's action drawn from
    softmax(scores * iT) by word 2 of the same philox block (mode SOFTMAX), or its argmax (mode ARGMAX)."""
    s = T.forward(layers, x)
    g = T.argmax_first(s)
    if mode == ARGMAX:
        probs = (np.arange(M)[:, None] == g[None, :]).astype(np.float32)
        a, coin = T.explore(seed, thr, lane, c, episode, M, g)
        return a, s, coin, probs
    _, _, w2, _ = T.philox4(seed, lane, c, episode)
    pick, probs, _, _ = softmax_sample(s, g, np.float32(iT), w2)
    a, coin = T.explore(seed, thr, lane, c, episode, M, pick)
    return a, s, coin, probs


def behaviour_probs(probs, M, thr):
    """The behaviour distribution with exploration: (1 - eps) * probs + eps * rho, eps = thr / 2^32, rho[m] the exact
    share of 32-bit words w0 with floor(w0 * M / 2^32) == m."""
    eps = thr / 2.0 ** 32
    edges = np.array([-((-m * 2 ** 32) // M) for m in range(M + 1)], np.float64)
    rho = np.diff(edges) / 2.0 ** 32
    return (1.0 - eps) * np.asarray(probs, np.float64) + eps * rho[:, None]
