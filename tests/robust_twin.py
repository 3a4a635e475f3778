"""numpy twin of RobustMPC's throughput estimate (include/abr_env.h: abr_mpc_robust; csrc/abr_lane_jump.h:
robust_estimate), float64 in the contract's operation order, so that it reproduces the device's state and estimates bit
for bit.  Sums are sequential loops (never np.sum, which is pairwise beyond 8 terms).

The state is a dict of arrays over lanes in the documented layout: cs1 int32 [N] (c* + 1, 0 = none), cnt int32 [N],
ps float64 [N] (p*), err float64 [W, N] (oldest first; rows at or past cnt hold no meaning but are reproduced too).
state_bytes / state_from_bytes convert to and from the device's byte image.

Scalar form: estimate_scalar(W, c, h, st, i) for lane i of st (the oracle's policy callback).  Vectorised form:
estimate_vec(W, c[N], hist[T, N], st, active[N]) over lanes.  Both return the estimate P (0.0 = no decision) and update
st in place.  select_scalar adds D12, previous_bitrate and the brute search (oracle.mpc_brute)."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def empty_state(n, window):
    return dict(cs1=np.zeros(n, np.int32), cnt=np.zeros(n, np.int32), ps=np.zeros(n, np.float64),
                err=np.zeros((window, n), np.float64))


def state_nbytes(n, window):
    return n * (8 + 8 * (1 + window))


def state_bytes(st):
    return np.concatenate([st["cs1"].view(np.uint8), st["cnt"].view(np.uint8), st["ps"].view(np.uint8),
                           np.ascontiguousarray(st["err"]).view(np.uint8).ravel()])


def state_from_bytes(b, n, window):
    b = np.ascontiguousarray(np.asarray(b, np.uint8))
    assert b.size >= state_nbytes(n, window)
    return dict(cs1=b[:4 * n].view(np.int32).copy(), cnt=b[4 * n:8 * n].view(np.int32).copy(),
                ps=b[8 * n:16 * n].view(np.float64).copy(),
                err=b[16 * n:16 * n + 8 * n * window].view(np.float64).reshape(window, n).copy())


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def estimate_scalar(W, c, h, st, i):
    """c = chunk_number, h = previous_bandwidths oldest first (len >= c)."""
    W, c = int(W), int(c)
    cs1, cnt, ps = int(st["cs1"][i]), int(st["cnt"][i]), float(st["ps"][i])
    err = st["err"][:, i]
    if cnt < 0 or cnt > W:
        cnt = 0
    if cs1 > 0 and cs1 == c:
        hc = float(h[c - 1])
        with np.errstate(all="ignore"):
            e = float(np.float64(abs(ps - hc)) / np.float64(hc))
        if cnt < W:
            err[cnt] = e
            cnt += 1
        else:
            for k in range(1, W):
                err[k - 1] = err[k]
            err[W - 1] = e
    elif not (cs1 > 0 and cs1 == c + 1):
        cnt = 0
    n = min(W, c)
    P = 0.0
    if n <= 0:
        cs1, cnt, ps = 0, 0, 0.0
    else:
        with np.errstate(all="ignore"):
            S = np.float64(0.0)
            for j in range(c - n, c):
                S = S + np.float64(1.0) / np.float64(h[j])
            hm = np.float64(n) / S
            E = np.float64(0.0)
            if cnt > 0:
                E = np.float64(err[0])
                for k in range(1, cnt):
                    E = err[k] if err[k] > E else E
            Pv = hm / (np.float64(1.0) + E)
        if not (hm > 0.0 and hm <= DBL_MAX):
            cs1, cnt, ps = 0, 0, 0.0
        else:
            ps, cs1 = float(hm), c + 1
            P = float(Pv) if Pv > 0.0 else 0.0
    st["cs1"][i], st["cnt"][i], st["ps"][i] = cs1, cnt, ps
    return P


def estimate_vec(W, c, hist, st, active=None):
    """c int [N], hist f64 [T, N] (row j = previous_bandwidths[j]), active bool [N] (None: all).  Returns P f64 [N]
    (0.0 where there is no decision or the lane is inactive); inactive lanes' state is untouched."""
    W = int(W)
    c = np.asarray(c, np.int64)
    N = len(c)
    act = np.ones(N, bool) if active is None else np.asarray(active, bool)
    lanes = np.arange(N)
    T = hist.shape[0]
    cs1, cnt, ps, err = st["cs1"].astype(np.int64), st["cnt"].astype(np.int64), st["ps"].copy(), st["err"].copy()
    cnt = np.where((cnt < 0) | (cnt > W), 0, cnt)
    with np.errstate(all="ignore"):
        push = act & (cs1 > 0) & (cs1 == c)
        keep = act & (cs1 > 0) & (cs1 == c + 1)
        hc = hist[np.clip(c - 1, 0, T - 1), lanes]
        e = np.abs(ps - hc) / hc
        full = push & (cnt >= W)
        for k in range(1, W):
            err[k - 1] = np.where(full, err[k], err[k - 1])
        slot = np.where(full, W - 1, np.minimum(cnt, W - 1))
        for k in range(W):
            err[k] = np.where(push & (slot == k), e, err[k])
        cnt = np.where(push & ~full, cnt + 1, cnt)
        cnt = np.where(act & ~push & ~keep, 0, cnt)
        n = np.minimum(W, c)
        S = np.zeros(N)
        for k in range(W):
            j = c - n + k
            ok = act & (k < n)
            S = np.where(ok, S + 1.0 / hist[np.clip(j, 0, T - 1), lanes], S)
        hm = n.astype(np.float64) / S
        E = np.where(cnt > 0, err[0], 0.0)
        for k in range(1, W):
            E = np.where((k < cnt) & (err[k] > E), err[k], E)
        Pv = hm / (1.0 + E)
    empty = act & ((n <= 0) | ~((hm > 0.0) & (hm <= DBL_MAX)))
    rec = act & ~empty
    P = np.where(rec & (Pv > 0.0), Pv, 0.0)
    cs1 = np.where(empty, 0, np.where(rec, c + 1, cs1))
    cnt = np.where(empty, 0, cnt)
    ps = np.where(empty, 0.0, np.where(rec, hm, ps))
    st["cs1"][:] = cs1.astype(np.int32)
    st["cnt"][:] = cnt.astype(np.int32)
    st["ps"][:] = ps
    st["err"][:] = np.where(act[None, :], err, st["err"])
    return P


def select_scalar(oracle, ocfg, br, sz, W, c, prev, buf, h, st, i, clip=True):
    """RobustMPC's whole decision for lane i: (action, flat, J) with (-1, -1, NaN) for no decision.  ocfg: an
    oracle.mpc_cfg at the full horizon; br / sz: [V][B]."""
    P = estimate_scalar(W, c, h, st, i)
    B, H, V = ocfg.n_rates, ocfg.horizon, ocfg.video_length
    he = H
    if c + H > V:
        he = (V - c) if clip else 0
    he = max(he, 0)
    if not (P > 0.0) or not (-B <= prev < B) or he == 0:
        return -1, -1, np.nan
    cfg = oracle.mpc_cfg(B, he, V, ocfg.chunk_length, ocfg.max_buffer, ocfg.variance_weight, ocfg.rebuffer_weight,
                         ocfg.startup_weight)
    f, jm, _ = oracle.mpc_brute(cfg, br, sz, c, prev, buf, np.full(he, P), want_J=False)
    return f // B ** (he - 1), f, jm
