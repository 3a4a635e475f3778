"""Numpy twins of the lane fork, the beam selection and the hindsight search (include/abr_env.h: abr_env_fork,
abr_beam_select; abrsimulator_amd/search.py), written from the header's text and sharing no code with the library."""
import numpy as np

OBS_DIM = 8
DONE_EPISODE = 1


def align(b, a=256):
    return (b + a - 1) // a * a


# (name, element bytes, rows) of every per-lane region of the workspace, in layout order (abr_env.hip: compute_layout)
def workspace_regions(V):
    return [("f64", 8, 8), ("i64", 8, 1), ("i32", 4, 15), ("u8", 1, 2), ("action_hist", 1, V), ("bw_hist", 8, V),
            ("ep_terms", 8, 4), ("mpc_action", 4, 1)]


def workspace_offsets(V, N, f64_off):
    """{name: (byte offset, elem, rows)} of the per-lane regions of a workspace whose float64 state starts at f64_off:
    every region starts at the next multiple of 256 bytes after the previous one."""
    out, o = {}, f64_off
    for name, elem, rows in workspace_regions(V):
        out[name] = (o, elem, rows)
        o = align(o + elem * rows * N)
    return out


def scratch_layout(V, count):
    """Byte offsets of the ten region images ([rows][count]) in the fork's scratch, and the total."""
    offs, o = [], 0
    for _, elem, rows in workspace_regions(V) + [("q_run", 8, 1), ("obs", 4, OBS_DIM)]:
        offs.append(o)
        o = align(o + rows * count * elem)
    return offs, o


def pairs(src, dst, N):
    """The (source, destination) pairs a fork moves: both indices inside [0, N)."""
    src = np.asarray(src, np.int64)
    dst = np.arange(len(src), dtype=np.int64) if dst is None else np.asarray(dst, np.int64)
    ok = (src >= 0) & (src < N) & (dst >= 0) & (dst < N)
    return src[ok], dst[ok]


def fork_columns(rows_by_lane, src, dst=None):
    """A [rows, N] array (any dtype) after the fork: column dst[i] = the OLD column src[i]."""
    a = np.asarray(rows_by_lane)
    s, d = pairs(src, dst, a.shape[-1])
    out = a.copy()
    out[..., d] = a[..., s]
    return out


def fork_workspace(ws, V, N, f64_off, src, dst=None):
    """The workspace bytes (uint8 array) after the fork."""
    out = ws.copy()
    for name, (o, elem, rows) in workspace_offsets(V, N, f64_off).items():
        view = ws[o:o + elem * rows * N].reshape(rows, N, elem)
        out[o:o + elem * rows * N] = fork_columns(view.transpose(0, 2, 1), src, dst).transpose(0, 2, 1).reshape(-1)
    return out


def lane_byte_mask(total, V, N, f64_off, lanes):
    """Boolean [total]: the bytes of the workspace that belong to one of `lanes` in a per-lane region."""
    m = np.zeros(total, bool)
    lanes = np.asarray(lanes, np.int64)
    for name, (o, elem, rows) in workspace_offsets(V, N, f64_off).items():
        v = m[o:o + elem * rows * N].reshape(rows, N, elem)
        v[:, lanes, :] = True
    return m


def select(S, M, wl, R_in, reward, lat, done, valid_in, key_override=None):
    """abr_beam_select over len(R_in) // S groups: (src int32, R_out f64, valid_out u8), lanes past the last group -1/0/0.
    Ranks by np.lexsort over (slot, key) on the valid candidates."""
    R_in = np.asarray(R_in, np.float64)
    n = len(R_in)
    G = n // S
    R_new = R_in + np.asarray(reward, np.float32).astype(np.float64)
    key = np.asarray(key_override, np.float64) if key_override is not None else R_new + np.float64(wl) * np.asarray(lat, np.float64)
    done = np.asarray(done, np.uint8)
    valid = (np.asarray(valid_in) != 0) & ((done & np.uint8(0xFF ^ DONE_EPISODE)) == 0) & (key == key)
    src = np.full(n, -1, np.int32)
    R_out = np.zeros(n, np.float64)
    valid_out = np.zeros(n, np.uint8)
    for g in range(G):
        b = g * S
        cand = np.nonzero(valid[b:b + S])[0]
        k = key[b + cand] + 0.0                                    # -0.0 + 0.0 == +0.0: the two zeros tie, the slot decides
        order = cand[np.lexsort((cand, k))]
        for s in range(S):
            r = s // M
            if r < len(order):
                src[b + s] = b + order[r]
                R_out[b + s] = R_new[b + order[r]]
                valid_out[b + s] = 1
    return src, R_out, valid_out


def search(evaluate, G, beam, M, V, wl):
    """The hindsight search on action prefixes instead of lanes.  evaluate(g, prefixes) -> (reward f32 [n], lat f64 [n],
    done u8 [n], qoe f64 [n]) of the LAST step of each prefix (a list of action tuples) on group g's pair; qoe matters
    for prefixes of length V only.  Returns (qoe [G], actions [V, G], per-iteration records)."""
    S = beam * M
    best_q, best_a, log = np.full(G, np.nan), np.zeros((V, G), np.int32), []
    for g in range(G):
        prefix = [()] * S                                          # every slot starts from the reset state
        R = np.zeros(S)
        valid = (np.arange(S) < M).astype(np.uint8)
        for t in range(V):
            cand = [prefix[s] + (s % M,) for s in range(S)]
            reward, lat, done, qoe = evaluate(g, cand)
            src, R_out, valid_out = select(S, M, wl, R, reward, lat, done, valid)
            log.append((g, t, src, R_out, valid_out))
            if t + 1 < V:
                prefix = [cand[src[s]] if src[s] >= 0 else cand[s] for s in range(S)]
                R, valid = R_out, valid_out
            else:
                src, _, ok = select(S, M, wl, R, reward, None, done, valid, key_override=qoe)
                if ok[0]:
                    best_q[g], best_a[:, g] = qoe[src[0]], cand[src[0]]
    return best_q, best_a, log
