"""Independent numpy twin of the episode sampler's contract (include/abr_env.h: abr_episode_sampler) -- TEST
INFRASTRUCTURE.  Written out from the header with policy_twin.philox4 and Python integers; the product's host mirror
(abrsimulator_amd/episodes.py) is checked against it, never used in its place."""
import numpy as np

import policy_twin as T


def twin(seed, lanes, eps, trace_len, pool=None, span=0):
    """(trace ids, start offsets), int32, of episodes `eps` of global lanes `lanes` (broadcast 1-D arrays)."""
    w0, w1, _, _ = T.philox4(seed, np.asarray(lanes, np.uint64), 0xFFFFFFFF, np.asarray(eps, np.uint64))
    tl = np.asarray(trace_len, np.int64)
    n = len(pool) if pool is not None else len(tl)
    t_out, off_out = [], []
    for a, b in zip(np.atleast_1d(w0).tolist(), np.atleast_1d(w1).tolist()):
        u = (a * n) >> 32
        t = int(pool[u]) if pool is not None else u
        length = int(tl[t])
        sp = min(span, length) if span > 0 else length
        t_out.append(t)
        off_out.append((b * sp) >> 32)
    return np.array(t_out, np.int32), np.array(off_out, np.int32)
