"""Host mirror of the episode sampler (include/abr_env.h: abr_episode_sampler; csrc/abr_lane_jump.h: episode_assign).

Under auto_reset with a sampler installed (BatchedABREnv.set_episode_sampler), every episode a lane starts -- a sampled
reset or a re-arm inside a fused launch -- runs on a (trace, start offset) pair that is a pure function of (seed, global
lane id, episode number).  EpisodeSampler.draw computes the same pairs in numpy, so that a trainer can tell which trace any
(lane, episode) of a rollout ran without reading anything back from the device.
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
EPISODE_STEP = 0xFFFFFFFF      # the philox counter's step word: never a chunk id


def _philox4(seed, lane, step, episode):
    """philox4x32-10 (Salmon et al. 2011) with key = seed and counter = (lane lo, lane hi, step, episode); uint64 arrays."""
    lane = np.asarray(lane, dtype=np.uint64)
    c0, c1 = lane & _M32, lane >> np.uint64(32)
    c2 = np.full(lane.shape, step, dtype=np.uint64)
    c3 = np.asarray(episode, dtype=np.uint64) & _M32
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & _M32, \
            p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


class EpisodeSampler:
    """seed: uint64 philox key; pool: None (every trace) or a sequence of trace ids; offset_span: 0 (the whole trace) or
    the number of leading positions of each trace a start offset is drawn from (capped at the trace's length)."""

    def __init__(self, seed, pool=None, offset_span=0):
        self.seed = int(seed) & (2 ** 64 - 1)
        self.offset_span = int(offset_span)
        if self.offset_span < 0:
            raise ValueError("offset_span must be >= 0")
        self.pool = None
        if pool is not None:
            p = np.asarray(pool).reshape(-1)
            if p.size < 1:
                raise ValueError("a pool needs at least one trace id")
            if not np.issubdtype(p.dtype, np.integer):
                raise ValueError("pool must hold integer trace ids")
            if int(p.min()) < 0 or int(p.max()) > np.iinfo(np.int32).max:
                raise ValueError("pool trace ids must be in [0, 2^31)")
            self.pool = p.astype(np.int32)

    def check(self, n_traces):
        """Raise ValueError if the pool names a trace outside [0, n_traces)."""
        if self.pool is not None and int(self.pool.max()) >= int(n_traces):
            raise ValueError(f"pool trace id {int(self.pool.max())} is outside [0, {int(n_traces)})")

    def draw(self, lane_ids, episodes, trace_len):
        """(trace_id, start_offset), int32 arrays of the broadcast shape of lane_ids (GLOBAL lane ids: lane_id_base + i)
        and episodes (episode numbers); trace_len: the length of every trace of the corpus, in trace-id order."""
        tl = np.asarray(trace_len, dtype=np.int64).reshape(-1)
        self.check(tl.size)
        g, e = np.broadcast_arrays(np.asarray(lane_ids, dtype=np.uint64), np.asarray(episodes, dtype=np.int64))
        w0, w1, _, _ = _philox4(self.seed, g, EPISODE_STEP, e.astype(np.uint64) & _M32)
        n = np.uint64(self.pool.size if self.pool is not None else tl.size)
        u = ((w0 * n) >> np.uint64(32)).astype(np.int64)
        t = self.pool[u].astype(np.int64) if self.pool is not None else u
        length = tl[t]
        span = np.minimum(self.offset_span, length) if self.offset_span > 0 else length
        off = (w1 * span.astype(np.uint64)) >> np.uint64(32)
        return t.astype(np.int32), off.astype(np.int32)
