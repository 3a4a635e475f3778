"""EpisodeLedger: the caller-owned blob the env kernels append one record per finished episode to
(include/abr_env.h: abr_episode_ledger), and the views and reductions over it.

The blob is struct-of-arrays with row stride n_lanes; every region starts at a multiple of 256 bytes:

    count   int32   [N]           episodes recorded for the lane since the blob was zeroed
    total   float64 [5][N]        running sums over all recorded episodes of the lane, in episode order
    rec_f64 float64 [rows][5][N]  the float fields of the record in each ring slot
    rec_i32 int32   [rows][5][N]  the int fields of the record in each ring slot

A record goes to slot count % rows, then count is incremented.  The layout arithmetic here is plain Python and the views
work on a CPU tensor as well, so everything but the kernels' appends can be used (and is tested) without a GPU.
"""
import torch

FLOAT_FIELDS = ("rebuffer_time", "start_up_time", "average_latency", "variance", "qoe")
INT_FIELDS = ("episode", "trace_id", "start_offset", "chunks", "done")
N_FIELDS = 5
ALIGN = 256


def _align(b):
    return (b + ALIGN - 1) // ALIGN * ALIGN


def ledger_layout(n_lanes, rows):
    """Byte offsets of the four regions and the blob's size: dict(count, total, rec_f64, rec_i32, bytes).  The same
    arithmetic as abr_env_ledger_bytes (csrc/abr_lane_jump.h: ledger_layout)."""
    n_lanes, rows = int(n_lanes), int(rows)
    if n_lanes < 1 or rows < 1:
        raise ValueError("an episode ledger needs n_lanes >= 1 and rows >= 1")
    lo = {"count": 0}
    lo["total"] = _align(4 * n_lanes)
    lo["rec_f64"] = lo["total"] + _align(N_FIELDS * 8 * n_lanes)
    lo["rec_i32"] = lo["rec_f64"] + _align(rows * N_FIELDS * 8 * n_lanes)
    lo["bytes"] = lo["rec_i32"] + _align(rows * N_FIELDS * 4 * n_lanes)
    return lo


class EpisodeLedger:
    """Owns the blob of an episode ledger: EpisodeLedger(n_lanes, rows, device).  BatchedABREnv.set_episode_ledger
    builds one and installs it; every view below aliases the blob, so it shows what the kernels have appended once the
    launches on the current stream have run."""

    def __init__(self, n_lanes, rows, device="cpu"):
        self.n_lanes, self.rows = int(n_lanes), int(rows)
        self.layout = ledger_layout(self.n_lanes, self.rows)
        self.device = torch.device(device)
        self.blob = torch.zeros(self.layout["bytes"], dtype=torch.uint8, device=self.device)
        if self.blob.data_ptr() % ALIGN and self.device.type != "cpu":
            raise RuntimeError("the ledger's blob is not 256-byte aligned")

    # -- raw views ---------------------------------------------------------
    def _region(self, name, dtype, shape):
        n = 1
        for s in shape:
            n *= s
        size = n * (8 if dtype == torch.float64 else 4)
        off = self.layout[name]
        return self.blob[off:off + size].view(dtype).view(*shape)

    def count(self):
        """Episodes recorded per lane since the blob was zeroed: int32 [N] view."""
        return self._region("count", torch.int32, (self.n_lanes,))

    def totals(self):
        """Per-lane running sums over ALL recorded episodes (added in episode order by the kernels): dict of float64 [N]
        views, one per float field."""
        t = self._region("total", torch.float64, (N_FIELDS, self.n_lanes))
        return {k: t[f] for f, k in enumerate(FLOAT_FIELDS)}

    def ring(self):
        """The ring as it lies in memory: dict of [rows, N] views, float64 for the float fields and int32 for the int
        fields.  Slot s of lane i is valid if s < min(count[i], rows); records() puts the valid ones in order."""
        f = self._region("rec_f64", torch.float64, (self.rows, N_FIELDS, self.n_lanes))
        w = self._region("rec_i32", torch.int32, (self.rows, N_FIELDS, self.n_lanes))
        out = {k: f[:, q] for q, k in enumerate(FLOAT_FIELDS)}
        out.update({k: w[:, q] for q, k in enumerate(INT_FIELDS)})
        return out

    # -- reductions --------------------------------------------------------
    def records(self):
        """Every valid record as flat 1-D tensors sorted by (lane, episode): dict(lane, episode, trace_id, start_offset,
        chunks, done, rebuffer_time, start_up_time, average_latency, variance, qoe).  A lane that has recorded more than
        `rows` episodes contributes its last `rows`; a lane with none contributes nothing."""
        R, N = self.rows, self.n_lanes
        c = self.count().to(torch.int64)                                   # [N]
        s = torch.arange(R, device=self.device, dtype=torch.int64).reshape(R, 1)
        valid = s < torch.clamp(c, max=R).reshape(1, N)                    # [R, N]
        # the newest record number r < count with r % rows == s
        rec_no = (c - 1).reshape(1, N) - torch.remainder((c - 1).reshape(1, N) - s, R)
        key = torch.where(valid, rec_no, torch.full_like(rec_no, torch.iinfo(torch.int64).max)).t().contiguous()
        order = torch.argsort(key, dim=1)                                  # [N, R]: the lane's slots, oldest first
        keep = torch.gather(valid.t().contiguous(), 1, order).reshape(-1)
        lane = torch.arange(N, device=self.device, dtype=torch.int64).reshape(N, 1).expand(N, R).reshape(-1)
        out = {"lane": lane[keep]}
        for k, v in self.ring().items():
            out[k] = torch.gather(v.t().contiguous(), 1, order).reshape(-1)[keep]
        return {k: out[k] for k in ("lane",) + INT_FIELDS + FLOAT_FIELDS}

    def per_trace(self, n_traces):
        """Count and mean of every float field per trace id over records(): dict(count int64 [n_traces], and one float64
        [n_traces] mean per float field; NaN for a trace without a record).  The sums are formed with index_add_, whose
        order of additions is not fixed on a GPU: a mean is reproducible only up to the error of a float64 sum of its
        n terms in any order, n * 2^-53 * sum|x| / (1 - n * 2^-53), never bit for bit.  The counts are exact."""
        n_traces = int(n_traces)
        rec = self.records()
        t = rec["trace_id"].to(torch.int64)
        cnt = torch.bincount(t, minlength=n_traces)
        out = {"count": cnt}
        for k in FLOAT_FIELDS:
            s = torch.zeros(n_traces, dtype=torch.float64, device=self.device).index_add_(0, t, rec[k])
            out[k] = s / cnt.to(torch.float64)
        return out

    def per_member(self, group, n_members):
        """Count and mean of every float field per member of a policy population (policy.PolicyPopulation: lane i
        belongs to member i // group) over ALL recorded episodes: dict(count int64 [n_members], and one float64
        [n_members] mean per float field).  Built from count() and totals(), not from the ring, so a lane that has
        recorded more than `rows` episodes still counts every one of them.  The counts are exact; a mean is the sum of
        its member's per-lane totals in an order that is not fixed, so it is reproducible up to the error of a float64
        sum of its n episodes in any order, n * 2^-53 * sum|x| / (1 - n * 2^-53), as per_trace.  A member without an
        episode reports count 0 and a mean of 0.0 (not per_trace's NaN: the fitness vector an evolution strategy
        ranks stays finite; look at count to tell)."""
        group, P = int(group), int(n_members)
        if group < 1 or P != -(-self.n_lanes // group):
            raise ValueError(f"{self.n_lanes} lanes in groups of {group} make {-(-self.n_lanes // max(group, 1))} "
                             f"members, not {P}")
        pad = P * group - self.n_lanes

        def by_member(v):                                                 # [N] -> [P] sums over each member's lanes
            if pad:
                v = torch.cat([v, torch.zeros(pad, dtype=v.dtype, device=v.device)])
            return v.reshape(P, group).sum(dim=1)

        cnt = by_member(self.count().to(torch.int64))
        out = {"count": cnt}
        den = torch.clamp(cnt, min=1).to(torch.float64)
        for k, v in self.totals().items():
            out[k] = by_member(v) / den
        return out

    # -- lifecycle ---------------------------------------------------------
    def clear(self):
        """Empty the ledger: zero the blob (on the current stream, in order with the launches)."""
        self.blob.zero_()

    def state_dict(self):
        return {"n_lanes": self.n_lanes, "rows": self.rows, "blob": self.blob.clone()}

    def load_state_dict(self, sd):
        if int(sd["n_lanes"]) != self.n_lanes or int(sd["rows"]) != self.rows:
            raise ValueError(f"the ledger state is for {sd['n_lanes']} lanes x {sd['rows']} rows, this ledger has "
                             f"{self.n_lanes} x {self.rows}")
        if sd["blob"].numel() != self.blob.numel():
            raise ValueError("the ledger state's blob has another size")
        self.blob.copy_(sd["blob"])
