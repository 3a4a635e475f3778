"""EpisodeQuality: the quality model of the env kernels (include/abr_env.h: abr_episode_quality) -- a weight, a utility
table and the caller-owned blob the kernels keep each lane's quality sums in -- and the views and reductions over it.

The blob is struct-of-arrays with row stride n_lanes; every region starts at a multiple of 256 bytes:

    count   int32   [N]         episodes recorded for the lane since the blob was zeroed
    q_run   float64 [N]         the running sum of the episode in flight
    q_last  float64 [N]         the sum of the lane's last finished episode
    total_q float64 [N]         running sum over all recorded episodes of the lane, in episode order
    rec_q   float64 [rows][N]   the sum of the record in each ring slot

A record goes to slot count % rows, then count is incremented: cleared together with an EpisodeLedger of the same rows,
slot s of the two describes the same episode.  The layout arithmetic and the tables are plain Python and the views work on
a CPU tensor as well, so everything but the kernels' writes can be used (and is tested) without a GPU.
"""
import math

import numpy as np
import torch

from .ledger import ALIGN, FLOAT_FIELDS, _align

UTILITIES = ("identity", "log", "log_top")


def quality_layout(n_lanes, rows):
    """Byte offsets of the five regions and the blob's size: dict(count, q_run, q_last, total_q, rec_q, bytes).  The same
    arithmetic as abr_env_quality_bytes (csrc/abr_lane_jump.h: quality_layout)."""
    n_lanes, rows = int(n_lanes), int(rows)
    if n_lanes < 1 or rows < 1:
        raise ValueError("a quality model needs n_lanes >= 1 and rows >= 1")
    lo = {"count": 0}
    lo["q_run"] = _align(4 * n_lanes)
    lo["q_last"] = lo["q_run"] + _align(8 * n_lanes)
    lo["total_q"] = lo["q_last"] + _align(8 * n_lanes)
    lo["rec_q"] = lo["total_q"] + _align(8 * n_lanes)
    lo["bytes"] = lo["rec_q"] + _align(rows * 8 * n_lanes)
    return lo


def utility_table(utility, bitrates, video_length):
    """The table u, float64 [video_length][n_rates], built on the host.  bitrates: one ladder [M] or a per-chunk table
    [V][M].  utility: "identity" (u = br[c][m], mpc.py's default utility), "log" (ln(br[c][m] / br[c][0]), BOLA's and
    Pensieve's), "log_top" (ln(br[c][m] / br[c][-1]), mpc.py's log_bitrate_utility), or a [V][M] array taken as it is."""
    V = int(video_length)
    br = np.asarray(bitrates, np.float64)
    if br.ndim == 1:
        br = np.broadcast_to(br, (V, br.size))
    if br.ndim != 2 or br.shape[0] != V:
        raise ValueError(f"bitrates must be [n_rates] or [{V}][n_rates]")
    if isinstance(utility, str):
        if utility not in UTILITIES:
            raise ValueError(f"utility must be one of {UTILITIES} or a [{V}][{br.shape[1]}] array, got {utility!r}")
        if utility == "identity":
            return np.array(br, np.float64)
        ref = br[:, 0] if utility == "log" else br[:, -1]
        # math.log, element by element: the C library's, whatever vector routine numpy would pick on this host
        return np.array([[math.log(br[c, m] / ref[c]) for m in range(br.shape[1])] for c in range(V)], np.float64)
    u = np.array(utility, np.float64)
    if u.shape != br.shape:
        raise ValueError(f"a utility table must be [{V}][{br.shape[1]}], got {tuple(u.shape)}")
    return u


class EpisodeQuality:
    """Owns a quality model: EpisodeQuality(n_lanes, rows, weight, table, device).  BatchedABREnv.set_quality builds one
    and installs it; every view below aliases the blob, so it shows what the kernels have written once the launches on
    the current stream have run."""

    def __init__(self, n_lanes, rows, weight, table, device="cpu"):
        self.n_lanes, self.rows = int(n_lanes), int(rows)
        self.weight = float(weight)
        if not math.isfinite(self.weight):
            raise ValueError("the quality weight must be finite")
        self.layout = quality_layout(self.n_lanes, self.rows)
        self.device = torch.device(device)
        t = np.ascontiguousarray(np.asarray(table, np.float64))
        if t.ndim != 2:
            raise ValueError("the utility table must be [video_length][n_rates]")
        self.table = torch.from_numpy(t.copy()).to(self.device).contiguous()
        self.blob = torch.zeros(self.layout["bytes"], dtype=torch.uint8, device=self.device)
        if self.blob.data_ptr() % ALIGN and self.device.type != "cpu":
            raise RuntimeError("the quality blob is not 256-byte aligned")

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

    def running(self):
        """The quality sum of each lane's episode in flight (mid-episode state): float64 [N] view."""
        return self._region("q_run", torch.float64, (self.n_lanes,))

    def last(self):
        """The quality sum of each lane's last finished episode: float64 [N] view."""
        return self._region("q_last", torch.float64, (self.n_lanes,))

    def totals(self):
        """Per-lane running sum over ALL recorded episodes (added in episode order by the kernels): float64 [N] view."""
        return self._region("total_q", torch.float64, (self.n_lanes,))

    def ring(self):
        """The ring as it lies in memory: float64 [rows, N] view.  Slot s of lane i is valid if s < min(count[i], rows)."""
        return self._region("rec_q", torch.float64, (self.rows, self.n_lanes))

    # -- reductions --------------------------------------------------------
    def _check(self, ledger):
        if ledger.rows != self.rows or ledger.n_lanes != self.n_lanes:
            raise ValueError(f"the ledger has {ledger.n_lanes} lanes x {ledger.rows} rows, the quality model "
                             f"{self.n_lanes} x {self.rows}: their slots do not coincide")
        if not torch.equal(ledger.count().to(self.device), self.count()):
            raise ValueError("the ledger and the quality model have recorded different episode counts (clear them "
                             "together): their slots do not coincide")

    def records(self, ledger=None):
        """Every valid record as flat 1-D tensors sorted by (lane, episode): dict(lane, quality).  With an EpisodeLedger
        of the same rows and counts: the ledger's records() plus `quality` and `qoe_q` = qoe - weight * quality, the
        episode's QoE with the quality term.  ValueError if the rows differ or the counts disagree."""
        R, N = self.rows, self.n_lanes
        c = self.count().to(torch.int64)
        s = torch.arange(R, device=self.device, dtype=torch.int64).reshape(R, 1)
        valid = s < torch.clamp(c, max=R).reshape(1, N)
        rec_no = (c - 1).reshape(1, N) - torch.remainder((c - 1).reshape(1, N) - s, R)
        key = torch.where(valid, rec_no, torch.full_like(rec_no, torch.iinfo(torch.int64).max)).t().contiguous()
        order = torch.argsort(key, dim=1)                                  # [N, R]: the lane's slots, oldest first
        keep = torch.gather(valid.t().contiguous(), 1, order).reshape(-1)
        q = torch.gather(self.ring().t().contiguous(), 1, order).reshape(-1)[keep]
        if ledger is None:
            lane = torch.arange(N, device=self.device, dtype=torch.int64).reshape(N, 1).expand(N, R).reshape(-1)
            return {"lane": lane[keep], "quality": q}
        self._check(ledger)
        out = dict(ledger.records())
        out["quality"] = q
        out["qoe_q"] = out["qoe"] - self.weight * q
        return out

    def per_trace(self, n_traces, ledger):
        """EpisodeLedger.per_trace with two more means, `quality` and `qoe_q`, over the joined records(ledger).  As
        there, the counts are exact and a mean is reproducible up to the error of a float64 sum of its n terms in any
        order, n * 2^-53 * sum|x| / (1 - n * 2^-53); NaN for a trace without a record."""
        n_traces = int(n_traces)
        rec = self.records(ledger)
        t = rec["trace_id"].to(torch.int64)
        cnt = torch.bincount(t, minlength=n_traces)
        out = {"count": cnt}
        for k in FLOAT_FIELDS + ("quality", "qoe_q"):
            s = torch.zeros(n_traces, dtype=torch.float64, device=self.device).index_add_(0, t, rec[k])
            out[k] = s / cnt.to(torch.float64)
        return out

    def per_member(self, group, n_members, ledger):
        """EpisodeLedger.per_member with two more means, `quality` and `qoe_q`, over ALL recorded episodes: built from the
        totals, not from the ring, so a lane that has recorded more than `rows` episodes still counts every one.
        qoe_q is mean qoe - weight * mean quality.  A member without an episode reports count 0 and means of 0.0."""
        self._check(ledger)
        out = ledger.per_member(group, n_members)
        group, P = int(group), int(n_members)
        v = self.totals()
        pad = P * group - self.n_lanes
        if pad:
            v = torch.cat([v, torch.zeros(pad, dtype=v.dtype, device=v.device)])
        den = torch.clamp(out["count"], min=1).to(torch.float64)
        out["quality"] = v.reshape(P, group).sum(dim=1) / den
        out["qoe_q"] = out["qoe"] - self.weight * out["quality"]
        return out

    # -- lifecycle ---------------------------------------------------------
    def clear(self):
        """Empty the model's records and sums: zero the blob (on the current stream, in order with the launches)."""
        self.blob.zero_()

    def state_dict(self):
        """The blob (q_run is mid-episode state: a checkpoint taken inside an episode needs it), the weight and the table."""
        return {"n_lanes": self.n_lanes, "rows": self.rows, "weight": self.weight, "table": self.table.clone(),
                "blob": self.blob.clone()}

    def load_state_dict(self, sd):
        if int(sd["n_lanes"]) != self.n_lanes or int(sd["rows"]) != self.rows:
            raise ValueError(f"the quality state is for {sd['n_lanes']} lanes x {sd['rows']} rows, this model has "
                             f"{self.n_lanes} x {self.rows}")
        if sd["blob"].numel() != self.blob.numel():
            raise ValueError("the quality state's blob has another size")
        t = sd["table"].to(self.device)
        if (float(sd["weight"]) != self.weight or t.shape != self.table.shape
                or not torch.equal(t.contiguous().view(torch.int64), self.table.view(torch.int64))):      # bits: a NaN is the caller's
            raise ValueError("the quality state was taken under another weight or utility table")
        self.blob.copy_(sd["blob"])
