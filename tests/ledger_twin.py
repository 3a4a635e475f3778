"""A numpy twin of the episode ledger's contract (include/abr_env.h: abr_episode_ledger), written from the header's text
and independent of abrsimulator_amd/ledger.py and of csrc/abr_lane_jump.h: the layout arithmetic and the append."""
import numpy as np

FLOATS = ("rebuffer_time", "start_up_time", "average_latency", "variance", "qoe")
INTS = ("episode", "trace_id", "start_offset", "chunks", "done")


def up256(b):
    return -(-int(b) // 256) * 256


def layout(n_lanes, rows):
    """Byte offsets (count, total, rec_f64, rec_i32) and the size of the blob."""
    o_total = up256(4 * n_lanes)
    o_f = o_total + up256(5 * 8 * n_lanes)
    o_i = o_f + up256(rows * 5 * 8 * n_lanes)
    return 0, o_total, o_f, o_i, o_i + up256(rows * 5 * 4 * n_lanes)


class TwinLedger:
    def __init__(self, n_lanes, rows):
        self.n, self.rows = int(n_lanes), int(rows)
        self.o = layout(self.n, self.rows)
        self.blob = np.zeros(self.o[4], np.uint8)
        n, r = self.n, self.rows
        self.count = self.blob[0:4 * n].view(np.int32)
        self.total = self.blob[self.o[1]:self.o[1] + 40 * n].view(np.float64).reshape(5, n)
        self.rf = self.blob[self.o[2]:self.o[2] + 40 * n * r].view(np.float64).reshape(r, 5, n)
        self.ri = self.blob[self.o[3]:self.o[3] + 20 * n * r].view(np.int32).reshape(r, 5, n)

    def append(self, lane, w, rb, su, lat, var, ints):
        """w = (wr, wv, ws, wl); ints = (episode, trace id, start offset, chunks, done byte)."""
        rb, su, lat, var = (np.float64(x) for x in (rb, su, lat, var))
        wr, wv, ws, wl = (np.float64(x) for x in w)
        qoe = ((wr * rb + wv * var) + ws * su) + wl * lat
        slot = int(self.count[lane]) % self.rows
        for q, x in enumerate((rb, su, lat, var, qoe)):
            self.total[q, lane] = self.total[q, lane] + x
            self.rf[slot, q, lane] = x
        for q, x in enumerate(ints):
            self.ri[slot, q, lane] = x
        self.count[lane] += 1
