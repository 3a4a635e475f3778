// CPU harness for the episode ledger (abr_lane_jump.h: ledger_layout, ledger_append): the same source the environment
// kernels compile for gfx950, built on the host by tests/test_episode_ledger_cpu.py and compared there with the numpy twin.
#include <stdint.h>
#include "abr_lane_jump.h"

extern "C" {

int lh_ledger_size(void) { return (int)sizeof(abrx::EpisodeLedger); }

// offsets of the four regions and the blob's size: out[5]
void lh_layout(int64_t n_lanes, int32_t rows, uint64_t *out) {
    const abrx::LedgerLayout lo = abrx::ledger_layout(n_lanes, rows);
    out[0] = lo.count; out[1] = lo.total; out[2] = lo.rec_f64; out[3] = lo.rec_i32; out[4] = lo.bytes;
}

// n episode ends in order: lane[e], the four QoE terms f[e][4] (rebuffer, start-up, latency, variance) and the five int
// fields w[e][5] (episode, trace, offset, chunks, done); weights = (wr, wv, ws, wl)
void lh_append(void *blob, int64_t n_lanes, int32_t rows, const double *weights, int64_t n, const int64_t *lane,
               const double *f, const int32_t *w) {
    abrx::EpisodeLedger L{};
    L.base = blob; L.rows = rows;
    for (int64_t e = 0; e < n; e++)
        abrx::ledger_append(L, n_lanes, lane[e], weights[0], weights[1], weights[2], weights[3], f[4 * e], f[4 * e + 1],
                            f[4 * e + 2], f[4 * e + 3], w[5 * e], w[5 * e + 1], w[5 * e + 2], w[5 * e + 3], w[5 * e + 4]);
}

}
