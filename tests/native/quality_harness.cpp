// CPU harness for the quality model (abr_lane_jump.h: quality_layout, quality_step, quality_close, quality_reset): the same
// source the environment kernels compile for gfx950, built on the host by tests/test_quality_cpu.py and compared there with
// the numpy twin.
#include <stdint.h>
#include "abr_lane_jump.h"

extern "C" {

int qh_quality_size(void) { return (int)sizeof(abrx::EpisodeQuality); }

// offsets of the five regions and the blob's size: out[6]
void qh_layout(int64_t n_lanes, int32_t rows, uint64_t *out) {
    const abrx::QualityLayout lo = abrx::quality_layout(n_lanes, rows);
    out[0] = lo.count; out[1] = lo.q_run; out[2] = lo.q_last; out[3] = lo.total_q; out[4] = lo.rec_q; out[5] = lo.bytes;
}

// n events in order.  kind[e]: 0 a step of lane[e] that completed the download of chunk[e] at rate action[e], whose reward
// without a model is rew[e] -- replaced by the reward with it; 1 a step without a completed download (nothing is called:
// rew[e] keeps every bit); 2 the lane's episode ends without a re-arm; 3 ... with one; 4 a reset of the lane.
void qh_run(void *blob, int64_t n_lanes, int32_t rows, int32_t n_rates, double wq, const double *u, int64_t n,
            const int32_t *kind, const int64_t *lane, const int32_t *chunk, const int32_t *action, double *rew) {
    abrx::EpisodeQuality Q{};
    Q.wq = wq; Q.u = u; Q.base = blob; Q.rows = rows;
    for (int64_t e = 0; e < n; e++) {
        if (kind[e] == 0) rew[e] = rew[e] - abrx::quality_step(Q, n_lanes, n_rates, lane[e], chunk[e], action[e]);
        else if (kind[e] == 1) rew[e] = rew[e] - 0.0;           // what the kernels do at such a step
        else if (kind[e] == 2 || kind[e] == 3) abrx::quality_close(Q, n_lanes, lane[e], kind[e] == 3);
        else if (kind[e] == 4) abrx::quality_reset(Q, n_lanes, lane[e]);
    }
}

}
