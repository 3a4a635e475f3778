// CPU harness for the lane fork and the beam selection (abr_lane_jump.h: ForkTable, fork_table_init, fork_pair_ok,
// fork_move; beam_r_new, beam_key, beam_valid, beam_before): the same source the kernels compile for gfx950, built on the
// host by tests/test_fork_cpu.py and compared there with the numpy twin (tests/fork_twin.py).
#include <stdint.h>
#include <vector>
#include "abr_lane_jump.h"

extern "C" {

int fh_regions(void) { return abrx::kForkRegions; }
int fh_rows_per_thread(void) { return abrx::kForkRowsPerThread; }

// elem[10], rows[10], scratch offsets[10]; returns the scratch bytes; *chunks_out the y extent of a launch
uint64_t fh_table(int32_t V, int64_t n_lanes, int64_t count, int32_t *elem, int32_t *rows, int64_t *scratch, int32_t *chunks_out) {
    abrx::ForkTable T;
    const size_t b = abrx::fork_table_init(T, V, n_lanes, count);
    for (int id = 0; id < abrx::kForkRegions; id++) { elem[id] = T.r[id].elem; rows[id] = T.r[id].rows; scratch[id] = T.r[id].scratch; }
    *chunks_out = T.chunks;
    return (uint64_t)b;
}

int fh_pair_ok(int64_t s, int64_t d, int64_t n_lanes) { return abrx::fork_pair_ok(s, d, n_lanes) ? 1 : 0; }

// The fork as the two launches run it: every (chunk, pair) thread of the gather, then every thread of the scatter, over a
// grid rounded up to 256 pairs as the kernels' is (the threads past `count` must do nothing).  off[10]: byte offset of each
// region in `ws`, or -1 for an absent one (q_run and obs live outside the workspace: pass them inside the same array).
// dst may be NULL.  Returns the scratch bytes used.
uint64_t fh_fork(uint8_t *ws, const int64_t *off, int32_t V, int64_t n_lanes, const int32_t *src, const int32_t *dst,
                 int64_t count, uint8_t *scratch) {
    abrx::ForkTable T;
    const size_t b = abrx::fork_table_init(T, V, n_lanes, count);
    for (int id = 0; id < abrx::kForkRegions; id++) T.r[id].base = off[id] >= 0 ? (char *)ws + off[id] : nullptr;
    const int64_t threads = (count + 255) / 256 * 256;
    for (int pass = 0; pass < 2; pass++)
        for (int32_t c = 0; c < T.chunks; c++)
            for (int64_t i = 0; i < threads; i++) abrx::fork_move(T, c, i, src, dst, (char *)scratch, pass == 1);
    return (uint64_t)b;
}

// abr_beam_select's arithmetic, group by group, in the kernel's order: keys and validity, ranks by counting, outputs
void fh_select(int32_t n_groups, int32_t beam, int32_t n_rates, double wl, const double *R_in, const float *reward,
               const double *lat, const uint8_t *done, const uint8_t *valid_in, const double *key_override, int32_t *src_out,
               double *R_out, uint8_t *valid_out) {
    const int32_t S = beam * n_rates;
    std::vector<double> key(S), Rn(S);
    std::vector<uint8_t> valid(S);
    std::vector<int32_t> slot(S);
    for (int32_t g = 0; g < n_groups; g++) {
        const int64_t base = (int64_t)g * S;
        for (int32_t s = 0; s < S; s++) {
            const int64_t i = base + s;
            Rn[s] = abrx::beam_r_new(R_in[i], reward[i]);
            key[s] = key_override ? key_override[i] : abrx::beam_key(Rn[s], wl, lat[i]);
            valid[s] = abrx::beam_valid(valid_in[i], done[i], key[s]) ? 1 : 0;
            slot[s] = -1;
        }
        for (int32_t s = 0; s < S; s++) {
            if (!valid[s]) continue;
            int32_t rank = 0;
            for (int32_t t = 0; t < S; t++) rank += (valid[t] && abrx::beam_before(key[t], t, key[s], s)) ? 1 : 0;
            slot[rank] = s;
        }
        for (int32_t s = 0; s < S; s++) {
            const int32_t c = slot[s / n_rates];
            src_out[base + s] = c >= 0 ? (int32_t)(base + c) : -1;
            R_out[base + s] = c >= 0 ? Rn[c] : 0.0;
            valid_out[base + s] = c >= 0 ? 1 : 0;
        }
    }
}

}
