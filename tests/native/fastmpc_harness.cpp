// CPU harness for FastMPC's lookup (abr_lane_jump.h: fastmpc_lookup): the same source the environment kernels compile for
// gfx950, built on the host with -ffp-contract=off by tests/test_fastmpc_cpu.py and compared there with the numpy twin
// (tests/fastmpc_twin.py).
#include <stdint.h>
#include "abr_lane_jump.h"

extern "C" {

// n cases against ONE blob (entries [rows][M][nb][nq] padded to 8, then the edges), window W, V chunks, horizon H,
// uniform layout or not; case i: chunk c[i], previous bitrate pv[i], buffer B[i], history h[i][0..c) (row stride hmax).
void fh_lookup(int64_t n, const uint8_t *blob, int32_t W, int32_t M, int32_t V, int32_t H, int32_t uniform, int32_t nb,
               int32_t nq, const int32_t *c, const int32_t *pv, const double *B, const double *h, int32_t hmax,
               int32_t *out) {
    abrx::RuleParams r{};
    r.kind = abrx::kRuleFastMpc; r.window = W;
    r.fm_table = blob; r.fm_uniform = uniform; r.fm_horizon = H; r.fm_nb = nb; r.fm_nq = nq;
    for (int64_t i = 0; i < n; i++) {
        const double *hi = h + i * hmax;
        const auto hf = [&](int32_t j) { return hi[j]; };
        const auto brf = [&](int32_t) { return 0.0; };
        out[i] = abrx::rule_select_at(r, brf, hf, M, V, c[i], pv[i], B[i]);
    }
}

}
