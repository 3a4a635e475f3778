// CPU harness for RobustMPC's throughput estimate (abr_lane_jump.h: robust_estimate): the same source the predictor kernel
// compiles for gfx950, built on the host with -ffp-contract=off by tests/test_robust_mpc_cpu.py and compared there with
// the numpy twin (tests/robust_twin.py).
#include <stdint.h>
#include "abr_lane_jump.h"

extern "C" {

// n cases; case i: window W[i], chunk c[i], history h[i][0..c) (row stride hmax), state cs1[i] / cnt[i] / ps[i] /
// err[i][0..16) updated in place.  P_out[i] = the estimate (0.0: no decision).
void rh_robust(int64_t n, const int32_t *W, const int32_t *c, const double *h, int32_t hmax, int32_t *cs1, int32_t *cnt,
               double *ps, double *err, double *P_out) {
    for (int64_t i = 0; i < n; i++) {
        const double *hi = h + i * hmax;
        double *ei = err + i * 16;
        const auto hf = [&](int32_t j) { return hi[j]; };
        const auto ef = [&](int32_t k) -> double & { return ei[k]; };
        P_out[i] = abrx::robust_estimate(W[i], c[i], hf, cs1[i], cnt[i], ps[i], ef);
    }
}

}
