// CPU harness for the bitrate rules of abr_lane_jump.h (rule_select): the same source the kernels compile for gfx950,
// built on the host with -ffp-contract=off by tests/test_rules_cpu.py and compared there with the numpy twin.
#include <stdint.h>
#include <vector>
#include "abr_lane_jump.h"

extern "C" {

// n cases; case i: rule kind[i] with its parameters, chunk c[i], buffer B[i], M[i] rates br[i][0..M) (row stride 16),
// history h[i][0..c) (row stride hmax), utility row u[i][0..M) (row stride 16).  out[i] = rule_select's answer.
void rh_select(int64_t n, const int32_t *kind, const int32_t *window, const double *reservoir, const double *cushion,
               const double *safety, const double *bola_v, const double *bola_gp, const int32_t *c, const double *B,
               const int32_t *M, const double *br, const double *h, int32_t hmax, const double *u, int32_t *out) {
    std::vector<double> ut;
    for (int64_t i = 0; i < n; i++) {
        const double *bri = br + i * 16, *hi = h + i * hmax;
        // the rule indexes utility[c * M + m]: give it a table whose row c is this case's row
        ut.assign((size_t)(c[i] + 1) * M[i], 0.0);
        for (int32_t m = 0; m < M[i]; m++) ut[(size_t)c[i] * M[i] + m] = u[i * 16 + m];
        abrx::RuleParams r;
        r.kind = kind[i]; r.window = window[i]; r.reservoir = reservoir[i]; r.cushion = cushion[i];
        r.safety = safety[i]; r.bola_v = bola_v[i]; r.bola_gp = bola_gp[i]; r.utility = ut.data();
        const auto brf = [&](int32_t m) { return bri[m]; };
        const auto hf = [&](int32_t j) { return hi[j]; };
        out[i] = abrx::rule_select(r, brf, hf, M[i], c[i], B[i]);
    }
}

}
