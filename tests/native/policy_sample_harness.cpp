// CPU harness for the learned policy's sampled decision (abr_lane_jump.h: exp_c, policy_softmax_sample, policy_decide):
// the same source policy_select_kernel<true> compiles for gfx950, built on the host with -ffp-contract=off by
// tests/test_policy_sample_cpu.py and compared there with the numpy twin (tests/policy_sample_twin.py).
#include <stdint.h>
#include <vector>
#include "abr_lane_jump.h"

extern "C" {

void ps_exp(int64_t n, const float *x, float *out) {
    for (int64_t i = 0; i < n; i++) out[i] = abrx::exp_c(x[i]);
}

// n draws: scores s [n][M], argmax g [n], inv_temperature iT [n], philox word 2 w2 [n] -> pick [n], probs [n][M],
// e [n][M] (what the draw leaves in its buffer)
void ps_sample(int64_t n, int32_t M, const float *s, const int32_t *g, const float *iT, const uint32_t *w2,
               int32_t *pick_out, float *probs_out, float *e_out) {
    for (int64_t i = 0; i < n; i++) {
        float b[abrx::kPolicyMaxRates];
        for (int32_t m = 0; m < M; m++) b[m] = s[i * M + m];
        float *po = probs_out + i * M;
        const auto buf = [&](int32_t m) -> float & { return b[m]; };
        const auto prob = [&](int32_t m, float v) { po[m] = v; };
        pick_out[i] = abrx::policy_softmax_sample(M, g[i], iT[i], w2[i], buf, prob);
        for (int32_t m = 0; m < M; m++) e_out[i * M + m] = b[m];
    }
}

// the forward pass on given features x [n][F], then the decision of `mode`: scores [n][M], probs [n][M], action [n]
void ps_decide(int64_t n, int32_t W, int32_t n_hidden, int32_t w0, int32_t w1, int32_t M, const float *weights,
               uint64_t seed, uint64_t thr, int32_t mode, float iT, const float *x_in, const uint64_t *lane,
               const int32_t *c, const int32_t *ep, float *s_out, float *probs_out, int32_t *act_out) {
    abrx::PolicyNet nt{};
    nt.window = W; nt.n_hidden = n_hidden; nt.w0 = w0; nt.w1 = w1; nt.M = M; nt.F = 4 + W + M;
    nt.seed = seed; nt.thr = thr;
    const abrx::PolicyLayout L = abrx::policy_layout(nt);
    std::vector<float> wp(L.total);
    for (int32_t d = 0; d < L.total; d++) wp[d] = abrx::policy_padded(nt, L, weights, d);
    for (int64_t i = 0; i < n; i++) {
        float x[abrx::kPolicyMaxF] = {};
        for (int32_t f = 0; f < nt.F; f++) x[f] = x_in[i * nt.F + f];
        float b[abrx::kPolicyMaxRates];
        float *so = s_out + i * M, *po = probs_out + i * M;
        const auto emit = [&](int32_t m, float v) { so[m] = v; b[m] = v; };
        const int32_t g = abrx::policy_forward(nt, wp.data(), x, emit);
        const auto buf = [&](int32_t m) -> float & { return b[m]; };
        const auto prob = [&](int32_t m, float v) { po[m] = v; };
        act_out[i] = abrx::policy_decide(nt, lane[i], c[i], ep[i], g, mode, iT, buf, prob);
    }
}

}
