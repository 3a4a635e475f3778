// CPU harness for the learned policy (abr_lane_jump.h: policy_features, policy_forward, policy_explore): the same source
// policy_select_kernel compiles for gfx950, built on the host with -ffp-contract=off (std::fmaf) by
// tests/test_policy_cpu.py and compared there with the numpy twin (tests/policy_twin.py).
#include <stdint.h>
#include <vector>
#include "abr_lane_jump.h"

extern "C" {

static abrx::PolicyNet net(int32_t W, int32_t n_hidden, int32_t w0, int32_t w1, int32_t M, const double *norm,
                           uint64_t seed, uint64_t thr) {
    abrx::PolicyNet n{};
    n.window = W; n.n_hidden = n_hidden; n.w0 = w0; n.w1 = w1; n.M = M; n.F = 4 + W + M;
    n.norm = norm; n.seed = seed; n.thr = thr;
    return n;
}

// the padded layout policy_select_kernel stages in LDS, built from the packed blob by the same code
static std::vector<float> padded(const abrx::PolicyNet &n, const float *blob) {
    const abrx::PolicyLayout L = abrx::policy_layout(n);
    std::vector<float> w(L.total);
    for (int32_t d = 0; d < L.total; d++) w[d] = abrx::policy_padded(n, L, blob, d);
    return w;
}

// n lanes at call sites: chunk c[i], previous bitrate a[i], buffer B[i], G[i], P[i], history h[i][0..hmax), one
// bitrate table br [V][M] for all lanes, lane id lane[i], episode ep[i].  Outputs x [n][F], scores [n][M], g [n] (the
// argmax) and action [n] (after the exploration draw).
void ph_run(int64_t n, int32_t W, int32_t n_hidden, int32_t w0, int32_t w1, int32_t M, int32_t V, const float *weights,
            const double *norm, uint64_t seed, uint64_t thr, const int32_t *c, const int32_t *a, const double *B,
            const double *G, const double *P, const double *h, int32_t hmax, const double *br, const uint64_t *lane,
            const int32_t *ep, float *x_out, float *s_out, int32_t *g_out, int32_t *act_out) {
    const abrx::PolicyNet nt = net(W, n_hidden, w0, w1, M, norm, seed, thr);
    const std::vector<float> wp = padded(nt, weights);
    for (int64_t i = 0; i < n; i++) {
        const double *hi = h + i * hmax;
        const auto hf = [&](int32_t j) { return hi[j]; };
        const auto brf = [&](int32_t r, int32_t m) { return br[(int64_t)r * M + m]; };
        float x[abrx::kPolicyMaxF];
        abrx::policy_features(nt, hf, brf, V, c[i], a[i], B[i], G[i], P[i], x);
        for (int32_t f = 0; f < nt.F; f++) x_out[i * nt.F + f] = x[f];
        float *so = s_out + i * M;
        const auto emit = [&](int32_t m, float v) { so[m] = v; };
        g_out[i] = abrx::policy_forward(nt, wp.data(), x, emit);
        act_out[i] = abrx::policy_explore(nt, lane[i], c[i], ep[i], g_out[i]);
    }
}

// the forward pass alone on given features x [n][F]: scores [n][M], g [n]
void ph_forward(int64_t n, int32_t W, int32_t n_hidden, int32_t w0, int32_t w1, int32_t M, const float *weights,
                const float *x_in, float *s_out, int32_t *g_out) {
    const abrx::PolicyNet nt = net(W, n_hidden, w0, w1, M, nullptr, 0, 0);
    const std::vector<float> wp = padded(nt, weights);
    for (int64_t i = 0; i < n; i++) {
        float x[abrx::kPolicyMaxF] = {};
        for (int32_t f = 0; f < nt.F; f++) x[f] = x_in[i * nt.F + f];
        float *so = s_out + i * M;
        const auto emit = [&](int32_t m, float v) { so[m] = v; };
        g_out[i] = abrx::policy_forward(nt, wp.data(), x, emit);
    }
}

}
