// CPU harness for the recurrent policy (abr_lane_jump.h: sig_c, tanh_c, policy_gru_layout, policy_gru_padded,
// policy_gru_forward): the same source policy_gru_kernel compiles for gfx950, built on the host with -ffp-contract=off by
// tests/test_policy_gru_cpu.py and compared there with the numpy twin (tests/policy_gru_twin.py).
#include <stdint.h>
#include <vector>
#include "abr_lane_jump.h"

extern "C" {

void pg_sig(int64_t n, const float *x, float *out) {
    for (int64_t i = 0; i < n; i++) out[i] = abrx::sig_c(x[i]);
}

void pg_tanh(int64_t n, const float *x, float *out) {
    for (int64_t i = 0; i < n; i++) out[i] = abrx::tanh_c(x[i]);
}

int32_t pg_layout_total(int32_t W, int32_t H, int32_t M, int32_t value) {
    abrx::PolicyNet nt{};
    nt.window = W; nt.n_hidden = 1; nt.w0 = H; nt.M = M; nt.F = 4 + W + M;
    return value ? abrx::policy_gru_layout<true>(nt).total : abrx::policy_gru_layout(nt).total;
}

// the padded layout itself, for the test that every slot is a blob entry or a pad of the right sign
void pg_padded(int32_t W, int32_t H, int32_t M, const float *weights, const float *head, float *out) {
    abrx::PolicyNet nt{};
    nt.window = W; nt.n_hidden = 1; nt.w0 = H; nt.M = M; nt.F = 4 + W + M;
    if (head) {
        const abrx::PolicyGruLayout L = abrx::policy_gru_layout<true>(nt);
        for (int32_t d = 0; d < L.total; d++) out[d] = abrx::policy_gru_padded<true>(nt, L, weights, d, head);
    } else {
        const abrx::PolicyGruLayout L = abrx::policy_gru_layout(nt);
        for (int32_t d = 0; d < L.total; d++) out[d] = abrx::policy_gru_padded(nt, L, weights, d);
    }
}

// n forward passes: features x [n][F], h_in [n][H] -> h' [n][H], scores [n][M], first argmax g [n], value [n] (head given)
void pg_forward(int64_t n, int32_t W, int32_t H, int32_t M, const float *weights, const float *head, const float *x_in,
                const float *h_in, float *hp_out, float *s_out, int32_t *g_out, float *v_out) {
    abrx::PolicyNet nt{};
    nt.window = W; nt.n_hidden = 1; nt.w0 = H; nt.M = M; nt.F = 4 + W + M;
    std::vector<float> wp;
    if (head) {
        const abrx::PolicyGruLayout L = abrx::policy_gru_layout<true>(nt);
        wp.resize(L.total);
        for (int32_t d = 0; d < L.total; d++) wp[d] = abrx::policy_gru_padded<true>(nt, L, weights, d, head);
    } else {
        const abrx::PolicyGruLayout L = abrx::policy_gru_layout(nt);
        wp.resize(L.total);
        for (int32_t d = 0; d < L.total; d++) wp[d] = abrx::policy_gru_padded(nt, L, weights, d);
    }
    for (int64_t i = 0; i < n; i++) {
        float x[abrx::kPolicyMaxF] = {}, h[abrx::kPolicyRowH] = {};
        for (int32_t f = 0; f < nt.F; f++) x[f] = x_in[i * nt.F + f];
        for (int32_t k = 0; k < H; k++) h[k] = h_in[i * H + k];
        float *hp = hp_out + i * H, *so = s_out + i * M;
        const auto hin = [&](int32_t j) { return h_in[i * H + j]; };
        const auto store = [&](int32_t j, float v) { hp[j] = v; };
        const auto emit = [&](int32_t m, float v) { so[m] = v; };
        float value = 0.0f;
        if (head) g_out[i] = abrx::policy_gru_forward<true>(nt, wp.data(), x, h, hin, store, emit, &value);
        else g_out[i] = abrx::policy_gru_forward(nt, wp.data(), x, h, hin, store, emit);
        if (v_out) v_out[i] = value;
    }
}

}
