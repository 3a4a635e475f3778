// CPU harness for the actor-critic additions (abr_lane_jump.h: policy_layout / policy_padded / policy_forward with VALUE,
// gae_lane): the same source policy_select_kernel<*, true> and gae_kernel compile for gfx950, built on the host with
// -ffp-contract=off (std::fmaf) by tests/test_actor_critic_cpu.py and compared there with tests/actor_critic_twin.py.
#include <stdint.h>
#include <vector>
#include "abr_lane_jump.h"

extern "C" {

static abrx::PolicyNet net(int32_t W, int32_t n_hidden, int32_t w0, int32_t w1, int32_t M) {
    abrx::PolicyNet n{};
    n.window = W; n.n_hidden = n_hidden; n.w0 = w0; n.w1 = w1; n.M = M; n.F = 4 + W + M;
    return n;
}

// the forward pass on given features x [n][F], with the value head (head [in + 1]) and without it: scores [n][M], g [n],
// value [n] of the VALUE build; scores0 [n][M], g0 [n] of the build without.  Returns the VALUE layout's size in floats.
int32_t ac_forward(int64_t n, int32_t W, int32_t n_hidden, int32_t w0, int32_t w1, int32_t M, const float *weights,
                   const float *head, const float *x_in, float *s_out, int32_t *g_out, float *v_out, float *s0_out,
                   int32_t *g0_out) {
    const abrx::PolicyNet nt = net(W, n_hidden, w0, w1, M);
    const abrx::PolicyLayout Lv = abrx::policy_layout<true>(nt), L0 = abrx::policy_layout(nt);
    std::vector<float> wv(Lv.total), wp(L0.total);
    for (int32_t d = 0; d < Lv.total; d++) wv[d] = abrx::policy_padded<true>(nt, Lv, weights, d, head);
    for (int32_t d = 0; d < L0.total; d++) wp[d] = abrx::policy_padded(nt, L0, weights, d);
    for (int64_t i = 0; i < n; i++) {
        float x[abrx::kPolicyMaxF] = {};
        for (int32_t f = 0; f < nt.F; f++) x[f] = x_in[i * nt.F + f];
        float *so = s_out + i * M, *s0 = s0_out + i * M;
        const auto emit = [&](int32_t m, float v) { so[m] = v; };
        const auto emit0 = [&](int32_t m, float v) { s0[m] = v; };
        g_out[i] = abrx::policy_forward<true>(nt, wv.data(), x, emit, &v_out[i]);
        g0_out[i] = abrx::policy_forward(nt, wp.data(), x, emit0);
    }
    return Lv.total;
}

// gae_lane on slabs [T][N] (row stride N), one lane after the other, in blocks of `rows` rows (1, 3 or 8: the result may
// not depend on it); actions may be NULL
void ac_gae(int32_t T, int64_t N, int32_t rows, const float *reward, const float *values, const float *last_value,
            const uint8_t *done, const int32_t *actions, float gamma, float lam, float *adv, float *ret) {
    for (int64_t i = 0; i < N; i++) {
        const auto rew = [&](int32_t t) { return reward[(int64_t)t * N + i]; };
        const auto val = [&](int32_t t) { return values[(int64_t)t * N + i]; };
        const auto term = [&](int32_t t) { return done[(int64_t)t * N + i] != 0; };
        const auto dead = [&](int32_t t) { return actions && actions[(int64_t)t * N + i] < 0; };
        const auto out = [&](int32_t t, float a, float r) { adv[(int64_t)t * N + i] = a; ret[(int64_t)t * N + i] = r; };
        if (rows == 1) abrx::gae_lane<1>(T, gamma, lam, last_value[i], rew, val, term, dead, out);
        else if (rows == 3) abrx::gae_lane<3>(T, gamma, lam, last_value[i], rew, val, term, dead, out);
        else abrx::gae_lane<8>(T, gamma, lam, last_value[i], rew, val, term, dead, out);
    }
}

}
