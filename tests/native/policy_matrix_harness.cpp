// CPU harness for the matrix engine of the learned policy (abr_lane_jump.h: mx_*): the index maps policy_mx_kernel
// compiles for gfx950, and an emulation of v_mfma_f32_32x32x2_f32 built from those maps -- per output element std::fmaf
// over the instruction's k in order -- that packs A and B and unpacks D through them over a whole layer chain, the way
// the kernel does.  tests/test_policy_matrix_cpu.py compares it with the numpy twin.  This pins the indexing, not the
// hardware's accumulation order (tests/test_policy_matrix_gpu.py does that).
#include <math.h>
#include <stdint.h>
#include <vector>
#include "abr_lane_jump.h"

using namespace abrx;

// one instruction on a wave: a[l], b[l] the lanes' operand registers, acc[l][r] their accumulators (C in, D out)
static void mfma_32x32x2(const float *a, const float *b, float (*acc)[kMxRegs]) {
    float A[32][2], B[2][32];
    for (int l = 0; l < kMxWave; l++) {
        A[mx_a_row(l)][mx_a_k(l)] = a[l];
        B[mx_b_k(l)][mx_b_col(l)] = b[l];
    }
    for (int l = 0; l < kMxWave; l++)
        for (int r = 0; r < kMxRegs; r++) {
            const int i = mx_d_row(l, r), j = mx_d_col(l);
            float c = acc[l][r];
            for (int k = 0; k < 2; k++) c = fmaf(A[i][k], B[k][j], c);
            acc[l][r] = c;
        }
}

// one layer on one column tile of one wave: b[l][s] the B registers; acc[T][l][r]
static void run_layer(const MxLayer &y, float (*b)[kMxMaxWidth / 2], std::vector<float> &acc) {
    const int tiles = mx_tiles(y), steps = mx_steps(y.in);
    std::vector<float> staged(mx_staged_floats(y));
    for (int32_t d = 0; d < (int32_t)staged.size(); d++) staged[d] = mx_staged(y, d);
    acc.assign((size_t)tiles * kMxWave * kMxRegs, 0.0f);
    for (int T = 0; T < tiles; T++) {
        float(*at)[kMxRegs] = reinterpret_cast<float(*)[kMxRegs]>(acc.data() + (size_t)T * kMxWave * kMxRegs);
        for (int l = 0; l < kMxWave; l++)
            for (int r = 0; r < kMxRegs; r++) at[l][r] = mx_bias(y, kMxTile * T + mx_acc_unit(l, r));
        for (int s = 0; s < steps; s++) {
            float a[kMxWave], bb[kMxWave];
            for (int l = 0; l < kMxWave; l++) { a[l] = staged[(T * steps + s) * kMxWave + l]; bb[l] = b[l][s]; }
            mfma_32x32x2(a, bb, at);
        }
    }
}

extern "C" {

// kind 0: mx_unit_row(a); 1: mx_row_unit(a); 2: mx_d_row(a, b); 3: mx_acc_unit(a, b); 4: mx_a_row(a); 5: mx_a_k(a);
// 6: mx_b_k(a); 7: mx_b_col(a); 8: mx_d_col(a); 9: mx_unit_reg(a); 10: mx_unit_half(a)
int32_t pm_index(int32_t kind, int32_t a, int32_t b) {
    switch (kind) {
    case 0: return mx_unit_row(a);
    case 1: return mx_row_unit(a);
    case 2: return mx_d_row(a, b);
    case 3: return mx_acc_unit(a, b);
    case 4: return mx_a_row(a);
    case 5: return mx_a_k(a);
    case 6: return mx_b_k(a);
    case 7: return mx_b_col(a);
    case 8: return mx_d_col(a);
    case 9: return mx_unit_reg(a);
    default: return mx_unit_half(a);
    }
}

int32_t pm_lds_floats(int32_t F, int32_t M, int32_t n_hidden, const int32_t *w, int32_t sampled, int32_t block) {
    return mx_lds_floats(F, M, n_hidden, w, sampled != 0, block);
}

int32_t pm_score_offset(int32_t F, int32_t n_hidden, const int32_t *w) { return mx_score_offset(F, n_hidden, w); }

// the forward pass of n env lanes, wave by wave: x_in [n][F] -> scores [n][M], value [n] (head nullable)
void pm_forward(int64_t n, int32_t F, int32_t M, int32_t n_hidden, const int32_t *w, const float *blob, const float *head,
                const float *x_in, float *s_out, float *v_out) {
    for (int64_t base = 0; base < n; base += kMxWave) {
        float x[kMxWave][kPolicyMaxF] = {};
        for (int l = 0; l < kMxWave && base + l < n; l++)
            for (int f = 0; f < F; f++) x[l][f] = x_in[(base + l) * F + f];
        for (int t = 0; t < 2; t++) {
            // the first layer's B registers: input 2 s + (l >> 5) of env lane 32 t + (l & 31)
            static float h[kMxWave][kMxMaxWidth / 2];
            for (int l = 0; l < kMxWave; l++)
                for (int s = 0; s < kPolicyMaxF / 2; s++) h[l][s] = x[kMxTile * t + mx_b_col(l)][2 * s + mx_b_k(l)];
            std::vector<float> acc;
            for (int li = 0; li < n_hidden; li++) {
                const MxLayer y = mx_layer(blob, head, F, M, n_hidden, w, li);
                run_layer(y, h, acc);
                for (int T = 0; T < mx_tiles(y); T++)
                    for (int l = 0; l < kMxWave; l++)
                        for (int r = 0; r < kMxRegs; r++)
                            h[l][kMxRegs * T + r] = relu_f32(acc[((size_t)T * kMxWave + l) * kMxRegs + r]);
            }
            run_layer(mx_layer(blob, head, F, M, n_hidden, w, n_hidden), h, acc);
            // unit u of env lane 32 t + j: register mx_unit_reg(u) of wave lane j + 32 mx_unit_half(u)
            for (int j = 0; j < kMxTile; j++) {
                const int64_t i = base + kMxTile * t + j;
                if (i >= n) continue;
                for (int u = 0; u < M; u++) s_out[i * M + u] = acc[(size_t)(j + kMxTile * mx_unit_half(u)) * kMxRegs + mx_unit_reg(u)];
                if (head) v_out[i] = acc[(size_t)(j + kMxTile * mx_unit_half(kMxValueUnit)) * kMxRegs + mx_unit_reg(kMxValueUnit)];
            }
        }
    }
}

}
