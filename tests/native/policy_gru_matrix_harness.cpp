// CPU harness for the matrix engine of the recurrent policy (abr_lane_jump.h: gru_mx_*): the index helpers
// policy_gru_mx_kernel compiles for gfx950, and a whole decision run through them on an emulation of
// v_mfma_f32_32x32x2_f32 built from the mx_* maps (per output element std::fmaf over the instruction's k in order, as
// tests/native/policy_matrix_harness.cpp emulates it) -- wave by wave, column tile by column tile, unit tile by unit
// tile, the way the kernel does: staged operands, groups of steps, gates on accumulator registers, h' folded into the
// output accumulator.  tests/test_policy_gru_matrix_cpu.py compares it with the numpy twin.  This pins the indexing, not
// the hardware's accumulation order (tests/test_policy_gru_matrix_gpu.py does that).
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

// one chain, a group of kGruMxGroup steps at a time: every step of a group that has begun is issued, on the staged row
// it finds (a pad row past the chain's last step) against b[l][s] (+0 there)
template <int MAXS>
static void chain(const float *staged, int32_t row0, int32_t steps, const float (*b)[MAXS], float (*acc)[kMxRegs]) {
    for (int g = 0; g < MAXS / kGruMxGroup; g++) {
        if (g * kGruMxGroup >= steps) continue;
        for (int j = 0; j < kGruMxGroup; j++) {
            const int s = g * kGruMxGroup + j;
            float a[kMxWave], bb[kMxWave];
            for (int l = 0; l < kMxWave; l++) { a[l] = staged[(row0 + s) * kMxWave + l]; bb[l] = b[l][s]; }
            mfma_32x32x2(a, bb, acc);
        }
    }
}

constexpr int kHSteps = kGruMxMaxHidden / 2, kXSteps = (kPolicyMaxF / 2 + kGruMxGroup - 1) / kGruMxGroup * kGruMxGroup;

extern "C" {

// kind 0: gru_mx_tiles(H); 1: gru_mx_chain_rows(a); 2: gru_mx_gate_rows(F, H); 3: gru_mx_rows(F, H);
// 4: gru_mx_ih_row(F, H, g); 5: gru_mx_hh_row(F, H, g); 6: gru_mx_out_row(F, H); 7: gru_mx_score_offset(F, H)
int32_t pgm_index(int32_t kind, int32_t F, int32_t H, int32_t g) {
    switch (kind) {
    case 0: return gru_mx_tiles(H);
    case 1: return gru_mx_chain_rows(F);
    case 2: return gru_mx_gate_rows(F, H);
    case 3: return gru_mx_rows(F, H);
    case 4: return gru_mx_ih_row(F, H, g);
    case 5: return gru_mx_hh_row(F, H, g);
    case 6: return gru_mx_out_row(F, H);
    default: return gru_mx_score_offset(F, H);
    }
}

int32_t pgm_lds_floats(int32_t F, int32_t H, int32_t M, int32_t sampled, int32_t block) {
    return gru_mx_lds_floats(F, H, M, sampled != 0, block);
}

// unit tile U's staged operands, [gru_mx_rows][64]
void pgm_staged(int32_t W, int32_t H, int32_t M, const float *weights, const float *head, int32_t U, float *out) {
    const int32_t F = 4 + W + M;
    const GruMx y = gru_mx(weights, head, F, H, M);
    for (int32_t q = 0; q < gru_mx_rows(F, H); q++)
        for (int l = 0; l < kMxWave; l++) out[q * kMxWave + l] = gru_mx_staged_at(y, U, q, l);
}

// n decisions, wave by wave: features x [n][F], h_in [n][H] -> h' [n][H], scores [n][M], value [n] (head given)
void pgm_forward(int64_t n, int32_t W, int32_t H, int32_t M, const float *weights, const float *head, const float *x_in,
                 const float *h_in, float *hp_out, float *s_out, float *v_out) {
    const int32_t F = 4 + W + M;
    const GruMx y = gru_mx(weights, head, F, H, M);
    const int32_t tiles = gru_mx_tiles(H), rows = gru_mx_rows(F, H), sF = mx_steps(F), sH = mx_steps(H);
    std::vector<float> staged((size_t)rows * kMxWave);
    for (int64_t base = 0; base < n; base += kMxWave) {
        for (int t = 0; t < 2; t++) {
            // this column tile's B registers: input 2 s + (l >> 5) of env lane 32 t + (l & 31); +0 past F, H and n
            static float xb[kMxWave][kXSteps], h[kMxWave][kHSteps];
            for (int l = 0; l < kMxWave; l++) {
                const int64_t col = base + kMxTile * t + mx_b_col(l);
                for (int s = 0; s < kXSteps; s++) {
                    const int k = 2 * s + mx_b_k(l);
                    xb[l][s] = col < n && k < F ? x_in[col * F + k] : 0.0f;
                }
                for (int s = 0; s < kHSteps; s++) {
                    const int k = 2 * s + mx_b_k(l);
                    h[l][s] = col < n && k < H ? h_in[col * H + k] : 0.0f;
                }
            }
            float out[kMxWave][kMxRegs];
            for (int l = 0; l < kMxWave; l++)
                for (int r = 0; r < kMxRegs; r++) out[l][r] = gru_mx_b_out(y, mx_acc_unit(l, r));
            for (int32_t U = 0; U < tiles; U++) {
                for (int32_t q = 0; q < rows; q++)
                    for (int l = 0; l < kMxWave; l++) staged[(size_t)q * kMxWave + l] = gru_mx_staged_at(y, U, q, l);
                const int32_t j0 = kMxTile * U;
                float rz[2][kMxWave][kMxRegs], hp[kMxWave][kMxRegs];
                for (int g = 0; g < 3; g++) {
                    float gi[kMxWave][kMxRegs], gh[kMxWave][kMxRegs];
                    for (int l = 0; l < kMxWave; l++)
                        for (int r = 0; r < kMxRegs; r++) {
                            gi[l][r] = gru_mx_b_ih(y, g, j0 + mx_acc_unit(l, r));
                            gh[l][r] = gru_mx_b_hh(y, g, j0 + mx_acc_unit(l, r));
                        }
                    chain<kXSteps>(staged.data(), gru_mx_ih_row(F, H, g), sF, xb, gi);
                    chain<kHSteps>(staged.data(), gru_mx_hh_row(F, H, g), sH, h, gh);
                    for (int l = 0; l < kMxWave; l++)
                        for (int r = 0; r < kMxRegs; r++) {
                            if (g < 2) rz[g][l][r] = gru_mx_gate(gi[l][r], gh[l][r]);
                            else hp[l][r] = gru_mx_unit(rz[0][l][r], rz[1][l][r], gi[l][r], gh[l][r], h[l][kMxRegs * U + r],
                                                        j0 + mx_acc_unit(l, r) < H);
                        }
                }
                // the commit: register r of lane l is unit j0 + mx_acc_unit(l, r) of env lane 32 t + (l & 31)
                for (int l = 0; l < kMxWave; l++) {
                    const int64_t col = base + kMxTile * t + mx_d_col(l);
                    for (int r = 0; r < kMxRegs; r++) {
                        const int32_t j = j0 + mx_acc_unit(l, r);
                        if (col < n && j < H) hp_out[col * H + j] = hp[l][r];
                    }
                }
                // h' as it stands is the B operand of output steps 16 U .. 16 U + 15
                for (int s = 0; s < kMxRegs; s++) {
                    float a[kMxWave], bb[kMxWave];
                    for (int l = 0; l < kMxWave; l++) {
                        a[l] = staged[(size_t)(gru_mx_out_row(F, H) + s) * kMxWave + l];
                        bb[l] = hp[l][s];
                    }
                    mfma_32x32x2(a, bb, out);
                }
            }
            for (int j = 0; j < kMxTile; j++) {
                const int64_t i = base + kMxTile * t + j;
                if (i >= n) continue;
                for (int u = 0; u < M; u++) s_out[i * M + u] = out[j + kMxTile * mx_unit_half(u)][mx_unit_reg(u)];
                if (head) v_out[i] = out[j + kMxTile * mx_unit_half(kMxValueUnit)][mx_unit_reg(kMxValueUnit)];
            }
        }
    }
}

}
