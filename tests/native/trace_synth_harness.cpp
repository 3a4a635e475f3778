// CPU harness for the trace generator (abr_lane_jump.h: trace_map, trace_compose, trace_apply, trace_initial, trace_value):
// the same source trace_synth_kernel compiles for gfx950, built on the host by tests/test_trace_synth_cpu.py and compared
// there with the numpy twin -- as a sequential chain, and as a host emulation of the kernel's tiled wave scan.
#include <stdint.h>
#include <string.h>
#include "abr_lane_jump.h"

extern "C" {

int th_model_size(void) { return (int)sizeof(abrx::TraceModel); }
uint32_t th_identity(void) { return abrx::kTraceIdentity; }

// model: the 776 bytes of abr_trace_model
static abrx::TraceModel load(const void *model) {
    abrx::TraceModel m;
    memcpy(&m, model, sizeof(m));
    return m;
}

uint32_t th_map(const void *model, uint32_t w0) { return abrx::trace_map(load(model), w0); }
uint32_t th_compose(uint32_t g, uint32_t f) { return abrx::trace_compose(g, f); }
uint32_t th_apply(uint32_t F, uint32_t s) { return abrx::trace_apply(F, s); }
uint32_t th_initial(const void *model, uint32_t w0) { return abrx::trace_initial(load(model), w0); }
double th_value(const void *model, uint32_t s, uint32_t w1, uint32_t w2) { return abrx::trace_value(load(model), s, w1, w2); }

// one trace, sample after sample: s_i = map_i(s_(i-1))
void th_chain(const void *model, uint64_t seed, uint32_t generation, uint64_t g, int32_t len, double *out, int32_t *state_out) {
    const abrx::TraceModel m = load(model);
    const uint64_t key = seed ^ abrx::kTraceKey;
    uint32_t w[4];
    abrx::philox4(key, g, abrx::kTraceInitStep, generation, w);
    uint32_t s = abrx::trace_initial(m, w[0]);
    for (int32_t i = 0; i < len; i++) {
        abrx::philox4(key, g, (uint32_t)i, generation, w);
        s = abrx::trace_apply(abrx::trace_map(m, w[0]), s);
        out[i] = abrx::trace_value(m, s, w[1], w[2]);
        if (state_out) state_out[i] = (int32_t)s;
    }
}

// the kernel's walk of one trace on 64-lane arrays: tiles of 64 samples, identity maps past the end, an inclusive
// Hillis-Steele scan by composition over distances 1, 2, 4, 8, 16, 32 (every lane reads the previous round's value of lane
// l - d, as __shfl_up hands it over), the carry into the next tile from lane 63
void th_scan(const void *model, uint64_t seed, uint32_t generation, uint64_t g, int32_t len, double *out, int32_t *state_out) {
    const abrx::TraceModel m = load(model);
    const uint64_t key = seed ^ abrx::kTraceKey;
    uint32_t w[64][4], F[64], up[64], s[64];
    abrx::philox4(key, g, abrx::kTraceInitStep, generation, w[0]);
    uint32_t carry = abrx::trace_initial(m, w[0][0]);
    for (int32_t base = 0; base < len; base += 64) {
        for (int l = 0; l < 64; l++) {
            const int32_t i = base + l;
            abrx::philox4(key, g, (uint32_t)i, generation, w[l]);
            F[l] = i < len ? abrx::trace_map(m, w[l][0]) : abrx::kTraceIdentity;
        }
        for (int d = 1; d < 64; d <<= 1) {
            for (int l = 0; l < 64; l++) up[l] = l >= d ? F[l - d] : F[l];
            for (int l = 0; l < 64; l++) F[l] = l >= d ? abrx::trace_compose(F[l], up[l]) : F[l];
        }
        for (int l = 0; l < 64; l++) {
            const int32_t i = base + l;
            s[l] = abrx::trace_apply(F[l], carry);
            if (i < len) {
                out[i] = abrx::trace_value(m, s[l], w[l][1], w[l][2]);
                if (state_out) state_out[i] = (int32_t)s[l];
            }
        }
        carry = s[63];
    }
}

}
