// CPU harness for the episode sampler (abr_lane_jump.h: episode_assign): the same source the environment kernels compile for
// gfx950, built on the host by tests/test_episode_sampler_cpu.py and compared there with the numpy twin.
#include <stdint.h>
#include "abr_lane_jump.h"

extern "C" {

// n draws: global lane id lane[i], episode number ep[i]; trace_len [n_traces]; pool nullable [n_pool]
void eh_draw(int64_t n, uint64_t seed, const int32_t *pool, int32_t n_pool, int32_t offset_span, int32_t n_traces,
             const int32_t *trace_len, const uint64_t *lane, const uint32_t *ep, int32_t *t_out, int32_t *off_out) {
    abrx::EpisodeSampler s{};
    s.seed = seed; s.pool = pool; s.n_pool = n_pool; s.offset_span = offset_span;
    for (int64_t i = 0; i < n; i++) abrx::episode_assign(s, lane[i], ep[i], n_traces, trace_len, t_out[i], off_out[i]);
}

int eh_sampler_size(void) { return (int)sizeof(abrx::EpisodeSampler); }

}
