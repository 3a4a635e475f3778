// CPU harness for the recurrent population's index helpers (abr_lane_jump.h: pop_member, pop_blob_offset,
// pop_head_offset) with the GRU blob's word count: what the POP instances of policy_gru_kernel and policy_gru_mx_kernel
// compile for gfx950, compiled for the host.  tests/test_policy_gru_population_cpu.py checks them against i / group.
#include <stdint.h>
#include "abr_lane_jump.h"

extern "C" {

// words of one member's blob (GRUCell's layout, then the head, unpadded) and of one value head
int64_t pgp_blob_words(int32_t F, int32_t H, int32_t M) { return (int64_t)3 * H * (F + H + 2) + (int64_t)M * (H + 1); }
int64_t pgp_head_words(int32_t H) { return (int64_t)H + 1; }

int64_t pgp_member(int64_t block_first_lane, int32_t group) { return abrx::pop_member(block_first_lane, group); }
int64_t pgp_blob_offset(int64_t member, int32_t words) { return abrx::pop_blob_offset(member, words); }
int64_t pgp_head_offset(int64_t member, int32_t words) { return abrx::pop_head_offset(member, words); }

// what a workgroup does: the member and the two offsets of the 256-lane block that holds local lane i, for a cell of
// H units over F features and M rates
void pgp_lane(int64_t i, int32_t group, int32_t F, int32_t H, int32_t M, int64_t *out) {
    const int64_t first = i / 256 * 256, m = abrx::pop_member(first, group);
    out[0] = m;
    out[1] = abrx::pop_blob_offset(m, (int32_t)pgp_blob_words(F, H, M));
    out[2] = abrx::pop_head_offset(m, (int32_t)pgp_head_words(H));
}

}
