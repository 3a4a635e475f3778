// CPU harness for the policy population's index helpers (abr_lane_jump.h: pop_member, pop_blob_offset,
// pop_head_offset): the functions the POP instances of policy_select_kernel and policy_mx_kernel compile for gfx950,
// compiled for the host.  tests/test_policy_population_cpu.py checks them against i / group.
#include <stdint.h>
#include "abr_lane_jump.h"

extern "C" {

int64_t pp_member(int64_t block_first_lane, int32_t group) { return abrx::pop_member(block_first_lane, group); }
int64_t pp_blob_offset(int64_t member, int32_t words) { return abrx::pop_blob_offset(member, words); }
int64_t pp_head_offset(int64_t member, int32_t words) { return abrx::pop_head_offset(member, words); }

// what a workgroup does: the member and the two offsets of the 256-lane block that holds local lane i
void pp_lane(int64_t i, int32_t group, int32_t blob_words, int32_t head_words, int64_t *out) {
    const int64_t first = i / 256 * 256, m = abrx::pop_member(first, group);
    out[0] = m;
    out[1] = abrx::pop_blob_offset(m, blob_words);
    out[2] = abrx::pop_head_offset(m, head_words);
}

}
