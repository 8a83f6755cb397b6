// verify_join.hpp -- the lookup and the join of verify.hip as mdbg_map_realign (realign.hip) launches them: the same kernels over the
// thinned set, the neighbour seen through its row's orientation.  Launches only: no host wait but the sort's.
#pragma once
#include "common.hpp"

namespace mdbg {

struct VerifyReads { const uint64_t *off; const uint32_t *mins, *pos; const uint8_t *dir; const uint32_t *len; uint32_t n_reads, first_read; };
struct VerifyAnchors { uint32_t *ri, *qi, *rpos, *qpos; uint8_t *rev; };

// keys (n_min, scratch), sorted, sorted_idx (n_min each): the set's minimizers by (read, value) and their indexes in the read
int verify_lookup(mdbg_ctx *ctx, const char *timer, const VerifyReads &rd, uint64_t n_min, uint64_t *keys, uint32_t *sorted, uint32_t *sorted_idx);
// n_anchors[row], placed[row] and *longest (zeroed by the caller) of every row; row_t / row_q: the reads' numbers in the set or VERIFY_NO_READ
void verify_join_count(mdbg_ctx *ctx, const VerifyReads &rd, const uint32_t *sorted, const uint32_t *sorted_idx, const uint32_t *row_t, const uint32_t *row_q, uint64_t n_rows,
                       uint32_t *n_anchors, uint32_t *placed, unsigned long long *longest);
// the anchors behind a_off, the neighbour of row s reverse-complemented where row_reversed[s] is set (realign_dev.hpp, the oriented view)
void verify_join_fill_oriented(mdbg_ctx *ctx, const VerifyReads &rd, const uint32_t *sorted, const uint32_t *sorted_idx, const uint32_t *row_t, const uint32_t *row_q,
                               const uint8_t *row_reversed, uint64_t n_rows, const uint64_t *a_off, const VerifyAnchors &out);

// ... and the kernel behind it, for realign.hip's list of step kernels ("realign_join_fill")
const void *verify_join_fill_oriented_kernel();

}  // namespace mdbg
