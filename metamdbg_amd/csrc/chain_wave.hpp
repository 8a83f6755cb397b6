// chain_wave.hpp -- the banded chain dynamic programme of one pair of reads on one wave: what map_chain_kernel (mapper.hip) and
// verify_chain_kernel (verify.hip) both run between their draw and lane 0's row.  The rules are mapper_dev.hpp's
// (map_lane_best); here are the wave's max, lane 0's store and the fence that lets the next anchor's lanes read it.
#pragma once
#include "common.hpp"
#include "mapper_dev.hpp"

namespace mdbg {

// anchors of a pair whose scores and parents fit a wave's share of LDS (8 KB a wave, 32 KB a block of four waves); a longer pair's live in
// a pooled global buffer.  Also the minimizers of a neighbour whose lookup the verifier's join stages in LDS (the same 8 KB).
constexpr uint32_t CHAIN_LDS_ANCHORS = 1024;
#ifdef __HIPCC__
struct ChainEnd { int32_t score; uint32_t i; };      // the best anchor of the pair (map_better_end) and its score; {0, 0} for n == 0

// The calling wave, all 64 lanes together, chains the pair's n anchors rp / qp / rv (ascending by (rp, qp)) into score[0 .. n) and
// parent[0 .. n), the wave's own: in LDS (in_lds) or in global memory.  n == 0: not chained, nothing is read or written.  All arguments uniform.
__device__ __forceinline__ ChainEnd chain_wave(uint32_t n, const uint32_t *rp, const uint32_t *qp, const uint8_t *rv, uint32_t band, int32_t *score, uint32_t *parent,
                                               bool in_lds) {
    const uint32_t lane = lane_id();
    ChainEnd end{0, 0u};
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t best = wave_max_u64(map_lane_best(score, rp, qp, rv, i, band, lane));
        const int32_t sc = map_candidate_score(best);
        if (lane == 0) { score[i] = sc; parent[i] = map_candidate_parent(best); }
        if (in_lds) wave_lds_sync(); else __threadfence_block();         // (the next anchor's lanes read what lane 0 wrote)
        if (map_better_end(sc, end.score)) { end.score = sc; end.i = i; }
    }
    return end;
}
#endif
}  // namespace mdbg
