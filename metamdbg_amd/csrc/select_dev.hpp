// select_dev.hpp -- the rules of the per-position selection (select.hip) that are plain arithmetic, for the device and for a host program
// (tests/host/test_select.cpp): the key the candidates of a query are ranked by, the step of a position's counter, the score of a match
// list, where a record of the alignment file starts.  The semantics are ReadMapper's (readSelection/ReadMapper.hpp): addAlignmentScore
// (:1233-1313) with AlignmentScoreComparator (:90-97), mergeAlignmentScore (:365-443), writeAlignments (:1391-1410).
//
// The reference keeps, per query position, a heap of `coverage` entries whose top is the lowest score and, among equal scores, the largest
// read index; a candidate replaces the top unless its score is lower, or equal with a larger read index.  Candidates arrive in ascending
// read index, so a tie never replaces, and the heap a position ends with is the first `coverage` of its candidates under the total order
// (score descending, read index ascending).  Walked in that order, a candidate is among them exactly when the position has been taken
// fewer than `coverage` times before it: one counter a position, no heap.
#pragma once
#include <cstdint>

namespace mdbg {

constexpr uint32_t SELECT_LDS_POSITIONS = 8192;      // positions of a query whose counters fit a wave's share of LDS (8 KB a wave, 32 KB a block)
constexpr uint32_t SELECT_MAX_COVERAGE = 255;        // a counter is one byte

// int32 -> uint32, order turned round: the largest score gets the smallest word
__host__ __device__ __forceinline__ uint32_t select_rank_word(int32_t score) { return ~((uint32_t)score ^ 0x80000000u); }
// The rank key: the query in the high half, so one stable sort ranks every query's candidates at once; equal keys keep the order they
// were made in, which is ascending read index.
__host__ __device__ __forceinline__ uint64_t select_rank_key(uint32_t query, int32_t score) { return ((uint64_t)query << 32) | select_rank_word(score); }

// The counter step: a position that was taken `count` times takes the candidate while count < coverage, and then stands at count + 1.
// coverage <= 255, so a counter never leaves its byte: it stops at coverage.
__host__ __device__ __forceinline__ bool select_takes(uint32_t count, uint32_t coverage) { return count < coverage; }

// The score of a match list of n strictly ascending query indexes first ... last (mergeAlignmentScore, :376-382): one a match, minus the
// indexes skipped between two matches: 2 n - (last - first + 1).  It equals n_matches - n_diff_query of the chain (:1031 / :1037, :1241).
__host__ __device__ __forceinline__ int32_t select_list_score(uint32_t n, uint32_t first, uint32_t last) {
    return (int32_t)(2 * (int64_t)n - ((int64_t)last - (int64_t)first + 1));
}

// Byte at which the record of a query starts in the alignment file (writeAlignments: u32 read, u32 n, u32 ref_read[n]; queries without a
// selected row write nothing): 8 bytes for every non-empty query before it and 4 for every row before its own.
__host__ __device__ __forceinline__ uint64_t select_record_start(uint64_t nonempty_before, uint64_t rows_before) { return 8u * nonempty_before + 4u * rows_before; }

}  // namespace mdbg
