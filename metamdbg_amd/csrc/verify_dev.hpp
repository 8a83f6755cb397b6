// verify_dev.hpp -- the rules of mdbg_map_verify (verify.hip) that are plain arithmetic, for the device and for a host program
// (tests/host/test_verify.cpp): which neighbour indexes a target minimizer meets, what a chain of a pair of reads leaves behind as an
// alignment summary, and whether the pair is kept.  The semantics are ReadCorrectionFunctor::filterAlignments
// (readSelection/ReadCorrection.hpp:5006-5117) and MinimizerChainer::computeChainingAlignment (readSelection/MinimizerChainer.hpp:114-705).
// The predecessor test, its score, the band and both tie rules of chainAnchors / argmaxPosition (:735-961) are ReadMapper's: mapper_dev.hpp
// (map_pred_gap, map_candidate, map_band_count, map_better_end), not restated here.
//
// Names: the TARGET is the read being corrected (the reference's referenceRead, a query of the selection), the NEIGHBOUR the other read
// (the reference's queryRead, a ref_read of the selection).  ri / qi are indexes into the target's / the neighbour's minimizers.
#pragma once
#include <cmath>
#include <cstdint>

#include "mapper_dev.hpp"

namespace mdbg {

constexpr uint32_t VERIFY_MIN_ANCHORS = 3;           // fewer anchors: no chain (:146)
constexpr uint32_t VERIFY_MIN_CHAIN = 4;             // a chain of 3 anchors or fewer is no chain (:268) -- the mapper's limit is 3
constexpr uint32_t VERIFY_TOO_LONG_FROM = MAP_CHAIN_TOO_LONG_FROM;      // integer scores equal the reference's floats below this many anchors
constexpr uint32_t VERIFY_NO_READ = 0xFFFFFFFFu;     // a global read number outside `reads`

// the number of global read `read` inside the set that holds [first, first + n), or VERIFY_NO_READ (_mReads4.find, ReadCorrection.hpp:5033)
__host__ __device__ __forceinline__ uint32_t verify_local_read(uint64_t read, uint32_t first, uint32_t n) {
    return read >= first && read - first < n ? (uint32_t)(read - first) : VERIFY_NO_READ;
}

// The neighbour's minimizers sorted by (value, index): keys[0 .. n) ascending, equal values in ascending index.  The entries of value
// `key` are one run [begin, begin + count): the neighbour indexes a target minimizer of that value meets, ascending (:5051-5069 walks the
// neighbour against a map of the target and sorts by (ref_position, query_position) afterwards, MinimizerChainer.hpp:154-159; positions
// ascend strictly inside a read, so that order is (ri, qi) -- the order in which a walk of the target against these runs produces them).
struct VerifyRun { uint32_t begin, count; };
__host__ __device__ __forceinline__ VerifyRun verify_run(const uint32_t *keys, uint32_t n, uint32_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (keys[mid] < key) lo = mid + 1u; else hi = mid;
    }
    VerifyRun r;
    r.begin = lo;
    hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (keys[mid] <= key) lo = mid + 1u; else hi = mid;
    }
    r.count = lo - r.begin;
    return r;
}

// the anchors of a pair that are chained at all: fewer than 3 is no chain (:146), VERIFY_TOO_LONG_FROM or more is refused
__host__ __device__ __forceinline__ uint32_t verify_placed_anchors(uint64_t n_anchors) {
    return n_anchors >= VERIFY_MIN_ANCHORS && n_anchors < VERIFY_TOO_LONG_FROM ? (uint32_t)n_anchors : 0u;
}

// first = the root of the chain, last = the best anchor (the chain read in ascending order, :270-274)
__host__ __device__ __forceinline__ uint32_t verify_query_reversed(uint32_t first_qi, uint32_t last_qi) { return first_qi > last_qi ? 1u : 0u; }

// Between two consecutive anchors a, b of the chain (:373-395, :424-427), in the reference's int arithmetic
struct VerifyGaps { int32_t mismatches, deletions, insertions; };
__host__ __device__ __forceinline__ void verify_gap(uint32_t a_ri, uint32_t a_qi, uint32_t b_ri, uint32_t b_qi, uint32_t reversed, VerifyGaps &g) {
    const int32_t rg = (int32_t)b_ri - (int32_t)a_ri - 1;
    const int32_t qg = reversed ? (int32_t)a_qi - (int32_t)b_qi - 1 : (int32_t)b_qi - (int32_t)a_qi - 1;
    const int32_t mis = rg < qg ? rg : qg;
    g.mismatches += mis;
    if (rg > qg) g.deletions += rg - mis; else g.insertions += qg - mis;
}

// What computeChainingAlignment leaves of a chain of n_matches anchors (:274-307, :547-569, :581-582, :614, :657-673).  tpos / qpos: the
// positions of the target's n_t / the neighbour's n_q minimizers, len_t / len_q the raw read lengths; `gaps` summed over the chain's
// consecutive anchors.  The `- 1` on the indexes is the reference's own; a chain of 4 strictly monotone anchors has last_ri >= 3, last_qi
// >= 3 when forward and first_qi >= 3 when reversed, so no index leaves its read.  Overhangs are int64 cut to 32 bits, as the field is.
struct VerifySummary {
    uint32_t query_reversed;
    int32_t n_matches, n_mismatches, n_deletions, n_insertions;
    uint32_t overhang_start, overhang_end, align_length, n_seeds, reference_start, reference_end, query_start, query_end;
};
__host__ __device__ __forceinline__ int64_t verify_min64(int64_t a, int64_t b) { return a < b ? a : b; }
// the runs of index-aligned pairs in front of the first and behind the last anchor (nbStartingMissmatches / nbEndingMissmatches, :291-306);
// mdbg_map_realign (realign_dev.hpp) emits them as entries
struct VerifyEdges { int64_t start_mis, end_mis; };
__host__ __device__ __forceinline__ VerifyEdges verify_edge_mismatches(uint32_t reversed, uint32_t first_ri, uint32_t first_qi, uint32_t last_ri, uint32_t last_qi, uint32_t n_t,
                                                                       uint32_t n_q) {
    VerifyEdges e;
    if (reversed) {
        e.start_mis = verify_min64((int64_t)first_ri, (int64_t)n_q - (int64_t)first_qi - 1);
        e.end_mis = verify_min64((int64_t)n_t - (int64_t)last_ri - 1, (int64_t)last_qi);
    } else {
        e.start_mis = verify_min64((int64_t)first_ri, (int64_t)first_qi);
        e.end_mis = verify_min64((int64_t)n_t - (int64_t)last_ri - 1, (int64_t)n_q - (int64_t)last_qi - 1);
    }
    return e;
}
__host__ __device__ __forceinline__ VerifySummary verify_summary(uint32_t n_matches, const VerifyGaps &gaps, uint32_t first_ri, uint32_t first_qi, uint32_t last_ri,
                                                                 uint32_t last_qi, const uint32_t *tpos, const uint32_t *qpos, uint32_t n_t, uint32_t n_q, uint32_t len_t,
                                                                 uint32_t len_q) {
    VerifySummary s;
    s.query_reversed = verify_query_reversed(first_qi, last_qi);
    int64_t over_start, over_end;
    if (s.query_reversed) {
        over_start = verify_min64((int64_t)tpos[first_ri], (int64_t)len_q - (int64_t)qpos[first_qi - 1u]);
        over_end = verify_min64((int64_t)len_t - (int64_t)tpos[last_ri - 1u], (int64_t)qpos[last_qi]);
    } else {
        over_start = verify_min64((int64_t)tpos[first_ri], (int64_t)qpos[first_qi]);
        over_end = verify_min64((int64_t)len_t - (int64_t)tpos[last_ri - 1u], (int64_t)len_q - (int64_t)qpos[last_qi - 1u]);
    }
    const VerifyEdges edge = verify_edge_mismatches(s.query_reversed, first_ri, first_qi, last_ri, last_qi, n_t, n_q);
    const int64_t start_mis = edge.start_mis, end_mis = edge.end_mis;
    s.n_matches = (int32_t)n_matches;
    s.n_mismatches = (int32_t)start_mis + gaps.mismatches + (int32_t)end_mis;
    s.n_deletions = gaps.deletions;
    s.n_insertions = gaps.insertions;
    s.overhang_start = (uint32_t)over_start;
    s.overhang_end = (uint32_t)over_end;
    const uint64_t ref_size = (uint64_t)((int64_t)s.n_matches + s.n_mismatches + s.n_deletions);          // :581-582
    const uint64_t query_size = (uint64_t)((int64_t)s.n_matches + s.n_mismatches + s.n_insertions);
    s.n_seeds = (uint32_t)(ref_size < query_size ? ref_size : query_size);                                  // :614
    s.align_length = tpos[last_ri] - tpos[first_ri];                                                        // alignEnd - alignStart (:418-419, :659)
    s.reference_start = tpos[first_ri];
    s.reference_end = tpos[last_ri];
    s.query_start = s.query_reversed ? qpos[last_qi] : qpos[first_qi];                                      // :664-673
    s.query_end = s.query_reversed ? qpos[first_qi] : qpos[last_qi];
    return s;
}

// Kept (ReadCorrection.hpp:5088-5094).  The identity test is a table look-up: min_matches[s] is the smallest n_matches whose identity at
// n_seeds = s passes (verify_min_matches below), table_n its length; an n_seeds the table does not reach keeps nothing.  The reference
// compares _alignLength with a float _minOverlapLength; the threshold here is a uint32_t.
__host__ __device__ __forceinline__ bool verify_kept(uint32_t overhang_start, uint32_t overhang_end, uint32_t align_length, int32_t n_matches, uint32_t n_seeds,
                                                     uint32_t max_overhang, uint32_t min_overlap_length, const uint32_t *min_matches, uint32_t table_n) {
    if (overhang_start > max_overhang) return false;
    if (overhang_end > max_overhang) return false;
    if (align_length < min_overlap_length) return false;
    if (n_seeds >= table_n) return false;
    return n_matches >= 0 && (uint32_t)n_matches >= min_matches[n_seeds];
}

// ---- host only: the identity and the table the device compares against --------------------------------------------------------------------
// _identity as computeChainingAlignment computes it (:614-630, :655): nbSeeds is a long double, the divergence a float, the identity a
// float again.
inline float verify_identity(uint32_t n_matches, uint32_t n_seeds, uint32_t minimizer_size) {
    const long double nbSeeds = (long double)n_seeds;
    float divergence = 0;
    if ((long double)n_matches == nbSeeds) divergence = 0;
    else if (n_matches == 0) divergence = 1;
    else divergence = (float)(1.0 - std::pow(((long double)n_matches / nbSeeds), (long double)(1.0 / (double)minimizer_size)));
    return (float)(1.0 - (double)divergence);
}
inline bool verify_identity_passes(uint32_t n_matches, uint32_t n_seeds, uint32_t minimizer_size, float min_identity) {
    return !(verify_identity(n_matches, n_seeds, minimizer_size) < min_identity);            // `if (identity < minIdentity) continue` (:5092)
}
// the smallest m in 0 ... s that passes, or s + 1: the identity does not fall as m grows, so a binary search finds it
inline uint32_t verify_min_matches_search(uint32_t s, uint32_t minimizer_size, float min_identity) {
    if (!verify_identity_passes(s, s, minimizer_size, min_identity)) return s + 1u;
    uint32_t lo = 0, hi = s;                    // hi passes
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (verify_identity_passes(mid, s, minimizer_size, min_identity)) hi = mid; else lo = mid + 1u;
    }
    return lo;
}
// ... and by the full scan (tests/host/test_verify.cpp holds the two equal)
inline uint32_t verify_min_matches_scan(uint32_t s, uint32_t minimizer_size, float min_identity) {
    for (uint32_t m = 0; m <= s; m++)
        if (verify_identity_passes(m, s, minimizer_size, min_identity)) return m;
    return s + 1u;
}

}  // namespace mdbg
