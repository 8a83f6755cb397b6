// mapper_dev.hpp -- the rules of the read-against-read mapper (mapper.hip) that are plain arithmetic, for the device and for a host
// program (tests/host/test_mapper.cpp): a read's windows of two minimizers, which index entries of a pair a query window takes, whether
// an anchor may follow another in a chain and what that scores, and the two tie rules.  The semantics are ReadMapper's at k = 2
// (readSelection/ReadMapper.hpp): ReadFunctor (:465-505), AlignReadsLowDensityFunctor::operator() (:668-756), chainAnchors and
// argmaxPosition (:887-1230).
#pragma once
#include <cstdint>

namespace mdbg {

constexpr uint32_t MAP_MIN_QUERY_MINIMIZERS = 10;    // Utils::isReadTooShort (Commons.hpp:2190): a shorter QUERY produces nothing
constexpr int32_t MAP_ANCHOR_SCORE = 20;             // w of chainAnchors (:894)
constexpr int32_t MAP_MAX_GAP = 100;                 // |d_r - d_q| above this: no predecessor (:1192)
constexpr int32_t MAP_MAX_DISTANCE = 5000;           // d_q or d_r above this: no predecessor (:1181)
constexpr uint32_t MAP_MIN_CHAIN = 3;                // a chain of fewer anchors is no chain (:1013)
constexpr uint32_t MAP_NO_PARENT = 0xFFFFFFFFu;
// The reference's scores are floats: sums of 20 - gap with an integer gap <= 100, so every partial sum of a pair of n anchors is an
// integer of magnitude <= 80 n and a float holds it exactly while 80 n < 2^24.  From this many anchors on a pair is not chained.
constexpr uint32_t MAP_CHAIN_TOO_LONG_FROM = (1u << 24) / 80u;      // 209 715

// Window i of a read: its minimizers a = m[i], b = m[i + 1] at positions pa < pb.
//   reversed   KmerVec::normalize (Commons.hpp:886-916): the equal case falls through to "reversed"
//   pair       packPair (:937): the smaller minimizer in the high half
//   position   the middle of the two positions, in 32 bits as the reference takes it (positions are < 2^31: no wrap)
struct MapWindow { uint64_t pair; uint32_t position; uint32_t reversed; };
__host__ __device__ __forceinline__ MapWindow map_window(uint32_t a, uint32_t b, uint32_t pa, uint32_t pb) {
    MapWindow w;
    w.reversed = a >= b ? 1u : 0u;
    w.pair = a < b ? ((uint64_t)a << 32) | b : ((uint64_t)b << 32) | a;
    w.position = (pa + pb) / 2u;
    return w;
}

// windows of a read of n minimizers
__host__ __device__ __forceinline__ uint32_t map_read_windows(uint64_t n_minimizers) { return n_minimizers ? (uint32_t)(n_minimizers - 1u) : 0u; }

// does a read of n minimizers ask at all
__host__ __device__ __forceinline__ bool map_query_asks(uint64_t n_minimizers) { return n_minimizers >= MAP_MIN_QUERY_MINIMIZERS; }

// first entry of reads[lo, hi) (ascending) that is >= key
__host__ __device__ __forceinline__ uint32_t map_lower_bound(const uint32_t *reads, uint32_t lo, uint32_t hi, uint32_t key) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (reads[mid] < key) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// The index entries [begin, end) of one pair are in (read, window) order, so the query's own entries -- those whose global read number is
// the query's (:733) -- are one block [self_begin, self_begin + self_count).  The window takes every other entry.
struct MapRun { uint32_t begin, count, self_begin, self_count; };      // count: anchors of the window = entries - self hits
__host__ __device__ __forceinline__ MapRun map_run(const uint32_t *entry_read, uint32_t begin, uint32_t end, uint32_t query_read) {
    MapRun r;
    r.begin = begin;
    r.self_begin = map_lower_bound(entry_read, begin, end, query_read);
    uint32_t self_end = r.self_begin;
    if (query_read != 0xFFFFFFFFu) self_end = map_lower_bound(entry_read, r.self_begin, end, query_read + 1u);
    else self_end = r.self_begin < end ? end : r.self_begin;           // (read 2^32 - 1: whatever is left is its own)
    r.self_count = self_end - r.self_begin;
    r.count = end - begin - r.self_count;
    return r;
}
// entry of the window's j-th anchor, j < count: the run without the self block
__host__ __device__ __forceinline__ uint32_t map_run_entry(uint32_t begin, uint32_t self_begin, uint32_t self_count, uint32_t j) {
    const uint32_t e = begin + j;
    return e >= self_begin ? e + self_count : e;
}

// an anchor's strand: both windows' flags (:738)
__host__ __device__ __forceinline__ uint32_t map_anchor_reversed(uint32_t ref_reversed, uint32_t query_reversed) { return ref_reversed != query_reversed ? 1u : 0u; }

// May anchor j precede anchor i (argmaxPosition, :1152-1201)?  The gap |d_r - d_q| if so, else -1.  Positions are < 2^31, so the
// reference's int32 differences are the true ones; "the query moves the wrong way for the strand" (:1196-1201) is d_q < 0 (d_q == 0 is
// the equal-position case above it).
__host__ __device__ __forceinline__ int32_t map_pred_gap(uint32_t ri, uint32_t qi, uint32_t rev_i, uint32_t rj, uint32_t qj, uint32_t rev_j) {
    if (rev_i != rev_j) return -1;
    if (ri == rj || qi == qj) return -1;
    const int64_t d_q = rev_i ? (int64_t)qj - (int64_t)qi : (int64_t)qi - (int64_t)qj;
    const int64_t d_r = (int64_t)ri - (int64_t)rj;
    if (d_q > MAP_MAX_DISTANCE || d_r > MAP_MAX_DISTANCE) return -1;
    if (d_r <= 0) return -1;
    const int64_t gap = d_r > d_q ? d_r - d_q : d_q - d_r;
    if (gap > MAP_MAX_GAP) return -1;
    if (d_q < 0) return -1;
    return (int32_t)gap;
}

// The candidate (new score, j) as one word: the score in the high half, j in the low -- so that ONE max over the candidates of an anchor
// implements "the best strictly positive score wins, on a tie the largest j" (the reference walks j downwards and replaces on > only).
// 0: no candidate (a score <= 0 never wins, :1133 + :1208).
__host__ __device__ __forceinline__ uint64_t map_candidate(int32_t score_j, int32_t gap, uint32_t j) {
    const int32_t s = score_j + MAP_ANCHOR_SCORE - gap;
    return gap < 0 || s <= 0 ? 0ull : ((uint64_t)(uint32_t)s << 32) | j;
}
__host__ __device__ __forceinline__ int32_t map_candidate_score(uint64_t c) { return c ? (int32_t)(c >> 32) : MAP_ANCHOR_SCORE; }
__host__ __device__ __forceinline__ uint32_t map_candidate_parent(uint64_t c) { return c ? (uint32_t)c : MAP_NO_PARENT; }

// predecessors of anchor i under the band: j = i - 1 down to i - band (:1147 breaks on i - j > band), not below 0
__host__ __device__ __forceinline__ uint32_t map_band_count(uint32_t i, uint32_t band) { return i < band ? i : band; }

// What ONE of 64 lanes sees for anchor i: lane t of a trip evaluates predecessor i - 1 - t, 64 a trip, ceil(count / 64) trips; the best
// packed candidate over the lane's trips.  The maximum over the 64 lanes is the anchor's (score, parent).  score[j], j < i, are final.
__host__ __device__ __forceinline__ uint64_t map_lane_best(const int32_t *score, const uint32_t *rp, const uint32_t *qp, const uint8_t *rv, uint32_t i, uint32_t band,
                                                           uint32_t lane) {
    const uint32_t ri = rp[i], qi = qp[i], rvi = rv[i];
    const uint32_t cnt = map_band_count(i, band);
    uint64_t best = 0;
    for (uint32_t base = 0; base < cnt; base += 64u) {
        const uint32_t t = base + lane;
        if (t < cnt) {
            const uint32_t j = i - 1u - t;
            const uint64_t c = map_candidate(score[j], map_pred_gap(ri, qi, rvi, rp[j], qp[j], rv[j]), j);
            best = c > best ? c : best;
        }
    }
    return best;
}

// the best anchor of a pair: the largest score, on a tie the smallest i (:963-967 replaces on > only, i ascending)
__host__ __device__ __forceinline__ bool map_better_end(int32_t score, int32_t best_so_far) { return score > best_so_far; }

// the chain that ends at best_i, walked by its parents: its length, and its root (the anchor without a parent)
__host__ __device__ __forceinline__ uint32_t map_chain_walk(const uint32_t *parent, uint32_t best_i, uint32_t *root) {
    uint32_t len = 0;
    for (uint32_t at = best_i; at != MAP_NO_PARENT; at = parent[at]) { *root = at; len++; }
    return len;
}

// What chainAnchors leaves of a chain (:1017-1047).  `first` is the BEST anchor, `last` the root of its chain.  The index differences
// are taken in 32 bits without sign and widened, as the reference's u_int32_t arithmetic does.
struct MapChain {
    int32_t score; uint32_t n_matches, query_reversed;
    int64_t n_diff_query, n_diff_reference, query_start, query_end, reference_start, reference_end, alignment_score;
};
__host__ __device__ __forceinline__ MapChain map_chain_fields(int32_t score, uint32_t n_matches, uint32_t first_qidx, uint32_t last_qidx, uint32_t first_ridx,
                                                              uint32_t last_ridx, uint32_t first_rpos, uint32_t last_rpos) {
    MapChain c;
    c.score = score;
    c.n_matches = n_matches;
    c.query_reversed = first_qidx > last_qidx ? 1u : 0u;
    if (c.query_reversed) {
        c.n_diff_query = (int64_t)(uint32_t)(first_qidx - last_qidx + 1u) - (int64_t)n_matches;
        c.query_start = last_qidx;
        c.query_end = first_qidx;
    } else {
        c.n_diff_query = (int64_t)(uint32_t)(last_qidx - first_qidx + 1u) - (int64_t)n_matches;
        c.query_start = first_qidx;
        c.query_end = last_qidx;
    }
    c.n_diff_reference = (int64_t)(uint32_t)(first_ridx - last_ridx + 1u) - (int64_t)n_matches;
    c.reference_start = first_rpos;
    c.reference_end = last_rpos;
    c.alignment_score = (int64_t)n_matches - c.n_diff_query;          // addAlignmentScore (:1241)
    return c;
}

}  // namespace mdbg
