// realign_dev.hpp -- the rules of mdbg_map_realign (realign.hip) that are plain arithmetic, for the device and for a host program
// (tests/host/test_realign.cpp): how a thinned neighbour is seen through its orientation, what a chain of the pair leaves as the list
// AlignmentResult2::_alignments, what normalizeAlignment makes of it, and what Graph::addAlignment2 reads of an entry.  The semantics are
// the first half of ReadCorrectionFunctor::performPoaCorrection4 (readSelection/ReadCorrection.hpp:5217-5285),
// MinimizerRead::toReverseComplement (Commons.hpp:1042-1079) and MinimizerChainer::computeChainingAlignment / normalizeAlignment
// (readSelection/MinimizerChainer.hpp:330-569, :1015-1111).  The chain itself, the gaps of a link and the runs at both ends are the
// verifier's and the mapper's (verify_dev.hpp: verify_gap, verify_edge_mismatches, verify_query_reversed; mapper_dev.hpp), not restated.
//
// Names: T' is the thinned target, N' the thinned neighbour AS ORIENTED (reverse-complemented when the kept row says so).  ri indexes T',
// qi indexes N'.  An entry is the pair (ref_index, query_index) of the reference's list, REALIGN_NONE for its -1.
#pragma once
#include <cstdint>

#include "verify_dev.hpp"

namespace mdbg {

constexpr uint32_t REALIGN_NONE = 0xFFFFFFFFu;
constexpr uint32_t REALIGN_LDS_ENTRIES = 1024;       // raw entries of a row up to which its list is normalised in LDS (8 KB a wave)
enum : uint8_t { REALIGN_MATCH = 0, REALIGN_MISMATCH = 1, REALIGN_INSERTION = 2, REALIGN_DELETION = 3 };

struct RealignEntry { uint32_t r, q; };

// ---- the oriented view (toReverseComplement, Commons.hpp:1042-1079): the order turned round, then dir = !dir, pos = length - pos ------------
// index j' of N' <-> index of the stored read (its own inverse)
__host__ __device__ __forceinline__ uint32_t realign_oriented_index(uint32_t j, uint32_t n_q, uint32_t reversed) { return reversed ? n_q - 1u - j : j; }
__host__ __device__ __forceinline__ uint32_t realign_oriented_position(uint32_t pos, uint32_t read_length, uint32_t reversed) { return reversed ? read_length - pos : pos; }
__host__ __device__ __forceinline__ uint32_t realign_oriented_direction(uint32_t dir, uint32_t reversed) { return reversed ? (dir ? 0u : 1u) : dir; }
// Entry k of a target minimizer's run in the neighbour's lookup (stored indexes ascending): under reversal the run is walked BACKWARDS, so
// the oriented indexes -- and with them the query positions -- still ascend and the anchors leave in the reference's sorted order.
__host__ __device__ __forceinline__ uint32_t realign_run_entry(uint32_t begin, uint32_t count, uint32_t k, uint32_t reversed) { return reversed ? begin + count - 1u - k : begin + k; }

// N' as the rules below read it: the stored thinned neighbour and its orientation
struct RealignQuery { const uint32_t *m; const uint8_t *quality; uint32_t n, reversed; };
__host__ __device__ __forceinline__ uint32_t realign_query_minimizer(const RealignQuery &q, uint32_t qi) { return q.m[realign_oriented_index(qi, q.n, q.reversed)]; }
__host__ __device__ __forceinline__ uint8_t realign_query_quality(const RealignQuery &q, uint32_t qi) { return q.quality[realign_oriented_index(qi, q.n, q.reversed)]; }

// does the pair take part at all (Utils::isReadTooShort of N', ReadCorrection.hpp:5253)
__host__ __device__ __forceinline__ bool realign_neighbour_short(uint64_t n_q, uint32_t min_minimizers) { return n_q < min_minimizers; }

// ---- the raw list (:330-569) ----------------------------------------------------------------------------------------------------------------
// the query index k steps on from qi: downwards when the chain is reversed
__host__ __device__ __forceinline__ uint32_t realign_query_step(uint32_t qi, uint32_t k, uint32_t chain_reversed) { return chain_reversed ? qi - k : qi + k; }

// A link a -> b of the chain (:356-501): the pair of a, then rg = mis + del pairs (r, none), then qg = mis + ins pairs (none, q)
struct RealignLink { uint32_t rg, qg; };
__host__ __device__ __forceinline__ RealignLink realign_link(uint32_t a_ri, uint32_t a_qi, uint32_t b_ri, uint32_t b_qi, uint32_t chain_reversed) {
    VerifyGaps g{0, 0, 0};
    verify_gap(a_ri, a_qi, b_ri, b_qi, chain_reversed, g);
    RealignLink l;
    l.rg = (uint32_t)(g.mismatches + g.deletions);
    l.qg = (uint32_t)(g.mismatches + g.insertions);
    return l;
}
__host__ __device__ __forceinline__ uint32_t realign_link_length(const RealignLink &l) { return 1u + l.rg + l.qg; }
// entry k < realign_link_length of the link
__host__ __device__ __forceinline__ RealignEntry realign_link_entry(uint32_t a_ri, uint32_t a_qi, const RealignLink &l, uint32_t chain_reversed, uint32_t k) {
    if (k == 0u) return RealignEntry{a_ri, a_qi};
    if (k <= l.rg) return RealignEntry{a_ri + k, REALIGN_NONE};
    return RealignEntry{REALIGN_NONE, realign_query_step(a_qi, k - l.rg, chain_reversed)};
}
// entry k < start_mis of the run in front of the first anchor f (:333-354): index-aligned pairs counting up to f
__host__ __device__ __forceinline__ RealignEntry realign_start_entry(uint32_t f_ri, uint32_t f_qi, uint32_t start_mis, uint32_t chain_reversed, uint32_t k) {
    const uint32_t back = start_mis - k;
    return RealignEntry{f_ri - back, chain_reversed ? f_qi + back : f_qi - back};
}
// entry k <= end_mis behind the links (:547-569): k = 0 the last anchor l itself, then the index-aligned pairs behind it
__host__ __device__ __forceinline__ RealignEntry realign_end_entry(uint32_t l_ri, uint32_t l_qi, uint32_t chain_reversed, uint32_t k) {
    return RealignEntry{l_ri + k, realign_query_step(l_qi, k, chain_reversed)};
}
// the raw length of a row whose links' lengths sum to `links`
__host__ __device__ __forceinline__ uint64_t realign_raw_length(uint64_t start_mis, uint64_t links, uint64_t end_mis) { return start_mis + links + 1u + end_mis; }

// ---- normalizeAlignment (:1015-1111) --------------------------------------------------------------------------------------------------------
// An erased entry stays where it is as (none, none) -- a tombstone: the look-aheads pass over it by construction (neither side is set), the
// pass must not visit it, and one compaction afterwards is the reference's erase.
__host__ __device__ __forceinline__ bool realign_tombstone(const RealignEntry &e) { return e.r == REALIGN_NONE && e.q == REALIGN_NONE; }

// The pass's step at entry i of list[0 .. n).  An insertion takes the reference index of the first entry at or behind it that has one when
// the two minimizers are equal; a deletion the query index likewise.  The robbed entry is visited later in the same pass.
__host__ __device__ __forceinline__ void realign_normalize_step(RealignEntry *list, uint32_t n, uint32_t i, const uint32_t *tm, const RealignQuery &q) {
    const RealignEntry e = list[i];
    if (realign_tombstone(e)) return;
    if (e.r == REALIGN_NONE) {
        uint32_t j = i;
        while (j < n && list[j].r == REALIGN_NONE) j++;                   // getNextMatchInReference (:1097-1103)
        if (j == n) return;
        const uint32_t r = list[j].r;
        if (tm[r] == realign_query_minimizer(q, e.q)) { list[i].r = r; list[j].r = REALIGN_NONE; }
    } else if (e.q == REALIGN_NONE) {
        uint32_t j = i;
        while (j < n && list[j].q == REALIGN_NONE) j++;                   // getNextMatchInQuery (:1105-1111)
        if (j == n) return;
        const uint32_t qq = list[j].q;
        if (tm[e.r] == realign_query_minimizer(q, qq)) { list[i].q = qq; list[j].q = REALIGN_NONE; }
    }
}
__host__ __device__ __forceinline__ void realign_normalize(RealignEntry *list, uint32_t n, const uint32_t *tm, const RealignQuery &q) {
    for (uint32_t i = 0; i < n; i++) realign_normalize_step(list, n, i, tm, q);
}

// ---- what Graph::addAlignment2 reads of an entry (:1179-1271) --------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint8_t realign_kind(const RealignEntry &e, const uint32_t *tm, const RealignQuery &q) {
    if (e.r == REALIGN_NONE) return REALIGN_INSERTION;
    if (e.q == REALIGN_NONE) return REALIGN_DELETION;
    return tm[e.r] == realign_query_minimizer(q, e.q) ? REALIGN_MATCH : REALIGN_MISMATCH;
}

}  // namespace mdbg
