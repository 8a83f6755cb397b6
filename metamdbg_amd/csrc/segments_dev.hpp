// segments_dev.hpp -- cutting a long read into segments the block-structured scan takes one wave each (scan.hip, "views"), for the
// device and for a host program (tests/host/test_scan_segments.cpp).
//
// A read of L raw bases is cut at multiples of G raw bases (G a multiple of the 2048-base tile, so every segment starts on a tile of
// the read).  Under homopolymer compression a base is a RUN START when it differs from the base in front of it (the read's first base
// always is one); the compressed read is the sequence of its run starts, and
//     c_s = number of run starts among the raw bases [0, s G)
// is where segment s begins in it -- exactly, also when the cut falls inside a run: the run's bases behind the cut start nothing.
// Without compression every base is a "run start" and c_s = s G.
//
// A VIEW is what one wave scans: the segment's raw bases plus a HALO of one tile behind it.  It OWNS the windows (l-mers) that start
// at the compressed positions [c_s, c_{s+1}); the owned ranges of a read's views partition [0, C), C the compressed length.  For every
// owned window the view must see the l bases of the window and, for the quality span [rle[pos], rle[pos + l]), the run start BEHIND
// the window: l further run starts behind its last owned position, not l - 1.  So a cut at raw base b is good when the tile [b, b + 2048)
// holds at least l run starts -- or reaches the read's end, where the read's own end rules apply.  A read with a cut that is not good
// (a homopolymer or another run-poor stretch of about 2000 bases behind it) is UNSEGMENTABLE and is scanned whole.
#pragma once
#include <cstdint>

namespace mdbg {

constexpr uint32_t SEG_TILE_BASES = 2048;            // a tile of the scan: 64 words of 32 bases
constexpr uint32_t SEG_DEFAULT_BASES = 16384;        // "scan_segment_bases": expected rows 16384 * 0.005 * 0.8 * 1.4 + 24 = 116 of the pre-filtered stage's 176

constexpr uint32_t SEG_FIRST = 1u;                   // the read's first view: the end trim in front, the first base starts a run whatever
constexpr uint32_t SEG_LAST = 2u;                    // the read's last view
constexpr uint32_t SEG_DEAD = 8u;                    // a view of an unsegmentable read: nothing to scan

struct SegView {
    uint32_t read;          // the read it belongs to
    uint32_t tile0;         // first tile of the read it covers (raw base tile0 * 2048)
    uint32_t raw_len;       // raw bases, halo included
    uint32_t c_s;           // compressed position of its first base in the read
    uint32_t n_own;         // windows it owns: those starting at view positions [0, n_own), i.e. c_{s+1} - c_s
    uint32_t flags;         // SEG_*
};

// the base "in front of" a read's first base: any other one, so that the first base starts a run
__host__ __device__ __forceinline__ uint32_t seg_first_prev(uint64_t first_word) { return ((uint32_t)first_word & 3u) ^ 1u; }

// run starts among the first `nvalid` (0 .. 32) bases of the packed word x (base i at bits [2i, 2i + 2)), `prev` the base in front of it
__host__ __device__ __forceinline__ uint32_t seg_word_run_starts(uint64_t x, uint32_t prev, uint32_t nvalid) {
    if (nvalid == 0u) return 0u;
    const uint64_t m5 = 0x5555555555555555ull;
    const uint64_t valid = nvalid >= 32u ? m5 : (((1ull << (2u * nvalid)) - 1ull) & m5);
    const uint64_t diff = x ^ ((x << 2) | (uint64_t)(prev & 3u));
    return (uint32_t)__builtin_popcountll((diff | (diff >> 1)) & valid);
}

// valid bases of word `wi` of a read of L bases
__host__ __device__ __forceinline__ uint32_t seg_word_valid(uint32_t L, uint32_t wi) {
    const uint64_t at = (uint64_t)wi * 32u;
    return at >= L ? 0u : (L - at >= 32u ? 32u : (uint32_t)(L - at));
}

// run starts of tile t of a read (words rw[0 ..), L bases): the previous base taken across word and tile borders
__host__ __device__ inline uint32_t seg_tile_run_starts(const uint64_t *rw, uint32_t L, uint32_t t) {
    const uint32_t nwords = (uint32_t)(((uint64_t)L + 31u) / 32u);
    uint32_t n = 0;
    for (uint32_t k = 0; k < 64u; k++) {
        const uint32_t wi = t * 64u + k;
        if (wi >= nwords) break;
        const uint32_t prev = wi ? (uint32_t)(rw[wi - 1u] >> 62) : seg_first_prev(rw[0]);
        n += seg_word_run_starts(rw[wi], prev, seg_word_valid(L, wi));
    }
    return n;
}

__host__ __device__ __forceinline__ uint32_t seg_tiles(uint32_t L) { return (uint32_t)(((uint64_t)L + SEG_TILE_BASES - 1u) / SEG_TILE_BASES); }
// segments of a read of L bases cut every G (0 or 1: not cut)
__host__ __device__ __forceinline__ uint32_t seg_count(uint32_t L, uint32_t G) { return (uint32_t)(((uint64_t)L + G - 1u) / G); }

// the cut at raw base b (a multiple of G, 0 < b < L) is good: `halo_runs` = run starts of the tile [b, b + 2048) (without compression:
// its bases)
__host__ __device__ __forceinline__ bool seg_cut_ok(uint32_t L, uint32_t b, uint32_t halo_runs, uint32_t K) {
    return (uint64_t)b + SEG_TILE_BASES >= L || halo_runs >= K;
}

// view s of the nS >= 2 views of read `read`: c_s / c_next = compressed positions of raw bases s G and (s + 1) G (c_next = the
// compressed length C for the last view)
__host__ __device__ __forceinline__ SegView seg_view_make(uint32_t read, uint32_t s, uint32_t nS, uint32_t L, uint32_t G, uint32_t c_s,
                                                          uint32_t c_next, bool live) {
    const uint64_t raw0 = (uint64_t)s * G;
    uint64_t end = raw0 + G + (s + 1u < nS ? SEG_TILE_BASES : 0u);
    if (end > L) end = L;
    SegView v;
    v.read = read;
    v.tile0 = (uint32_t)(raw0 / SEG_TILE_BASES);
    v.raw_len = (uint32_t)(end - raw0);
    v.c_s = c_s;
    v.n_own = c_next - c_s;
    v.flags = (s == 0u ? SEG_FIRST : 0u) | (s + 1u == nS ? SEG_LAST : 0u) | (live ? 0u : SEG_DEAD);
    return v;
}

// compressed position of raw base s G from the exclusive prefix sums of the read's per-tile run starts (`tile_excl`; null without
// compression), C the compressed length
__host__ __device__ __forceinline__ uint32_t seg_offset(const uint32_t *tile_excl, uint32_t s, uint32_t nS, uint32_t L, uint32_t G, uint32_t C) {
    if (s >= nS) return tile_excl ? C : L;
    return tile_excl ? tile_excl[(uint64_t)s * (G / SEG_TILE_BASES)] : s * G;
}

}  // namespace mdbg
