// spans_dev.hpp -- the pieces of mdbg_kminmer_spans (spans.hip) that are plain arithmetic, for the device and for a host program
// (tests/host/test_spans.cpp): the run-start flags of a packed word, the j-th flag of such a word, and the ReadKminmer fields of a
// window composed from its minimizers' spans (MDBG::getKminmers, Commons.hpp:5401-5526).
//
// Under homopolymer compression a base is a RUN START when it differs from the base in front of it as a CHARACTER (EncoderRLE::execute,
// Commons.hpp:4163-4203): a change of 2-bit code, a change of the invalid bit (N against G), a bit of the break mask ("aA", IUPAC
// letters that share a code), and the read's first base whatever precedes it; padding behind the last base never counts -- the rule of
// the scan's general path (scan.hip, "run starts / compaction").  rle[j], the original coordinate of compressed position j, is the
// position of the j-th run start; rle[L'] is the read's length.
//
// A FLAG WORD holds the 32 flags of a packed word in the word's own geometry: bit 2i set = base i starts a run (the odd bits are 0).
#pragma once
#include <cstdint>

namespace mdbg {

constexpr uint32_t SPANS_TILE_WORDS = 64;            // a tile of the coordinate map: 64 words of 32 bases, as the scan's
constexpr uint32_t SPANS_TILE_BASES = 32 * SPANS_TILE_WORDS;
constexpr uint64_t SPANS_EVEN = 0x5555555555555555ull;

// bit i of v -> bit 2i
__host__ __device__ __forceinline__ uint64_t spans_spread(uint32_t v) {
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & SPANS_EVEN;
    return x;
}

// valid bases of word `wi` of a read of L bases
__host__ __device__ __forceinline__ uint32_t spans_word_valid(uint32_t L, uint32_t wi) {
    const uint64_t at = (uint64_t)wi * 32u;
    return at >= L ? 0u : (L - at >= 32u ? 32u : (uint32_t)(L - at));
}

// The flag word of the packed word x.  prev_code / prev_inv: the 2-bit code and the invalid bit of the base in front of the word
// (ignored for the read's first word); inv / brk: the word's bits of the two side masks (0 for a batch without them); nvalid: how many
// of its 32 bases belong to the read.
__host__ __device__ __forceinline__ uint64_t spans_word_flags(uint64_t x, uint32_t prev_code, uint32_t inv, uint32_t prev_inv, uint32_t brk,
                                                              bool first_word, uint32_t nvalid) {
    if (nvalid == 0u) return 0ull;
    const uint64_t diff = x ^ ((x << 2) | (uint64_t)(prev_code & 3u));
    uint64_t d = (diff | (diff >> 1)) & SPANS_EVEN;
    const uint32_t side = (inv ^ ((inv << 1) | (prev_inv & 1u))) | brk;
    if (side) d |= spans_spread(side);
    if (first_word) d |= 1ull;
    return nvalid >= 32u ? d : d & ((1ull << (2u * nvalid)) - 1ull);
}

// The flag word of word `wi` of a read: rw its packed words, inv / brk its words of the side masks (null without), L its bases.
// wi < ceil(L / 32); reads rw[wi], rw[wi - 1] and the same two of inv, nothing else.
__host__ __device__ __forceinline__ uint64_t spans_read_word_flags(const uint64_t *rw, const uint32_t *inv, const uint32_t *brk, uint32_t L, uint32_t wi) {
    const uint32_t prev_code = wi ? (uint32_t)(rw[wi - 1u] >> 62) : 0u;
    const uint32_t prev_inv = (inv && wi) ? inv[wi - 1u] >> 31 : 0u;
    return spans_word_flags(rw[wi], prev_code, inv ? inv[wi] : 0u, prev_inv, brk ? brk[wi] : 0u, wi == 0u, spans_word_valid(L, wi));
}

__host__ __device__ __forceinline__ uint32_t spans_count_flags(uint64_t d) { return (uint32_t)__builtin_popcountll(d); }

// Base (0 .. 31) of the j-th flag of the flag word d, j counted from 0 and below spans_count_flags(d).  Five halvings: the lower half
// holds the flag or its count is taken off j.
__host__ __device__ __forceinline__ uint32_t spans_select_flag(uint64_t d, uint32_t j) {
    uint32_t at = 0;
#pragma unroll
    for (uint32_t sh = 32u; sh >= 2u; sh >>= 1) {
        const uint32_t c = (uint32_t)__builtin_popcountll(d & ((1ull << sh) - 1ull));
        if (j >= c) { j -= c; d >>= sh; at += sh; }
    }
    return at >> 1;
}

// One read's part of the coordinate map: per tile the run starts of the read in front of it (tile_excl, n_tiles entries, the first 0),
// per word the run starts of its tile in front of it (word_excl, 64 entries a tile, words behind the read included: they repeat the
// tile's total), L' = comp_len.
struct SpansReadMap {
    const uint64_t *rw;             // the read's packed words
    const uint32_t *inv, *brk;      // its words of the side masks (null without)
    uint32_t L, comp_len, n_tiles;
    const uint32_t *tile_excl;
    const uint16_t *word_excl;
};

// rle[j], 0 <= j <= L': the tile (binary search), the word (three rounds of three reads over the tile's 64 offsets), then the flag.
// An empty tile or word -- the inside of a long run -- shares its offset with the one behind it; the LAST tile / word whose offset is
// at most j is the one that holds run start j.
__host__ __device__ __forceinline__ uint32_t spans_rle(const SpansReadMap &m, uint32_t j) {
    if (j >= m.comp_len) return m.L;
    uint32_t lo = 0, hi = m.n_tiles;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (m.tile_excl[mid] <= j) lo = mid; else hi = mid;
    }
    const uint32_t rel = j - m.tile_excl[lo];
    const uint16_t *o = m.word_excl + (uint64_t)lo * SPANS_TILE_WORDS;
    uint32_t w = 0;
#pragma unroll
    for (uint32_t st = 16u; st >= 1u; st >>= 2) {
        const uint32_t o1 = o[w + st], o2 = o[w + 2u * st], o3 = o[w + 3u * st];
        w += st * ((o1 <= rel ? 1u : 0u) + (o2 <= rel ? 1u : 0u) + (o3 <= rel ? 1u : 0u));
    }
    const uint32_t nwords = (uint32_t)(((uint64_t)m.L + 31u) / 32u);
    uint32_t wi = lo * SPANS_TILE_WORDS + w;
    if (wi >= nwords) wi = nwords - 1u;                  // (words behind the read hold no flag and are never chosen)
    return wi * 32u + spans_select_flag(spans_read_word_flags(m.rw, m.inv, m.brk, m.L, wi), rel - o[w]);
}

// The fields of a window's ReadKminmer (Commons.hpp:5474-5516) from the spans [S, E) of its minimizers in original coordinates:
// s_first / s_second = S of the window's first and second minimizer, e_before_last / e_last = E of its last but one and last.  For
// k = 2 the second minimizer is the last and the first is the last but one.
struct SpanFields {
    uint32_t pos_start, pos_end, seq_length_start, seq_length_end;
};
__host__ __device__ __forceinline__ SpanFields spans_compose(uint32_t s_first, uint32_t s_second, uint32_t e_before_last, uint32_t e_last, bool reversed) {
    const uint32_t f = s_second - s_first, b = e_last - e_before_last;
    SpanFields o;
    o.pos_start = s_first;
    o.pos_end = e_last;
    o.seq_length_start = reversed ? b : f;
    o.seq_length_end = reversed ? f : b;
    return o;
}

}  // namespace mdbg
