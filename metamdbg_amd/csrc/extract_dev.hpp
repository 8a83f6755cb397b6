// extract_dev.hpp -- the word composition of mdbg_spans_extract / mdbg_reads_extract_ranges (extract.hip), for the device and for a host
// program (tests/host/test_extract.cpp): which range of its read a (window, part) request names, which request an output word belongs
// to, and one 64-bit OUTPUT word of a range, in DnaBitset2's layout (utils/DnaBitset.hpp:118-242) or as characters.
//
// The source (objects.hpp): 32 bases a 64-bit word, base i at bits [2i, 2i + 2), codes A 0, C 1, T 2, G 3; one 32-bit word of the
// invalid mask per packed word, bit i = base i had bit 3 set (N, n, K, M, Y ...).
// The BITSET output: base i of a sequence in byte i / 4 at bits 6 - 2 (i % 4), codes A 0, C 1, G 2, T 3; stored as 64-bit little-endian
// words, byte b of a word is bits [8b, 8b + 8), so base i of a word (0 .. 31) sits at bit 8 (i / 4) + 6 - 2 (i % 4).
//
// One output word w of a range [start, start + length) holds nb = min(32, length - 32 w) bases.  Both orientations GATHER nb
// consecutive source bases from position p into groups 0 .. nb - 1 of a word g (group j = bits [2j, 2j + 2)): the word that holds p
// shifted down, and -- only when p % 32 + nb > 32, i.e. when the last base wanted lies in it -- the next word shifted up.  That second
// word then holds a base of the range, so it is one of the read's own words: nothing outside the read is touched.
//     forward    p = start + 32 w                 output base i = source base p + i
//     reversed   p = start + length - 32 w - nb   output base i = complement of source base p + nb - 1 - i
// Codes: c ^ (c >> 1) turns the library's code into DnaBitset2's (T 2 -> 3, G 3 -> 2; the low bit xored with the high bit).  The
// complement is c ^ 2 in the library's codes (A <-> T, C <-> G), which is c ^ 3 behind the exchange: the reversed word is the
// exchanged word with every bit flipped.  Then the groups under the invalid mask (gathered the same way, bit j -> group j) and the
// groups from nb up are cleared: an invalid base is code 0 (A) in both orientations, as DnaBitset2 stores any character outside ACGT.
// Order: let P reverse the four groups inside every byte, B reverse the eight bytes (a byte swap), R reverse all 32 groups;
// R = B P = P B and P P = identity.
//     forward    group j must go to byte j / 4, position 3 - j % 4 of it: out = P(g).
//     reversed   output base i is group nb - 1 - i.  Shifted up by 32 - nb groups it is group 31 - i, so R puts it at group i and P
//                into its place in the byte: out = P(R(g << 2 (32 - nb))) = P P B (..) = B(g << 2 (32 - nb)) -- the two group
//                reversals cancel and a byte swap is all that is left (two v_perm_b32).  The groups the shift left empty land behind
//                the sequence's last base, where the padding is zero anyway.
// P is two mask-and-shift steps (pairs of groups, then nibbles); the gather is a 64-bit funnel shift.
//
// The ASCII output holds 8 characters a word: the same gather with nb = min(8, length - 8 w) and 8 in place of 32 in p, then one
// byte a base, 'N' under the invalid mask.  The packed reads keep no case and no IUPAC letter: a base comes out as the upper-case
// letter its code names.
#pragma once
#include <cstdint>

namespace mdbg {

constexpr uint32_t EXTRACT_ENTIRE = 0, EXTRACT_LEFT = 1, EXTRACT_RIGHT = 2;    // MDBG_SEQ_ENTIRE / LEFT / RIGHT
constexpr uint32_t EXTRACT_BITSET = 0, EXTRACT_ASCII = 1;                      // MDBG_SEQ_BITSET / ASCII

// what the plan found: (request << 8) | reason, the smallest wins; EXTRACT_FINE = nothing
constexpr unsigned long long EXTRACT_FINE = ~0ull;
constexpr uint32_t EXTRACT_BAD_PART = 1, EXTRACT_BAD_RESERVED = 2, EXTRACT_BAD_WINDOW = 3, EXTRACT_BAD_READ = 4, EXTRACT_BAD_READ_LENGTH = 5,
                   EXTRACT_BAD_OVERHANG = 6, EXTRACT_BAD_RANGE = 7;

struct ExtractRange { uint32_t read, start, length, reversed; };               // mdbg_seq_range

// The range a (window, part) request names (ToBasespaceGfa::extractKminmerSequence, toBasespace/ToBasespaceGfa.hpp:1050-1103: the
// window [ps, pe) is copied, reverse-complemented when the window is reversed, and the first ls / last le characters OF THAT STRING
// are kept -- for a reversed window they are the range's far end / near end).  0 = fine, else the reason.
__host__ __device__ __forceinline__ uint32_t extract_part_range(uint32_t ps, uint32_t pe, uint32_t ls, uint32_t le, bool reversed, uint32_t part,
                                                                uint32_t &start, uint32_t &length) {
    if (pe < ps) return EXTRACT_BAD_RANGE;
    const uint32_t len = pe - ps;
    if (ls > len || le > len) return EXTRACT_BAD_OVERHANG;
    if (part == EXTRACT_ENTIRE) { start = ps; length = len; }
    else if (part == EXTRACT_LEFT) { start = reversed ? pe - ls : ps; length = ls; }
    else if (part == EXTRACT_RIGHT) { start = reversed ? ps : pe - le; length = le; }
    else return EXTRACT_BAD_PART;
    return 0u;
}

// meaningful bytes of a sequence of `length` bases, and the 64-bit words it takes (a sequence starts at a multiple of 8 bytes)
__host__ __device__ __forceinline__ uint64_t extract_bytes(uint32_t length, uint32_t form) {
    return form == EXTRACT_ASCII ? (uint64_t)length : ((uint64_t)length + 3u) / 4u;
}
__host__ __device__ __forceinline__ uint32_t extract_words(uint32_t length, uint32_t form) { return (uint32_t)((extract_bytes(length, form) + 7u) / 8u); }

// The request that owns byte `at` of the output, for a lane that has left request `from`: off[from + 1] <= at < off[n] (off: the n + 1
// byte offsets of the sequences).  The steps from the old owner double until an offset lies behind `at`, and the search closes in
// between: a request d further on costs about 2 log2 d offsets, whatever n is.  The LAST request whose offset is at most `at` is the
// one -- empty requests share their offset with the request behind them.
__host__ __device__ __forceinline__ uint32_t extract_next_owner(const uint64_t *off, uint32_t n, uint32_t from, uint64_t at) {
    uint32_t lo = from + 1u, hi = lo, step = 1u;
    for (;;) {
        hi = n - lo > step ? lo + step : n;                 // (off[n] > at: the loop ends, at step 2^31 at the latest)
        if (off[hi] > at) break;
        lo = hi;
        step <<= 1;
    }
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= at) lo = mid; else hi = mid;
    }
    return lo;
}

// nb (1 .. 32) consecutive bases of a read from position p, in groups 0 .. nb - 1; the groups above hold whatever follows
__host__ __device__ __forceinline__ uint64_t extract_gather(const uint64_t *rw, uint32_t p, uint32_t nb) {
    const uint32_t wi = p >> 5, sh = p & 31u;
    const uint64_t lo = rw[wi];
    if (sh == 0u) return lo;
    const uint64_t hi = sh + nb > 32u ? rw[wi + 1u] : 0ull;
    return (lo >> (2u * sh)) | (hi << (64u - 2u * sh));
}

// ... and their bits of the invalid mask, bit j = base p + j
__host__ __device__ __forceinline__ uint32_t extract_gather_mask(const uint32_t *inv, uint32_t p, uint32_t nb) {
    const uint32_t wi = p >> 5, sh = p & 31u;
    const uint32_t lo = inv[wi];
    if (sh == 0u) return lo;
    const uint32_t hi = sh + nb > 32u ? inv[wi + 1u] : 0u;
    return (lo >> sh) | (hi << (32u - sh));
}

// bit i of v -> bits 2i and 2i + 1
__host__ __device__ __forceinline__ uint64_t extract_spread_groups(uint32_t v) {
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x * 3ull;
}

// P: the four groups of every byte reversed
__host__ __device__ __forceinline__ uint64_t extract_reverse_in_bytes(uint64_t x) {
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    return ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
}

// Output word w of a range in BITSET form.  rw / inv: the read's packed words and its words of the invalid mask (null without);
// w < extract_words(length, EXTRACT_BITSET).
__host__ __device__ __forceinline__ uint64_t extract_word_bitset(const uint64_t *rw, const uint32_t *inv, uint32_t start, uint32_t length, bool reversed,
                                                                 uint32_t w) {
    const uint32_t left = length - 32u * w, nb = left < 32u ? left : 32u;
    const uint32_t p = reversed ? start + left - nb : start + 32u * w;
    uint64_t g = extract_gather(rw, p, nb);
    g ^= (g >> 1) & 0x5555555555555555ull;                                     // A C T G -> A C G T
    if (reversed) g = ~g;                                                      // the complement
    uint64_t keep = nb < 32u ? (1ull << (2u * nb)) - 1ull : ~0ull;
    if (inv) keep &= ~extract_spread_groups(extract_gather_mask(inv, p, nb));
    g &= keep;
    if (!reversed) return extract_reverse_in_bytes(g);
    return __builtin_bswap64(nb < 32u ? g << (2u * (32u - nb)) : g);
}

// Output word w of a range in ASCII form: 8 characters, the first in the low byte; zero behind the last.
__host__ __device__ __forceinline__ uint64_t extract_word_ascii(const uint64_t *rw, const uint32_t *inv, uint32_t start, uint32_t length, bool reversed,
                                                                uint32_t w) {
    const uint32_t left = length - 8u * w, nb = left < 8u ? left : 8u;
    const uint32_t p = reversed ? start + left - nb : start + 8u * w;
    uint32_t g = (uint32_t)extract_gather(rw, p, nb);
    if (reversed) g ^= 0xAAAAu;                                                // the complement in the library's codes: c ^ 2
    const uint32_t bad = inv ? extract_gather_mask(inv, p, nb) : 0u;
    uint64_t out = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) {
        const uint32_t j = reversed ? nb - 1u - i : i;                         // (wraps for i >= nb: not used)
        const uint32_t c = (g >> (2u * (j & 7u))) & 3u;
        const uint32_t ch = ((bad >> (j & 7u)) & 1u) ? 0x4Eu : (0x47544341u >> (8u * c)) & 0xFFu;      // 'N', or "ACTG"[c]
        if (i < nb) out |= (uint64_t)ch << (8u * i);
    }
    return out;
}

__host__ __device__ __forceinline__ uint64_t extract_word(const uint64_t *rw, const uint32_t *inv, uint32_t start, uint32_t length, bool reversed, uint32_t w,
                                                          uint32_t form) {
    return form == EXTRACT_ASCII ? extract_word_ascii(rw, inv, start, length, reversed, w) : extract_word_bitset(rw, inv, start, length, reversed, w);
}

}  // namespace mdbg
