// stitch_dev.hpp -- the word composition of mdbg_spans_stitch / mdbg_reads_stitch_ranges and the byte rule of
// mdbg_sequences_to_fasta_bytes (stitch.hip), for the device and for a host program (tests/host/test_stitch.cpp), over extract_dev.hpp.
//
// A contig is the concatenation of oriented pieces (ToBasespaceGfa::CreateBaseContigsFunctor, toBasespace/ToBasespaceGfa.hpp:1479-1754:
// to_string() of the stored DnaBitset2, Utils::revcomp when the contig's window is reversed, +=).  Piece i of the batch begins at base
// pbase[i] of ALL pieces' bases (an exclusive scan of their lengths), so a contig whose first piece is p0 holds the bases
// [pbase[p0], pbase[p1]) and its output word w the bases a0 = pbase[p0] + 32 w ... (ASCII: 8 w).  The word is the OR of what every piece
// that meets [a0, a0 + nb) contributes: bases [s, s + m) of an oriented piece (start, length) are an oriented range of the read again,
//     forward    (start + s, m)                  reversed    (start + length - s - m, m)
// and extract_gather / extract_gather_mask bring them into groups 0 .. m - 1 (group j = bits [2j, 2j + 2)).  What is new is the place:
// the m bases go to bases d .. d + m - 1 of the word.  With P the reversal of the four groups inside every byte and B the byte swap
// (extract_dev.hpp), a forward part lands at P(g << 2d).  A reversed part alone would be B(g << 2 (32 - m)); moved up by d bases in
// DnaBitset2's order that is B(g << 2 (32 - m - d)) -- the shift never loses a group because d + m <= 32.  P and B are linear over OR, so
// the forward parts of a word are collected in one accumulator, the reversed ones in another, and P and B are applied once a word.
//
// The invalid code.  The reference keeps a piece as DnaBitset2 in the READ window's orientation: a character outside ACGT is A.  A
// reversed contig window then runs Utils::revcomp over the string: that A becomes T.  So a base under the invalid mask is code 0 when the
// piece is not flipped and code 3 when it is, whatever the net orientation; the ranges entry has no flip and always gives 0.  ASCII: N.
#pragma once
#include "extract_dev.hpp"

namespace mdbg {

constexpr uint64_t STITCH_NONE = ~0ull;                                        // MDBG_STITCH_NONE

// What the copy reads of a piece, one 16-byte load: where its read's words begin (a word index below 2^62), bit 63 = the net
// orientation is reversed, bit 62 = an invalid base is T (the piece is flipped); the range.
struct alignas(16) StitchRec { uint64_t w0_bits; uint32_t start, length; };
constexpr uint64_t STITCH_REC_REVERSED = 1ull << 63, STITCH_REC_INVALID_T = 1ull << 62, STITCH_REC_WORD = (1ull << 62) - 1ull;

// the piece a lane is inside of: its index, its bases [lo, hi) of all pieces' bases, its record
struct StitchPiece { uint32_t p; uint64_t lo, hi; StitchRec rec; };

__host__ __device__ __forceinline__ void stitch_piece_load(StitchPiece &pc, uint32_t p, const uint64_t *pbase, const StitchRec *recs) {
    pc.p = p;
    pc.lo = pbase[p];
    pc.hi = pbase[p + 1u];
    pc.rec = recs[p];
}

// the two accumulators of a BITSET word, and the word they make
struct StitchWord { uint64_t fwd, rev; };
__host__ __device__ __forceinline__ uint64_t stitch_word_finish(StitchWord a) { return extract_reverse_in_bytes(a.fwd) | __builtin_bswap64(a.rev); }

// m (1 .. 32) bases from base s of an oriented piece, to bases d .. d + m - 1 of a word (d + m <= 32)
__host__ __device__ __forceinline__ void stitch_add_bitset(StitchWord &acc, const uint64_t *rw, const uint32_t *inv, uint32_t start, uint32_t length, bool reversed,
                                                           bool invalid_t, uint32_t s, uint32_t m, uint32_t d) {
    const uint32_t p = reversed ? start + length - s - m : start + s;
    uint64_t g = extract_gather(rw, p, m);
    g ^= (g >> 1) & 0x5555555555555555ull;                                     // A C T G -> A C G T
    if (reversed) g = ~g;                                                      // the complement
    const uint64_t keep = m < 32u ? (1ull << (2u * m)) - 1ull : ~0ull;
    g &= keep;
    if (inv) {
        const uint64_t bad = extract_spread_groups(extract_gather_mask(inv, p, m)) & keep;
        g = invalid_t ? g | bad : g & ~bad;                                    // T behind the contig window's revcomp, else A
    }
    if (reversed) acc.rev |= g << (2u * (32u - m - d));
    else acc.fwd |= g << (2u * d);
}

// ... m (1 .. 8) characters to bytes d .. d + m - 1 of a word
__host__ __device__ __forceinline__ uint64_t stitch_part_ascii(const uint64_t *rw, const uint32_t *inv, uint32_t start, uint32_t length, bool reversed, uint32_t s,
                                                               uint32_t m, uint32_t d) {
    const uint32_t p = reversed ? start + length - s - m : start + s;
    return extract_word_ascii(rw, inv, p, m, reversed, 0u) << (8u * d);
}

// The output word that holds the nb (1 .. 32, ASCII 1 .. 8) bases from base a0 of all pieces' bases; they lie in one contig.  pc: the
// piece the lane was inside of last, pc.lo <= a0; it moves on by extract_next_owner's doubling search, which steps over empty pieces,
// and is left at the piece of the word's last base.  src(w0) / src.mask(w0): the packed words and the invalid-mask words (null without)
// of the read whose words begin at w0.  *n_met (optional) receives the pieces the word met.
template <typename Src>
__host__ __device__ __forceinline__ uint64_t stitch_word(const Src &src, const uint64_t *pbase, uint32_t n_pieces, const StitchRec *recs, StitchPiece &pc, uint64_t a0,
                                                         uint32_t nb, uint32_t form, uint32_t *n_met = nullptr) {
    if (a0 >= pc.hi) stitch_piece_load(pc, extract_next_owner(pbase, n_pieces, pc.p, a0), pbase, recs);
    StitchWord acc{0ull, 0ull};
    uint64_t chars = 0ull;
    uint32_t d = 0u, met = 0u;
    for (;;) {
        const uint64_t a = a0 + d;
        const uint32_t s = (uint32_t)(a - pc.lo), left = (uint32_t)(pc.hi - a), m = left < nb - d ? left : nb - d;
        const uint64_t w0 = pc.rec.w0_bits & STITCH_REC_WORD;
        const bool reversed = (pc.rec.w0_bits & STITCH_REC_REVERSED) != 0ull;
        if (form == EXTRACT_ASCII) chars |= stitch_part_ascii(src.words(w0), src.mask(w0), pc.rec.start, pc.rec.length, reversed, s, m, d);
        else stitch_add_bitset(acc, src.words(w0), src.mask(w0), pc.rec.start, pc.rec.length, reversed, (pc.rec.w0_bits & STITCH_REC_INVALID_T) != 0ull, s, m, d);
        met++;
        d += m;
        if (d >= nb) break;
        stitch_piece_load(pc, extract_next_owner(pbase, n_pieces, pc.p, a0 + d), pbase, recs);
    }
    if (n_met) *n_met = met;
    return form == EXTRACT_ASCII ? chars : stitch_word_finish(acc);
}

// bases a word of a contig holds: word w of a contig of `length` bases
__host__ __device__ __forceinline__ uint32_t stitch_word_bases(uint32_t length, uint32_t w, uint32_t form) {
    const uint32_t per = form == EXTRACT_ASCII ? 8u : 32u, left = length - per * w;
    return left < per ? left : per;
}

// ---- the text ---------------------------------------------------------------------------------------------------------------------------
// A record of CreateBaseContigsFunctor (:1756-1785): ">ctg" + to_string(name) + "l" / "c" + '\n' + the bases + '\n'; an empty sequence is
// ">ctg" + to_string(name) + "l\nA\n" whatever its flag.  The functor narrows the flag to `bool isCircular` (:1487) before it compares it
// with CONTIG_LINEAR / CONTIG_CIRCULAR / CONTIG_CIRCULAR_RESCUED, so a rescued circular contig (flag 2) is written "c" like flag 1 and
// the "rc" of :1774-1776 is never reached; the text here is the text the reference writes.
__host__ __device__ __forceinline__ uint32_t fasta_digits(uint32_t v) {
    uint32_t n = 1u;
    while (v >= 10u) { v /= 10u; n++; }
    return n;
}

__host__ __device__ __forceinline__ uint32_t fasta_header_bytes(uint32_t name, uint32_t flag, uint32_t length) {
    (void)flag; (void)length;
    return 4u + fasta_digits(name) + 2u;
}

__host__ __device__ __forceinline__ uint64_t fasta_record_bytes(uint32_t name, uint32_t flag, uint32_t length) {
    return (uint64_t)fasta_header_bytes(name, flag, length) + (length ? length : 1u) + 1u;
}

// the characters of bases i .. i + 7 of a sequence (i + 8 <= length), the first in the low byte: two or three of its bytes
__host__ __device__ __forceinline__ uint64_t fasta_bases8(const uint8_t *seq, uint64_t i) {
    const uint64_t q = i / 4u;
    const uint32_t r = (uint32_t)(i % 4u);
    const uint32_t v = (((uint32_t)seq[q] << 16 | (uint32_t)seq[q + 1u] << 8 | (r ? (uint32_t)seq[q + 2u] : 0u)) >> (8u - 2u * r)) & 0xFFFFu;
    uint64_t out = 0;
#pragma unroll
    for (uint32_t t = 0; t < 8u; t++) out |= (uint64_t)((0x54474341u >> (8u * ((v >> (14u - 2u * t)) & 3u))) & 0xFFu) << (8u * t);
    return out;
}

// byte k of a record whose header takes `header` bytes (fasta_header_bytes); seq: the sequence's DnaBitset2 bytes (read only for a base)
__host__ __device__ __forceinline__ uint8_t fasta_byte(uint32_t name, uint32_t flag, uint32_t length, uint32_t header, const uint8_t *seq, uint64_t k) {
    const uint32_t digits = header - 6u;
    if (k < 4u)return (uint8_t)(0x6774633Eu >> (8u * (uint32_t)k));                         // ">ctg", '>' in the low byte
    if (k < 4u + digits) {
        uint32_t v = name;
        for (uint32_t i = (uint32_t)k - 4u + 1u; i < digits; i++) v /= 10u;
        return (uint8_t)(0x30u + v % 10u);
    }
    if (k + 1u < header) return length == 0u || flag == 0u ? 0x6Cu : 0x63u;                     // l, c
    if (k < header) return 0x0Au;
    const uint64_t i = k - header;
    if (length == 0u) return i == 0u ? 0x41u : 0x0Au;                                          // "A\n"
    if (i >= length) return 0x0Au;
    return (uint8_t)(0x54474341u >> (8u * ((seq[i / 4u] >> (6u - 2u * (uint32_t)(i % 4u))) & 3u)));      // "ACGT"[code]
}

}  // namespace mdbg
