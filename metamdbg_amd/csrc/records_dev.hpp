// records_dev.hpp -- the bytes of a record file composed from a minimizer set's arrays, for the device (records_write_kernel,
// minimizers.hip) and for a host program (tests/host/test_records_layout.cpp): the inverse of records_gather_kernel.
//
// Two forms, little-endian, no padding anywhere.  With o = off[r] and n = off[r + 1] - o, all in 64-bit arithmetic:
//
//   PLAIN  `u32 n; u8 circular; u32 m[n]`  (read_data_corrected.txt, unitig_data.txt; the reference writes it in
//          readSelection/ReadSelection.hpp:1420-1426).  Record r starts at byte 5 r + 4 o: count at +0, circular (0) at +4, values at +5.
//   INIT   `u32 n; u8 circular; u32 m[n]; u32 pos[n]; u8 dir[n]; u8 qual[n]; f32 meanQ; u32 len`  (read_data_init.txt,
//          readSelection/ReadSelection.hpp:415-467).  Record r starts at byte 13 r + 10 o: count +0, circular (0) +4, m at +5, pos at
//          +5 + 4 n, dir at +5 + 8 n, qual at +5 + 9 n, the bits of meanQ at +5 + 10 n, len at +9 + 10 n.
//
// A record's SECTIONS are its count, its flag byte, m, pos, dir, qual, meanQ and len.  The composition (rec_emit) hands its stores to
// a sink, `word(at, v)` for an aligned 4-byte store and `byte(at, v)` for one byte, under one rule that makes the kernel free of races
// without a memset and without atomics:
//   - a word is stored only where all four of its bytes belong to ONE section of ONE record.  m and pos share one misalignment for the
//     whole record, (start + 5) & 3 (pos begins 4 n bytes behind m): an interior word is the upper bytes of one value and the lower
//     bytes of the next, one v_alignbyte.  An interior word of dir / qual is four source bytes;
//   - every other byte is a byte store: the head and tail of a section up to the next word border, the count, meanQ and len where they
//     straddle words, the flag byte, and everything in a record too short to have an interior word;
//   - the output is never read, no byte is written twice, nothing is written outside the record's own [start, start + bytes).
// The lanes that share a record (16 in the kernel, any number here) split the values, the words of dir / qual and the few edge bytes by
// index; lane and lane count change who stores a byte, never which bytes are stored.
#pragma once
#include <cstdint>

namespace mdbg {

constexpr int REC_PLAIN = 0;                         // MDBG_RECORDS_PLAIN
constexpr int REC_INIT = 1;                          // MDBG_RECORDS_INIT

// first byte of record r, `o` minimizers in front of it
__host__ __device__ __forceinline__ uint64_t rec_start(int form, uint64_t r, uint64_t o) { return form == REC_INIT ? 13ull * r + 10ull * o : 5ull * r + 4ull * o; }
// bytes of a record of n minimizers; rec_start(form, n_reads, n_min) is the whole file
__host__ __device__ __forceinline__ uint64_t rec_bytes(int form, uint64_t n) { return form == REC_INIT ? 13ull + 10ull * n : 5ull + 4ull * n; }

// bytes [8 sh, 8 sh + 32) of the 64-bit value hi:lo, sh = 1 .. 3
__host__ __device__ __forceinline__ uint32_t rec_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * sh));
#endif
}

// The arrays a record is composed from (CSR order: the values of record r at [off[r], off[r + 1])).  PLAIN reads `m` alone.
struct RecSource {
    const uint32_t *m, *pos;
    const uint8_t *dir, *qual;
    const uint32_t *meanq_bits;     // per read, the bit patterns of the mean qualities (NaN travels as it is); null: every read has meanq_all
    uint32_t meanq_all;
    const uint32_t *len;
};

// one u32 field of its own (count, meanQ, len): a word when it is aligned, four bytes otherwise
template <typename Sink>
__host__ __device__ __forceinline__ void rec_put_u32(uint64_t at, uint32_t v, Sink &out) {
    if ((at & 3u) == 0u) { out.word(at, v); return; }
    for (uint32_t b = 0; b < 4u; b++) out.byte(at + b, (uint8_t)(v >> (8u * b)));
}

// a section of n u32 values v[0 .. n) at byte `at`
template <typename Sink>
__host__ __device__ __forceinline__ void rec_put_values(uint64_t at, const uint32_t *v, uint64_t n, uint32_t lane, uint32_t lanes, Sink &out) {
    const uint32_t sh = (uint32_t)(at & 3u);
    if (sh == 0u) {
        for (uint64_t j = lane; j < n; j += lanes) out.word(at + 4u * j, v[j]);
        return;
    }
    const uint32_t lo = 4u - sh;                    // bytes of a value in front of the word border inside it
    const uint64_t w0 = at + lo;                    // the section's first whole word: the upper sh bytes of v[0], the lower `lo` of v[1]
    for (uint64_t j = lane; j < n; j += lanes) {
        const uint32_t x = v[j];
        if (j == 0) for (uint32_t b = 0; b < lo; b++) out.byte(at + b, (uint8_t)(x >> (8u * b)));                          // head
        if (j + 1 < n) out.word(w0 + 4u * j, rec_alignbyte(v[j + 1], x, lo));
        else for (uint32_t b = lo; b < 4u; b++) out.byte(at + 4u * j + b, (uint8_t)(x >> (8u * b)));                       // tail
    }
}

// a section of n bytes s[0 .. n) at byte `at`
template <typename Sink>
__host__ __device__ __forceinline__ void rec_put_bytes(uint64_t at, const uint8_t *s, uint64_t n, uint32_t lane, uint32_t lanes, Sink &out) {
    uint64_t head = (4u - (uint32_t)(at & 3u)) & 3u;            // bytes in front of the first word border
    if (head > n) head = n;
    const uint64_t words = (n - head) >> 2;
    const uint64_t tail0 = head + 4u * words;                   // the bytes [tail0, n) follow the last whole word
    for (uint64_t w = lane; w < words; w += lanes) {
        const uint8_t *p = s + head + 4u * w;
        out.word(at + head + 4u * w, (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    }
    const uint64_t edge = head + (n - tail0);                   // at most six bytes
    for (uint64_t e = lane; e < edge; e += lanes) {
        const uint64_t i = e < head ? e : tail0 + (e - head);
        out.byte(at + i, s[i]);
    }
}

// Lane `lane` of `lanes`: its share of the stores of record r -- `o` minimizers in front of it, n of its own.
template <typename Sink>
__host__ __device__ __forceinline__ void rec_emit(int form, const RecSource &src, uint64_t r, uint64_t o, uint64_t n, uint32_t lane, uint32_t lanes, Sink &out) {
    const uint64_t at = rec_start(form, r, o);
    if (lane == 0u) {
        rec_put_u32(at, (uint32_t)n, out);
        out.byte(at + 4u, 0);                                   // circular
    }
    rec_put_values(at + 5u, src.m + o, n, lane, lanes, out);
    if (form != REC_INIT) return;
    rec_put_values(at + 5u + 4u * n, src.pos + o, n, lane, lanes, out);
    rec_put_bytes(at + 5u + 8u * n, src.dir + o, n, lane, lanes, out);
    rec_put_bytes(at + 5u + 9u * n, src.qual + o, n, lane, lanes, out);
    // (the last lane: the first has the header, and both are busy with edge bytes)
    if (lane == lanes - 1u) {
        rec_put_u32(at + 5u + 10u * n, src.meanq_bits ? src.meanq_bits[r] : src.meanq_all, out);
        rec_put_u32(at + 9u + 10u * n, src.len[r], out);
    }
}

}  // namespace mdbg
