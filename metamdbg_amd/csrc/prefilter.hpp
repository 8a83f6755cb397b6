// prefilter.hpp -- the selected-key bitmap of the block-structured scan (scan.hip, the PFW variants of scan_fast_kernel).
//
// Under homopolymer compression at l = 15 every hashed window of a read -- forward or reverse complement -- has no two equal
// adjacent digits, so the canonical keys a read can produce are the 9 565 938 repeat-free 15-digit values that are their own
// canonical form, and which of them are selected depends on the threshold alone: 47 791 at density 0.005f.  A one-hash Bloom
// bitmap of those keys answers "certainly not selected" for most positions with one multiply and one LDS read; the positions
// that pass are hashed in full afterwards.  No false negative is the one property correctness rests on: every selected key's
// bit is set, because the builder below and the kernel's probe use the same index function.
//
// Everything here compiles for the host too (tests/host/test_prefilter_bitmap.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "murmur.hpp"

namespace mdbg {

constexpr unsigned PREFILTER_L = 15;                    // the one minimizer length the bitmap is built for
constexpr unsigned PREFILTER_LOG2_BITS = 19;            // 2^19 bits = 64 KB of LDS, one probe
constexpr unsigned PREFILTER_MIN_LOG2_BITS = 10;        // "scan_prefilter_log2_bits" (tests): a bitmap in which nearly every bit is set
constexpr unsigned PREFILTER_BYTES = (1u << PREFILTER_LOG2_BITS) / 8u;
constexpr uint32_t PREFILTER_KEYS = 1u << (2 * PREFILTER_L);

// bit of key v in a bitmap of 2^log2_bits bits (a multiplicative index: 8.65 % false positives at 64 KB where an xor-shift
// index has 11.6 %)
__host__ __device__ __forceinline__ uint32_t prefilter_index(uint32_t v, unsigned log2_bits) { return (v * 0x9E3779B1u) >> (32u - log2_bits); }

// no two equal adjacent digits among the 15 base-4 digits of v
__host__ __device__ __forceinline__ bool prefilter_repeat_free(uint32_t v) {
    const uint32_t x = v ^ (v >> 2);                               // digit i ^ digit i + 1 in bits 2i, 2i + 1 (i = 0 .. 13)
    return (((x | (x >> 1)) & 0x05555555u) == 0x05555555u);
}

// reverse complement of a 15-digit key (complement = digit ^ 2: A 0, C 1, T 2, G 3)
__host__ __device__ __forceinline__ uint32_t prefilter_revcomp(uint32_t v) {
    uint32_t r = v;
    r = ((r & 0x33333333u) << 2) | ((r >> 2) & 0x33333333u);
    r = ((r & 0x0F0F0F0Fu) << 4) | ((r >> 4) & 0x0F0F0F0Fu);
    r = ((r & 0x00FF00FFu) << 8) | ((r >> 8) & 0x00FF00FFu);
    r = (r << 16) | (r >> 16);                                     // 16 digits reversed: the unused top digit is now the lowest
    return (r >> 2) ^ 0x2AAAAAAAu;
}

// a key a compressed read can produce as the canonical form of a window (l odd: no key is its own reverse complement)
__host__ __device__ __forceinline__ bool prefilter_key_possible(uint32_t v) { return prefilter_repeat_free(v) && v < prefilter_revcomp(v); }

__host__ __device__ __forceinline__ bool prefilter_key_selected(uint32_t v, uint64_t threshold) {
    return prefilter_key_possible(v) && kmer_hash32(v) < threshold;
}

// The builder: keys first, first + stride, ... below 4^15; set_bit(index) for every selected one.  The device kernel calls it
// with an atomic OR on the global buffer, a host program with a plain store.
template <class SetBit>
__host__ __device__ __forceinline__ void prefilter_build_range(uint32_t first, uint32_t stride, uint64_t threshold, unsigned log2_bits, SetBit set_bit) {
    for (uint64_t v = first; v < PREFILTER_KEYS; v += stride)
        if (prefilter_key_selected((uint32_t)v, threshold)) set_bit(prefilter_index((uint32_t)v, log2_bits));
}

// ---- The selected-key TABLE: the exact verdict of a candidate, looked up instead of hashed (scan.hip, confirm) ----
//
// h = v * 0x9E3779B1 is a bijection of the 32-bit words, so (h >> 16, h & 0xFFFF) names v: a bucket chosen by the top bits of h that
// stores the low 16 bits of h as a tag holds its keys exactly once the bucket bits and the tag together cover all 32.  A bucket is
// 16 bytes, one load: seven 16-bit tags and a 16-bit state word,
//     word 0 .. 2: tags 0 .. 5,  word 3: tag 6 in the low half, the state in the high half
//     state 0 = no key (the tags are zero and mean nothing), CONFIRM_VALID = all seven tags are keys of the bucket (a bucket with
//     fewer repeats its first), CONFIRM_OVERFLOW (alone or with VALID) = ask the hash: the bucket had more than seven keys, or -- in a
//     geometry of fewer than 2^16 buckets, where tag and bucket no longer name the key -- a possible key that is NOT selected shares a
//     stored tag (confirm_table_verify_range finds those; with 2^16 buckets there are none and the pass is skipped).
// So no tag has to be proved impossible: an empty slot is never compared on its own.  2^16 buckets are 1 MB; at density 0.005f the
// fullest holds 7 of the 47 791 keys, at 0.01f (95 524 keys) a handful overflow (tests/host/test_confirm_table.cpp prints both).
constexpr unsigned CONFIRM_LOG2_BUCKETS = 16;           // 2^16 buckets of 16 bytes = 1 MB: resident in every XCD's L2
constexpr unsigned CONFIRM_MIN_LOG2_BUCKETS = 10;       // "scan_confirm_table_log2_buckets" (tests): nearly every bucket overflows
constexpr unsigned CONFIRM_SLOTS = 7;
constexpr unsigned CONFIRM_BUCKET_WORDS = 4;
constexpr uint32_t CONFIRM_VALID = 1u, CONFIRM_OVERFLOW = 2u;
constexpr uint32_t CONFIRM_NO = 0u, CONFIRM_YES = 1u, CONFIRM_ASK = 2u;      // what a look-up answers

// the one index function of builder and probe: h, its bucket and its tag
__host__ __device__ __forceinline__ uint32_t confirm_hash(uint32_t v) { return v * 0x9E3779B1u; }
__host__ __device__ __forceinline__ uint32_t confirm_bucket(uint32_t h, unsigned log2_buckets) { return h >> (32u - log2_buckets); }
__host__ __device__ __forceinline__ uint32_t confirm_tag(uint32_t h) { return h & 0xFFFFu; }

// the verdict of the key with hash h from its bucket's four words
__host__ __device__ __forceinline__ uint32_t confirm_verdict(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t h) {
    const uint32_t t = confirm_tag(h), state = w3 >> 16;
    if (state & CONFIRM_OVERFLOW) return CONFIRM_ASK;
    const bool hit = (w0 & 0xFFFFu) == t || (w0 >> 16) == t || (w1 & 0xFFFFu) == t || (w1 >> 16) == t || (w2 & 0xFFFFu) == t || (w2 >> 16) == t ||
                     (w3 & 0xFFFFu) == t;
    return (hit && state == CONFIRM_VALID) ? CONFIRM_YES : CONFIRM_NO;
}
__host__ __device__ __forceinline__ uint32_t confirm_lookup(const uint32_t *table, unsigned log2_buckets, uint32_t v) {
    const uint32_t h = confirm_hash(v);
    const uint32_t *b = table + (size_t)confirm_bucket(h, log2_buckets) * CONFIRM_BUCKET_WORDS;
    return confirm_verdict(b[0], b[1], b[2], b[3], h);
}

// The builder, in three steps over a zeroed table and zeroed per-bucket counters.  Ops::add / Ops::orr return the old value: atomics on
// the device, the host compiler's in a host program.
// 1. every selected key claims a slot of its bucket by the bucket's counter; the first seven store their tags
template <class Ops>
__host__ __device__ __forceinline__ void confirm_table_insert_range(uint32_t first, uint32_t stride, uint64_t threshold, unsigned log2_buckets, uint32_t *table,
                                                                    uint32_t *counts, Ops ops) {
    for (uint64_t v = first; v < PREFILTER_KEYS; v += stride) {
        if (!prefilter_key_selected((uint32_t)v, threshold)) continue;
        const uint32_t h = confirm_hash((uint32_t)v), b = confirm_bucket(h, log2_buckets);
        const uint32_t slot = ops.add(&counts[b], 1u);
        if (slot < CONFIRM_SLOTS) ops.orr(&table[(size_t)b * CONFIRM_BUCKET_WORDS + (slot >> 1)], confirm_tag(h) << (16u * (slot & 1u)));
    }
}
// 2. one bucket gets its state; the unused slots of a bucket with keys repeat its first tag.  True: the bucket overflowed
__host__ __device__ __forceinline__ bool confirm_table_finish_bucket(uint32_t *bucket, uint32_t count) {
    if (count == 0u) return false;
    if (count > CONFIRM_SLOTS) { bucket[3] = (bucket[3] & 0xFFFFu) | (CONFIRM_OVERFLOW << 16); return true; }
    const uint32_t t0 = bucket[0] & 0xFFFFu;
    for (uint32_t s = count; s < CONFIRM_SLOTS; s++) bucket[s >> 1] |= t0 << (16u * (s & 1u));
    bucket[3] |= CONFIRM_VALID << 16;
    return false;
}
// 3. fewer than 2^16 buckets only: a possible key that is not selected and yet answered YES marks its bucket.  marked(): called
// once per bucket newly marked
template <class Ops, class Marked>
__host__ __device__ __forceinline__ void confirm_table_verify_range(uint32_t first, uint32_t stride, uint64_t threshold, unsigned log2_buckets, uint32_t *table,
                                                                    Ops ops, Marked marked) {
    for (uint64_t v = first; v < PREFILTER_KEYS; v += stride) {
        if (!prefilter_key_possible((uint32_t)v) || kmer_hash32((uint32_t)v) < threshold) continue;
        if (confirm_lookup(table, log2_buckets, (uint32_t)v) != CONFIRM_YES) continue;
        uint32_t *w3 = &table[(size_t)confirm_bucket(confirm_hash((uint32_t)v), log2_buckets) * CONFIRM_BUCKET_WORDS + 3u];
        if (!(ops.orr(w3, CONFIRM_OVERFLOW << 16) & (CONFIRM_OVERFLOW << 16))) marked();
    }
}
__host__ __device__ constexpr bool confirm_table_needs_verify(unsigned log2_buckets) { return log2_buckets < 16u; }

}  // namespace mdbg
