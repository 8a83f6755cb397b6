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

}  // namespace mdbg
