// scan.hip -- reads -> minimizers on the device.
//
// One wavefront (64 lanes) owns one read at a time and walks it in tiles of 64 packed words
// (2048 bases).  Per tile:
//   1. every lane holds one u64 word (32 bases); run-start flags for homopolymer compression come
//      from a bit trick on the packed word (x ^ (x<<2 | prev base)), a wave prefix sum of their
//      popcounts gives each lane its offset in the compressed stream        [EncoderRLE, Commons.hpp:4163-4203]
//   2. lanes squeeze their kept bases to contiguous 2-bit fields (a 1024-entry LDS table: 5 bases per
//      look-up) and OR them into a per-wave LDS bit stream (carry of the last K bases from the
//      previous tile in front)
//   3. lanes take 4 adjacent k-mers per trip: one 3-word LDS read + v_alignbit extracts the bases
//      LSB-first (E); revcomp = E ^ 0xAAAA.., forward = digit-reverse(E) once, then one shift-in per
//      position; canonical = min; closed-form 8-byte Murmur3 (seed 42) on explicit 32-bit halves and
//      an integer threshold replace the u64-vs-double compare
//                                                           [KmerModel::iterate + MinimizerParser::parse,
//                                                            utils/kmer/Kmer.hpp:531-611, :1373-1456]
//   4. selected lanes are compacted in position order with ballot + popcount.
// A k-mer is evaluated only once the base after it is known, which drops the last k-mer of the
// read exactly as the reference's loop bound (pos < nK-1) does, for any homopolymer tail.
// Low-complexity reads (computeSequenceComplexity, ReadSelection.hpp:1171-1228) are detected with a
// 2-mer upper bound per 64-position window and confirmed by an exact 3-mer pass only when needed.
//
// Template variants: HAS_N adds a 1-bit "invalid" stream (characters with bit 3 set, Kmer.hpp:462;
// k-mers touching one have the value -1, :567 and :574-580, whose hash no density up to 0.71 selects); HAS_QUAL records, for every selected minimizer,
// the ORIGINAL coordinates [rle[pos], rle[pos+K]) its per-minimizer minimum quality spans
// (ReadSelection.hpp:1047-1142) -- the quality bytes themselves are read by the gather kernel.
#include "common.hpp"
#include "complexity_dev.hpp"
#include "murmur.hpp"
#include "objects.hpp"
#include "prefilter.hpp"
#include "scan_plan.hpp"
#include "segments_dev.hpp"

#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>

namespace mdbg {

constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_WAVES = SCAN_BLOCK / 64;
constexpr int TILE_WORDS = 64;                 // u64 words per tile (one per lane)
constexpr int STREAM_WORDS = 136;              // u32: (16 carry + 2048 new bases) / 16 = 129, + slack for the w+1 read
constexpr int ISTREAM_WORDS = 68;              // u32: 1 bit per compressed base (HAS_N)
constexpr uint64_t M5 = 0x5555555555555555ull;
constexpr uint8_t READ_SUSPECT = 0x80;         // internal: 2-mer complexity bound exceeded, exact pass pending

struct ScanArgs {
    const uint64_t *words;
    const uint64_t *word_off;
    const uint32_t *len;
    const uint32_t *invalid;      // per word mask (HAS_N)
    const uint32_t *brk;          // per word mask of character changes the 2-bit codes do not show (HAS_N; may be null)
    const uint8_t *qual;          // phred+33 bytes (inline min-quality in the overflow re-run)
    const uint64_t *qual_off;
    uint32_t n_reads;
    uint32_t K;
    uint64_t threshold;           // hash < threshold  <=>  (double)hash < density * 2^64
    uint32_t select_invalid;      // HAS_N: the hash of the value -1, which a k-mer touching an invalid character has, is below the threshold
                                  // (densities above 0.7135): such k-mers are then selected, as 0xFFFFFFFF (Kmer.hpp:567, :580, :1434)
    uint32_t trim;                // MinimizerParser::_trimBps: 1 (default) skips the first and last l-mer, 0 keeps them
    uint32_t q_last;              // 1: quality span ends ON the last base of the l-mer (correction scan), 0: at the next run
    const uint32_t *rep;          // sorted repetitive minimizers
    uint32_t n_rep;
    int apply_filters;
    const uint32_t *subset;       // optional list of read indices to process (overflow re-run)
    // outputs (padded per read: slots [cap_off[r], cap_off[r+1]))
    const uint64_t *cap_off;
    uint32_t *out_min;
    uint32_t *out_pos;
    uint8_t *out_dir;
    uint32_t *out_os;             // HAS_QUAL: original start of the minimizer's span
    uint32_t *out_oe;             // HAS_QUAL: original end (exclusive)
    uint8_t *out_mqual;           // HAS_QUAL && inline_minq: min quality written directly
    int inline_minq;
    uint32_t *out_count;          // per read: number selected (may exceed capacity -> overflow)
    uint8_t *out_flags;           // per read: MDBG_READ_* | READ_SUSPECT
    // scan_fast_kernel, bump mode (cursor != null; cap_off unused): a wave takes room for a finished read with one atomic
    // add and writes its rows there; reads that outgrow the LDS stage and suspects of the complexity bound are listed
    unsigned long long *cursor;   // [g]: rows handed out so far in region g of the output arrays (one address takes about 80 M
                                  // returning atomics per second on this part; a million 10 kb reads finish in 11 ms)
    uint32_t n_regions;           // power of two
    uint64_t out_capacity;        // rows one region holds
    uint64_t *out_begin;          // per read: first row
    uint32_t *over_list, *suspect_list;
    uint32_t *list_counters;      // [0] = reads in over_list, [1] = reads in suspect_list
    const uint8_t *skip;          // scan_fast_kernel: reads flagged here carry side-mask bits (N, mixed case) and are left to the general kernel
    uint32_t cand_slack;          // scan_fast_kernel<.., APPROX>: extra width of the candidate test (0 but in tests)
    uint32_t guard_slack;         // scan_fast_kernel<.., APPROX>: extra width of the shared hash's guard test (0 but in tests)
    uint32_t wave_priority;       // scan_fast_kernel: s_setprio level of its waves (0 = leave alone)
    // scan_fast_kernel<.., PFW> (the pre-filtered variant): the selected-key bitmap (prefilter.hpp; PREFILTER_BYTES whatever its geometry)
    const uint32_t *pf_bits;
    uint32_t pf_shift;            // 32 - log2(bits of the bitmap): a key's bit is (v * 0x9E3779B1) >> pf_shift
    uint32_t pf_chunk;            // reads a workgroup deals out to its waves
    const uint4 *pf_table;        // the selected-key table confirm looks its candidates up in (prefilter.hpp); null: confirm hashes them
    uint32_t pf_table_shift;      // 32 - log2(buckets of the table)
    uint32_t pf_len_split;        // > 0: that variant passes over the reads of this many bases or more -- too long for its stage, they are
                                  // the four-wave kernel's, launched in front of it with the other reads flagged in `skip` (launch_scan)
    // scan_fast_kernel<.., SEG> (views of long reads, segments_dev.hpp): n_reads counts views, and out_begin / out_count / out_flags /
    // over_list / list_counters / cursor and the row arrays are the views' own; the join kernels put the reads together
    const SegView *views;
    unsigned long long *view_cx;  // per view: its words' share of the read's complexity sum
    uint32_t seg_tiles;           // tiles of a segment ("scan_segment_bases" / 2048)
    // scan_fast_kernel<.., PFW>, the persistent launch (scan_plan.hpp): non-null, the waves of every workgroup draw runs of pf_grab
    // consecutive items from this one counter (zeroed on the launch's stream in front of it) instead of from their workgroup's chunk
    unsigned long long *pf_counter;
    uint32_t pf_grab;
};

// squeeze the 2-bit fields of x whose flag bit (bit 2i of d) is set down to the low end
__device__ __forceinline__ uint64_t compress_pairs(uint64_t x, uint64_t d) {
    // zero the dropped fields once, then deposit field i at 2 * (number of kept fields below it)
    uint64_t xm = x & (d | (d << 1));
    uint32_t xl = (uint32_t)xm, xh = (uint32_t)(xm >> 32);
    uint32_t dl = (uint32_t)d, dh = (uint32_t)(d >> 32);
    uint32_t lo = 0, hi = 0;
    unsigned n = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        lo |= ((xl >> (2 * i)) & 3u) << n;
        n += (dl >> (2 * i) & 1u) << 1;
    }
    const unsigned nlo = n;
    n = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        hi |= ((xh >> (2 * i)) & 3u) << n;
        n += (dh >> (2 * i) & 1u) << 1;
    }
    return (uint64_t)lo | ((uint64_t)hi << nlo);
}

// Table-driven homopolymer compaction.  For 4 bases (8 bits) and the base before them, which bases
// start a run depends on those 10 bits only, so a 1024-entry table gives the squeezed bits (low byte)
// and twice the number kept (high byte) in one LDS lookup per 4 bases.
constexpr int HPC_LUT_SIZE = 1024;
constexpr uint16_t hpc_lut_entry(unsigned idx) {
    unsigned prev = idx & 3u, out = 0, n = 0;
    for (int i = 0; i < 4; i++) {
        unsigned b = (idx >> (2 + 2 * i)) & 3u;
        if (b != prev) { out |= b << n; n += 2; }
        prev = b;
    }
    return (uint16_t)(out | (n << 8));
}
static_assert(hpc_lut_entry(0x000u) == 0x0000u, "AAAA after A: nothing kept");
static_assert(hpc_lut_entry(0x001u) == 0x0200u, "AAAA after C: the first A");
static_assert(hpc_lut_entry(0x390u) == 0x0639u, "ACTG (codes 0 1 2 3) after A: the A is dropped, C T G are kept");
static_assert(hpc_lut_entry(0x391u) == 0x08E4u, "ACTG after C: all four kept");
static_assert(hpc_lut_entry(0x3FFu) == 0x0000u, "GGGG after G: nothing kept");

// The two byte tables a block works from (compress_pairs_lut), built by the compiler from the one rule above and copied to LDS
// 16 bytes a thread when a block starts (the blocks used to evaluate the rule themselves: 4 entries and 8 byte stores a thread,
// once per 8 reads)
struct alignas(16) HpcLutImage {
    uint8_t bits[HPC_LUT_SIZE], twice_kept[HPC_LUT_SIZE];
};
constexpr HpcLutImage make_hpc_lut_image() {
    HpcLutImage t{};
    for (unsigned i = 0; i < (unsigned)HPC_LUT_SIZE; i++) { const uint16_t e = hpc_lut_entry(i); t.bits[i] = (uint8_t)e; t.twice_kept[i] = (uint8_t)(e >> 8); }
    return t;
}
static __device__ const HpcLutImage hpc_lut_image = make_hpc_lut_image();
static_assert(sizeof(HpcLutImage) == 2 * HPC_LUT_SIZE && sizeof(HpcLutImage) % 16 == 0, "copied as uint4");

// all of a block's threads: the image into a block's LDS copy (`lut`, 16-byte aligned); the caller synchronises
__device__ __forceinline__ void hpc_lut_to_lds(uint8_t *lut, unsigned tid, unsigned n_threads) {
    for (unsigned i = tid; i < sizeof(HpcLutImage) / 16u; i += n_threads)
        reinterpret_cast<uint4 *>(lut)[i] = reinterpret_cast<const uint4 *>(&hpc_lut_image)[i];
}

// x squeezed to its run starts given the base `pl` preceding the word; *nbits = 2 * kept
// (the two halves of an entry live in two tables: LDS reads are not what this kernel is short of, and the merge below
// then is one shift-or and one add per entry instead of four operations)
struct HpcLut { const uint8_t *bits, *twice_kept; };
__device__ __forceinline__ uint64_t compress_pairs_lut(HpcLut lut, uint64_t x, uint32_t pl, unsigned *nbits) {
    const uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32);
    const uint32_t i0 = ((xl & 0xFFu) << 2) | pl, i1 = (xl >> 6) & 0x3FFu, i2 = (xl >> 14) & 0x3FFu, i3 = xl >> 22;
    const uint32_t i4 = __builtin_amdgcn_alignbit(xh, xl, 30) & 0x3FFu, i5 = (xh >> 6) & 0x3FFu, i6 = (xh >> 14) & 0x3FFu, i7 = xh >> 22;
    uint32_t lo = lut.bits[i0];
    unsigned n = lut.twice_kept[i0];
    lo |= (uint32_t)lut.bits[i1] << n; n += lut.twice_kept[i1];
    lo |= (uint32_t)lut.bits[i2] << n; n += lut.twice_kept[i2];
    lo |= (uint32_t)lut.bits[i3] << n; n += lut.twice_kept[i3];
    uint32_t hi = lut.bits[i4];
    unsigned m = lut.twice_kept[i4];
    hi |= (uint32_t)lut.bits[i5] << m; m += lut.twice_kept[i5];
    hi |= (uint32_t)lut.bits[i6] << m; m += lut.twice_kept[i6];
    hi |= (uint32_t)lut.bits[i7] << m; m += lut.twice_kept[i7];
    *nbits = n + m;
    return (uint64_t)lo | ((uint64_t)hi << n);
}

// same for 1-bit fields: keep bit i of v where bit 2i of d is set
__device__ __forceinline__ uint32_t compress_bits(uint32_t v, uint64_t d) {
    uint32_t out = 0;
    unsigned n = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        unsigned f = (unsigned)(d >> (2 * i)) & 1u;
        out |= ((v >> i) & f) << n;
        n += f;
    }
    return out;
}

// bit i of v -> bit 2i
__device__ __forceinline__ uint64_t spread_bits(uint32_t v) {
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// K bases starting at stream position j, LSB-first
__device__ __forceinline__ uint32_t stream_extract(const uint32_t *S, unsigned j, uint32_t kmask) {
    unsigned b = 2u * j, w = b >> 5, sh = b & 31u;
    uint32_t lo = S[w], hi = S[w + 1];
    return __builtin_amdgcn_alignbit(hi, lo, sh) & kmask;
}

__device__ __forceinline__ uint32_t istream_extract(const uint32_t *SI, unsigned j, uint32_t mask) {
    unsigned w = j >> 5, sh = j & 31u;
    uint32_t lo = SI[w], hi = SI[w + 1];
    return __builtin_amdgcn_alignbit(hi, lo, sh) & mask;
}

// reverse the order of the K 2-bit digits of e
__device__ __forceinline__ uint32_t digit_reverse(uint32_t e, unsigned K) {
    uint32_t r = __builtin_bitreverse32(e);
    r = ((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u);
    return r >> (32u - 2u * K);
}

constexpr unsigned REP_FILTER_BITS = 4096;            // 512 bytes of LDS a block
__device__ __forceinline__ uint32_t rep_filter_bit(uint32_t v) { return (v * 0x9E3779B1u) >> 20; }      // 12 bits

__device__ __forceinline__ bool rep_contains(const uint32_t *rep, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        uint32_t mid = (lo + hi) >> 1;
        uint32_t x = rep[mid];
        if (x < v) lo = mid + 1; else hi = mid;
    }
    return lo < n && rep[lo] == v;
}

// indicator masks in "spread" form: bit 2i set iff base i of the word equals c
__device__ __forceinline__ void base_eq_masks(uint64_t x, uint64_t eq[4]) {
    uint64_t lo = x & M5, hi = (x >> 1) & M5;
    eq[0] = ~(lo | hi) & M5;
    eq[1] = lo & ~hi;
    eq[2] = hi & ~lo;
    eq[3] = lo & hi;
}

// For the window of 64 positions starting at base 0 of x0 (bases from x0, x1 and the first two of
// x2): sum over all 2-mers (ORDER=2) or 3-mers (ORDER=3) v of count(v)^2.  S = (sum - 64) / 2 is
// sum_v c(c-1)/2, the numerator of the reference's window score (ReadSelection.hpp:1206-1216).
template <int ORDER>
__device__ __forceinline__ uint32_t window_sq_sum(uint64_t x0, uint64_t x1, uint64_t x2) {
    uint64_t a0[4], a1[4], a2[4];
    base_eq_masks(x0, a0);
    base_eq_masks(x1, a1);
    base_eq_masks(x2, a2);
    uint32_t sum = 0;
#pragma unroll
    for (int c0 = 0; c0 < 4; c0++) {
#pragma unroll
        for (int c1 = 0; c1 < 4; c1++) {
            // positions i with base(i)==c0 and base(i+1)==c1, for i in word0 / word1
            uint64_t p0 = a0[c0] & ((a0[c1] >> 2) | (a1[c1] << 62));
            uint64_t p1 = a1[c0] & ((a1[c1] >> 2) | (a2[c1] << 62));
            if (ORDER == 2) {
                uint32_t c = __popcll(p0) + __popcll(p1);
                sum += c * c;
            } else {
#pragma unroll
                for (int c2 = 0; c2 < 4; c2++) {
                    uint64_t t0 = p0 & ((a0[c2] >> 4) | (a1[c2] << 60));
                    uint64_t t1 = p1 & ((a1[c2] >> 4) | (a2[c2] << 60));
                    uint32_t c = __popcll(t0) + __popcll(t1);
                    sum += c * c;
                }
            }
        }
    }
    return sum;
}

// sum of a 32-bit value over the wave, as a scalar; the caller sees to it that the sum fits 32 bits.  The ladder of
// wave_inclusive_sum_dpp and one v_readlane: 7 vector instructions and no LDS crossbar where six rounds of 64-bit
// __shfl_xor took 12 ds_bpermute, their addresses and 12 adds with carry.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_sum_dpp(v), 63);
}

// Exact complexity decision for one read (second pass, rare): returns 1 when the reference's
// mean window score is > 5.  sum_w S_w / (61 nW) > 5  <=>  sum_w S_w > 305 nW; the equality case
// is resolved by replaying the reference's sequential double arithmetic.
__device__ int exact_low_complexity(const uint64_t *rw, uint32_t L, unsigned lane) {
    if (L < 66) return 0;                       // no full window -> NaN > 5 is false
    uint32_t nW = (L - 66) / 32 + 1;
    uint64_t total = 0;
    for (uint32_t base = 0; base < nW; base += 64) {
        uint32_t w = base + lane;
        uint64_t s = 0;
        if (w < nW) {
            uint32_t nwords = (L + 31) / 32;
            uint64_t x0 = rw[w], x1 = (w + 1 < nwords) ? rw[w + 1] : 0, x2 = (w + 2 < nwords) ? rw[w + 2] : 0;
            s = (window_sq_sum<3>(x0, x1, x2) - 64u) / 2u;
        }
        total += wave_sum_u64(s);
    }
    uint64_t rhs = 305ull * nW;
    if (total != rhs) return total > rhs;
    // tie: replay sequentially in double (all lanes redundantly; practically never taken)
    double acc = 0;
    uint32_t nwords = (L + 31) / 32;
    for (uint32_t w = 0; w < nW; w++) {
        uint64_t x0 = rw[w], x1 = (w + 1 < nwords) ? rw[w + 1] : 0, x2 = (w + 2 < nwords) ? rw[w + 2] : 0;
        double sc = (double)((window_sq_sum<3>(x0, x1, x2) - 64u) / 2u);
        sc /= 61.0;
        acc += sc;
    }
    return (acc / (double)nW) > 5.0;
}

// one wave per suspect read: exact decision; low-complexity reads lose their minimizers but keep
// their (empty) record (ReadSelection.hpp:890-899)
__global__ __launch_bounds__(256) void complexity_exact_kernel(const uint64_t *words, const uint64_t *word_off, const uint32_t *len,
                                                               const uint32_t *list, uint32_t n_list, uint32_t *count, uint8_t *flags,
                                                               unsigned long long *dropped /* may be null: sum of the counts cleared */) {
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, n_waves = (gridDim.x * 256u) >> 6;
    for (uint32_t i = wave; i < n_list; i += n_waves) {
        const uint32_t r = list[i];
        int low = exact_low_complexity(words + word_off[r], len[r], lane);
        if (lane == 0) {
            flags[r] = low ? (uint8_t)MDBG_READ_LOW_COMPLEXITY : (uint8_t)0;
            if (low) { if (dropped && count[r]) atomicAdd(dropped, (unsigned long long)count[r]); count[r] = 0; }
        }
    }
}

// per-wave LDS used by the HAS_QUAL && HPC variant: the original coordinate (rlePositions[hpc index], i.e. the
// start of the run) of every position of the compressed stream -- [carry (cb)] [new bases (C)] like the stream
// itself.  Filled by the lanes while they compact their words (one 4-byte LDS store per kept base), read twice
// per selected minimizer.
constexpr int ORIG_WORDS = 16 + 64 * 32;
struct QualMap {
    uint32_t orig[ORIG_WORDS];
};

#ifndef SCAN_PP
#define SCAN_PP 4          // adjacent k-mer positions per lane per trip of the hash loop (1..4)
#endif

// One trip of the hash loop: PP adjacent stream positions per lane, j = j0 + PP * lane + u.
template <bool HPC, bool HAS_QUAL, bool HAS_N>
struct KmerTrip {
    const ScanArgs &a;
    const uint32_t *S, *SI;
    const QualMap *Q;
    unsigned K;
    uint32_t kmask, kbits, comp_mask;
    unsigned lane, nk;
    uint32_t hp_base;
    unsigned cb;
    uint32_t tile_base;
    uint64_t cap0;
    uint32_t cap, r;

    // INTERIOR: every position of the trip is a real k-mer followed by a known base and none is the read's trimmed
    // first position -- the per-position range tests fall away (all full trips but the very first of a read).
    template <int PP, bool INTERIOR>
    __device__ __forceinline__ uint32_t run(unsigned j0, uint32_t nout) const {
        const unsigned jb = j0 + (unsigned)PP * lane;
        // 64 stream bits from position jb (enough for K + PP - 1 <= 19 bases)
        const unsigned b = 2u * jb, w = b >> 5, sh = b & 31u;
        uint32_t a0, a1;
        if (INTERIOR || w + 2 < STREAM_WORDS) {   // interior trips end K + 4 bases before the end of the stream: always in range
            const uint32_t w0 = S[w], w1 = S[w + 1], w2 = S[w + 2];
            a0 = __builtin_amdgcn_alignbit(w1, w0, sh);
            a1 = __builtin_amdgcn_alignbit(w2, w1, sh);
        } else { a0 = 0; a1 = 0; }   // lanes far beyond nk in a short last trip
        bool sel[PP];
        uint32_t val[PP];
        bool touches_invalid[PP];
        uint32_t fwd = 0;
#pragma unroll
        for (int u = 0; u < PP; u++) {
            const unsigned j = jb + u;
            const uint32_t e = (u == 0 ? a0 : __builtin_amdgcn_alignbit(a1, a0, 2 * u)) & kmask;
            const uint32_t rev = e ^ comp_mask;
            // forward k-mer: full digit reversal once, then shift in the newest base (top digit of e)
            fwd = u == 0 ? digit_reverse(e, K) : (((fwd << 2) | (e >> (2u * K - 2u))) & kmask);
            val[u] = fwd < rev ? fwd : rev;             // canonical; the direction is worked out for the selected few
#if defined(SCAN_ABLATE) && SCAN_ABLATE == 1
            sel[u] = val[u] == 0x12345u;                                                // ablation: no hash
#else
            sel[u] = kmer_hash32(val[u]) < a.threshold;
#endif
            // a k-mer that touches an invalid character counts with the value -1 (Kmer.hpp:567, :574-580): it is selected when THAT
            // value's hash is below the threshold (ScanArgs::select_invalid), and then written as 0xFFFFFFFF with its own direction
            touches_invalid[u] = HAS_N && istream_extract(SI, j < nk ? j : nk - 1u, kbits) != 0u;
            if (HAS_N && touches_invalid[u]) sel[u] = a.select_invalid != 0u;
            // first k-mer of the read skipped (Kmer.hpp:1395); the range test comes last, so it holds for both branches above and for
            // the invalid k-mers alike
            if (!INTERIOR) sel[u] = sel[u] && (hp_base + j >= a.trim) && (j < nk);
        }
        unsigned long long bal[PP];
        unsigned long long any = 0;
#pragma unroll
        for (int u = 0; u < PP; u++) { bal[u] = __ballot(sel[u]); any |= bal[u]; }
        if (any) {
            if (a.n_rep) {   // Kmer.hpp:1437
#pragma unroll
                for (int u = 0; u < PP; u++) {
                    if (sel[u]) sel[u] = !rep_contains(a.rep, a.n_rep, touches_invalid[u] ? 0xFFFFFFFFu : val[u]);
                    bal[u] = __ballot(sel[u]);
                }
            }
            // output order = position order = (lane, u): everything selected by lower lanes comes first
            const unsigned long long lt = lanemask_lt();
            uint32_t idx = nout, total = 0;
#pragma unroll
            for (int u = 0; u < PP; u++) { idx += (uint32_t)__popcll(bal[u] & lt); total += (uint32_t)__popcll(bal[u]); }
#pragma unroll
            for (int u = 0; u < PP; u++) {
                if (sel[u]) {
                    const unsigned j = jb + u;
                    const uint32_t p = hp_base + j;
                    if (idx < cap) {
                        // direction 1 iff the reverse complement is the canonical form, ties included (Kmer.hpp:427)
                        const uint32_t e = (u == 0 ? a0 : __builtin_amdgcn_alignbit(a1, a0, 2 * u)) & kmask;
                        a.out_min[cap0 + idx] = touches_invalid[u] ? 0xFFFFFFFFu : val[u];
                        a.out_pos[cap0 + idx] = p;
                        a.out_dir[cap0 + idx] = (uint8_t)(val[u] == (e ^ comp_mask) ? 1u : 0u);
                        if (HAS_QUAL) {
                            uint32_t os, oe;   // [rle[pos], rle[pos + K]) in original coordinates, or [.., rle[pos + K - 1]]
                            if (HPC) { os = Q->orig[j]; oe = Q->orig[j + K - a.q_last] + a.q_last; }
                            else { os = p; oe = p + K; }
                            if (a.inline_minq) {
                                const uint8_t *qq = a.qual + a.qual_off[r];
                                uint8_t mq = 255;   // getMinQuality (ReadSelection.hpp:1302-1320)
                                for (uint32_t bq = os; bq < oe; bq++) { uint8_t q = (uint8_t)(qq[bq] - 33); if (q < mq) mq = q; }
                                a.out_mqual[cap0 + idx] = mq;
                            } else {
                                a.out_os[cap0 + idx] = os;
                                a.out_oe[cap0 + idx] = oe;
                            }
                        }
                    }
                    idx++;
                }
            }
            nout += total;
        }
        return nout;
    }
};
// Waves per SIMD the register allocator must allow for the plain variant (no qualities, no N).  With the wave-uniform
// values in scalar registers it needs 76 VGPRs (6 waves fit); asking for 7 (72 VGPRs, no spill) makes the kernel no
// faster alone (14.0 vs 13.8 ms) and starves the other batch's table kernels when two batches are in flight; 8 spills.
#ifndef SCAN_MIN_WAVES
#define SCAN_MIN_WAVES 5
#endif

template <bool HPC, bool HAS_QUAL, bool HAS_N>
__global__ __launch_bounds__(SCAN_BLOCK, (HAS_QUAL || HAS_N) ? 1 : SCAN_MIN_WAVES) void scan_kernel(ScanArgs a) {
    __shared__ uint32_t lds_stream[SCAN_WAVES][STREAM_WORDS];
    __shared__ uint32_t lds_istream[HAS_N ? SCAN_WAVES : 1][HAS_N ? ISTREAM_WORDS : 1];
    __shared__ QualMap lds_qmap[(HAS_QUAL && HPC) ? SCAN_WAVES : 1];
    __shared__ alignas(16) uint8_t lds_lut[(HPC && !HAS_N) ? 2 * HPC_LUT_SIZE : 16];
    const uint8_t *lds_lut_b = lds_lut, *lds_lut_n = lds_lut + ((HPC && !HAS_N) ? HPC_LUT_SIZE : 0);
    if (HPC && !HAS_N) {
        hpc_lut_to_lds(lds_lut, threadIdx.x, SCAN_BLOCK);
        __syncthreads();
    }
    const unsigned lane = threadIdx.x & 63u;
    // everything that depends only on the wave (its read, the read's length, tile counts, stream lengths) is told to the
    // compiler as wave-uniform, so it lives in scalar registers and the loops around the tiles and trips are scalar branches
    const unsigned wv = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *S = lds_stream[wv];
    uint32_t *SI = lds_istream[HAS_N ? wv : 0];
    QualMap *Q = &lds_qmap[(HAS_QUAL && HPC) ? wv : 0];
    const unsigned K = a.K;
    const uint32_t kmask = (K >= 16) ? 0xFFFFFFFFu : ((1u << (2 * K)) - 1u);
    const uint32_t kbits = (1u << K) - 1u;
    const uint32_t comp_mask = 0xAAAAAAAAu & kmask;

    // a wave takes a few reads and retires (scan_blocks sizes the grid); written as a grid-stride loop
    const uint32_t wave_global = blockIdx.x * (SCAN_BLOCK / 64) + wv;
    const uint32_t n_waves = (gridDim.x * SCAN_BLOCK) >> 6;
    for (uint32_t slot = wave_global; slot < a.n_reads; slot += n_waves) {
        const uint32_t r = a.subset ? a.subset[slot] : slot;

        const uint32_t L = a.len[r];
        const uint64_t w_base = a.word_off[r];
        const uint64_t *rw = a.words + w_base;
        const uint32_t nwords = (L + 31u) / 32u;
        const uint32_t ntiles = (nwords + TILE_WORDS - 1) / TILE_WORDS;
        const uint64_t cap0 = a.cap_off[r];
        const uint32_t cap = (uint32_t)(a.cap_off[r + 1] - cap0);

        uint32_t carry = 0;        // last cb bases of the compressed stream, LSB-first
        uint32_t icarry = 0;       // their invalid bits (HAS_N)
        unsigned cb = 0;
        uint32_t hp_total = 0;     // compressed bases seen so far
        uint32_t nout = 0;
        uint32_t prev_last = 0;    // last base of the previous tile's last word
        uint32_t prev_inv = 0;     // its invalid bit (HAS_N)
        uint64_t cx_bound = 0;     // sum over windows of the 2-mer bound numerator
        uint64_t prev_word = 0;    // last word of the previous tile (complexity bound of lane 0)

        uint64_t x_next = (lane < nwords) ? rw[lane] : 0;

        for (uint32_t t = 0; t < ntiles; t++) {
            const uint64_t x = x_next;
            const uint32_t wi = t * TILE_WORDS + lane;
            {   // prefetch the next tile
                uint32_t nwi = wi + TILE_WORDS;
                x_next = (nwi < nwords) ? rw[nwi] : 0;
            }
            const int rem = (int)L - (int)(wi * 32u);
            const unsigned nvalid = rem <= 0 ? 0u : (rem >= 32 ? 32u : (unsigned)rem);
            const uint64_t vspread = nvalid == 32 ? M5 : (((1ull << (2 * nvalid)) - 1ull) & M5);
            uint32_t iv = 0;
            if (HAS_N) iv = (wi < nwords) ? a.invalid[w_base + wi] : 0u;

            // ---- complexity: upper bound from per-word 2-mer counts --------------------------------
            // window w = words w, w+1 (64 positions).  With a_v / b_v the 2-mer counts of the two words,
            // sum_v (a_v + b_v)^2 <= 2 (Q_w + Q_{w+1}),  Q = sum_v count^2, and 3-mer collisions <= 2-mer
            // collisions, so  S_w <= Q_w + Q_{w+1} - 32.  Each word's Q enters at most two windows.  (Q here is sq(w) of
            // complexity_dev.hpp, which computes it as 64 + Q'/4 and moves the constants into the one compare per read.)
            // Lane l evaluates the word BEFORE its own (lane 0: the last word of the previous tile): the base
            // after that word is the lane's own first base, so nothing here waits for the prefetched tile.
#if defined(SCAN_ABLATE) && SCAN_ABLATE == 3
            if (false) {                                                                          // ablation: no complexity bound
#else
            if (a.apply_filters) {
#endif
                uint64_t xp = __shfl_up(x, 1, 64);
                if (lane == 0) xp = prev_word;
                prev_word = __shfl(x, 63, 64);
                if (wi >= 1u && (uint64_t)wi * 32u + 1u <= L) {          // word wi-1 is full and has a successor base
                    const uint32_t wq = wi - 1u;
                    const uint32_t mult = complexity_word_weight(wq, complexity_windows(L));
                    if (mult) cx_bound += (uint64_t)mult * word_pair_q(xp, (uint32_t)x);
                }
            }

            // ---- 1. run starts / compaction ---------------------------------------------------
            const uint32_t tile_base_now = t * TILE_WORDS * 32u;
            uint64_t y, d;
            unsigned c;
            if (HPC) {
                uint32_t pl = (uint32_t)__shfl_up((uint32_t)(x >> 62), 1, 64);
                if (lane == 0) pl = prev_last;
                if (!HAS_N) {
                    // the first base of the read starts a run whatever precedes it: pretend a different base does
                    if (wi == 0) pl = ((uint32_t)x & 3u) ^ 1u;
                    unsigned nbits;
                    y = compress_pairs_lut(HpcLut{lds_lut_b, lds_lut_n}, x, pl, &nbits);
                    c = nbits >> 1;
                    d = 0;
                    if (HAS_QUAL || nvalid < 32) {
                        // run-start flags themselves: needed for the coordinate map, and to cut a partial word
                        // (zero padding after the last base may look like one more run start)
                        uint64_t diff = x ^ ((x << 2) | (uint64_t)pl);
                        d = (diff | (diff >> 1)) & vspread;
                        c = (unsigned)__popcll(d);
                        y &= c >= 32 ? ~0ull : ((1ull << (2 * c)) - 1ull);
                    }
                } else {
                    uint64_t diff = x ^ ((x << 2) | (uint64_t)pl);
                    d = (diff | (diff >> 1)) & M5;
                    // a change of the invalid bit also starts a run (N vs G share code 3)
                    uint32_t pi = (uint32_t)__shfl_up(iv >> 31, 1, 64);
                    if (lane == 0) pi = prev_inv;
                    d |= spread_bits(iv ^ ((iv << 1) | pi));
                    // ... and so does any other change of character ("aA", IUPAC letters sharing a code): HPC compares
                    // characters (Commons.hpp:4177-4178)
                    if (a.brk) d |= spread_bits((wi < nwords) ? a.brk[w_base + wi] : 0u);
                    prev_inv = (uint32_t)__shfl(iv >> 31, 63, 64);
                    if (wi == 0) d |= 1ull;
                    d &= vspread;
                    c = (unsigned)__popcll(d);
                    y = compress_pairs(x, d);
                }
                prev_last = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 62), 63);
            } else {
                d = vspread;
                c = nvalid;
                y = x & (vspread | (vspread << 1));
            }
            const unsigned inc = wave_inclusive_sum(c);
            const unsigned o = inc - c;
            const unsigned C = (unsigned)__builtin_amdgcn_readlane((int)inc, 63);

            // ---- 2. LDS bit stream: [carry (cb bases)] [new C bases] ---------------------------
            S[lane] = 0;
            S[lane + 64] = 0;
            if (lane < STREAM_WORDS - 128) S[lane + 128] = 0;
            if (HAS_N) { SI[lane] = 0; if (lane < ISTREAM_WORDS - 64) SI[lane + 64] = 0; }
            if (HAS_QUAL && HPC) {
                // d: bit 2i set iff base i of this lane's word starts a run; the r-th set bit is stream position cb + o + r
                uint32_t *dst = Q->orig + cb + o;
                const uint32_t w0 = tile_base_now + lane * 32u;
#pragma unroll
                for (int half = 0; half < 2; half++) {          // 32-bit halves: cheaper bit scans than on the u64
                    uint32_t m = half ? (uint32_t)(d >> 32) : (uint32_t)d;
                    const uint32_t wb = w0 + 16u * half;
                    while (m) {
                        *dst++ = wb + (((uint32_t)__ffs((int)m) - 1u) >> 1);
                        m &= m - 1u;
                    }
                }
            }
            wave_lds_sync();
            if (lane == 0 && cb) { atomicOr(&S[0], carry); if (HAS_N && icarry) atomicOr(&SI[0], icarry); }
            if (c) {
                unsigned dst = 2u * (cb + o), w = dst >> 5, sh = dst & 31u;
                uint32_t yl = (uint32_t)y, yh = (uint32_t)(y >> 32);
                uint32_t p0 = yl << sh;
                uint32_t p1 = sh ? ((yl >> (32u - sh)) | (yh << sh)) : yh;
                uint32_t p2 = sh ? (yh >> (32u - sh)) : 0u;
                atomicOr(&S[w], p0);
                if (p1) atomicOr(&S[w + 1], p1);
                if (p2) atomicOr(&S[w + 2], p2);
                if (HAS_N) {
                    uint32_t ic = HPC ? compress_bits(iv, d) : (iv & (nvalid == 32 ? 0xFFFFFFFFu : ((1u << nvalid) - 1u)));
                    if (ic) {
                        unsigned di = cb + o, wq = di >> 5, sq = di & 31u;
                        atomicOr(&SI[wq], ic << sq);
                        if (sq && (ic >> (32u - sq))) atomicOr(&SI[wq + 1], ic >> (32u - sq));
                    }
                }
            }
            wave_lds_sync();

            // ---- 3./4. k-mers, hash, select, compact -------------------------------------------
            const unsigned tot = cb + C;
            const unsigned nk = tot > K ? tot - K : 0u;
            const uint32_t hp_base = hp_total - cb;    // compressed-stream position of S base 0
            const uint32_t tile_base = t * TILE_WORDS * 32u;
            // Each lane takes PP ADJACENT positions per trip: one LDS read and one digit reversal serve all of
            // them (the forward k-mer of the next position is a shift-in of one base), and the PP hash chains
            // interleave.  The last trip of a tile uses the smallest PP that covers what is left.
            for (unsigned j0 = 0; j0 < nk; j0 += 64 * SCAN_PP) {
                const unsigned left = nk - j0;
                const unsigned pp = left >= 64u * SCAN_PP ? (unsigned)SCAN_PP : (left + 63u) / 64u;
                KmerTrip<HPC, HAS_QUAL, HAS_N> trip{a, S, SI, Q, K, kmask, kbits, comp_mask, lane, nk, hp_base, cb, tile_base, cap0, cap, r};
                // full trips are interior unless this is the trimmed start of the read
                if (pp == (unsigned)SCAN_PP && left >= 64u * SCAN_PP && hp_base + j0 >= a.trim) {
                    nout = trip.template run<SCAN_PP, true>(j0, nout);
                } else {
#if SCAN_PP <= 4
                    switch (pp) {
                        case 1: nout = trip.template run<1, false>(j0, nout); break;
                        case 2: nout = trip.template run<2, false>(j0, nout); break;
                        case 3: nout = trip.template run<3, false>(j0, nout); break;
                        default: nout = trip.template run<4, false>(j0, nout); break;
                    }
#else
                    if (pp <= 2) nout = trip.template run<2, false>(j0, nout);
                    else if (pp <= 4) nout = trip.template run<4, false>(j0, nout);
                    else nout = trip.template run<SCAN_PP, false>(j0, nout);
#endif
                }
            }

            // ---- carry the last min(tot, K) bases ----------------------------------------------
            const unsigned cbn = tot < K ? tot : K;
            const uint32_t cmask = (cbn >= 16) ? 0xFFFFFFFFu : ((1u << (2 * cbn)) - 1u);
            carry = cbn ? stream_extract(S, tot - cbn, cmask) : 0u;
            if (HAS_N) icarry = cbn ? istream_extract(SI, tot - cbn, (1u << cbn) - 1u) : 0u;
            uint32_t my_orig = 0;
            if (HAS_QUAL && HPC) { if (lane < cbn) my_orig = Q->orig[tot - cbn + lane]; }
            cb = cbn;
            hp_total += C;
            wave_lds_sync();   // all reads of S / Q done before the next tile rewrites them
            if (HAS_QUAL && HPC) { if (lane < cbn) Q->orig[lane] = my_orig; }
        }

        // ---- _trimBps == 0 (GenerateGfa.hpp:366): the last l-mer, which the tiles never evaluate because
        // no base follows it.  Its K bases are the carry; one lane does the work.
        if (a.trim == 0u && hp_total >= K) {
            if (HAS_QUAL && HPC) wave_lds_sync();   // carry_orig of the last tile
            const uint32_t e = carry & kmask;
            const uint32_t rev = e ^ comp_mask, fwd = digit_reverse(e, K);
            const uint32_t d = fwd < rev ? 0u : 1u;
            uint32_t v = d ? rev : fwd;
            bool s1 = kmer_hash32(v) < a.threshold;
            if (HAS_N && icarry != 0u) { s1 = a.select_invalid != 0u; v = 0xFFFFFFFFu; }      // (as in KmerTrip::run)
            if (s1 && a.n_rep) s1 = !rep_contains(a.rep, a.n_rep, v);
            if (s1) {
                if (lane == 0 && nout < cap) {
                    const uint32_t p = hp_total - K;
                    a.out_min[cap0 + nout] = v;
                    a.out_pos[cap0 + nout] = p;
                    a.out_dir[cap0 + nout] = (uint8_t)d;
                    if (HAS_QUAL) {
                        const uint32_t os = HPC ? Q->orig[0] : p;
                        const uint32_t oe = a.q_last ? (HPC ? Q->orig[K - 1] : p + K - 1u) + 1u : L;
                        if (a.inline_minq) {
                            const uint8_t *qq = a.qual + a.qual_off[r];
                            uint8_t mq = 255;
                            for (uint32_t bq = os; bq < oe; bq++) { uint8_t q = (uint8_t)(qq[bq] - 33); if (q < mq) mq = q; }
                            a.out_mqual[cap0 + nout] = mq;
                        } else {
                            a.out_os[cap0 + nout] = os;
                            a.out_oe[cap0 + nout] = oe;
                        }
                    }
                }
                nout++;
            }
        }

        // ---- per-read epilogue -----------------------------------------------------------------
        uint8_t flags = 0;
        if (a.apply_filters && L >= 66) {
            // sum_w (sq_w + sq_{w+1}) - 32 nW over 61 nW >= true mean score; only reads whose bound exceeds ~4.9 need the exact
            // pass, which runs as its own (rare) kernel so its registers do not cap this kernel's occupancy
            // (sum of sq > 332 nW, taken on the +-1 form: complexity_dev.hpp)
            if (complexity_suspect(wave_sum_u64(cx_bound), complexity_windows(L))) flags |= READ_SUSPECT;
        }
        if (lane == 0) {
            a.out_count[r] = nout;
            a.out_flags[r] = flags;
        }
    }
}

// ================================================================================================================
// scan_fast_kernel<HPC> -- the variant every upper-case ACGT FASTA batch takes (no qualities, no side masks).
//
// Same arithmetic as scan_kernel, reorganised around what the instructions cost on gfx950 (tools/ubench/op_rates.hip,
// profiles/r02a_op_rates_gfx950.txt: and/or/xor/add/sub/right shifts/v_bitop3 issue in 2.6 cycles per wave64, everything
// else -- left shifts, min, compares, v_alignbit, DPP, every multiply -- in 4.4 to 4.8, a scalar instruction in 2.1, an
// LDS read in 9, an LDS write or atomic in 17):
//   * the compressed bases go to a per-wave LDS RING (8192 bases); whenever 2048 positions are complete (each followed
//     by a known base) the wave hashes them as one BLOCK: lane l owns the 32 CONTIGUOUS positions 32 l .. 32 l + 31, reads
//     its three stream words once and walks them in registers with compile-time shifts -- one v_alignbit per position,
//     the forward k-mer rolled by one base, no address arithmetic, no scalar bookkeeping, no branches;
//   * "selected" is recorded with two instructions per position (v_cmp + v_addc: a per-lane bit vector); the few selected
//     positions of a block (about 10 of 2048) are materialised ONCE PER BLOCK, the lanes that own one recomputing its
//     value from the ring -- instead of ballots, prefix counts and exec-masked stores after every 256 positions;
//   * the minimizers of a read are staged in LDS and leave in coalesced rows;
//   * the tail of a read (at most 2048 positions) runs the same arithmetic on spans of exactly ceil(npos / 64) <= 32
//     positions per lane, two half spans side by side like the block, its stream words read once and the steps counted
//     by a scalar loop.
// ================================================================================================================
constexpr int FAST_BLOCK = 256;                       // threads per workgroup (4 independent waves)
constexpr int FAST_WAVES = FAST_BLOCK / 64;
constexpr unsigned RING_BASES = 16384;                // per wave: DEFER_BLOCKS blocks awaiting materialisation + 2 * 2048 + 16 + 1 live bases
constexpr unsigned DEFER_BLOCKS = 3;                  // blocks whose selected positions may wait in the list before they are materialised
constexpr unsigned SPAN = 32;                         // positions per lane in a full block
constexpr unsigned BLOCK_POS = 64 * SPAN;             // 2048
constexpr bool DUAL_CHAIN = true;                      // the unrolled block walks two half spans of a lane side by side (aligned_block)
constexpr int STAGE_CAP = 384;                        // minimizers of one read staged per wave before a flush

// One position of a lane's span: canonical k-mer from the 32 stream bits T that start at the position, Murmur3, compare,
// and the verdict shifted into `bits` (the oldest position ends up in the highest of the bits used).
struct SpanState {
    uint32_t fwd;         // forward k-mer of the previous position
    uint32_t bits;
};

// APPROX: the verdict is taken on the upper half of the hash with the finalisers' last multiplications merged into one
// (kmer_hash32_hi_merged, murmur.hpp): s = that is hi(hash), hi(hash) + 1 or hi(hash) + 2, so  hash < threshold  implies
// s < hi(threshold) + 3.  The positions recorded are a superset of the selected ones, off by about one in 2^31; every one of
// them is hashed in full when it is materialised (emit), and a read with a false one is handed to the general kernel.
// (Rounds 2 - 5 took hi(mix a) + hi(mix b) + 1 by two separate multiplications: 9 cycles per position more.)
// K15 (l = 15, what the reference's presets use): the digit that enters the forward k-mer at this position is the top digit of
// the PREVIOUS position's 32 stream bits, so the roll is one v_alignbit and a mask instead of shift, field extract and merge.
template <bool APPROX, bool K15 = false>
__device__ __forceinline__ void span_step(SpanState &st, uint32_t T, bool first, uint32_t kmask, uint32_t comp_mask, unsigned top_shift,
                                          unsigned K, uint64_t threshold, uint32_t cand_limit, uint32_t Tprev = 0u) {
    const uint32_t rev = (T ^ comp_mask) & kmask;                      // complement of every digit, already in reversed order
    // forward k-mer: digits in reading order; rolled: drop the oldest digit, append the newest (the top digit of T's k-mer)
    if (K15) st.fwd = first ? digit_reverse(T & kmask, K) : (__builtin_amdgcn_alignbit(st.fwd, Tprev, 30) & kmask);
    else st.fwd = first ? digit_reverse(T & kmask, K) : (((st.fwd << 2) | ((T >> top_shift) & 3u)) & kmask);
    const uint32_t val = st.fwd < rev ? st.fwd : rev;
    if (APPROX) {
        const uint32_t s1 = kmer_hash32_hi_merged(val);
        asm("v_cmp_lt_u32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(st.bits) : "v"(s1), "s"(cand_limit) : "vcc");
    } else {
        const uint64_t h = kmer_hash32(val);
        // bits = 2 * bits + (h < threshold): one compare into vcc, one add-with-carry
        asm("v_cmp_lt_u64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(st.bits) : "v"(h), "s"(threshold) : "vcc");
    }
}

// the 32 stream bits that start at ring position p (any p), from LDS
__device__ __forceinline__ uint32_t ring_window(const uint32_t *S, unsigned p, unsigned wmask) {
    const unsigned b = 2u * p, w = (b >> 5) & wmask, sh = b & 31u;
    return __builtin_amdgcn_alignbit(S[(w + 1) & wmask], S[w], sh);
}

// QUAL (reads with qualities): the minimum quality over every minimizer's ORIGINAL bases (getMinQuality,
// ReadSelection.hpp:1302-1320; ReadCorrection.hpp:2467-2481) is taken when the minimizer is materialised and travels with its
// row.  Without homopolymer compression original and compressed coordinates coincide.  With it, rlePositions[j] -- the original
// start of run j (Commons.hpp:4188-4190) -- is looked up for the few selected positions only, instead of being stored for all
// of them: per tile every lane keeps its offset in the compressed stream (HIST_TILES tiles back, 2 bytes per word), a selected
// lane finds the tile, then the word (binary search over the 64 offsets), re-reads that word and picks the k-th run start.
constexpr int HIST_TILES = 8;

// PFW > 0: the PRE-FILTERED variant (HPC, l = 15, no qualities, APPROX, no slack: launch_scan).  Which canonical keys a compressed
// read can produce and which of them are selected is fixed by (l, threshold): the walks probe a bitmap of the selected keys in LDS
// (prefilter.hpp) instead of hashing -- one multiply, one shift, one ds_read_u8 and two field extracts a position where the candidate
// hash takes 28 instructions -- and the positions that pass (8.65 % false positives + the selected ones, about 190 of a block's
// 2048) are listed and hashed in full 64 at a time; the lane that confirms one holds its position, both orientations and the verdict,
// and writes the finished row to the stage from there (confirm): the variant has no emit, no materialise and defers no block.
// The bitmap exists once per CU: ONE workgroup of PFW = 16 (or 8) waves per CU copies its 64 KB at set-up.  What a wave owns shrinks
// to make room beside it: a ring of 8192 bases (released after every block), a stage of PF_STAGE_CAP rows and a list of
// PF_LIST_CAP candidate positions.  The waves of a workgroup take reads from a
// counter in LDS over the workgroup's chunk of reads, so that a CU is not left to the slowest of 16 fixed shares.
constexpr unsigned PF_RING_BASES = 8192;              // per wave: 2 * 2048 + 16 + 1 live bases = 4113 (a power of two)
constexpr unsigned PF_DEFER_BLOCKS = 0;               // a block's rows are finished when its confirmation is: the ring keeps none
constexpr int PF_STAGE_CAP = 176;
constexpr unsigned PF_LIST_CAP = 224;                 // candidate positions confirmed per pass (a block has 187 +- 13; more take further passes)
template <int PFW> struct FastGeometry {
    static constexpr bool PF = PFW > 0;
    static constexpr int WAVES = PF ? PFW : FAST_WAVES, BLOCK = 64 * WAVES, STAGE = PF ? PF_STAGE_CAP : STAGE_CAP;
    static constexpr unsigned RING = PF ? PF_RING_BASES : RING_BASES, DEFER = PF ? PF_DEFER_BLOCKS : DEFER_BLOCKS;
    static constexpr unsigned RING_WORDS = RING / 16, RING_WMASK = RING_WORDS - 1;      // u32 words of the ring
    // LDS of a workgroup of the pre-filtered variant: bitmap, tables, per wave ring + stage + list, the read counter
    static constexpr size_t PF_LDS = PREFILTER_BYTES + 2 * HPC_LUT_SIZE + REP_FILTER_BITS / 8 + 16 +
                                     (size_t)WAVES * (RING / 4 + STAGE * 8 + PF_LIST_CAP * 2);
};
static_assert(FastGeometry<16>::PF_LDS + 28672 <= 163840, "16 waves fit beside the 28 KB the benchmark's other batch asks for");

// SEG: the items are VIEWS of long reads (segments_dev.hpp; mdbg_scan, "scan_segments") instead of reads.  A view is scanned like a
// read that begins at a tile of its read and ends one tile behind its segment, with four differences: the base in front of it is the
// read's (no run start is made up, the complexity bound's boundary word is the read's), the end trim applies at the read's ends only,
// it lists the windows it OWNS and no others, and its words enter the complexity sum with the weights of their place in the whole read --
// the sum goes to view_cx and the decision is taken once per read, after the join.  Rows carry view positions; the join adds c_s.
template <bool HPC, bool QUAL, bool APPROX, int PFW = 0, bool SEG = false>
__global__ __launch_bounds__(FastGeometry<PFW>::BLOCK, PFW ? PFW / 4 : 5) void scan_fast_kernel(ScanArgs a) {
    using Geo = FastGeometry<PFW>;          // this instantiation's workgroup, ring and stage
    constexpr bool PF = Geo::PF;
    static_assert(!PF || (HPC && !QUAL && APPROX), "the bitmap holds the keys of compressed reads; its candidates are confirmed like APPROX ones");
    static_assert(Geo::DEFER * BLOCK_POS + 2 * BLOCK_POS + 17 <= Geo::RING, "deferred blocks + live bases fit the ring");
    // PF: the variant needs 92 - 93 vector registers, one granule of eight less than the 104 it is allotted beside the first pass's
    // kernels (tests/test_gpu_step_residency.py pins which of them fit beside it).  Which kernels share a CU with the scan
    // is a decision of its own, with a measurement of its own: the allotment stays 104 -- v103 is named here, where nothing is live
    if constexpr (PF) asm volatile("" ::: "v103");
    __shared__ uint8_t lds_stage_q[QUAL ? Geo::WAVES : 1][QUAL ? Geo::STAGE : 1];
    __shared__ uint16_t lds_hist_o[(QUAL && HPC) ? Geo::WAVES * HIST_TILES * 64 : 1];
    __shared__ uint32_t lds_hist_c[(QUAL && HPC) ? Geo::WAVES : 1][(QUAL && HPC) ? HIST_TILES : 1];
    __shared__ alignas(16) uint32_t lds_ring[Geo::WAVES][Geo::RING_WORDS];
    __shared__ uint2 lds_stage[Geo::WAVES][Geo::STAGE];
    __shared__ alignas(16) uint8_t lds_lut[HPC ? 2 * HPC_LUT_SIZE : 16];
    const uint8_t *lds_lut_b = lds_lut, *lds_lut_n = lds_lut + (HPC ? HPC_LUT_SIZE : 0);
    // the repetitive minimizers (ONT: a hundred or so values, sorted, in global memory) behind a filter of REP_FILTER_BITS bits: a
    // candidate whose bit is clear is not among them, and only the others pay the binary search -- eight dependent loads that a
    // lane of every block used to wait for (9 % of the ONT scan: profiles/round6_p_scan_ablation_ont_before_the_repetitive_filter_in_lds.txt, round6_q_* after)
    __shared__ alignas(16) uint32_t lds_rep_filter[REP_FILTER_BITS / 32];
    // block set-up, once per workgroup (8 reads of the four-wave kernel, 32 of the 16-wave variant): everything in 16-byte LDS stores (the table image: one load and one store for half the threads)
    if (HPC) hpc_lut_to_lds(lds_lut, threadIdx.x, Geo::BLOCK);
    static_assert((Geo::WAVES * Geo::RING_WORDS) % (4 * Geo::BLOCK) == 0 && (REP_FILTER_BITS / 32) % 4 == 0, "cleared as uint4");
#pragma unroll
    for (unsigned i = 0; i < Geo::WAVES * Geo::RING_WORDS / 4u; i += Geo::BLOCK) reinterpret_cast<uint4 *>(&lds_ring[0][0])[i + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    if (threadIdx.x < REP_FILTER_BITS / 128u) reinterpret_cast<uint4 *>(lds_rep_filter)[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    // PF: the bitmap from global memory (it stays in L2 between workgroups), the workgroup's read counter, the waves' lists
    const uint8_t *pf_map = nullptr;
    uint16_t *pf_list_all = nullptr;
    uint32_t *pf_next = nullptr;
    if constexpr (PF) {
        __shared__ alignas(16) uint32_t lds_pf_map[PREFILTER_BYTES / 4];
        __shared__ uint16_t lds_pf_list[Geo::WAVES][PF_LIST_CAP];
        __shared__ uint32_t lds_pf_next;
        for (unsigned i = threadIdx.x; i < PREFILTER_BYTES / 16u; i += Geo::BLOCK)
            reinterpret_cast<uint4 *>(lds_pf_map)[i] = reinterpret_cast<const uint4 *>(a.pf_bits)[i];
        if (threadIdx.x == 0) lds_pf_next = 0u;
        pf_map = reinterpret_cast<const uint8_t *>(lds_pf_map);
        pf_list_all = &lds_pf_list[0][0]; pf_next = &lds_pf_next;
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < a.n_rep; i += Geo::BLOCK) {
        const uint32_t b = rep_filter_bit(a.rep[i]);
        atomicOr(&lds_rep_filter[b >> 5], 1u << (b & 31u));
    }
    __syncthreads();
    // the kernel is bound by instruction issue: next to the table kernels of other batches (bound by memory latency) its waves
    // go first on their SIMD
    if (a.wave_priority == 1u) __builtin_amdgcn_s_setprio(1);
    else if (a.wave_priority == 2u) __builtin_amdgcn_s_setprio(2);
    else if (a.wave_priority >= 3u) __builtin_amdgcn_s_setprio(3);
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wv = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *S = lds_ring[wv];
    uint2 *stage = lds_stage[wv];
    uint8_t *stage_q = lds_stage_q[QUAL ? wv : 0];
    uint16_t *hist_o = lds_hist_o + ((QUAL && HPC) ? wv * HIST_TILES * 64 : 0);      // [tile % HIST_TILES][lane]
    uint32_t *hist_c = lds_hist_c[(QUAL && HPC) ? wv : 0];
    const unsigned K = a.K;
    const uint32_t kmask = (K >= 16) ? 0xFFFFFFFFu : ((1u << (2 * K)) - 1u);
    const uint32_t comp_mask = 0xAAAAAAAAu & kmask;
    const unsigned top_shift = 2u * K - 2u;
    const uint64_t threshold = a.threshold;
    // APPROX (bump mode only: a read with a false candidate needs the host's re-run): see span_step.  cand_slack widens the
    // superset on purpose (tests of the re-run path)
    // (saturating: a threshold near 2^64 -- densities close to 1 -- must not wrap the limit around to "nothing is a candidate")
    const uint64_t cand_limit64 = (threshold >> 32) + 3ull + (uint64_t)a.cand_slack;
    const uint32_t cand_limit = cand_limit64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cand_limit64;
    // APPROX: the position loops hash with the finalisers' upper half shared (kmer_hash32_hi_shared_x2, murmur.hpp), which is the
    // candidate value exactly when the guard word is >= 68.  A lane keeps the minimum g of its span's guard words; a lane with
    // g < guard_limit walks its span again with the exact candidate test (guarded_redo), so the candidates are the same set in
    // every case.  guard_slack widens the test on purpose (tests of that slow path: any value is valid, the slow path is exact)
    const uint64_t guard_limit64 = 68ull + (uint64_t)a.guard_slack;
    const uint32_t guard_limit = guard_limit64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)guard_limit64;
    // GUARD (compile-time, beside K15): under HPC with l = 15 no guard is needed.  Every hashed window of a compressed read, forward
    // or reverse complement, has no two equal adjacent digits; of the 2^32 keys 65 fail the guard, 14 of them are below 2^30 and
    // every one of those has an adjacent repeat -- proved by enumeration, tests/test_murmur_shared_hi_host.py.  (A window that
    // reaches past `fill` holds zeros and may hash to anything: emit masks those positions whatever they hash to.)  So that
    // instantiation carries no minimum, no ballot and no slow path; every other l, uncompressed reads and any guard_slack take
    // the guarded one.
    const bool unguarded = HPC && K == 15u && a.guard_slack == 0u;

    const uint32_t wave_global = blockIdx.x * Geo::WAVES + wv;
    const uint32_t n_waves = gridDim.x * Geo::WAVES;
    // PF: this wave's list of candidate positions, the bitmap's shift
    uint16_t *pf_list = PF ? pf_list_all + wv * PF_LIST_CAP : nullptr;
    const uint32_t pf_shift = a.pf_shift;
    const uint4 *const pf_table = PF ? a.pf_table : nullptr;      // wave-uniform; null: confirm hashes its candidates
    const uint32_t pf_table_shift = a.pf_table_shift;
    // PF: the workgroup's chunk of reads [chunk0, chunk0 + chunk_n) is dealt out read by read; NO_READ when it is used up
    constexpr uint32_t NO_READ = 0xFFFFFFFFu;               // no read has this index: n_reads is a 32-bit count
    const uint64_t chunk0 = (uint64_t)blockIdx.x * a.pf_chunk;
    const uint32_t chunk_n = PF ? (chunk0 >= a.n_reads ? 0u : (uint32_t)(a.n_reads - chunk0 < a.pf_chunk ? a.n_reads - chunk0 : a.pf_chunk)) : 0u;
    // ... or, in the persistent launch, runs of pf_grab consecutive items come from one counter in device memory for the whole grid
    // (scan_plan.hpp: persistent_run_end, persistent_region).  run_next .. run_end is what is left of this wave's run; all wave-uniform
    unsigned long long *const pf_counter = PF ? a.pf_counter : nullptr;
    uint32_t run_next = 0, run_end = 0, run_region = 0;
    auto take_read = [&]() -> uint32_t {
        if (pf_counter) {
            if (run_next == run_end) {
                uint32_t lo = 0, hi = 0;
                if (lane == 0) {
                    const unsigned long long s0 = __hip_atomic_fetch_add(pf_counter, (unsigned long long)a.pf_grab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    lo = (uint32_t)s0; hi = (uint32_t)(s0 >> 32);
                }
                lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo); hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)hi);
                if (hi || lo >= a.n_reads) return NO_READ;        // used up: this wave leaves
                run_next = lo;
                run_end = a.n_reads - lo < a.pf_grab ? a.n_reads : lo + a.pf_grab;        // the last run is clipped
                run_region = (lo / a.pf_grab) & (a.n_regions - 1u);
            }
            return run_next++;
        }
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(pf_next, 1u);
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        return k < chunk_n ? (uint32_t)chunk0 + k : NO_READ;
    };
    for (uint32_t r = PF ? take_read() : wave_global; PF ? r != NO_READ : r < a.n_reads; r = PF ? take_read() : r + n_waves) {
        if constexpr (PF && !SEG) { if (a.pf_len_split && a.len[r] >= a.pf_len_split) continue; }      // the four-wave launch's read
        if (!SEG && a.skip && a.skip[r]) {          // a read with an N or a case flip: the host sends it through the general kernel
            if (a.cursor && lane == 0) { a.out_begin[r] = 0; a.out_count[r] = 0; a.out_flags[r] = 0; }
            continue;
        }
        SegView view{};
        if constexpr (SEG) {
            view = a.views[r];
            if (view.flags & SEG_DEAD) {        // a view of an unsegmentable read: the read is scanned whole elsewhere
                if (lane == 0) { a.out_begin[r] = 0; a.out_count[r] = 0; a.out_flags[r] = 0; a.view_cx[r] = 0ull; }
                continue;
            }
        }
        const uint32_t rd = SEG ? view.read : r;                       // the read whose words, qualities and length these are
        const bool seg_inner = SEG && !(view.flags & SEG_FIRST);       // a view with the read's own bases in front of it
        const uint32_t L = SEG ? view.raw_len : a.len[r];
        const uint64_t w_base = a.word_off[rd] + (SEG ? (uint64_t)view.tile0 * TILE_WORDS : 0ull);
        const uint64_t *rw = a.words + w_base;
        // the end trim in front (Kmer.hpp:1395) is the read's: its first view's
        const uint32_t trim_first = seg_inner ? 0u : a.trim;
        const uint32_t nwords = (L + 31u) / 32u;
        const uint32_t ntiles = (nwords + TILE_WORDS - 1) / TILE_WORDS;
        const bool bump = PF || a.cursor != nullptr;      // (every launch of the variant has a cursor: launch_scan, choose_prefilter)
        const uint64_t cap0 = bump ? 0ull : a.cap_off[r];
        const uint32_t cap = bump ? 0u : (uint32_t)(a.cap_off[r + 1] - cap0);
        uint32_t t_done = 0;       // raw tiles appended to the ring so far (HPC && QUAL: their offsets are in hist_*)
        uint32_t fill = 0;         // compressed bases written to the ring so far (= stream length)
        bool outgrown = false;     // the read selected more than the stage holds, or needs a run start the history no longer has:
                                   // listed, placed and re-run by the host with the general kernel

        // rlePositions[j]: the original coordinate of compressed position j (HPC && QUAL); j == fill at the end of the read is the
        // sentinel `length` (Commons.hpp:4188-4190).  0xFFFFFFFF: the tile is no longer in the history.
        auto orig_of = [&](uint32_t j, bool at_end) -> uint32_t {
            if (at_end && j >= fill) return L;
            uint32_t tt = t_done - 1u;
            const uint32_t t_low = t_done > (uint32_t)HIST_TILES ? t_done - (uint32_t)HIST_TILES : 0u;
            while (tt > t_low && hist_c[tt % HIST_TILES] > j) tt--;
            const uint32_t c0 = hist_c[tt % HIST_TILES];
            if (c0 > j) return 0xFFFFFFFFu;
            const uint32_t rel = j - c0;
            const uint16_t *o = hist_o + (tt % HIST_TILES) * 64u;
            uint32_t lo = 0;           // last word whose first run starts at or before rel: three rounds of three reads each
#pragma unroll
            for (uint32_t st = 16; st >= 1; st >>= 2) {
                const uint32_t o1 = o[lo + st], o2 = o[lo + 2 * st], o3 = o[lo + 3 * st];
                lo += st * ((o1 <= rel ? 1u : 0u) + (o2 <= rel ? 1u : 0u) + (o3 <= rel ? 1u : 0u));
            }
            uint32_t k = rel - o[lo];
            const uint32_t wi = tt * TILE_WORDS + lo;
            const uint64_t x = rw[wi];
            const uint32_t pl = (wi || seg_inner) ? (uint32_t)(rw[(int64_t)wi - 1] >> 62) : (((uint32_t)x & 3u) ^ 1u);   // the first base of the read starts a run
            const int rem = (int)L - (int)(wi * 32u);
            const unsigned nvalid = rem >= 32 ? 32u : (unsigned)rem;
            const uint64_t vspread = nvalid == 32 ? M5 : (((1ull << (2 * nvalid)) - 1ull) & M5);
            const uint64_t diff = x ^ ((x << 2) | (uint64_t)pl);
            uint64_t m = (diff | (diff >> 1)) & vspread;          // bit 2i: base i starts a run
            uint32_t pos = 0;
#pragma unroll
            for (int sh = 32; sh >= 2; sh >>= 1) {                // the k-th set bit (k counted from 0)
                const uint32_t c = (uint32_t)__popcll(m & ((1ull << sh) - 1ull));
                if (k >= c) { k -= c; m >>= sh; pos += (uint32_t)sh; }
            }
            return wi * 32u + (pos >> 1);
        };
        const uint8_t *qq = QUAL ? a.qual + a.qual_off[rd] + (SEG ? (uint64_t)view.tile0 * SEG_TILE_BASES : 0ull) : nullptr;
        // minimum quality of the minimizer at compressed position j; unknown = false when a run start has left the history
        auto min_quality = [&](uint32_t j, bool &known) -> uint8_t {
            uint32_t os = j, oe = j + K;
            if (HPC) {     // [rle[pos], rle[pos + l]) (ReadSelection.hpp:1135) or [rle[pos], rle[pos + l - 1]] (ReadCorrection.hpp:2340)
                os = orig_of(j, false);
                const uint32_t last = orig_of(j + K - a.q_last, true);
                if (os == 0xFFFFFFFFu || last == 0xFFFFFFFFu) { known = false; return 0; }
                oe = last + a.q_last;
            }
            // 16 bytes per step in two unaligned 8-byte loads (the quality buffer is padded by 32 bytes) instead of a chain of
            // dependent byte loads: a selected lane would otherwise wait longer than its whole block took to hash
            uint8_t mq = 255;
            for (uint32_t b0 = os; b0 < oe; b0 += 16) {
                uint64_t w[2];
                __builtin_memcpy(w, qq + b0, 16);
                const uint32_t nb = oe - b0 < 16u ? oe - b0 : 16u;
#pragma unroll
                for (unsigned b = 0; b < 16; b++) {
                    const uint8_t q = (uint8_t)((uint8_t)(w[b >> 3] >> (8 * (b & 7))) - 33);
                    if (b < nb && q < mq) mq = q;
                }
            }
            return mq;
        };

        bool lost = false;         // per lane: a quality span could not be resolved, or a recorded position turned out not to be
                                   // selected (APPROX): folded into `outgrown` at the end of the read
        uint32_t n_false = 0;      // APPROX: recorded positions the full hash rejected (the read's count is nout - n_false)
        uint32_t n_staged_at_outgrowth = 0;     // APPROX: rows in the stage when the read outgrew it
        uint32_t done = 0;         // positions already evaluated (= ring position of the next block, a multiple of 2048)
        uint32_t nout = 0;         // minimizers of this read so far
        uint32_t flushed = 0;      // ... of which already written to the output slot
        uint32_t n_mat = 0;        // ... of which materialised (rows [n_mat, nout) of the stage hold a position only)
        uint32_t zero_from = 0;    // ring position from which bases are still kept (<= done): the oldest block with listed positions
        uint32_t prev_last = seg_inner ? (uint32_t)(rw[-1] >> 62) : 0u;
        // complexity bound: sum of weight x Q over the read's words (complexity_dev.hpp).  Q <= CX_Q_MAX = 3840 and the weights of a
        // read sum to 2 nW <= L / 16, so below 2^24 bases the whole sum is under 240 * 2^24 < 2^32: a lane adds its words up in 32
        // bits and the wave sum is taken once per read, in 32 bits.  A longer read (wave-uniform test on L) folds the lanes' sums
        // into a scalar 64-bit total after every tile instead (a tile adds at most 64 x 2 x 3840).
        static_assert((uint64_t)CX_Q_MAX * ((1ull << 24) / 16u) < (1ull << 32), "the 32-bit sum of a read below 2^24 bases");
        uint32_t cx_acc = 0;       // per lane
        uint64_t cx_total = 0;     // wave-uniform: what the tiles of a long read have folded so far
        const bool cx_long = L >= (1u << 24);
        uint64_t prev_word = seg_inner ? rw[-1] : 0ull;     // (a view: the boundary word is counted here, in the view behind the cut)
        const uint32_t cx_nW = complexity_windows(SEG ? a.len[rd] : L);      // number of complexity windows (ReadSelection.hpp:1171-1228)
        // a view adds the words of its own tiles (the halo's are the next view's), at their place in the read
        const uint32_t cx_tiles = SEG ? ((view.flags & SEG_LAST) ? ntiles : a.seg_tiles) : ntiles;
        const uint32_t cx_t0 = SEG ? view.tile0 : 0u;

        // ---- materialisation of the listed positions, one per lane: window, canonical form, direction and, with qualities, the
        // look-ups behind min_quality.  Deferred over up to Geo::DEFER blocks (a block lists about ten positions: materialised
        // there, five lanes in six idled through the longest dependent chain of the kernel) ----
        auto materialise = [&]() {
            const uint32_t pend = nout - n_mat;
            if (pend == 0u) return;
            if (outgrown) { n_mat = nout; return; }       // counted only: the read is re-run by the general kernel
            const uint32_t base = n_mat - flushed;
            for (uint32_t i = lane; i < pend; i += 64) {
                const uint32_t j = stage[base + i].y;
                const uint32_t e = ring_window(S, j, Geo::RING_WMASK) & kmask;
                const uint32_t rev = e ^ comp_mask, fw = digit_reverse(e, K);
                // direction 1 iff the reverse complement is the canonical form, ties included (Kmer.hpp:427)
                const uint32_t d = fw < rev ? 0u : 1u;
                if (QUAL) { bool known = true; stage_q[base + i] = min_quality(j, known); if (!known) lost = true; }
                stage[base + i] = make_uint2(d ? rev : fw, (j << 1) | d);
            }
            n_mat = nout;
            wave_lds_sync();
        };
        // bases of [zero_from, upto) are not needed any more: back to zero for the next lap of the ring
        auto release_ring = [&](uint32_t upto) {
            const unsigned zb = zero_from >> 4, nz = (upto - zero_from) >> 4;
            for (unsigned i = lane; i < nz; i += 64) S[(zb + i) & Geo::RING_WMASK] = 0;
            zero_from = upto;
        };

        // ---- emission: list the positions recorded in `bits` (span length P per lane, oldest position in bit P-1) ----
        // (the four-wave kernels'; the variant's rows are staged by confirm, below)
        auto emit = [&](uint32_t bits, unsigned P, uint32_t npos_limit) {
            // positions at or beyond npos_limit (tail lanes past the end) and the trimmed first position of the read
            {
                if (P < 32u) bits &= (1u << P) - 1u;
                const uint32_t first_j = lane * P;                 // span-relative index of this lane's first position
                if (first_j >= npos_limit) bits = 0;
                else if (first_j + P > npos_limit) bits &= ~((1u << (first_j + P - npos_limit)) - 1u);
                if (done == 0u && lane == 0u && trim_first) bits &= ~(1u << (P - 1u));      // Kmer.hpp:1395
            }
            if (__ballot(bits != 0u) == 0ull) return;
            if (a.n_rep) {          // Kmer.hpp:1437: repetitive minimizers are not selected
                uint32_t b2 = bits;
                while (b2) {
                    const unsigned bit = 31u - (unsigned)__clz((int)b2);
                    b2 &= ~(1u << bit);
                    const unsigned u = P - 1u - bit;
                    const uint32_t e = ring_window(S, done + lane * P + u, Geo::RING_WMASK) & kmask;
                    const uint32_t rev = e ^ comp_mask, fw = digit_reverse(e, K);
                    const uint32_t v = fw < rev ? fw : rev, fb = rep_filter_bit(v);
                    if (((lds_rep_filter[fb >> 5] >> (fb & 31u)) & 1u) && rep_contains(a.rep, a.n_rep, v)) bits &= ~(1u << bit);
                }
            }
            const unsigned cnt = (unsigned)__popc(bits);
            const unsigned incl = wave_inclusive_sum_dpp(cnt);
            const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
            if (total == 0u) return;
            if (bump) {
                if (outgrown || nout + total > (unsigned)Geo::STAGE) {
                    if (!outgrown) { materialise(); n_staged_at_outgrowth = nout; }
                    if (APPROX) {          // the count the host places the read by must be exact: hash the candidates in full
                        uint32_t bad = 0;
                        while (bits) {
                            const unsigned bit = 31u - (unsigned)__clz((int)bits);
                            bits &= ~(1u << bit);
                            const uint32_t e = ring_window(S, done + lane * P + (P - 1u - bit), Geo::RING_WMASK) & kmask;
                            const uint32_t rev = e ^ comp_mask, fw = digit_reverse(e, K);
                            if (!(kmer_hash32(fw < rev ? fw : rev) < threshold)) bad++;
                        }
                        n_false += (uint32_t)wave_sum_u64(bad);
                    }
                    outgrown = true; nout += total; return;
                }
            } else if (nout - flushed + total > (unsigned)Geo::STAGE) {       // make room: the staged rows leave for the output slot
                materialise();
                const uint32_t ns = nout - flushed;
                for (uint32_t i = lane; i < ns; i += 64) {
                    const uint32_t idx = flushed + i;
                    if (idx < cap) {
                        const uint2 e = stage[i];
                        a.out_min[cap0 + idx] = e.x; a.out_pos[cap0 + idx] = e.y >> 1; a.out_dir[cap0 + idx] = (uint8_t)(e.y & 1u);
                        if (QUAL) a.out_mqual[cap0 + idx] = stage_q[i];
                    }
                }
                flushed = nout;
                wave_lds_sync();
            }
            if (total <= (unsigned)Geo::STAGE) {
                // the selected positions are listed in the stage; materialise() takes them one per lane later
                uint32_t at = nout - flushed + incl - cnt;
                while (bits) {
                    const unsigned bit = 31u - (unsigned)__clz((int)bits);
                    bits &= ~(1u << bit);
                    stage[at++].y = done + lane * P + (P - 1u - bit);          // position in the compressed read
                }
                wave_lds_sync();
            } else {
                // more selected positions in one block than the stage holds (densities near 1): straight to the slot
                uint32_t at = nout + incl - cnt;
                while (bits) {
                    const unsigned bit = 31u - (unsigned)__clz((int)bits);
                    bits &= ~(1u << bit);
                    const unsigned u = P - 1u - bit;
                    const uint32_t j = done + lane * P + u;
                    const uint32_t e = ring_window(S, j, Geo::RING_WMASK) & kmask;
                    const uint32_t rev = e ^ comp_mask, fw = digit_reverse(e, K);
                    const uint32_t d = fw < rev ? 0u : 1u;
                    if (at < cap) {
                        a.out_min[cap0 + at] = d ? rev : fw; a.out_pos[cap0 + at] = j; a.out_dir[cap0 + at] = (uint8_t)d;
                        if (QUAL) { bool known = true; a.out_mqual[cap0 + at] = min_quality(j, known); if (!known) lost = true; }
                    }
                    at++;
                }
                flushed = nout + total;
                n_mat = nout + total;
            }
            nout += total;
        };

        // ---- PF: one probe of the bitmap for key v, the answer shifted into b ----
        auto pf_probe = [&](uint32_t v, uint32_t &b) {
            const uint32_t h = v * 0x9E3779B1u;                  // prefilter_index(v) = h >> pf_shift
            const uint32_t byte = pf_map[h >> (pf_shift + 3u)];
            b = (b << 1) | ((byte >> ((h >> pf_shift) & 7u)) & 1u);
        };
        // ---- PF: confirmation, behind a walk: what the four-wave kernels' emit and materialise do, for the variant.  `bits` (span length
        // P per lane, oldest position in bit P - 1) holds the positions whose probe passed.  The set positions are listed in LDS in lane
        // order (6 bits of lane, 5 of bit), i.e. in position order; the lanes take listed positions 64 at a time (a ROUND), rebuild the
        // window from the ring and take its exact verdict; the lane of a selected one holds position, both orientations and verdict, and
        // writes the finished row to the stage at its rank in the round's ballot.  Rounds and passes go up through the positions, so the
        // rows stay in position order.  The list holds PF_LIST_CAP positions: what a pass cannot list stays in `bits` for the next
        // pass, so a block with any number of candidates is confirmed exactly.  A round that would pass the stage's end makes the
        // read `outgrown`; from there on the rounds count only (the host places and re-runs the read by that count) ----
        auto confirm = [&](uint32_t bits, unsigned P, uint32_t npos_limit) {
            // positions at or beyond npos_limit (tail lanes past the end) and the trimmed first position of the read are nobody's
            if (P < 32u) bits &= (1u << P) - 1u;
            {
                const uint32_t first_j = lane * P;
                if (first_j >= npos_limit) bits = 0;
                else if (first_j + P > npos_limit) bits &= ~((1u << (first_j + P - npos_limit)) - 1u);
                if (done == 0u && lane == 0u && trim_first) bits &= ~(1u << (P - 1u));      // Kmer.hpp:1395
            }
            // the row of listed position q (6 bits of owner lane, 5 of bit): v the canonical form, y = (position << 1) | direction,
            // direction 1 iff the reverse complement is the canonical form, ties included (Kmer.hpp:427)
            auto listed_row = [&](uint32_t q, uint32_t &v, uint32_t &y) {
                const uint32_t j = done + (q >> 5) * P + (P - 1u - (q & 31u));
                const uint32_t e = ring_window(S, j, Geo::RING_WMASK) & kmask;
                const uint32_t rev = e ^ comp_mask, fw = digit_reverse(e, K);
                const uint32_t d = fw < rev ? 0u : 1u;
                v = d ? rev : fw; y = (j << 1) | d;
            };
            // Kmer.hpp:1437: a repetitive minimizer is not selected
            auto repetitive = [&](uint32_t v) -> bool {
                const uint32_t fb = rep_filter_bit(v);
                return ((lds_rep_filter[fb >> 5] >> (fb & 31u)) & 1u) && rep_contains(a.rep, a.n_rep, v);
            };
            // one round's rows leave for the stage: rank = the selected lanes below this one
            auto stage_round = [&](bool sel, uint32_t v, uint32_t y) {
                if (a.n_rep) { if (sel && repetitive(v)) sel = false; }
                const uint64_t m = __ballot(sel);
                if (m == 0ull) return;
                const unsigned c = (unsigned)__popcll(m);
                if (outgrown || nout + c > (unsigned)Geo::STAGE) outgrown = true;       // counted only: the read is re-run by the general kernel
                else if (sel) stage[nout - flushed + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = make_uint2(v, y);
                nout += c;
            };
            unsigned cnt = (unsigned)__popc(bits);
            unsigned incl = wave_inclusive_sum_dpp(cnt);
            unsigned total = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
            while (total != 0u) {
                unsigned at = incl - cnt;
                while (bits && at < PF_LIST_CAP) {
                    const unsigned bit = 31u - (unsigned)__clz((int)bits);
                    bits &= ~(1u << bit);
                    pf_list[at++] = (uint16_t)((lane << 5) | bit);
                }
                const unsigned n = total < PF_LIST_CAP ? total : PF_LIST_CAP;
                wave_lds_sync();
                if (pf_table != nullptr) {
                    // the verdicts from the selected-key table (prefilter.hpp): the loads of every round of the pass are issued before
                    // the first is waited for; a lane without a listed position keeps a bucket of zeros, which selects nothing
                    constexpr unsigned ROUNDS = (PF_LIST_CAP + 63u) / 64u;
                    uint32_t lv[ROUNDS], ly[ROUNDS];
                    uint4 lw[ROUNDS];
#pragma unroll
                    for (unsigned k = 0; k < ROUNDS; k++) {
                        lv[k] = 0u; ly[k] = 0u; lw[k] = make_uint4(0u, 0u, 0u, 0u);
                        if (64u * k < n) {
                            const unsigned i = lane + 64u * k;
                            if (i < n) {
                                listed_row(pf_list[i], lv[k], ly[k]);
                                lw[k] = pf_table[confirm_hash(lv[k]) >> pf_table_shift];
                            }
                        }
                    }
#pragma unroll
                    for (unsigned k = 0; k < ROUNDS; k++) {
                        if (64u * k < n) {
                            const uint32_t verdict = confirm_verdict(lw[k].x, lw[k].y, lw[k].z, lw[k].w, confirm_hash(lv[k]));
                            bool sel = verdict == CONFIRM_YES;
                            // keys of buckets the builder marked ask the hash (no bucket is marked at density 0.005f), within their round:
                            // the rows stay in order
                            if (__ballot(verdict == CONFIRM_ASK) != 0ull) {
                                if (verdict == CONFIRM_ASK) sel = kmer_hash32(lv[k]) < threshold;
                            }
                            stage_round(sel, lv[k], ly[k]);
                        }
                    }
                } else {
                    for (unsigned i0 = 0u; i0 < n; i0 += 64u) {
                        uint32_t v = 0u, y = 0u;
                        bool sel = false;
                        if (i0 + lane < n) {
                            listed_row(pf_list[i0 + lane], v, y);
                            sel = kmer_hash32(v) < threshold;
                        }
                        stage_round(sel, v, y);
                    }
                }
                if (total <= PF_LIST_CAP) break;      // everything was listed: nothing is left in `bits`
                wave_lds_sync();          // the list is read before the next pass rewrites it
                cnt = (unsigned)__popc(bits);
                incl = wave_inclusive_sum_dpp(cnt);
                total -= PF_LIST_CAP;
            }
        };

        // ---- the slow path of the shared hash (APPROX, guarded walks): this lane's span of P positions once more, position by
        // position from the ring with the exact candidate test, the oldest position in the highest used bit as the walks leave it.
        // Called by the lanes whose guard minimum is below guard_limit only -- about 3 blocks in 10^5 have one ----
        auto guarded_redo = [&](unsigned P) -> uint32_t {
            SpanState rs{0u, 0u};
#pragma nounroll
            for (unsigned u = 0; u < P; u++)
                span_step<APPROX>(rs, ring_window(S, done + lane * P + u, Geo::RING_WMASK), u == 0u, kmask, comp_mask, top_shift, K, threshold, cand_limit);
            return rs.bits;
        };

        // ---- 64 * SP positions from `done` on, each followed by a known base: lane l owns positions SP l .. SP l + SP - 1, i.e.
        // 2 SP stream bits that start on a word boundary of the ring; walked in registers with compile-time shifts ----
        auto aligned_block = [&](auto sp_tag) {
            constexpr int SP = decltype(sp_tag)::value;              // 32 or 16
            constexpr unsigned WPL = (unsigned)SP / 16u;               // stream words per lane
            const unsigned wb = ((done >> 4) + WPL * lane) & Geo::RING_WMASK;
            const uint32_t W0 = S[wb], W1 = S[(wb + 1) & Geo::RING_WMASK], W2 = SP > 16 ? S[(wb + 2) & Geo::RING_WMASK] : 0u;
            SpanState st{0u, 0u};
            auto walk = [&](auto k15_tag, auto guard_tag) {
                constexpr bool K15 = decltype(k15_tag)::value;
                constexpr bool GUARD = APPROX && decltype(guard_tag)::value;
                if (SP == 32 && DUAL_CHAIN) {
                    // two independent chains per lane -- positions 0 .. 15 and 16 .. 31 side by side -- so that a wave has another
                    // instruction to issue while a multiply's result is on its way (at 4 - 5 waves per SIMD one chain leaves gaps:
                    // tools/ubench/hash_rates.hip, chains=1 against chains=2)
                    uint32_t fa = 0u, fb = 0u, ba = 0u, bb = 0u, pa = 0u, pb = 0u;
                    uint32_t g = 0xFFFFFFFFu;      // GUARD: the minimum of the span's guard words
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        const uint32_t Ta = u == 0 ? W0 : __builtin_amdgcn_alignbit(W1, W0, 2 * u);
                        const uint32_t Tb = u == 0 ? W1 : __builtin_amdgcn_alignbit(W2, W1, 2 * u);
                        const uint32_t reva = (Ta ^ comp_mask) & kmask, revb = (Tb ^ comp_mask) & kmask;
                        if (u == 0) { fa = digit_reverse(Ta & kmask, K); fb = digit_reverse(Tb & kmask, K); }
                        else if (K15) { fa = __builtin_amdgcn_alignbit(fa, pa, 30) & kmask; fb = __builtin_amdgcn_alignbit(fb, pb, 30) & kmask; }
                        else { fa = ((fa << 2) | ((Ta >> top_shift) & 3u)) & kmask; fb = ((fb << 2) | ((Tb >> top_shift) & 3u)) & kmask; }
                        const uint32_t va = fa < reva ? fa : reva, vb = fb < revb ? fb : revb;
                        if (PF) {
                            pf_probe(va, ba); pf_probe(vb, bb);
                        } else if (APPROX) {
                            uint32_t ra, rb;
                            kmer_hash32_hi_shared_x2<GUARD>(va, vb, ra, rb, g);
                            asm("v_cmp_lt_u32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(ba) : "v"(ra), "s"(cand_limit) : "vcc");
                            asm("v_cmp_lt_u32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(bb) : "v"(rb), "s"(cand_limit) : "vcc");
                        } else {
                            const uint64_t ha = kmer_hash32(va), hb = kmer_hash32(vb);
                            asm("v_cmp_lt_u64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(ba) : "v"(ha), "s"(threshold) : "vcc");
                            asm("v_cmp_lt_u64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(bb) : "v"(hb), "s"(threshold) : "vcc");
                        }
                        pa = Ta; pb = Tb;
                    }
                    st.bits = (ba << 16) | bb;
                    if (GUARD && __ballot(g < guard_limit) != 0ull) {
                        if (g < guard_limit) st.bits = guarded_redo(32u);
                    }
                    return;
                }
                uint32_t Tprev = 0u;
#pragma unroll
                for (int u = 0; u < SP; u++) {
                    const uint32_t T = u == 0 ? W0 : (u < 16 ? __builtin_amdgcn_alignbit(W1, W0, 2 * u)
                                                             : (u == 16 ? W1 : __builtin_amdgcn_alignbit(W2, W1, 2 * (u - 16))));
                    span_step<APPROX, K15>(st, T, u == 0, kmask, comp_mask, top_shift, K, threshold, cand_limit, Tprev);
                    Tprev = T;
                }
            };
            if constexpr (PF) {          // l = 15, compressed, no slack (launch_scan): the one walk, then the exact verdicts as staged rows
                walk(std::true_type(), std::false_type());
                confirm(st.bits, (unsigned)SP, 64u * (unsigned)SP);
                wave_lds_sync();
                done += 64u * (unsigned)SP;
                release_ring(done);      // its rows are finished: nothing of the block is read again
                wave_lds_sync();
            } else {
                if (K == 15u) { if (APPROX && !unguarded) walk(std::true_type(), std::true_type()); else walk(std::true_type(), std::false_type()); }
                else walk(std::false_type(), std::integral_constant<bool, APPROX>());
                emit(st.bits, (unsigned)SP, 64u * (unsigned)SP);
                wave_lds_sync();
                done += 64u * (unsigned)SP;
                // materialise when most of a wave's lanes have a position to take, or when the ring cannot keep the blocks any longer
                // (with qualities under HPC the run starts of a listed position must still be in the tile history: one block less)
                constexpr unsigned defer = (QUAL && HPC) ? Geo::DEFER - 1u : Geo::DEFER;
                if (nout - n_mat >= 48u || nout == n_mat || done - zero_from > defer * BLOCK_POS) {
                    materialise();
                    release_ring(done);
                }
                wave_lds_sync();
            }
        };

        uint64_t x_next = (lane < nwords) ? rw[lane] : 0;
        for (uint32_t t = 0; t < ntiles; t++) {
            const uint64_t x = x_next;
            const uint32_t wi = t * TILE_WORDS + lane;
            {
                const uint32_t nwi = wi + TILE_WORDS;
                x_next = (nwi < nwords) ? rw[nwi] : 0;
            }
            const int rem = (int)L - (int)(wi * 32u);
            const unsigned nvalid = rem <= 0 ? 0u : (rem >= 32 ? 32u : (unsigned)rem);

            // ---- complexity: upper bound from per-word 2-mer counts (as in scan_kernel; the word below comes over DPP) ----
            if (a.apply_filters && (!SEG || t < cx_tiles)) {
                const uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32);
                const uint32_t pl32 = lane_below(xl, (uint32_t)prev_word), ph32 = lane_below(xh, (uint32_t)(prev_word >> 32));
                prev_word = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)xh, 63) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)xl, 63);
                // word wq = wi - 1 enters window wq (if wq < nW) and window wq - 1 (if 1 <= wq <= nW): weight 1 at wq = 0 and nW, 2 between
                const uint32_t q = word_pair_q(((uint64_t)ph32 << 32) | pl32, xl);
                const uint32_t tg = t + cx_t0;                    // the tile's place in the read
                if (tg != 0u && tg * TILE_WORDS + (TILE_WORDS - 1u) <= cx_nW) {
                    cx_acc += q + q;                              // a tile in the middle of the read (wave-uniform test): words 1 .. nW - 1 only
                } else {
                    const uint32_t wq = cx_t0 * TILE_WORDS + wi - 1u;      // lane 0 of tile 0: wraps around, weight 0
                    const uint32_t w2 = wq < cx_nW ? q : 0u, w1 = (wq - 1u) < cx_nW ? q : 0u;
                    cx_acc += w2 + w1;
                }
                if (cx_long) { cx_total += wave_sum_u32(cx_acc); cx_acc = 0; }
            }

            // ---- run starts / compaction of this lane's word ----
            uint64_t y;
            unsigned c;
            if (HPC) {
                uint32_t pl = lane_below((uint32_t)(x >> 62), prev_last);
                if (wi == 0 && !seg_inner) pl = ((uint32_t)x & 3u) ^ 1u;      // the first base of the read starts a run whatever precedes it
                unsigned nbits;
                y = compress_pairs_lut(HpcLut{lds_lut_b, lds_lut_n}, x, pl, &nbits);
                c = nbits >> 1;
                if (nvalid < 32) {
                    const uint64_t vspread = ((1ull << (2 * nvalid)) - 1ull) & M5;
                    const uint64_t diff = x ^ ((x << 2) | (uint64_t)pl);
                    const uint64_t d = (diff | (diff >> 1)) & vspread;
                    c = (unsigned)__popcll(d);
                    y &= c >= 32 ? ~0ull : ((1ull << (2 * c)) - 1ull);
                }
                prev_last = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 62), 63);
            } else {
                c = nvalid;
                y = nvalid == 32 ? x : (x & ((1ull << (2 * nvalid)) - 1ull));
            }
            const unsigned inc = wave_inclusive_sum_dpp(c);
            const unsigned o = inc - c;
            const unsigned C = (unsigned)__builtin_amdgcn_readlane((int)inc, 63);

            // ---- append to the ring (the region ahead of `fill` is zero) ----
            if (c) {
                const unsigned dst = 2u * ((fill + o) & (Geo::RING - 1u)), w = dst >> 5, sh = dst & 31u;
                const uint32_t yl = (uint32_t)y, yh = (uint32_t)(y >> 32);
                const uint32_t p0 = yl << sh;
                const uint32_t p1 = sh ? ((yl >> (32u - sh)) | (yh << sh)) : yh;
                const uint32_t p2 = sh ? (yh >> (32u - sh)) : 0u;
                atomicOr(&S[w], p0);
                if (p1) atomicOr(&S[(w + 1) & Geo::RING_WMASK], p1);
                if (p2) atomicOr(&S[(w + 2) & Geo::RING_WMASK], p2);
            }
            if (HPC && QUAL) {         // where this tile's words start in the compressed stream (for rlePositions look-ups)
                hist_o[(t % HIST_TILES) * 64u + lane] = (uint16_t)o;
                if (lane == 0) hist_c[t % HIST_TILES] = fill;
                t_done = t + 1u;
            }
            fill += C;
            wave_lds_sync();

            // ---- full blocks: 2048 positions, every one followed by a known base ----
            // (with _trimBps == 0 the last l-mer is a position too: a block also runs at exactly 2048 + K bases, or the tail would
            // be left with 2049 positions -- 36 per lane, four more than a lane's verdict vector holds)
            // (a view: whole blocks of OWNED positions only; what it owns beyond them is the tail's)
            while (fill - done >= BLOCK_POS + K + a.trim && (!SEG || view.n_own - done >= BLOCK_POS)) aligned_block(std::integral_constant<int, (int)SPAN>());
        }
        // (a last half block of 1024 positions, 16 per lane, in front of the group-of-four, one-chain tail of rounds 2 - 6 was measured:
        // 11.73 against 11.76 ms, not kept.  What that tail cost was its padding -- spans of 4 ceil(npos / 256) positions, 1536 hashed
        // for the 1341 of a 10 kb HiFi read -- and its single chain; the exact-span, two-chain tail below hashes 1408 of them in 43
        // vector instructions per position where it took 45: 66.08 -> 65.51 G wave instructions per launch of 10 M reads, busy cycles
        // - 1.9 %, the scan in the bench 111.8 -> 110.0 ms and the step 112.9 -> 111.2 ms, three runs each, alternating
        // (profiles/tail_two_chains_*) -- about half of the 3 % reasoned beforehand)

        // ---- tail: the positions left (each followed by a known base; with _trimBps == 0 also the last l-mer) ----
        {
            const uint32_t live = fill - done;
            uint32_t npos = live > K ? live - K : 0u;
            if (a.trim == 0u && live >= K) npos = live - K + 1u;
            // a view stops at the last window it owns: the halo behind it has completed every one of them (segments_dev.hpp), and the
            // block loop has left fewer than 2048 of them or fewer than 2048 + l + trim bases
            if (SEG && npos > view.n_own - done) npos = view.n_own - done;
            // (the same in every lane, but derived from loads the compiler takes for per-lane values: as a scalar, so that the walk
            // below is counted and branched on by the scalar unit)
            npos = (uint32_t)__builtin_amdgcn_readfirstlane((int)npos);
            if (npos) {
                // spans of exactly P = ceil(npos / 64) <= 32 positions per lane (the block loop above leaves at most 2048 positions
                // whatever _trimBps is; the verdicts of a lane are a 32-bit vector): lane l owns done + l P ... done + l P + P - 1, at
                // most 63 positions are hashed for nothing.  A lane walks its span as two half spans of Ph = ceil(P / 2) positions side
                // by side, as aligned_block does: chain a from the span's first position, chain b Ph positions on.
                if (npos > BLOCK_POS) __builtin_trap();
                const unsigned P = (npos + 63u) >> 6;
                const unsigned Ph = (P + 1u) >> 1;
                // A chain needs 32 + 2 (Ph - 1) <= 62 stream bits from its first position on: three ring words, read once and aligned
                // to the position (a per-lane shift); the walk then takes its window with the uniform shift 2 u and reads no LDS.
                // The words may lie up to 48 bases past a chain's first position, i.e. below done + 63 P + Ph + 48 <= done + 2080:
                // with the Geo::DEFER blocks kept behind `done` that is 8224 of the four-wave ring's 16384 bases (the variant keeps none: 2080 of its 8192), so they never lap into kept
                // bases; what they hold beyond `fill` is zero, and positions at or beyond npos are masked in emit whatever they hash to.
                auto chain_words = [&](unsigned p, uint32_t &lo, uint32_t &hi) {
                    const unsigned b = 2u * p, w = (b >> 5) & Geo::RING_WMASK, sh = b & 31u;
                    const uint32_t w0 = S[w], w1 = S[(w + 1) & Geo::RING_WMASK], w2 = S[(w + 2) & Geo::RING_WMASK];
                    lo = __builtin_amdgcn_alignbit(w1, w0, sh); hi = __builtin_amdgcn_alignbit(w2, w1, sh);
                };
                uint32_t bits = 0u;
                auto tail_walk = [&](auto k15_tag, auto guard_tag) {
                    constexpr bool K15 = decltype(k15_tag)::value;
                    constexpr bool GUARD = APPROX && decltype(guard_tag)::value;
                    uint32_t A0, A1, B0, B1;
                    chain_words(done + lane * P, A0, A1);
                    chain_words(done + lane * P + Ph, B0, B1);
                    uint32_t Ta = A0, Tb = B0;
                    uint32_t fa = digit_reverse(Ta & kmask, K), fb = digit_reverse(Tb & kmask, K);     // the first position of EACH chain
                    uint32_t ba = 0u, bb = 0u;
                    uint32_t g = 0xFFFFFFFFu;      // GUARD: the minimum of the guard words of both chains (with P odd also of the one
                                                   // position chain b hashes beyond its own: at worst a span redone for nothing)
                    // one body for every P, counted by a scalar (an unrolled body per P would not fit the instruction cache); the roll
                    // behind the last step is not used -- without a way out in the middle the loop stays one block with one scalar branch
                    unsigned u = 0u;
#pragma nounroll
                    do {
                        const uint32_t reva = (Ta ^ comp_mask) & kmask, revb = (Tb ^ comp_mask) & kmask;
                        const uint32_t va = fa < reva ? fa : reva, vb = fb < revb ? fb : revb;
                        if (PF) {
                            pf_probe(va, ba); pf_probe(vb, bb);
                        } else if (APPROX) {
                            uint32_t ra, rb;
                            kmer_hash32_hi_shared_x2<GUARD>(va, vb, ra, rb, g);
                            asm("v_cmp_lt_u32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(ba) : "v"(ra), "s"(cand_limit) : "vcc");
                            asm("v_cmp_lt_u32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(bb) : "v"(rb), "s"(cand_limit) : "vcc");
                        } else {
                            const uint64_t ha = kmer_hash32(va), hb = kmer_hash32(vb);
                            asm("v_cmp_lt_u64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(ba) : "v"(ha), "s"(threshold) : "vcc");
                            asm("v_cmp_lt_u64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(bb) : "v"(hb), "s"(threshold) : "vcc");
                        }
                        u++;
                        const uint32_t Na = __builtin_amdgcn_alignbit(A1, A0, 2u * u), Nb = __builtin_amdgcn_alignbit(B1, B0, 2u * u);
                        if (K15) { fa = __builtin_amdgcn_alignbit(fa, Ta, 30) & kmask; fb = __builtin_amdgcn_alignbit(fb, Tb, 30) & kmask; }
                        else { fa = ((fa << 2) | ((Na >> top_shift) & 3u)) & kmask; fb = ((fb << 2) | ((Nb >> top_shift) & 3u)) & kmask; }
                        Ta = Na; Tb = Nb;
                    } while (u < Ph);
                    // the oldest position in bit P - 1.  With P odd chain b has hashed one position more than it owns (the next lane's
                    // first: a guarded last step would need a second, one-chain copy of the hash): its youngest bit is dropped here
                    bits = (ba << (P - Ph)) | (bb >> (2u * Ph - P));
                    if (GUARD && __ballot(g < guard_limit) != 0ull) {
                        if (g < guard_limit) bits = guarded_redo(P);
                    }
                };
                if constexpr (PF) {
                    tail_walk(std::true_type(), std::false_type());
                    confirm(bits, P, npos);
                } else if (K == 15u) { if (APPROX && !unguarded) tail_walk(std::true_type(), std::true_type()); else tail_walk(std::true_type(), std::false_type()); }
                else tail_walk(std::false_type(), std::integral_constant<bool, APPROX>());
                if constexpr (!PF) emit(bits, P, npos);
            }
            wave_lds_sync();
            if constexpr (!PF) materialise();
            // leave the ring zero for the next read: everything from `zero_from` to `fill`
            release_ring(((fill + 15u) & ~15u) + 16u);
        }

        if (APPROX && !PF) {
            // the full hash of every staged position, once per read (a block stages about ten of them: confirming them there kept
            // five lanes in six idle); a false one loses the read to the re-run.  The positions of a read that outgrew the stage
            // after these were confirmed as they came (emit).  (PF: every staged position passed confirm, whose verdicts are exact)
            const uint32_t n_staged = outgrown ? n_staged_at_outgrowth : nout;
            for (uint32_t i = lane; i < ((n_staged + 63u) & ~63u); i += 64) {
                const uint64_t fb = __ballot(i < n_staged && !(kmer_hash32(stage[i].x) < threshold));
                if (fb) { n_false += (uint32_t)__popcll(fb); lost = true; }
            }
        }
        if (((QUAL && HPC) || (APPROX && !PF)) && __ballot(lost) != 0ull) outgrown = true;      // a run start had left the history, or a false candidate:
                                                                                        // the general kernel redoes the read
        uint8_t flags = 0;
        if constexpr (SEG) {          // the read's decision is the join's, over the sums of all its views
            const uint64_t cx_view = a.apply_filters ? cx_total + wave_sum_u32(cx_acc) : 0ull;
            if (lane == 0) a.view_cx[r] = cx_view;
        } else if (a.apply_filters && L >= 66) {
            if (complexity_suspect(cx_total + wave_sum_u32(cx_acc), cx_nW)) flags |= READ_SUSPECT;
        }
        // ---- the staged minimizers leave in rows ----
        if (bump) {
            uint64_t start = 0;
            if (!outgrown && nout) {
                uint32_t lo = 0, hi = 0;
                const uint32_t region = pf_counter ? run_region : wave_global & (a.n_regions - 1u);
                if (lane == 0) { const unsigned long long s0 = atomicAdd(a.cursor + region, (unsigned long long)nout); lo = (uint32_t)s0; hi = (uint32_t)(s0 >> 32); }
                start = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)hi) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
                const bool fits = start + nout <= a.out_capacity;
                start += (uint64_t)region * a.out_capacity;
                if (fits) {
                    for (uint32_t i = lane; i < nout; i += 64) {
                        const uint2 e = stage[i];
                        a.out_min[start + i] = e.x; a.out_pos[start + i] = e.y >> 1; a.out_dir[start + i] = (uint8_t)(e.y & 1u);
                        if (QUAL) a.out_mqual[start + i] = stage_q[i];
                    }
                }
            }
            if (lane == 0) {
                a.out_begin[r] = start;
                a.out_count[r] = nout - n_false;    // also for a read that outgrew the stage: the host places and re-runs it
                a.out_flags[r] = flags;
                if (outgrown) a.over_list[atomicAdd(&a.list_counters[0], 1u)] = r;
                if (flags & READ_SUSPECT) a.suspect_list[atomicAdd(&a.list_counters[1], 1u)] = r;
            }
        } else {
            const uint32_t ns = nout - flushed;
            for (uint32_t i = lane; i < ns; i += 64) {
                const uint32_t idx = flushed + i;
                if (idx < cap) {
                    const uint2 e = stage[i];
                    a.out_min[cap0 + idx] = e.x; a.out_pos[cap0 + idx] = e.y >> 1; a.out_dir[cap0 + idx] = (uint8_t)(e.y & 1u);
                    if (QUAL) a.out_mqual[cap0 + idx] = stage_q[i];
                }
            }
            if (lane == 0) {
                a.out_count[r] = nout;
                a.out_flags[r] = flags;
            }
        }
        wave_lds_sync();       // ring zeroed, stage drained: the next read starts clean
    }
}

// The selected-key bitmap of the pre-filtered variant, built once per (l, hpc, threshold, geometry): every 15-digit key through
// prefilter.hpp's rule, the selected ones ORed into `bitmap` (zeroed by the caller), the bits newly set counted in *n_set.
__global__ __launch_bounds__(256) void prefilter_build_kernel(uint32_t *bitmap, uint64_t threshold, unsigned log2_bits, uint32_t *n_set) {
    prefilter_build_range(blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, threshold, log2_bits, [&](uint32_t idx) {
        const uint32_t bit = 1u << (idx & 31u);
        if (!(atomicOr(&bitmap[idx >> 5], bit) & bit)) atomicAdd(n_set, 1u);
    });
}

// The selected-key table of the variant's confirm step (prefilter.hpp), built beside the bitmap in the header's three steps: `table`
// and `counts` zeroed by the caller, the buckets marked "ask the hash" counted in *n_over.
struct ConfirmAtomicOps {
    __device__ uint32_t add(uint32_t *p, uint32_t v) const { return atomicAdd(p, v); }
    __device__ uint32_t orr(uint32_t *p, uint32_t v) const { return atomicOr(p, v); }
};
__global__ __launch_bounds__(256) void confirm_table_insert_kernel(uint32_t *table, uint32_t *counts, uint64_t threshold, unsigned log2_buckets) {
    confirm_table_insert_range(blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, threshold, log2_buckets, table, counts, ConfirmAtomicOps());
}
__global__ __launch_bounds__(256) void confirm_table_finish_kernel(uint32_t *table, const uint32_t *counts, unsigned log2_buckets, uint32_t *n_over) {
    for (uint32_t b = blockIdx.x * 256u + threadIdx.x; b < (1u << log2_buckets); b += gridDim.x * 256u)
        if (confirm_table_finish_bucket(table + (size_t)b * CONFIRM_BUCKET_WORDS, counts[b])) atomicAdd(n_over, 1u);
}
__global__ __launch_bounds__(256) void confirm_table_verify_kernel(uint32_t *table, uint64_t threshold, unsigned log2_buckets, uint32_t *n_over) {
    confirm_table_verify_range(blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, threshold, log2_buckets, table, ConfirmAtomicOps(),
                               [&]() { atomicAdd(n_over, 1u); });
}

// A batch the pre-filtered variant shares with the four-wave kernel: the reads the four-wave launch leaves alone -- those shorter than
// `limit` (the variant's) and those flagged in `masked` (the general kernel's; may be null)
// ; *long_bases: the bases of the reads of `limit` bases or more (grid-stride, one atomic a wave)
__global__ __launch_bounds__(256) void split_skip_kernel(const uint32_t *len, const uint8_t *masked, uint32_t n_reads, uint32_t limit, uint8_t *skip,
                                                         unsigned long long *long_bases) {
    uint64_t sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_reads; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t L = len[i];
        skip[i] = (uint8_t)((L < limit || (masked && masked[i])) ? 1u : 0u);
        if (L >= limit) sum += L;
    }
    sum = wave_sum_u64(sum);
    if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(long_bases, (unsigned long long)sum);
}

// ---- long reads as views (segments_dev.hpp; mdbg_scan, "scan_segments") ------------------------------------------------------------
// The pre-pass: which reads are cut (plain reads of more than one segment), their tiles and views counted ...
__global__ __launch_bounds__(256) void seg_count_kernel(const uint32_t *len, const uint8_t *masked, uint32_t n_reads, uint32_t G,
                                                        uint32_t *tiles_per_read, uint32_t *views_per_read, uint8_t *skip) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_reads; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t L = len[i];
        const bool plain = !(masked && masked[i]);
        const bool cut = plain && L > G;
        tiles_per_read[i] = cut ? seg_tiles(L) : 0u;
        views_per_read[i] = cut ? seg_count(L, G) : 0u;
        skip[i] = (uint8_t)(plain ? 0u : 1u);            // (seg_plan_kernel adds the reads it cuts)
    }
}

// ... the run starts of every tile of those reads, one wave a tile (homopolymer compression only) ...
__global__ __launch_bounds__(256) void seg_tile_runs_kernel(const uint64_t *words, const uint64_t *word_off, const uint32_t *len, uint32_t n_reads,
                                                            const uint64_t *tile_off /* n_reads + 1 */, uint32_t *tile_runs) {
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t n_tiles = tile_off[n_reads];
    for (uint64_t gt = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; gt < n_tiles; gt += ((uint64_t)gridDim.x * 256u) >> 6) {
        uint32_t lo = 0, hi = n_reads;                   // the read of tile gt: the last r with tile_off[r] <= gt
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (tile_off[mid] <= gt) lo = mid; else hi = mid; }
        const uint32_t r = lo, L = len[r], t = (uint32_t)(gt - tile_off[r]);
        const uint64_t *rw = words + word_off[r];
        const uint32_t nwords = (uint32_t)(((uint64_t)L + 31u) / 32u), wi = t * 64u + lane;
        uint32_t c = 0;
        if (wi < nwords) {
            const uint32_t prev = wi ? (uint32_t)(rw[wi - 1u] >> 62) : seg_first_prev(rw[0]);
            c = seg_word_run_starts(rw[wi], prev, seg_word_valid(L, wi));
        }
        c = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_sum_dpp(c), 63);
        if (lane == 0) tile_runs[gt] = c;
    }
}

// ... and, one wave a read, the exclusive scan of its tiles' run starts (in place), the verdict on its cuts and its views.
// totals: [0] reads cut, [1] their views.  The reads it cuts are flagged in `skip` beside the masked ones.
__global__ __launch_bounds__(256) void seg_plan_kernel(const uint32_t *len, uint32_t n_reads, uint32_t G, uint32_t K, int hpc, const uint64_t *tile_off,
                                                       const uint64_t *view_off, const uint32_t *tile_runs, uint32_t *tile_excl /* exclusive sums of tile_runs inside a read */,
                                                       SegView *views, uint8_t *skip, uint8_t *read_cut, unsigned long long *totals) {
    const unsigned lane = threadIdx.x & 63u;
    for (uint64_t r = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; r < n_reads; r += ((uint64_t)gridDim.x * 256u) >> 6) {
        const uint32_t nS = (uint32_t)(view_off[r + 1] - view_off[r]);
        if (nS == 0u) { if (lane == 0) read_cut[r] = 0; continue; }
        const uint32_t L = len[r], nT = (uint32_t)(tile_off[r + 1] - tile_off[r]), per = G / SEG_TILE_BASES;
        const uint32_t *tr = tile_runs + tile_off[r];
        uint32_t *te = tile_excl + tile_off[r];
        bool bad = false;
        uint32_t C = L;
        if (hpc) {
            for (uint32_t s = 1u + lane; s < nS; s += 64u) bad = bad || !seg_cut_ok(L, s * G, tr[(uint64_t)s * per], K);
            uint32_t carry = 0;
            for (uint32_t t0 = 0; t0 < nT; t0 += 64u) {
                const uint32_t t = t0 + lane, c = t < nT ? tr[t] : 0u;
                const uint32_t inc = wave_inclusive_sum_dpp(c);
                if (t < nT) te[t] = carry + inc - c;
                carry += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            }
            C = carry;
            __threadfence();          // the lanes read each other's sums below
        } else {
            for (uint32_t s = 1u + lane; s < nS; s += 64u) {
                const uint64_t b = (uint64_t)s * G;
                bad = bad || !seg_cut_ok(L, (uint32_t)b, (uint32_t)(L - b < SEG_TILE_BASES ? L - b : SEG_TILE_BASES), K);
            }
        }
        const bool live = __ballot(bad) == 0ull;
        const uint32_t *excl = hpc ? te : nullptr;
        for (uint32_t s = lane; s < nS; s += 64u)
            views[view_off[r] + s] = seg_view_make((uint32_t)r, s, nS, L, G, seg_offset(excl, s, nS, L, G, C), seg_offset(excl, s + 1u, nS, L, G, C), live);
        if (lane == 0) {
            read_cut[r] = (uint8_t)(live ? 1u : 0u);
            if (live) { skip[r] = 1; atomicAdd(&totals[0], 1ull); atomicAdd(&totals[1], (unsigned long long)nS); }
        }
    }
}

// The join.  Views that outgrew their stage or met a false candidate are on the views' own list: flagged per view ...
__global__ __launch_bounds__(256) void seg_mark_views_kernel(const uint32_t *view_over_list, const uint32_t *n_over, uint32_t n_views, uint8_t *view_bad) {
    const uint32_t n = *n_over < n_views ? *n_over : n_views;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) view_bad[view_over_list[i]] = 1;
}

// ... then, one wave a cut read: its views' counts and complexity sums added up, its rows placed behind the regions where the
// exclusive scan over ALL views' counts (row_off) puts its first view -- so a read's rows are contiguous, in view order -- its
// count, flags and begin set.  A read with a flagged view goes whole the way outgrown reads go (a.over_list), with its exact count.
// totals: [2] rows joined, [3] reads joined, [4] = 1 when the joined rows did not fit `join_cap`
__global__ __launch_bounds__(256) void seg_join_reads_kernel(ScanArgs a /* the batch's: out_*, lists, len */, uint32_t n_reads, const uint64_t *view_off,
                                                             const uint64_t *row_off, const uint8_t *view_bad,
                                                             const unsigned long long *view_cx, uint8_t *read_cut, uint64_t join_base, uint64_t join_cap,
                                                             unsigned long long *totals) {
    const unsigned lane = threadIdx.x & 63u;
    for (uint64_t r = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; r < n_reads; r += ((uint64_t)gridDim.x * 256u) >> 6) {
        if (!read_cut[r]) continue;
        const uint64_t v0 = view_off[r], v1 = view_off[r + 1];
        uint64_t cx = 0;
        bool bad = false;
        for (uint64_t v = v0 + lane; v < v1; v += 64u) { cx += view_cx[v]; bad = bad || view_bad[v]; }
        cx = wave_sum_u64(cx);
        const bool fell_back = __ballot(bad) != 0ull;
        const uint64_t first = row_off[v0], rows = row_off[v1] - first;
        const bool fits = first + rows <= join_cap;
        if (lane == 0) {
            const uint32_t L = a.len[r];
            const uint8_t flags = (a.apply_filters && L >= 66u && complexity_suspect(cx, complexity_windows(L))) ? READ_SUSPECT : (uint8_t)0;
            a.out_count[r] = (uint32_t)rows;
            a.out_flags[r] = flags;
            a.out_begin[r] = fell_back || !fits ? 0ull : join_base + first;
            if (flags & READ_SUSPECT) a.suspect_list[atomicAdd(&a.list_counters[1], 1u)] = (uint32_t)r;
            if (fell_back) { a.over_list[atomicAdd(&a.list_counters[0], 1u)] = (uint32_t)r; read_cut[r] = 2; }
            else if (!fits) { totals[4] = 1ull; read_cut[r] = 2; }
            else { atomicAdd(&totals[2], (unsigned long long)rows); atomicAdd(&totals[3], 1ull); }
        }
    }
}

// ... and, one wave a view, its rows copied to their place in the read's, c_s added to the positions.
__global__ __launch_bounds__(256) void seg_join_rows_kernel(const SegView *views, uint32_t n_views, const uint8_t *read_cut, const uint64_t *row_off,
                                                            const uint64_t *view_begin, const uint32_t *view_cnt, uint64_t view_rows_extent,
                                                            const uint32_t *vmin, const uint32_t *vpos, const uint8_t *vdir, const uint8_t *vmq, int has_q,
                                                            uint32_t *omin, uint32_t *opos, uint8_t *odir, uint8_t *omq, uint64_t join_base, uint64_t join_cap) {
    const unsigned lane = threadIdx.x & 63u;
    for (uint64_t v = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; v < n_views; v += ((uint64_t)gridDim.x * 256u) >> 6) {
        const SegView vw = views[v];
        if ((vw.flags & SEG_DEAD) || read_cut[vw.read] != 1) continue;
        const uint64_t src = view_begin[v], dst = row_off[v];
        const uint32_t n = view_cnt[v];
        if (dst + n > join_cap || src + n > view_rows_extent) continue;       // (never: seg_join_reads_kernel placed the read inside, the view wrote inside)
        for (uint32_t i = lane; i < n; i += 64u) {
            omin[join_base + dst + i] = vmin[src + i];
            opos[join_base + dst + i] = vpos[src + i] + vw.c_s;
            odir[join_base + dst + i] = vdir[src + i];
            if (has_q) omq[join_base + dst + i] = vmq[src + i];
        }
    }
}

// ---- padded -> dense CSR (+ per-minimizer minimum quality) -------------------------------------
// G lanes per read: 16 when reads hold a few dozen minimizers (4 reads in flight per wave: the kernel is a chain of
// dependent loads per read, so reads in flight are what it runs on), 64 for long reads / high densities.
template <bool HAS_QUAL, int G>
__global__ __launch_bounds__(256) void compact_minimizers_kernel(
    const uint64_t *cap_off, const uint64_t *off, uint32_t n_reads,
    const uint32_t *pmin, const uint32_t *ppos, const uint8_t *pdir, const uint32_t *pos_s, const uint32_t *pos_e,
    const uint8_t *qual, const uint64_t *qual_off,
    uint32_t *omin, uint32_t *opos, uint8_t *odir, uint8_t *oqual) {
    const unsigned lane = threadIdx.x & (unsigned)(G - 1);
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) / G;
    for (uint64_t r = wave; r < n_reads; r += nwaves) {
        uint64_t src = cap_off[r], dst = off[r];
        uint32_t n = (uint32_t)(off[r + 1] - dst);
        uint32_t ncopy = (uint32_t)(cap_off[r + 1] - src);   // padded capacity (overflowed reads are re-run)
        if (ncopy > n) ncopy = n;
        for (uint32_t i = lane; i < n; i += G) {
            uint8_t mq = 1;   // no qualities: ReadSelection.hpp:1047-1051
            if (i < ncopy) {
                omin[dst + i] = pmin[src + i];
                opos[dst + i] = ppos[src + i];
                odir[dst + i] = pdir[src + i];
                if (HAS_QUAL) {   // getMinQuality over the original span (ReadSelection.hpp:1302-1320)
                    const uint8_t *qq = qual + qual_off[r];
                    mq = 255;
                    for (uint32_t b = pos_s[src + i], e = pos_e[src + i]; b < e; b++) {
                        uint8_t q = (uint8_t)(qq[b] - 33);
                        if (q < mq) mq = q;
                    }
                }
            }
            oqual[dst + i] = mq;
        }
    }
}

// Exact sum of per-base error probabilities as a 128-bit fixed-point integer (units of 2^-64): sum_q T[q] with
// T[q] = float table entry * 2^64 (exact).  The host turns it into the reference's long double error sum
// (ReadSelection.hpp:870-879).  Every T[q] is a multiple of 2^QSHIFT (24-bit mantissas, smallest entry 10^-9.4;
// checked on the host), so T >> QSHIFT fits 56 bits: a lane adds 16 table entries per 16-byte load into a u64 and
// carries into a u32 above it.  One wave per read, 1 KB per wave per load; the 96-entry table sits in LDS.
constexpr int QBINS = 96;   // bins 0..94 = chars 33..127, bin 95 = everything else (contributes 0)
constexpr int QSHIFT = 9;
__global__ __launch_bounds__(256) void quality_sum_kernel(const uint8_t *qual, const uint64_t *qual_off, const uint32_t *len,
                                                          uint32_t n_reads, const uint64_t *tab_shifted,
                                                          uint64_t *sum_lo, uint64_t *sum_hi) {
    // the table by the quality CHARACTER itself (256 entries, zero outside 33 .. 127): a byte of the load is an address after one shift
    // and one mask -- no subtraction, no clamp.  This kernel runs beside the scan, which is bound by the vector unit: what it issues
    // there the scan pays for (6 ms of a 57 ms ONT scan before, tools/scan_ablate_ont.py)
    __shared__ uint64_t T[256];
    for (unsigned i = threadIdx.x; i < 256u; i += blockDim.x) T[i] = (i >= 33u && i < 33u + (unsigned)(QBINS - 1)) ? tab_shifted[i - 33u] : 0ull;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = wave; r < n_reads; r += nwaves) {
        const uint64_t begin = qual_off[r], end = begin + len[r];
        uint64_t acc_lo = 0;
        uint32_t acc_hi = 0;
        for (uint64_t chunk = (begin & ~15ull) + 16ull * lane; chunk < end; chunk += 16ull * 64ull) {
            const uint4 v = *reinterpret_cast<const uint4 *>(qual + chunk);   // the buffer is 16-byte padded at both ends
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
            if (!(chunk >= begin && chunk + 16 <= end)) {       // a read's first and last chunk: the bytes outside it become character 0
#pragma unroll
                for (int b = 0; b < 16; b++)
                    if (chunk + b < begin || chunk + b >= end) w[b >> 2] &= ~(0xFFu << (8 * (b & 3)));
            }
            uint64_t part = 0, part2 = 0;
#pragma unroll
            for (int b = 0; b < 16; b += 2) {
                part += T[(w[b >> 2] >> (8 * (b & 3))) & 0xFFu];
                part2 += T[(w[(b + 1) >> 2] >> (8 * ((b + 1) & 3))) & 0xFFu];
            }
            part += part2;
            const uint64_t nlo = acc_lo + part;
            acc_hi += nlo < acc_lo ? 1u : 0u;
            acc_lo = nlo;
        }
        for (int dlt = 32; dlt >= 1; dlt >>= 1) {     // 96-bit wave reduction
            const uint64_t olo = __shfl_xor(acc_lo, dlt, 64);
            const uint32_t ohi = __shfl_xor(acc_hi, dlt, 64);
            const uint64_t nlo = acc_lo + olo;
            acc_hi += ohi + (nlo < acc_lo ? 1u : 0u);
            acc_lo = nlo;
        }
        if (lane == 0) {
            sum_lo[r] = acc_lo << QSHIFT;
            sum_hi[r] = ((uint64_t)acc_hi << QSHIFT) | (acc_lo >> (64 - QSHIFT));
        }
    }
}

__global__ void capacity_kernel(const uint32_t *len, uint32_t n_reads, float density, uint32_t *cap) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_reads) {
        // generous first guess: 3x the expected count + slack; overflowing reads are re-run exactly
        float e = (float)len[i] * density * 3.0f + 32.0f;
        cap[i] = (uint32_t)e;
    }
}

// after the main launch: list the reads that overflowed their padded slots and the complexity suspects
__global__ void post_scan_lists_kernel(const uint32_t *count, const uint32_t *cap, const uint8_t *flags, uint32_t n_reads,
                                       uint32_t *over_list, uint32_t *suspect_list, uint32_t *counters /* [0]=over [1]=suspect */) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    if (count[i] > cap[i]) over_list[atomicAdd(&counters[0], 1u)] = (uint32_t)i;
    if (flags[i] & READ_SUSPECT) suspect_list[atomicAdd(&counters[1], 1u)] = (uint32_t)i;
}

// reads that outgrew the fast kernel's stage: their counts, then their places behind the regions
__global__ void gather_counts_kernel(const uint32_t *list, uint32_t n_list, const uint32_t *count, uint32_t *out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_list) out[i] = count[list[i]];
}

// suspects of the complexity bound among the listed reads (the general kernel only flags them): appended to the suspect list
__global__ void listed_suspects_kernel(const uint32_t *list, uint32_t n_list, const uint8_t *flags, uint32_t *suspect_list, uint32_t *n_suspect) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_list && (flags[list[i]] & READ_SUSPECT)) suspect_list[atomicAdd(n_suspect, 1u)] = list[i];
}

__global__ void place_overflow_kernel(const uint32_t *list, const uint64_t *start, const uint32_t *cnt, uint32_t n_list, uint64_t *cap_off,
                                      uint64_t *begin) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_list) return;
    const uint32_t r = list[i];
    cap_off[r] = start[i];
    cap_off[r + 1] = start[i] + cnt[i];      // consecutive listed reads (the list is sorted) agree on this entry
    begin[r] = start[i];
}

__global__ void apply_low_quality_kernel(const uint8_t *low, uint32_t n_reads, uint32_t *count, uint8_t *flags,
                                         unsigned long long *dropped /* may be null: sum of the counts cleared */) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_reads && low[i]) {
        if (dropped && count[i]) atomicAdd(dropped, (unsigned long long)count[i]);
        count[i] = 0; flags[i] |= (uint8_t)MDBG_READ_LOW_QUALITY;
    }
}

}  // namespace mdbg

using namespace mdbg;

// ReadSelection.hpp:870-879: float meanReadError = errorSum / n; meanReadQuality = -10.0f * log10(meanReadError).
// Evaluated at run time (volatile) so that n == 0 yields the same NaN bits (0xFFC00000 on x86-64)
// the reference writes into read_data_init.txt.
static float mean_quality_from_sum(long double error_sum_in, size_t n_in) {
    volatile long double error_sum = error_sum_in;
    volatile size_t n = n_in;
    volatile float mean_err = (float)(error_sum / n);
    return -10.0f * log10f(mean_err);
}

// grow-only pinned host buffer of the context (device -> host copies that must not wait for the main stream)
static int pinned_reserve(mdbg_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->pinned_bytes) return MDBG_OK;
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    ctx->pinned = nullptr; ctx->pinned_bytes = 0;
    const size_t want = bytes + bytes / 4;
    hipError_t e = hipHostMalloc(&ctx->pinned, want, hipHostMallocDefault);
    if (e != hipSuccess) { ctx->pinned = nullptr; return set_error(ctx, MDBG_ENOMEM, "hipHostMalloc(%zu): %s", want, hipGetErrorString(e)); }
    ctx->pinned_bytes = want;
    return MDBG_OK;
}

// A/B switch for the rule "one scan kernel at a time per device" (profiles/r03b_scan_mutex_ab.txt)
static bool scans_may_interleave() {
    static const bool on = getenv("MDBG_SCAN_NO_MUTEX") != nullptr;
    return on;
}

static std::mutex &device_scan_mutex(int device) {
    static std::mutex m[64];
    return m[(unsigned)device % 64u];
}

// The same rule ACROSS processes (two tools on one GPU, the ranks of a test sharing device 0): an advisory lock on a file named after
// the device's PCI address, taken inside the process-wide mutex.  Best effort: no lock file, no cross-process turn-taking
// (MDBG_SCAN_NO_XPROC_LOCK=1 switches it off).  flock costs about a microsecond; a scan launch is milliseconds.
static int device_scan_lockfile(int device) {
    static int fds[64];
    static std::once_flag once[64];
    const unsigned d = (unsigned)device % 64u;
    std::call_once(once[d], [&] {
        fds[d] = -1;
        if (getenv("MDBG_SCAN_NO_XPROC_LOCK")) return;
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) snprintf(bus, sizeof bus, "device%d", device);
        for (char *c = bus; *c; c++) if (*c == ':' || *c == '.' || *c == '/') *c = '_';
        for (const char *dir : {"/dev/shm", "/tmp"}) {
            std::string path = std::string(dir) + "/mdbg_scan_turn_" + bus + ".lock";
            const int fd = open(path.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0666);
            if (fd >= 0) { (void)fchmod(fd, 0666); fds[d] = fd; return; }
        }
    });
    return fds[d];
}

// one scan kernel at a time per device: the turn is held from the launch to the read-back of the counters
struct ScanTurn {
    std::unique_lock<std::mutex> in_process;
    int fd = -1;
    bool held = false;
    explicit ScanTurn(int device) : in_process(device_scan_mutex(device), std::defer_lock), fd(device_scan_lockfile(device)) {}
    void lock() {
        in_process.lock();
        if (fd >= 0) while (flock(fd, LOCK_EX) != 0 && errno == EINTR) {}
        held = true;
    }
    void unlock() {
        if (!held) return;
        if (fd >= 0) (void)flock(fd, LOCK_UN);
        in_process.unlock();
        held = false;
    }
    bool owns_lock() const { return held; }
    ~ScanTurn() { unlock(); }
};

// The context's bitmap for (l = 15, compressed, threshold, log2_bits): built on the context's stream when the key changes (a run of
// the tool has one key; tests change it), kept until the context goes.  *fill_ok: the bitmap is sparse enough to pay -- at most a
// quarter of its bits set (density 0.005f: 45 657 of 524 288, 8.7 %; from about density 0.013f on the existing walk is taken).  A
// geometry forced by "scan_prefilter_log2_bits" is a test's and is used whatever its fill.
static int prefilter_ensure(mdbg_ctx *ctx, uint64_t threshold, unsigned log2_bits, bool forced, bool *fill_ok) {
    constexpr size_t WORDS = PREFILTER_BYTES / 4;               // the buffer: the bitmap (always 64 KB: the kernel copies all of it) + the count
    if (!ctx->prefilter_bits) {
        std::lock_guard<std::mutex> g(hip_mem_mutex());
        hipError_t e = hipMalloc((void **)&ctx->prefilter_bits, (WORDS + 4) * 4);
        if (e != hipSuccess) { ctx->prefilter_bits = nullptr; return set_error(ctx, MDBG_ENOMEM, "hipMalloc of the scan's key bitmap: %s", hipGetErrorString(e)); }
        ctx->prefilter_valid = false;
    }
    if (!ctx->prefilter_valid || ctx->prefilter_threshold != threshold || ctx->prefilter_log2 != log2_bits) {
        ctx->prefilter_valid = false;
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(ctx->prefilter_bits, 0, (WORDS + 4) * 4, ctx->stream));
        {
            LaunchTimer timer(ctx, "scan_prefilter_build");
            hipLaunchKernelGGL(prefilter_build_kernel, dim3((unsigned)ctx->n_cu * 16u), dim3(256), 0, ctx->stream, ctx->prefilter_bits, threshold, log2_bits,
                               ctx->prefilter_bits + WORDS);
        }
        MDBG_HIP_CHECK(ctx, hipGetLastError());
        uint32_t n_set = 0;
        hipError_t e = memcpy_sync(ctx, &n_set, ctx->prefilter_bits + WORDS, 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return set_error(ctx, MDBG_EHIP, "the scan's key bitmap: %s", hipGetErrorString(e));
        ctx->prefilter_threshold = threshold; ctx->prefilter_log2 = log2_bits; ctx->prefilter_set = n_set;
        ctx->prefilter_valid = true;
        ctx->scan_info[2]++; ctx->scan_info[3] = n_set; ctx->scan_info[4] = log2_bits;
    }
    *fill_ok = forced || (uint64_t)ctx->prefilter_set * 4ull <= (1ull << log2_bits);
    // the selected-key table of the confirm step, for the same threshold: rebuilt with it or when its own geometry changes
    if (*fill_ok && ctx->scan_confirm_table) {
        constexpr size_t TABLE_WORDS = ((size_t)1 << CONFIRM_LOG2_BUCKETS) * CONFIRM_BUCKET_WORDS;      // allocated once, whatever the geometry
        const unsigned log2_buckets = ctx->scan_confirm_table_log2_buckets ? ctx->scan_confirm_table_log2_buckets : CONFIRM_LOG2_BUCKETS;
        if (!ctx->confirm_table) {
            std::lock_guard<std::mutex> g(hip_mem_mutex());
            hipError_t e = hipMalloc((void **)&ctx->confirm_table, (TABLE_WORDS + 4) * 4);
            if (e != hipSuccess) { ctx->confirm_table = nullptr; return set_error(ctx, MDBG_ENOMEM, "hipMalloc of the scan's key table: %s", hipGetErrorString(e)); }
            ctx->confirm_valid = false;
        }
        if (!ctx->confirm_valid || ctx->confirm_threshold != threshold || ctx->confirm_log2 != log2_buckets) {
            ctx->confirm_valid = false;
            const size_t words = ((size_t)1 << log2_buckets) * CONFIRM_BUCKET_WORDS;
            DevBuf<uint32_t> counts;
            MDBG_TRY(counts.alloc(ctx, (size_t)1 << log2_buckets));
            MDBG_HIP_CHECK(ctx, hipMemsetAsync(ctx->confirm_table, 0, words * 4, ctx->stream));
            MDBG_HIP_CHECK(ctx, hipMemsetAsync(ctx->confirm_table + TABLE_WORDS, 0, 16, ctx->stream));
            MDBG_HIP_CHECK(ctx, hipMemsetAsync(counts.p, 0, ((size_t)1 << log2_buckets) * 4, ctx->stream));
            {
                LaunchTimer timer(ctx, "scan_confirm_table_build");
                const dim3 grid((unsigned)ctx->n_cu * 16u), block(256);
                hipLaunchKernelGGL(confirm_table_insert_kernel, grid, block, 0, ctx->stream, ctx->confirm_table, counts.p, threshold, log2_buckets);
                hipLaunchKernelGGL(confirm_table_finish_kernel, dim3(grid_for((uint64_t)1 << log2_buckets, 256, (unsigned)ctx->n_cu * 16u)), block, 0, ctx->stream,
                                   ctx->confirm_table, counts.p, log2_buckets, ctx->confirm_table + TABLE_WORDS);
                if (confirm_table_needs_verify(log2_buckets))
                    hipLaunchKernelGGL(confirm_table_verify_kernel, grid, block, 0, ctx->stream, ctx->confirm_table, threshold, log2_buckets, ctx->confirm_table + TABLE_WORDS);
            }
            MDBG_HIP_CHECK(ctx, hipGetLastError());
            uint32_t n_over = 0;
            hipError_t e = memcpy_sync(ctx, &n_over, ctx->confirm_table + TABLE_WORDS, 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return set_error(ctx, MDBG_EHIP, "the scan's key table: %s", hipGetErrorString(e));
            ctx->confirm_threshold = threshold; ctx->confirm_log2 = log2_buckets;
            ctx->confirm_valid = true;
            ctx->scan_confirm_info[0]++; ctx->scan_confirm_info[1] = 1ull << log2_buckets; ctx->scan_confirm_info[2] = n_over;
        }
    }
    return MDBG_OK;
}

// The scan's A/B switches, each read here and nowhere else: MDBG_SCAN_NO_FAST (the general kernel for everything; includes the other two),
// MDBG_SCAN_NO_APPROX (the full 64-bit verdict at every position), MDBG_SCAN_NO_BUMP (mdbg_scan leaves its block path alone)
struct ScanSwitches { bool no_fast, approx_allowed, bump_allowed; };
static const ScanSwitches &scan_switches() {
    static const bool no_fast = getenv("MDBG_SCAN_NO_FAST") != nullptr;
    static const ScanSwitches s{no_fast, !no_fast && !getenv("MDBG_SCAN_NO_APPROX"), !no_fast && !getenv("MDBG_SCAN_NO_BUMP")};
    return s;
}

using ScanKernel = void (*)(ScanArgs);

static ScanKernel select_general_kernel(bool hpc, bool has_q, bool has_n) {
    static const ScanKernel k[8] = {scan_kernel<false, false, false>, scan_kernel<false, false, true>, scan_kernel<false, true, false>, scan_kernel<false, true, true>,
                                    scan_kernel<true, false, false>,  scan_kernel<true, false, true>,  scan_kernel<true, true, false>,  scan_kernel<true, true, true>};
    return k[(hpc ? 4 : 0) + (has_q ? 2 : 0) + (has_n ? 1 : 0)];
}

// pf_waves 16 or 8: the pre-filtered variant (compressed reads without qualities, candidate test); 0: a four-wave kernel -- bump mode:
// candidates by the upper half of the hash (span_step<APPROX>); the host's re-run of a read covers a false one.  seg: views (approx only)
static ScanKernel select_fast_kernel(bool hpc, bool has_q, bool approx, unsigned pf_waves, bool seg) {
    if (pf_waves == 16) return seg ? scan_fast_kernel<true, false, true, 16, true> : scan_fast_kernel<true, false, true, 16>;
    if (pf_waves == 8) return seg ? scan_fast_kernel<true, false, true, 8, true> : scan_fast_kernel<true, false, true, 8>;
    static const ScanKernel four_wave[3][4] = {      // [exact, approx, views][hpc, qualities]
        {scan_fast_kernel<false, false, false>, scan_fast_kernel<false, true, false>, scan_fast_kernel<true, false, false>, scan_fast_kernel<true, true, false>},
        {scan_fast_kernel<false, false, true>, scan_fast_kernel<false, true, true>, scan_fast_kernel<true, false, true>, scan_fast_kernel<true, true, true>},
        {scan_fast_kernel<false, false, true, 0, true>, scan_fast_kernel<false, true, true, 0, true>, scan_fast_kernel<true, false, true, 0, true>,
         scan_fast_kernel<true, true, true, 0, true>}};
    return four_wave[seg ? 2 : (approx ? 1 : 0)][(hpc ? 2 : 0) + (has_q ? 1 : 0)];
}

// static LDS of a kernel (0: the query failed)
static size_t kernel_static_lds(const void *kernel) {
    hipFuncAttributes at;
    if (hipFuncGetAttributes(&at, kernel) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return at.sharedSizeBytes;
}

// The pre-filtered variant ("scan_prefilter", MDBG_SCAN_PREFILTER): compressed reads at l = 15 without qualities, the candidate
// test as it is by default, a batch most of whose reads fit its smaller stage (mdbg_scan), a bitmap sparse enough (prefilter_ensure) -- and as many
// waves a workgroup as leave "scan_lds_reserve" free: 16, else 8, else the four-wave kernels with their padding.  Decided, and
// the bitmap queued on the context's stream, before the "scan" timer and the hand-over to the scan's stream.  *pf_waves: 0 when not taken.
static int choose_prefilter(mdbg_ctx *ctx, const ScanArgs &a, bool approx, bool hpc, bool has_q, uint32_t pf_len_limit, unsigned *pf_waves) {
    *pf_waves = 0;
    if (!(approx && hpc && !has_q && a.K == PREFILTER_L && a.cand_slack == 0u && a.guard_slack == 0u && pf_len_limit && ctx->scan_prefilter && !ctx->scan_lds_pad))
        return MDBG_OK;
    static const size_t lds16 = kernel_static_lds(reinterpret_cast<const void *>(scan_fast_kernel<true, false, true, 16>)),       // asked once
                        lds8 = kernel_static_lds(reinterpret_cast<const void *>(scan_fast_kernel<true, false, true, 8>));      // (the same with SEG)
    if (!lds16 || !lds8) return set_error(ctx, MDBG_EHIP, "hipFuncGetAttributes of the pre-filtered scan kernels failed");
    const unsigned waves = prefilter_wave_count(ctx->lds_per_cu, ctx->scan_lds_reserve, lds16, lds8);
    if (!waves) return MDBG_OK;
    const bool forced = ctx->scan_prefilter_log2_bits != 0u;
    bool fill_ok = false;
    MDBG_TRY(prefilter_ensure(ctx, a.threshold, forced ? ctx->scan_prefilter_log2_bits : PREFILTER_LOG2_BITS, forced, &fill_ok));
    if (fill_ok) *pf_waves = waves;
    return MDBG_OK;
}

// pf_split: flags in d_split what the four-wave launch in front of the variant skips -- every read but the long ones -- and counts
// the long reads' bases: *split false when they outweigh the split (long_reads_outweigh_split; the batch then keeps the four-wave kernel)
static int split_long_reads(mdbg_ctx *ctx, const ScanArgs &a, uint32_t n_items, uint32_t pf_len_limit, uint64_t batch_bases, DevBuf<uint8_t> &d_split, bool *split) {
    DevBuf<unsigned long long> d_long;
    MDBG_TRY(d_split.alloc(ctx, n_items));
    MDBG_TRY(d_long.alloc(ctx, 1));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(d_long.p, 0, 8, ctx->stream));
    hipLaunchKernelGGL(split_skip_kernel, dim3(grid_for(n_items, 256, (unsigned)ctx->n_cu * 8u)), dim3(256), 0, ctx->stream, a.len, a.skip, n_items, pf_len_limit,
                       d_split.p, d_long.p);
    unsigned long long long_bases = 0;
    if (memcpy_sync(ctx, &long_bases, d_long.p, 8, hipMemcpyDeviceToHost) != hipSuccess) return set_error(ctx, MDBG_EHIP, "scan: the long reads' bases could not be counted");
    *split = !long_reads_outweigh_split(long_bases, batch_bases);
    return MDBG_OK;
}

// "table_cu_count": the context's own stream is confined to a few CUs; the block-structured kernel goes to a stream over all of
// them, ordered after what the context has queued so far (take) and before what it queues next (give_back)
struct ScanStreamLoan {
    hipStream_t on = nullptr;
    hipEvent_t ordered = nullptr;
    int take(mdbg_ctx *ctx, bool fast) {
        on = ctx->stream;
        if (!(fast && ctx->scan_stream)) return MDBG_OK;
        MDBG_HIP_CHECK(ctx, hipEventCreateWithFlags(&ordered, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ordered, ctx->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->scan_stream, ordered, 0);
        if (e != hipSuccess) { (void)hipEventDestroy(ordered); return set_error(ctx, MDBG_EHIP, "scan stream hand-over: %s", hipGetErrorString(e)); }
        on = ctx->scan_stream;
        return MDBG_OK;
    }
    int give_back(mdbg_ctx *ctx) {
        if (!ordered) return MDBG_OK;
        hipError_t e = hipEventRecord(ordered, on);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ordered, 0);
        (void)hipEventDestroy(ordered);         // released by the runtime once the recorded work is done
        if (e != hipSuccess) return set_error(ctx, MDBG_EHIP, "scan stream hand-back: %s", hipGetErrorString(e));
        return MDBG_OK;
    }
};

// "scan_lds_pad" / "scan_lds_reserve" (scan_lds_padding): the kernel's static LDS is asked only where the reserve decides
static unsigned four_wave_lds_pad(const mdbg_ctx *ctx, ScanKernel fk) {
    const bool by_reserve = !ctx->scan_lds_pad && ctx->scan_lds_reserve;
    return scan_lds_padding(ctx->scan_lds_pad, ctx->scan_lds_reserve, ctx->lds_per_cu, by_reserve ? kernel_static_lds(reinterpret_cast<const void *>(fk)) : 0);
}

// The counter of one persistent launch: the context's next slot, zeroed on the stream the launch goes to.  A call makes more than one
// such launch (the batch's, its views'); each has a slot of its own, and a slot comes round again only SCAN_COUNTER_SLOTS launches
// later on a stream that orders them.
static int scan_counter_take(mdbg_ctx *ctx, hipStream_t on, unsigned long long **counter) {
    if (!ctx->scan_counters) {
        std::lock_guard<std::mutex> g(hip_mem_mutex());
        hipError_t e = hipMalloc((void **)&ctx->scan_counters, mdbg_ctx::SCAN_COUNTER_SLOTS * sizeof(unsigned long long));
        if (e != hipSuccess) { ctx->scan_counters = nullptr; return set_error(ctx, MDBG_ENOMEM, "hipMalloc of the scan's read counters: %s", hipGetErrorString(e)); }
    }
    *counter = ctx->scan_counters + ctx->scan_counter_next;
    ctx->scan_counter_next = (ctx->scan_counter_next + 1u) % mdbg_ctx::SCAN_COUNTER_SLOTS;
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(*counter, 0, sizeof(unsigned long long), on));
    return MDBG_OK;
}

// pf_len_limit > 0: the batch may take the pre-filtered variant, whose stage a read shorter than that is expected to fit; pf_split:
// the batch also holds longer reads -- a launch of the four-wave kernel in front of it scans those (ScanArgs::pf_len_split)
// seg: the items are views of long reads (ScanArgs::views): the SEG instantiations of the block-structured kernels, chosen as for reads
static int launch_scan(mdbg_ctx *ctx, ScanArgs &a, bool hpc, bool has_q, bool has_n, uint32_t n_items, uint32_t pf_len_limit = 0, bool pf_split = false,
                       uint64_t batch_bases = 0, bool seg = false) {
    a.n_reads = n_items;
    a.pf_counter = nullptr; a.pf_grab = 0;
    const ScanSwitches &sw = scan_switches();
    const bool fast = (!has_q || a.cursor) && !has_n && !a.subset && !sw.no_fast;
    const bool approx = fast && a.cursor && sw.approx_allowed && candidate_test_usable(a.threshold, a.cand_slack);
    if (seg && !approx) return set_error(ctx, MDBG_EINVAL, "scan: views are scanned by the candidate-hash kernels only");
    unsigned pf_waves = 0;
    MDBG_TRY(choose_prefilter(ctx, a, approx, hpc, has_q, pf_len_limit, &pf_waves));
    pf_split = pf_split && pf_waves;
    DevBuf<uint8_t> d_split;        // pf_split: what the four-wave launch skips (back to the pool on return: reuse is ordered on the context's stream)
    if (pf_split) {
        MDBG_TRY(split_long_reads(ctx, a, n_items, pf_len_limit, batch_bases, d_split, &pf_split));
        if (!pf_split) pf_waves = 0;
    }
    ScanStreamLoan loan;
    MDBG_TRY(loan.take(ctx, fast));
    if (fast) ctx->scan_info[6] = pf_waves ? 1 : 0;
    if (fast) ctx->scan_confirm_info[3] = 0;      // set below by a pre-filtered launch that takes the table
    {
        LaunchTimer timer(ctx, "scan", loan.on);
        const uint8_t *const batch_skip = a.skip;
        if (pf_split) a.skip = d_split.p;           // first the long reads, by the four-wave kernel below
        if (fast && (!pf_waves || pf_split)) {
            // plain ACGT without qualities: the block-structured kernel; a few reads per wave, then the wave retires
            ctx->scan_info[1]++;
            const ScanKernel fk = select_fast_kernel(hpc, has_q, approx, 0, seg);
            hipLaunchKernelGGL(fk, dim3(scan_blocks(n_items, FAST_WAVES, ctx->scan_reads_per_wave)), dim3(FAST_BLOCK), four_wave_lds_pad(ctx, fk), loan.on, a);
        } else if (!fast) {       // (else the pre-filtered variant below takes every read)
            hipLaunchKernelGGL(select_general_kernel(hpc, has_q, has_n), dim3(scan_blocks(n_items, SCAN_WAVES, ctx->scan_reads_per_wave)), dim3(SCAN_BLOCK), 0, ctx->stream, a);
        }
        a.skip = batch_skip;
        if (pf_waves) {
            // one workgroup of pf_waves waves per CU; it deals its chunk of reads out to its waves
            a.pf_bits = ctx->prefilter_bits;
            a.pf_shift = 32u - ctx->prefilter_log2;
            const bool by_table = ctx->scan_confirm_table && ctx->confirm_valid && ctx->confirm_threshold == a.threshold;
            a.pf_table = by_table ? reinterpret_cast<const uint4 *>(ctx->confirm_table) : nullptr;
            a.pf_table_shift = by_table ? 32u - ctx->confirm_log2 : 0u;
            ctx->scan_confirm_info[3] = by_table ? 1 : 0;
            a.pf_len_split = pf_split ? pf_len_limit : 0u;
            if (persistent_taken(ctx->scan_persistent, ctx->scan_reads_per_wave)) {
                // as many workgroups as CUs and none pending; every wave draws runs of reads from the launch's counter until it is used up
                unsigned long long *counter = nullptr;
                MDBG_TRY(scan_counter_take(ctx, loan.on, &counter));
                a.pf_counter = counter;
                a.pf_grab = persistent_grab(ctx->scan_grab_reads);
                a.pf_chunk = 0;
                const unsigned blocks = persistent_grid(n_items, pf_waves, a.pf_grab, ctx->n_cu, ctx->scan_persistent_blocks);
                hipLaunchKernelGGL(select_fast_kernel(true, false, true, pf_waves, seg), dim3(blocks), dim3(64u * pf_waves), 0, loan.on, a);
                ctx->scan_persistent_info[0] = 1; ctx->scan_persistent_info[1] = blocks; ctx->scan_persistent_info[2] = a.pf_grab; ctx->scan_persistent_info[3]++;
            } else {
                const PrefilterGrid grid = prefilter_grid(n_items, pf_waves, ctx->scan_reads_per_wave, ctx->n_cu);
                a.pf_chunk = grid.chunk;
                a.pf_counter = nullptr; a.pf_grab = 0;
                hipLaunchKernelGGL(select_fast_kernel(true, false, true, pf_waves, seg), dim3(grid.blocks), dim3(64u * pf_waves), 0, loan.on, a);
                ctx->scan_persistent_info[0] = 0; ctx->scan_persistent_info[1] = grid.blocks; ctx->scan_persistent_info[2] = 0;
            }
            ctx->scan_info[0]++; ctx->scan_info[5] = pf_waves;
        }
    }
    MDBG_TRY(loan.give_back(ctx));
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    return MDBG_OK;
}

// The plan of a batch whose long reads are cut into views (segments_dev.hpp): built on the device by the pre-pass, of which the host
// learns the totals only
struct SegPlan : SegTotals {
    DevBuf<uint32_t> tiles_per_read, views_per_read, tile_runs, tile_excl;
    DevBuf<uint64_t> tile_off, view_off;
    DevBuf<SegView> views;
    DevBuf<uint8_t> skip, read_cut;      // per read: left out of the batch's own launch (masked or cut); 1 = cut, 2 = cut but fallen back
    DevBuf<unsigned long long> totals;   // [0] reads cut, [1] their views, [2] rows joined, [3] reads joined, [4] the joined rows did not fit
};

static int seg_prepass(mdbg_ctx *ctx, const mdbg_reads *reads, const uint8_t *masked, uint32_t G, uint32_t K, bool hpc, SegPlan &sp) {
    const uint32_t n = reads->n_reads;
    const uint64_t max_tiles = reads->n_bases / SEG_TILE_BASES + n, max_views = reads->n_bases / G + n;
    MDBG_TRY(sp.tiles_per_read.alloc(ctx, n)); MDBG_TRY(sp.views_per_read.alloc(ctx, n));
    MDBG_TRY(sp.tile_off.alloc(ctx, (size_t)n + 1)); MDBG_TRY(sp.view_off.alloc(ctx, (size_t)n + 1));
    MDBG_TRY(sp.tile_runs.alloc(ctx, hpc ? max_tiles : 1)); MDBG_TRY(sp.tile_excl.alloc(ctx, hpc ? max_tiles : 1));
    MDBG_TRY(sp.views.alloc(ctx, max_views)); MDBG_TRY(sp.skip.alloc(ctx, n)); MDBG_TRY(sp.read_cut.alloc(ctx, n)); MDBG_TRY(sp.totals.alloc(ctx, 8));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(sp.totals.p, 0, 64, ctx->stream));
    const unsigned cap = (unsigned)ctx->n_cu * 16u;
    {
        LaunchTimer timer(ctx, "scan_segments");
        hipLaunchKernelGGL(seg_count_kernel, dim3(grid_for(n, 256, cap)), dim3(256), 0, ctx->stream, reads->d_len.p, masked, n, G, sp.tiles_per_read.p,
                           sp.views_per_read.p, sp.skip.p);
        MDBG_TRY(exclusive_scan_u32(ctx, sp.tiles_per_read.p, sp.tile_off.p, n));
        MDBG_TRY(exclusive_scan_u32(ctx, sp.views_per_read.p, sp.view_off.p, n));
        if (hpc) hipLaunchKernelGGL(seg_tile_runs_kernel, dim3(grid_for(max_tiles * 64u, 256, cap)), dim3(256), 0, ctx->stream, reads->d_words.p,
                                    reads->d_word_off.p, reads->d_len.p, n, sp.tile_off.p, sp.tile_runs.p);
        hipLaunchKernelGGL(seg_plan_kernel, dim3(grid_for((uint64_t)n * 64u, 256, cap)), dim3(256), 0, ctx->stream, reads->d_len.p, n, G, K, hpc ? 1 : 0,
                           sp.tile_off.p, sp.view_off.p, sp.tile_runs.p, sp.tile_excl.p, sp.views.p, sp.skip.p, sp.read_cut.p, sp.totals.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    unsigned long long h[3] = {0, 0, 0};
    hipError_t e;
    if ((e = hipMemcpyAsync(&h[0], sp.totals.p, 8, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(&h[1], sp.view_off.p + n, 8, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(&h[2], sp.tile_off.p + n, 8, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
        return set_error(ctx, MDBG_EHIP, "scan: the plan of the long reads' segments failed: %s", hipGetErrorString(e));
    sp.n_cut = h[0]; sp.n_views = h[1]; sp.n_tiles = h[2];
    if (sp.n_views > max_views || sp.n_tiles > max_tiles || sp.n_views > 0xFFFFFFFFull) return set_error(ctx, MDBG_EHIP, "scan: inconsistent segment plan");
    return MDBG_OK;
}

// ---- mean read quality (exact 128-bit sums on the device, long double finish on the host) ----
struct QualitySums {
    std::vector<uint8_t> low_quality;
    bool any_low_quality = false;
    DevBuf<uint64_t> d_qtab, d_slo, d_shi;
    struct SideGuard { hipStream_t s = nullptr; ~SideGuard() { if (s) (void)hipStreamSynchronize(s); } } side_guard;   // before the buffers go
    bool pending = false;

    // the table, the sums beside (or in front of) the scan, their downloads queued behind them
    int start(mdbg_ctx *ctx, const mdbg_reads *reads, mdbg_minimizers *m, bool has_q) {
        const uint32_t n = reads->n_reads;
        hipError_t e;
        if (!(has_q && n)) {
            // no qualities: every read's mean quality is the NaN the reference writes; kept as one value, not n of them (a 40 MB
            // host fill per 10 M reads sat on the critical path in front of the kernel launch)
            m->h_mean_quality.clear();
            m->mean_quality_all = mean_quality_from_sum(0, 0);
            return MDBG_OK;
        }
        // table exactly as the reference builds it (ReadSelection.hpp:101-104, Commons.hpp:2338-2341)
        std::vector<uint64_t> tsh(QBINS, 0);
        for (int q = 33; q <= 127; q++) {
            float qq = (float)(uint8_t)(q - 33);
            float t = powf(10.0f, -qq / 10.0f);
            long double scaled = (long double)t * 18446744073709551616.0L;   // * 2^64, exact (24-bit mantissa)
            unsigned __int128 v = (unsigned __int128)scaled;
            if ((uint64_t)v & ((1ull << QSHIFT) - 1ull)) return set_error(ctx, MDBG_EINVAL, "quality table entry %d is not a multiple of 2^%d", q, QSHIFT);
            tsh[q - 33] = (uint64_t)(v >> QSHIFT);
        }
        MDBG_TRY(d_qtab.alloc(ctx, QBINS)); MDBG_TRY(d_slo.alloc(ctx, n)); MDBG_TRY(d_shi.alloc(ctx, n));
        if ((e = memcpy_sync(ctx, d_qtab.p, tsh.data(), QBINS * 8, hipMemcpyHostToDevice)) != hipSuccess)
            return set_error(ctx, MDBG_EHIP, "quality table upload failed: %s", hipGetErrorString(e));
        // The sums run BESIDE the scan, on the side stream (round 5; until then in front of it, on the context's stream: 61 ms of a 0.52 s
        // pass over 200 Gbp of ONT reads): they are a second pass over the quality bytes at 3 TB/s -- memory traffic the VALU-bound scan
        // leaves idle -- in blocks of 768 bytes of LDS that fit beside the scan's.  Their way to the host (pinned memory) and the host's share
        // (finish) follow on the same stream: nothing of the mean quality is needed before the rows are counted.
        // ("scan_quality_stream" 0: in front of the scan as before, A/B.)
        MDBG_TRY(pinned_reserve(ctx, (size_t)n * 20));
        const bool beside = ctx->scan_quality_beside != 0;
        hipStream_t qs = beside ? ctx->side_stream : ctx->stream;
        hipEvent_t ev;
        if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return set_error(ctx, MDBG_EHIP, "hipEventCreate: %s", hipGetErrorString(e));
        if (beside) {                                   // behind whatever the context's stream has queued so far (the reads, the table upload)
            (void)hipEventRecord(ev, ctx->stream);
            (void)hipStreamWaitEvent(ctx->side_stream, ev, 0);
        }
        side_guard.s = ctx->side_stream;     // from here on every way out waits for the side stream before d_slo / d_shi / d_qtab go back to the pool (round-5 ADVICE)
        {
            LaunchTimer timer(ctx, "quality_sum", qs);
            unsigned blocks = grid_for((uint64_t)n * 64, 256, (unsigned)ctx->n_cu * 8u);
            hipLaunchKernelGGL(quality_sum_kernel, dim3(blocks), dim3(256), 0, qs, reads->d_qual.p, reads->d_qual_off.p,
                               reads->d_len.p, n, d_qtab.p, d_slo.p, d_shi.p);
        }
        if (!beside) {
            (void)hipEventRecord(ev, ctx->stream);
            (void)hipStreamWaitEvent(ctx->side_stream, ev, 0);
        }
        (void)hipEventDestroy(ev);
        uint8_t *h = (uint8_t *)ctx->pinned;
        if ((e = hipMemcpyAsync(h, d_slo.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->side_stream)) != hipSuccess ||
            (e = hipMemcpyAsync(h + (size_t)n * 8, d_shi.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->side_stream)) != hipSuccess ||
            (e = hipMemcpyAsync(h + (size_t)n * 16, reads->d_len.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->side_stream)) != hipSuccess)
            return set_error(ctx, MDBG_EHIP, "quality sums download failed: %s", hipGetErrorString(e));
        pending = true;
        return MDBG_OK;
    }

    // the host's share of the mean qualities: the reference's long double division and log10 per read, on a few host threads.  Called
    // once the scan kernel is queued and before the first blocking download -- host work while the kernel runs; a second call does nothing
    int finish(mdbg_ctx *ctx, const mdbg_scan_params *p, mdbg_minimizers *m) {
        if (!pending) return MDBG_OK;
        pending = false;
        hipError_t qe;
        if ((qe = hipStreamSynchronize(ctx->side_stream)) != hipSuccess)
            return set_error(ctx, MDBG_EHIP, "quality sums download failed: %s", hipGetErrorString(qe));
        const uint32_t n = m->n_reads;
        const uint64_t *slo = (const uint64_t *)ctx->pinned, *shi = slo + n;
        const uint32_t *lens = (const uint32_t *)(shi + n);
        m->h_mean_quality.resize(n);
        low_quality.assign(n, 0);
        const bool filter = p->apply_read_filters != 0;
        const float min_q = p->min_read_quality;
        const unsigned n_thr = n < 65536 ? 1u : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
        std::vector<char> any(n_thr, 0);
        auto work = [&](unsigned t) {
            const uint32_t r0 = (uint32_t)((uint64_t)n * t / n_thr), r1 = (uint32_t)((uint64_t)n * (t + 1) / n_thr);
            for (uint32_t r = r0; r < r1; r++) {
                long double sq = ((long double)shi[r] * 18446744073709551616.0L + (long double)slo[r]) / 18446744073709551616.0L;
                float mq = mean_quality_from_sum(sq, lens[r]);
                m->h_mean_quality[r] = mq;
                if (filter && mq < min_q) { low_quality[r] = 1; any[t] = 1; }   // ReadSelection.hpp:901-909
            }
        };
        if (n_thr == 1) work(0);
        else {
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < n_thr; t++) pool.emplace_back(work, t);
            for (auto &th : pool) th.join();
        }
        for (char c : any) any_low_quality |= c != 0;
        return MDBG_OK;
    }
};

constexpr uint32_t CTL_OVER = 64, CTL_DROPPED = 65, CTL_WORDS = 66;     // the block path's u64 words: cursors, {n_over, n_suspect}, rows dropped
constexpr uint32_t SCTL_WORDS = 66;                                     // the views' cursors and [64] = {views listed, -}

// the block path's buffers that are not the batch's output
struct BlockBufs {
    DevBuf<uint32_t> d_over, d_susp;
    DevBuf<unsigned long long> d_ctl;
    DevBuf<uint32_t> sv_min, sv_pos, sv_cnt, sv_over;       // the views' own rows, counts and counters
    DevBuf<uint8_t> sv_dir, sv_mq, sv_flags, sv_bad;
    DevBuf<uint64_t> sv_begin, sv_row_off;
    DevBuf<unsigned long long> sv_cx, sv_ctl;
};

// what the phases of one mdbg_scan share.  (The order of the members is the order in which they go: the quality sums first -- their side
// stream waited for, then their buffers -- then the batch's own.)
struct ScanJob {
    mdbg_ctx *ctx;
    const mdbg_reads *reads;
    const mdbg_scan_params *p;
    mdbg_minimizers *m;
    uint32_t n;
    bool hpc, has_q, has_n;
    DevBuf<uint32_t> d_cap, d_count, d_rep;
    DevBuf<uint64_t> d_cap_off;
    QualitySums quality;


    // the fields of ScanArgs that the block path and the general path set alike
    ScanArgs base_scan_args() {
        ScanArgs a{};
        a.words = reads->d_words.p; a.word_off = reads->d_word_off.p; a.len = reads->d_len.p;
        a.qual = has_q ? reads->d_qual.p : nullptr; a.qual_off = has_q ? reads->d_qual_off.p : nullptr;
        a.K = p->minimizer_size; a.threshold = density_threshold(p->density);
        a.select_invalid = kmer_hash64(INVALID_KMER) < a.threshold ? 1u : 0u;
        a.trim = p->no_end_trim ? 0u : 1u; a.q_last = p->quality_window == 1 ? 1u : 0u;
        a.rep = d_rep.p; a.n_rep = p->n_repetitive; a.apply_filters = p->apply_read_filters;
        a.out_flags = m->d_flags.p;
        return a;
    }

    // The exact complexity pass over the few reads the 2-mer bound could not clear, then the reads below --min-read-quality, which keep
    // their (empty) record (ReadSelection.hpp:901-909).  d_dropped: the block path's counter of the rows these passes take away, read back
    // into *dropped after each; null on the general path, which counts its rows afterwards.
    int apply_read_verdicts(const uint32_t *d_suspects, uint32_t n_suspect, uint32_t *d_counts, unsigned long long *d_dropped, uint64_t *dropped) {
        hipError_t e;
        if (n_suspect) {
            LaunchTimer timer(ctx, "complexity_exact");
            hipLaunchKernelGGL(complexity_exact_kernel, dim3(grid_for((uint64_t)n_suspect * 64, 256, (unsigned)ctx->n_cu * 8u)), dim3(256), 0,
                               ctx->stream, reads->d_words.p, reads->d_word_off.p, reads->d_len.p, d_suspects, n_suspect,
                               d_counts, m->d_flags.p, d_dropped);
            if (d_dropped && (e = memcpy_sync(ctx, dropped, d_dropped, 8, hipMemcpyDeviceToHost)) != hipSuccess)
                return set_error(ctx, MDBG_EHIP, "complexity pass failed: %s", hipGetErrorString(e));
        }
        if (quality.any_low_quality) {
            DevBuf<uint8_t> d_low;
            MDBG_TRY(d_low.alloc(ctx, n));
            if ((e = memcpy_sync(ctx, d_low.p, quality.low_quality.data(), n, hipMemcpyHostToDevice)) != hipSuccess)
                return set_error(ctx, MDBG_EHIP, "low-quality flags upload failed: %s", hipGetErrorString(e));
            hipLaunchKernelGGL(apply_low_quality_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_low.p, n, d_counts, m->d_flags.p, d_dropped);
            if (d_dropped) {
                if ((e = memcpy_sync(ctx, dropped, d_dropped, 8, hipMemcpyDeviceToHost)) != hipSuccess)
                    return set_error(ctx, MDBG_EHIP, "low-quality pass failed: %s", hipGetErrorString(e));
            } else if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return set_error(ctx, MDBG_EHIP, "low-quality pass failed");
        }
        return MDBG_OK;
    }

    // the views, in one launch of the variant a batch of reads of segment length would take; then the join
    int scan_views_and_join(const ScanArgs &a, SegPlan &seg, const RegionPlan &rp, BlockBufs &b) {
        const uint32_t nv = (uint32_t)seg.n_views;
        ScanArgs v = a;
        v.views = seg.views.p; v.view_cx = b.sv_cx.p; v.seg_tiles = ctx->scan_segment_bases / SEG_TILE_BASES;
        v.out_min = b.sv_min.p; v.out_pos = b.sv_pos.p; v.out_dir = b.sv_dir.p; v.out_mqual = b.sv_mq.p;
        v.out_count = b.sv_cnt.p; v.out_flags = b.sv_flags.p; v.out_begin = b.sv_begin.p;
        v.cursor = b.sv_ctl.p; v.n_regions = rp.seg_regions; v.out_capacity = rp.seg_region_cap;
        v.over_list = b.sv_over.p; v.suspect_list = nullptr; v.list_counters = (uint32_t *)(b.sv_ctl.p + 64);
        v.skip = nullptr;
        MDBG_TRY(launch_scan(ctx, v, hpc, has_q, false, nv, rp.seg_pf_limit, false, 0, true));
        MDBG_TRY(exclusive_scan_u32(ctx, b.sv_cnt.p, b.sv_row_off.p, nv));
        {
            LaunchTimer timer(ctx, "scan_segments");
            const unsigned cap_blocks = (unsigned)ctx->n_cu * 16u;
            hipLaunchKernelGGL(seg_mark_views_kernel, dim3(grid_for(nv, 256, cap_blocks)), dim3(256), 0, ctx->stream, b.sv_over.p, (const uint32_t *)(b.sv_ctl.p + 64), nv, b.sv_bad.p);
            hipLaunchKernelGGL(seg_join_reads_kernel, dim3(grid_for((uint64_t)n * 64u, 256, cap_blocks)), dim3(256), 0, ctx->stream, a, n, seg.view_off.p,
                               b.sv_row_off.p, b.sv_bad.p, b.sv_cx.p, seg.read_cut.p, rp.capacity, rp.seg_rows, seg.totals.p);
            hipLaunchKernelGGL(seg_join_rows_kernel, dim3(grid_for((uint64_t)nv * 64u, 256, cap_blocks)), dim3(256), 0, ctx->stream, seg.views.p, nv, seg.read_cut.p,
                               b.sv_row_off.p, b.sv_begin.p, b.sv_cnt.p, rp.seg_region_cap * rp.seg_regions, b.sv_min.p, b.sv_pos.p, b.sv_dir.p, b.sv_mq.p, has_q ? 1 : 0,
                               m->d_min.p, m->d_pos.p, m->d_dir.p, m->d_mqual.p, rp.capacity, rp.seg_rows);
        }
        hipError_t e;
        if ((e = hipGetLastError()) != hipSuccess) return set_error(ctx, MDBG_EHIP, "scan: the join of the views failed: %s", hipGetErrorString(e));
        return MDBG_OK;
    }

    // the reads the block kernel skipped for their side masks: counted here by the general kernel with no room to write (masked_args is
    // what their re-run takes); their suspects join the list, and *n_suspect is read again
    int count_masked_reads(ScanArgs &masked_args, BlockBufs &b, std::vector<uint32_t> &m_cnt, uint32_t *n_suspect) {
        const uint32_t n_masked = reads->n_masked;
        hipError_t e;
        if ((e = hipMemsetAsync(d_cap_off.p, 0, ((size_t)n + 1) * 8, ctx->stream)) != hipSuccess)
            return set_error(ctx, MDBG_EHIP, "capacity clear failed: %s", hipGetErrorString(e));
        masked_args.cursor = nullptr; masked_args.skip = nullptr;
        masked_args.subset = reads->d_masked_list.p;
        masked_args.cap_off = d_cap_off.p;                       // every read: no room -- the pass only counts
        masked_args.invalid = reads->d_invalid.p;
        masked_args.brk = reads->has_break ? reads->d_break.p : nullptr;
        masked_args.inline_minq = 1;           // (counts and flags go where the block kernel's go)
        MDBG_TRY(launch_scan(ctx, masked_args, hpc, has_q, true, n_masked));
        hipLaunchKernelGGL(listed_suspects_kernel, dim3(grid_for(n_masked, 256)), dim3(256), 0, ctx->stream, reads->d_masked_list.p, n_masked,
                           m->d_flags.p, b.d_susp.p, (uint32_t *)(b.d_ctl.p + CTL_OVER) + 1);
        DevBuf<uint32_t> d_mc;
        MDBG_TRY(d_mc.alloc(ctx, n_masked));
        hipLaunchKernelGGL(gather_counts_kernel, dim3(grid_for(n_masked, 256)), dim3(256), 0, ctx->stream, reads->d_masked_list.p, n_masked, m->d_cnt.p, d_mc.p);
        m_cnt.resize(n_masked);
        unsigned long long ctl_over = 0;
        if ((e = memcpy_sync(ctx, m_cnt.data(), d_mc.p, (size_t)n_masked * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
            (e = memcpy_sync(ctx, &ctl_over, b.d_ctl.p + CTL_OVER, 8, hipMemcpyDeviceToHost)) != hipSuccess)
            return set_error(ctx, MDBG_EHIP, "masked counts copy failed: %s", hipGetErrorString(e));
        *n_suspect = (uint32_t)(ctl_over >> 32);
        return MDBG_OK;
    }

    // Both kinds of unfinished reads are placed in read order behind the regions (place_unfinished_reads) and scanned by the general kernel,
    // each kind with its own variant.  *placed stays false when they do not fit the reserve.
    int rerun_unfinished_reads(const ScanArgs &a, const ScanArgs &masked_args, const RegionPlan &rp, BlockBufs &b, uint32_t n_over, bool route_masked,
                               const std::vector<uint32_t> &m_cnt, uint64_t h_join_rows, uint64_t *rows, bool *placed) {
        hipError_t e;
        std::vector<uint32_t> list(n_over), cnts(n_over);
        DevBuf<uint32_t> d_oc;
        MDBG_TRY(d_oc.alloc(ctx, (size_t)n_over + 1));
        if (n_over) {
            hipLaunchKernelGGL(gather_counts_kernel, dim3(grid_for(n_over, 256)), dim3(256), 0, ctx->stream, b.d_over.p, n_over, m->d_cnt.p, d_oc.p);
            if ((e = memcpy_sync(ctx, list.data(), b.d_over.p, (size_t)n_over * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
                (e = memcpy_sync(ctx, cnts.data(), d_oc.p, (size_t)n_over * 4, hipMemcpyDeviceToHost)) != hipSuccess)
                return set_error(ctx, MDBG_EHIP, "overflow list copy failed: %s", hipGetErrorString(e));
        }
        std::vector<uint32_t> m_list(route_masked ? reads->n_masked : 0u);
        if (!m_list.empty() && (e = memcpy_sync(ctx, m_list.data(), reads->d_masked_list.p, m_list.size() * 4, hipMemcpyDeviceToHost)) != hipSuccess)
            return set_error(ctx, MDBG_EHIP, "masked list copy failed: %s", hipGetErrorString(e));
        const Placement pl = place_unfinished_reads(list, cnts, m_list, m_cnt, rp.capacity, rp.capacity + h_join_rows /* behind the joined reads */, rp.reserve);
        if (!pl.fits) return MDBG_OK;
        DevBuf<uint32_t> scratch_count;
        DevBuf<uint8_t> scratch_flags;
        MDBG_TRY(scratch_count.alloc(ctx, n)); MDBG_TRY(scratch_flags.alloc(ctx, n));
        DevBuf<uint64_t> d_start[2];
        DevBuf<uint32_t> d_list[2], d_cnt2[2];
        for (int kind = 0; kind < 2; kind++) {
            const uint32_t nk = (uint32_t)pl.list[kind].size();
            if (!nk) continue;
            MDBG_TRY(d_start[kind].alloc(ctx, nk)); MDBG_TRY(d_list[kind].alloc(ctx, nk)); MDBG_TRY(d_cnt2[kind].alloc(ctx, nk));
            if ((e = memcpy_sync(ctx, d_list[kind].p, pl.list[kind].data(), (size_t)nk * 4, hipMemcpyHostToDevice)) != hipSuccess ||
                (e = memcpy_sync(ctx, d_cnt2[kind].p, pl.cnt[kind].data(), (size_t)nk * 4, hipMemcpyHostToDevice)) != hipSuccess ||
                (e = memcpy_sync(ctx, d_start[kind].p, pl.start[kind].data(), (size_t)nk * 8, hipMemcpyHostToDevice)) != hipSuccess)
                return set_error(ctx, MDBG_EHIP, "overflow plan upload failed: %s", hipGetErrorString(e));
            hipLaunchKernelGGL(place_overflow_kernel, dim3(grid_for(nk, 256)), dim3(256), 0, ctx->stream, d_list[kind].p, d_start[kind].p, d_cnt2[kind].p, nk,
                               d_cap_off.p, m->d_begin.p);
        }
        for (int kind = 0; kind < 2; kind++) {
            const uint32_t nk = (uint32_t)pl.list[kind].size();
            if (!nk) continue;
            ScanArgs r = kind ? masked_args : a;
            r.cursor = nullptr; r.skip = nullptr;
            r.subset = d_list[kind].p;
            r.cap_off = d_cap_off.p;
            r.inline_minq = 1;
            r.out_count = scratch_count.p; r.out_flags = scratch_flags.p;
            MDBG_TRY(launch_scan(ctx, r, hpc, has_q, kind == 1, nk));
        }
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return set_error(ctx, MDBG_EHIP, "overflow re-run failed: %s", hipGetErrorString(e));
        *rows += pl.rows;
        *placed = true;
        return MDBG_OK;
    }

    // ---- plain ACGT without qualities: the block-structured kernel writes every read's rows once, where a wave found room
    // (mdbg_minimizers::scattered); one read-back instead of four.  Batches it cannot take -- a read selecting more than the
    // LDS stage holds, more rows than the estimate allowed for -- go through the general path: *done stays false (not this batch).
    int scan_block_path(const BlockRoute &route, SegPlan &seg, bool *done) {
        const uint32_t n_masked = has_n ? reads->n_masked : 0u;
        const bool route_masked = route.route_masked;
        hipError_t e;
        const RegionPlan rp = plan_regions(n, reads->n_bases, reads->max_len, p->density, hpc, seg, ctx->scan_segment_bases, SEG_TILE_BASES, PF_STAGE_CAP);
        const uint64_t extent = rp.capacity + rp.reserve;
        BlockBufs b;
        MDBG_TRY(m->d_begin.alloc(ctx, n)); MDBG_TRY(m->d_cnt.alloc(ctx, n)); MDBG_TRY(b.d_over.alloc(ctx, n)); MDBG_TRY(b.d_susp.alloc(ctx, n));
        MDBG_TRY(b.d_ctl.alloc(ctx, CTL_WORDS)); MDBG_TRY(m->d_min.alloc(ctx, extent)); MDBG_TRY(m->d_pos.alloc(ctx, extent));
        MDBG_TRY(m->d_dir.alloc(ctx, extent)); MDBG_TRY(m->d_mqual.alloc(ctx, extent));
        (void)hipMemsetAsync(b.d_ctl.p, 0, CTL_WORDS * 8, ctx->stream);
        ScanArgs a = base_scan_args();
        a.out_min = m->d_min.p; a.out_pos = m->d_pos.p; a.out_dir = m->d_dir.p; a.out_mqual = m->d_mqual.p; a.out_count = m->d_cnt.p;
        a.cursor = b.d_ctl.p; a.n_regions = rp.n_regions; a.out_capacity = rp.region_cap; a.out_begin = m->d_begin.p;
        a.over_list = b.d_over.p; a.suspect_list = b.d_susp.p; a.list_counters = (uint32_t *)(b.d_ctl.p + CTL_OVER);
        a.cand_slack = ctx->scan_cand_slack; a.guard_slack = ctx->scan_guard_slack; a.wave_priority = ctx->scan_wave_priority;
        a.skip = seg.n_cut ? seg.skip.p : (route_masked ? reads->d_masked.p : nullptr);       // (the plan's flags: masked or cut)
        const uint32_t nv = (uint32_t)seg.n_views;
        if (seg.n_cut) {
            const uint64_t ext = rp.seg_region_cap * rp.seg_regions;
            MDBG_TRY(b.sv_min.alloc(ctx, ext)); MDBG_TRY(b.sv_pos.alloc(ctx, ext)); MDBG_TRY(b.sv_dir.alloc(ctx, ext)); MDBG_TRY(b.sv_mq.alloc(ctx, has_q ? ext : 1));
            MDBG_TRY(b.sv_cnt.alloc(ctx, nv)); MDBG_TRY(b.sv_over.alloc(ctx, nv)); MDBG_TRY(b.sv_flags.alloc(ctx, nv)); MDBG_TRY(b.sv_bad.alloc(ctx, nv));
            MDBG_TRY(b.sv_begin.alloc(ctx, nv)); MDBG_TRY(b.sv_row_off.alloc(ctx, (size_t)nv + 1)); MDBG_TRY(b.sv_cx.alloc(ctx, nv)); MDBG_TRY(b.sv_ctl.alloc(ctx, SCTL_WORDS));
            if ((e = hipMemsetAsync(b.sv_ctl.p, 0, SCTL_WORDS * 8, ctx->stream)) != hipSuccess || (e = hipMemsetAsync(b.sv_bad.p, 0, nv, ctx->stream)) != hipSuccess)
                return set_error(ctx, MDBG_EHIP, "scan: clearing the views' counters failed: %s", hipGetErrorString(e));
        }
        unsigned long long h_ctl[CTL_WORDS], h_sctl[SCTL_WORDS] = {0}, h_seg[8] = {0}, h_join_rows = 0;
        {
            ScanTurn scan_turn(ctx->device);      // one scan kernel at a time per device (see scan_general_path)
            if (!scans_may_interleave()) scan_turn.lock();
            // (a batch all of whose reads are cut or masked -- contigs -- has nothing for its own launch: the join and the masked pass below
            // set those reads' begin, count and flags)
            const bool nothing_left = seg.n_cut && seg.n_cut + (route_masked ? (uint64_t)n_masked : 0ull) >= n;
            if (!nothing_left) MDBG_TRY(launch_scan(ctx, a, hpc, has_q, false, n, rp.pf_len_limit, rp.pf_split, reads->n_bases));
            if (seg.n_cut) MDBG_TRY(scan_views_and_join(a, seg, rp, b));
            MDBG_TRY(quality.finish(ctx, p, m));          // host work while the kernel runs
            e = memcpy_sync(ctx, h_ctl, b.d_ctl.p, CTL_WORDS * 8, hipMemcpyDeviceToHost);
            if (e == hipSuccess && seg.n_cut) {
                if ((e = memcpy_sync(ctx, h_sctl, b.sv_ctl.p, SCTL_WORDS * 8, hipMemcpyDeviceToHost)) == hipSuccess &&
                    (e = memcpy_sync(ctx, h_seg, seg.totals.p, 64, hipMemcpyDeviceToHost)) == hipSuccess)
                    e = memcpy_sync(ctx, &h_join_rows, b.sv_row_off.p + nv, 8, hipMemcpyDeviceToHost);
            }
        }
        if (e != hipSuccess) return set_error(ctx, MDBG_EHIP, "scan counters copy failed: %s", hipGetErrorString(e));
        uint64_t rows = 0;
        bool fits = true;
        for (uint32_t g = 0; g < rp.n_regions; g++) { rows += h_ctl[g]; fits = fits && h_ctl[g] <= rp.region_cap; }
        if (seg.n_cut) {          // the views' rows fitted their regions and the joined reads their room; the rows of the reads joined
            for (uint32_t g = 0; g < rp.seg_regions; g++) fits = fits && h_sctl[g] <= rp.seg_region_cap;
            fits = fits && h_seg[4] == 0ull && h_join_rows <= rp.seg_rows;
            rows += h_seg[2];
        }
        const uint32_t n_over = (uint32_t)h_ctl[CTL_OVER];
        uint32_t n_suspect = (uint32_t)(h_ctl[CTL_OVER] >> 32);
        // ---- reads the block kernel did not finish: those that outgrew its stage (long reads; listed with their exact counts) and
        // those it skipped for their side masks
        ScanArgs masked_args = a;
        std::vector<uint32_t> m_cnt;
        bool counted = true;
        if (fits && n_masked && route_masked) MDBG_TRY(count_masked_reads(masked_args, b, m_cnt, &n_suspect));
        else if (n_masked && route_masked) counted = false;
        bool placed = n_over == 0 && (!route_masked || n_masked == 0);
        if (fits && counted && !placed && overflowing_reads_are_few(n_over, n))
            MDBG_TRY(rerun_unfinished_reads(a, masked_args, rp, b, n_over, route_masked, m_cnt, h_join_rows, &rows, &placed));
        if (!(placed && fits)) {
            // not this batch: give the buffers back and take the general path
            m->d_begin.release(); m->d_cnt.release(); m->d_min.release(); m->d_pos.release(); m->d_dir.release(); m->d_mqual.release();
            return MDBG_OK;
        }
        uint64_t dropped = 0;
        MDBG_TRY(apply_read_verdicts(b.d_susp.p, n_suspect, m->d_cnt.p, b.d_ctl.p + CTL_DROPPED, &dropped));
        if (!has_q) (void)hipMemsetAsync(m->d_mqual.p, 1, extent, ctx->stream);     // no qualities: ReadSelection.hpp:1047-1051
        m->scattered = true;
        m->owner = ctx;
        m->n_rows = extent;        // extent of the row arrays (regions are not filled to the brim)
        m->n_min = rows - dropped;
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return set_error(ctx, MDBG_EHIP, "scan failed: %s", hipGetErrorString(e));
        ctx->scan_info[7] = h_seg[3];
        *done = true;
        return MDBG_OK;
    }

    template <bool Q, int G>
    void launch_compact(unsigned blocks, const uint32_t *p_min, const uint32_t *p_pos, const uint8_t *p_dir, const uint32_t *p_os, const uint32_t *p_oe) {
        hipLaunchKernelGGL((compact_minimizers_kernel<Q, G>), dim3(blocks), dim3(256), 0, ctx->stream, d_cap_off.p, m->d_off.p, n, p_min, p_pos, p_dir,
                           Q ? p_os : nullptr, Q ? p_oe : nullptr, Q ? reads->d_qual.p : nullptr, Q ? reads->d_qual_off.p : nullptr,
                           m->d_min.p, m->d_pos.p, m->d_dir.p, m->d_mqual.p);
    }

    // every kind of batch: padded slots per read, the general kernel (or, for plain reads, a block-structured one without cursors), the
    // counts, then dense rows
    int scan_general_path() {
        hipError_t e;
        if (n) hipLaunchKernelGGL(capacity_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream,
                                  reads->d_len.p, n, p->density, d_cap.p);
        MDBG_TRY(exclusive_scan_u32(ctx, d_cap.p, d_cap_off.p, n));
        uint64_t cap_total = 0;
        e = memcpy_sync(ctx, &cap_total, d_cap_off.p + n, 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return set_error(ctx, MDBG_EHIP, "cap total copy failed");

        DevBuf<uint32_t> p_min, p_pos, p_os, p_oe;
        DevBuf<uint8_t> p_dir;
        MDBG_TRY(p_min.alloc(ctx, cap_total)); MDBG_TRY(p_pos.alloc(ctx, cap_total)); MDBG_TRY(p_dir.alloc(ctx, cap_total));
        if (has_q) { MDBG_TRY(p_os.alloc(ctx, cap_total)); MDBG_TRY(p_oe.alloc(ctx, cap_total)); }

        ScanArgs a = base_scan_args();
        a.invalid = has_n ? reads->d_invalid.p : nullptr;
        a.brk = reads->has_break ? reads->d_break.p : nullptr;
        a.cap_off = d_cap_off.p;
        a.out_min = p_min.p; a.out_pos = p_pos.p; a.out_dir = p_dir.p;
        a.out_os = p_os.p; a.out_oe = p_oe.p; a.out_mqual = nullptr; a.inline_minq = 0;
        a.out_count = d_count.p;
        // One scan kernel at a time per device, whatever the number of contexts: two of them interleaved workgroup by
        // workgroup each run at half speed and worse (measured: 2 x 15.5 ms alone, 2 x 30 ms interleaved), while everything
        // else a second context does -- table building, purge, RCCL -- overlaps a running scan nicely.  The lock covers the
        // launch and is released when the kernel has finished (the counter download below waits for it).
        ScanTurn scan_turn(ctx->device);
        if (!scans_may_interleave()) scan_turn.lock();
        if (n) MDBG_TRY(launch_scan(ctx, a, hpc, has_q, has_n, n));
        MDBG_TRY(quality.finish(ctx, p, m));                  // host work while the kernel runs (once: an abandoned block path has done it)

        // overflow handling (reads that selected more than their padded capacity are re-run with exact room)
        // and the exact complexity pass over the few reads the 2-mer bound could not clear
        DevBuf<uint32_t> d_list, d_suspects, d_nlist;
        MDBG_TRY(d_list.alloc(ctx, n)); MDBG_TRY(d_suspects.alloc(ctx, n)); MDBG_TRY(d_nlist.alloc(ctx, 2));
        (void)hipMemsetAsync(d_nlist.p, 0, 8, ctx->stream);
        if (n) hipLaunchKernelGGL(post_scan_lists_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream,
                                  d_count.p, d_cap.p, m->d_flags.p, n, d_list.p, d_suspects.p, d_nlist.p);
        uint32_t h_counters[2] = {0, 0};
        e = memcpy_sync(ctx, h_counters, d_nlist.p, 8, hipMemcpyDeviceToHost);
        if (scan_turn.owns_lock()) scan_turn.unlock();
        if (e != hipSuccess) return set_error(ctx, MDBG_EHIP, "overflow count copy failed: %s", hipGetErrorString(e));
        const uint32_t n_over = h_counters[0], n_suspect = h_counters[1];
        MDBG_TRY(apply_read_verdicts(d_suspects.p, n_suspect, d_count.p, nullptr, nullptr));

        // dense offsets from the true counts
        MDBG_TRY(exclusive_scan_u32(ctx, d_count.p, m->d_off.p, n));
        uint64_t total = 0;
        e = memcpy_sync(ctx, &total, m->d_off.p + n, 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return set_error(ctx, MDBG_EHIP, "total copy failed");
        m->n_min = total;
        MDBG_TRY(m->d_min.alloc(ctx, total)); MDBG_TRY(m->d_pos.alloc(ctx, total)); MDBG_TRY(m->d_dir.alloc(ctx, total)); MDBG_TRY(m->d_mqual.alloc(ctx, total));

        if (n) {
            const bool few = total / (n ? n : 1) < 96;   // minimizers per read
            unsigned blocks = grid_for((uint64_t)n * (few ? 16 : 64), 256, (unsigned)ctx->n_cu * (few ? 32u : 8u));
            LaunchTimer timer(ctx, "scan_compact");
            if (has_q) { if (few) launch_compact<true, 16>(blocks, p_min.p, p_pos.p, p_dir.p, p_os.p, p_oe.p); else launch_compact<true, 64>(blocks, p_min.p, p_pos.p, p_dir.p, p_os.p, p_oe.p); }
            else { if (few) launch_compact<false, 16>(blocks, p_min.p, p_pos.p, p_dir.p, nullptr, nullptr); else launch_compact<false, 64>(blocks, p_min.p, p_pos.p, p_dir.p, nullptr, nullptr); }
        }
        DevBuf<uint32_t> scratch_count;     // (of the re-run below: they go after the last synchronisation)
        DevBuf<uint8_t> scratch_flags;
        if (n_over) {
            // reads that overflowed their padded slots are re-run straight into their dense slots
            // (capacity == exact count), after the gather so the exact rows win over the truncated prefix
            ScanArgs r = a;
            r.subset = d_list.p;
            r.cap_off = m->d_off.p;
            r.out_min = m->d_min.p; r.out_pos = m->d_pos.p; r.out_dir = m->d_dir.p;
            r.out_mqual = m->d_mqual.p; r.inline_minq = 1;
            MDBG_TRY(scratch_count.alloc(ctx, n)); MDBG_TRY(scratch_flags.alloc(ctx, n));
            r.out_count = scratch_count.p; r.out_flags = scratch_flags.p;
            MDBG_TRY(launch_scan(ctx, r, hpc, has_q, has_n, n_over));
        }
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return set_error(ctx, MDBG_EHIP, "scan failed: %s", hipGetErrorString(e));
        return MDBG_OK;
    }
};

extern "C" int mdbg_scan(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_scan_params *p, mdbg_minimizers **out) try {
    if (!ctx || !reads || !p || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_scan: null argument");
    if (p->quality_window != 0 && p->quality_window != 1) return set_error(ctx, MDBG_EINVAL, "mdbg_scan: quality_window must be 0 or 1");
    if (p->minimizer_size < 2 || p->minimizer_size > 16)
        return set_error(ctx, MDBG_EINVAL, "mdbg_scan: minimizer_size %u outside [2,16]", p->minimizer_size);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_HIP_CHECK(ctx, reads_ready_on(ctx, reads));        // an upload still in flight (mdbg_reads_from_packed_async): ordered on the device
    const uint32_t n = reads->n_reads;
    ctx->scan_info[7] = 0;
    std::unique_ptr<mdbg_minimizers> m(new mdbg_minimizers());     // released into *out on success
    m->n_reads = n;
    m->from_scan = true;
    ScanJob j{ctx, reads, p, m.get(), n, p->hpc != 0, reads->has_qual && !p->ignore_qualities, reads->has_invalid};
    MDBG_TRY(j.d_cap.alloc(ctx, n)); MDBG_TRY(j.d_count.alloc(ctx, n)); MDBG_TRY(j.d_cap_off.alloc(ctx, (size_t)n + 1));
    MDBG_TRY(m->d_flags.alloc(ctx, n)); MDBG_TRY(m->d_len.alloc(ctx, n)); MDBG_TRY(m->d_off.alloc(ctx, (size_t)n + 1));
    hipError_t e;
    if (p->n_repetitive) {
        std::vector<uint32_t> rep(p->repetitive, p->repetitive + p->n_repetitive);
        std::sort(rep.begin(), rep.end());
        MDBG_TRY(j.d_rep.alloc(ctx, rep.size()));
        e = memcpy_sync(ctx, j.d_rep.p, rep.data(), rep.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return set_error(ctx, MDBG_EHIP, "copy of repetitive set failed");
    }
    e = hipMemcpyAsync(m->d_len.p, reads->d_len.p, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream);
    if (e != hipSuccess) return set_error(ctx, MDBG_EHIP, "len copy failed: %s", hipGetErrorString(e));
    MDBG_TRY(j.quality.start(ctx, reads, m.get(), j.has_q));

    const ScanSwitches &sw = scan_switches();
    const BlockRoute route = plan_block_route(n, reads->n_bases, reads->max_len, p->density, j.hpc, j.has_n, reads->d_masked.p != nullptr, j.has_n ? reads->n_masked : 0u,
                                              sw.bump_allowed, STAGE_CAP);
    SegPlan seg;
    if (segments_wanted(route, ctx->scan_segments, reads->max_len, ctx->scan_segment_bases, STAGE_CAP, sw.approx_allowed, density_threshold(p->density), ctx->scan_cand_slack))
        MDBG_TRY(seg_prepass(ctx, reads, route.route_masked ? reads->d_masked.p : nullptr, ctx->scan_segment_bases, p->minimizer_size, j.hpc, seg));
    bool done = false;
    if (route.block_path_but_length && (route.avg_fits_stage || seg.n_cut)) MDBG_TRY(j.scan_block_path(route, seg, &done));
    if (!done) MDBG_TRY(j.scan_general_path());
    *out = m.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_scan_confirm_info(const mdbg_ctx *ctx, uint64_t info[4]) {
    if (!ctx || !info) return MDBG_EINVAL;
    for (int i = 0; i < 4; i++) info[i] = ctx->scan_confirm_info[i];
    return MDBG_OK;
}

extern "C" int mdbg_scan_persistent_info(const mdbg_ctx *ctx, uint64_t info[4]) {
    if (!ctx || !info) return MDBG_EINVAL;
    for (int i = 0; i < 4; i++) info[i] = ctx->scan_persistent_info[i];
    return MDBG_OK;
}

extern "C" int mdbg_scan_info(const mdbg_ctx *ctx, uint64_t info[8]) {
    if (!ctx || !info) return MDBG_EINVAL;
    for (int i = 0; i < 8; i++) info[i] = ctx->scan_info[i];
    return MDBG_OK;
}

namespace mdbg {
const StepKernel *scan_step_kernels(uint32_t *n) {
    static const StepKernel k[] = {
        {"scan_prefiltered_16", reinterpret_cast<const void *>(scan_fast_kernel<true, false, true, 16>), 1024, 0},
    };
    *n = (uint32_t)(sizeof(k) / sizeof(k[0]));
    return k;
}
}  // namespace mdbg
