// stitch.hip -- mdbg_spans_stitch / mdbg_reads_stitch_ranges: contig sequences put together from oriented pieces of the packed reads on the
// device, and mdbg_sequences_to_fasta_bytes: the text ToBasespaceGfa::CreateBaseContigsFunctor (toBasespace/ToBasespaceGfa.hpp:1464-1795)
// hands to gzwrite.  The last step of the path mdbg_kminmer_spans and mdbg_spans_extract walk: spans -> pieces -> contigs -> FASTA text.
//
// The stitch, two steps, over the parts of extract.hip (extract_plan.hpp, extract_dev.hpp):
//   the plan    one lane a piece: its range and every check as mdbg_spans_extract makes them (extract_request_range / extract_given_range),
//               a 16-byte record (where the read's words begin, start, length, the net orientation, the invalid code).  An exclusive scan
//               of the piece lengths gives each piece its base offset; a contig's length is the difference of two of them, its words
//               extract_words of that; a second scan gives the contigs' offsets.  One status word and the totals travel back.
//   the copy    the OUTPUT WORDS of the whole batch are dealt to the waves in contiguous spans (wave_span), one lane an aligned pair of
//               words and one 16-byte store.  A lane keeps its contig and its piece in registers and moves on by extract_next_owner's
//               doubling search -- over the contigs' byte offsets, over the pieces' base offsets.  A word is the OR of what the pieces
//               that meet it contribute (stitch_dev.hpp).
// The text, two steps: the plan counts a record's bytes (header by the decimal width of the name, bases, newlines) and scans them in 64
// bits; the write deals the OUTPUT WORDS of the text to the waves the same way, a lane composes 16 bytes from the per-byte rule of
// stitch_dev.hpp (eight bases at a time where a word lies inside one sequence) and stores them once; nothing is read from the output and
// nothing stored behind its last byte.
// No LDS, no scratch; every buffer comes from the context's pool.
#include "extract_plan.hpp"
#include "stitch_dev.hpp"

#include <algorithm>
#include <memory>
#include <vector>

namespace mdbg {

static_assert(sizeof(mdbg_stitch_piece) == 16 && sizeof(StitchRec) == 16, "16 bytes a piece");
static_assert(MDBG_STITCH_NONE == STITCH_NONE, "the header's sentinel is the composition's");

constexpr uint32_t STITCH_CONTIG_TOO_LONG = 8;           // beside the EXTRACT_BAD_* reasons

// what a lane of the plan leaves behind: the record and the length; a refused piece takes no room
__device__ __forceinline__ uint32_t stitch_emit(uint64_t i, uint32_t why, ExtractRange rg, bool flip, const uint64_t *word_off, StitchRec *recs, uint32_t *plen,
                                                unsigned long long *status) {
    if (why) {
        atomicMin(status, ((unsigned long long)i << 8) | why);
        rg.length = 0u;
    }
    if (rg.length == 0u) {                                // (nothing of it is ever looked at: extract_next_owner steps over empty pieces)
        recs[i] = StitchRec{0ull, 0u, 0u};
        plen[i] = 0u;
        return 0u;
    }
    recs[i] = StitchRec{word_off[rg.read] | ((rg.reversed != 0u) != flip ? STITCH_REC_REVERSED : 0ull) | (flip ? STITCH_REC_INVALID_T : 0ull), rg.start, rg.length};
    plen[i] = rg.length;
    return rg.length;
}

// (window, part, flip) pieces
__global__ __launch_bounds__(256) void stitch_plan_kernel(const mdbg_stitch_piece *in, uint64_t n, const uint32_t *read_len, uint32_t n_reads, SpansView sp,
                                                          const uint64_t *word_off, StitchRec *recs, uint32_t *plen, unsigned long long *status) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const mdbg_stitch_piece q = in[i];
        ExtractRange rg{0u, 0u, 0u, 0u};
        const uint32_t why = q.window == STITCH_NONE ? 0u : extract_request_range(q.window, q.part, sp, read_len, n_reads, rg);
        stitch_emit(i, why, rg, q.flip != 0u, word_off, recs, plen, status);
    }
}

// ranges given by the caller
__global__ __launch_bounds__(256) void stitch_plan_ranges_kernel(const mdbg_seq_range *in, uint64_t n, const uint32_t *read_len, uint32_t n_reads,
                                                                 const uint64_t *word_off, StitchRec *recs, uint32_t *plen, unsigned long long *status) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const mdbg_seq_range q = in[i];
        const ExtractRange rg{q.read, q.start, q.length, q.reversed ? 1u : 0u};
        stitch_emit(i, extract_given_range(q.read, q.start, q.length, read_len, n_reads), rg, false, word_off, recs, plen, status);
    }
}

// a contig's bases and words from the base offsets of its first piece and of the next contig's
__global__ __launch_bounds__(256) void stitch_contigs_kernel(const uint64_t *pbase, const uint64_t *poff, uint64_t n, uint32_t form, uint32_t *lengths, uint32_t *words,
                                                             unsigned long long *too_long) {
    for (uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; c < n; c += (uint64_t)gridDim.x * 256u) {
        uint64_t len = pbase[poff[c + 1u]] - pbase[poff[c]];
        if (len >= (1ull << 32)) { atomicMin(too_long, (unsigned long long)c); len = 0u; }
        lengths[c] = (uint32_t)len;
        words[c] = extract_words((uint32_t)len, form);
    }
}

struct StitchGlobalSrc {
    const uint64_t *w; const uint32_t *inv;
    __device__ __forceinline__ const uint64_t *words(uint64_t w0) const { return w + w0; }
    __device__ __forceinline__ const uint32_t *mask(uint64_t w0) const { return inv ? inv + w0 : nullptr; }
};

// The contig a lane is inside of: its index, its bytes [lo, hi) of the output, the base offset of its first piece, its bases.
struct StitchContig { uint32_t c; uint64_t lo, hi, base0; uint32_t length; };

__device__ __forceinline__ void contig_load(StitchContig &o, uint32_t c, const uint64_t *off, const uint64_t *poff, const uint64_t *pbase, const uint32_t *lengths) {
    o.c = c;
    o.lo = off[c];
    o.hi = off[c + 1u];
    o.base0 = pbase[poff[c]];
    o.length = lengths[c];
}

// The copy, one lane an aligned PAIR of output words stored as 16 bytes, as extract_copy_kernel.  off: the contigs' byte offsets (multiples
// of 8); pbase: the pieces' base offsets (n_pieces + 1); poff: the contigs' first pieces.
__global__ __launch_bounds__(256) void stitch_copy_kernel(StitchGlobalSrc src, const StitchRec *recs, const uint64_t *pbase, uint32_t n_pieces, const uint64_t *poff,
                                                          const uint64_t *off, const uint32_t *lengths, uint32_t n, uint64_t n_words, uint32_t form, uint64_t *out) {
    const WaveSpan sp = wave_span((n_words + 1u) / 2u, 64u);
    if (sp.begin >= sp.end) return;
    const uint32_t per = form == EXTRACT_ASCII ? 8u : 32u;
    StitchContig o;
    contig_load(o, csr_owner(off, n, sp.begin * 16u), off, poff, pbase, lengths);
    StitchPiece pc;
    stitch_piece_load(pc, csr_owner(pbase, n_pieces, o.base0 + (uint64_t)per * (2u * sp.begin - o.lo / 8u)), pbase, recs);
    for (uint64_t p = sp.begin + (threadIdx.x & 63u); p < sp.end; p += 64u) {
        uint64_t v[2] = {0ull, 0ull};
#pragma unroll
        for (uint32_t h = 0; h < 2u; h++) {
            const uint64_t g = 2u * p + h;
            if (g >= n_words) break;
            if (g * 8u >= o.hi) contig_load(o, extract_next_owner(off, n, o.c, g * 8u), off, poff, pbase, lengths);
            const uint32_t w = (uint32_t)(g - o.lo / 8u);
            v[h] = stitch_word(src, pbase, n_pieces, recs, pc, o.base0 + (uint64_t)per * w, stitch_word_bases(o.length, w, form), form);
        }
        if (2u * p + 1u < n_words) *reinterpret_cast<ulonglong2 *>(out + 2u * p) = make_ulonglong2(v[0], v[1]);
        else out[2u * p] = v[0];
    }
}

// ---- the text ---------------------------------------------------------------------------------------------------------------------------
// names / flags: null = the index / 0
__global__ __launch_bounds__(256) void fasta_plan_kernel(const uint32_t *lengths, const uint32_t *names, const uint8_t *flags, uint64_t n, uint64_t *rbytes) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
        rbytes[i] = fasta_record_bytes(names ? names[i] : (uint32_t)i, flags ? flags[i] : 0u, lengths[i]);
}

// the record a lane is inside of: its index, its bytes [lo, hi) of the text, what its header is made of, its sequence
struct FastaRecord { uint32_t r; uint64_t lo, hi; uint32_t name, flag, length, header; const uint8_t *seq; };

__device__ __forceinline__ void record_load(FastaRecord &o, uint32_t r, const uint64_t *roff, const uint32_t *lengths, const uint32_t *names, const uint8_t *flags,
                                            const uint64_t *seq_off, const uint8_t *seq_bytes) {
    o.r = r;
    o.lo = roff[r];
    o.hi = roff[r + 1u];
    o.name = names ? names[r] : r;
    o.flag = flags ? flags[r] : 0u;
    o.length = lengths[r];
    o.header = fasta_header_bytes(o.name, o.flag, o.length);
    o.seq = seq_bytes + seq_off[r];
}

// The write, one lane an aligned pair of 8-byte words of the text.  A record is at least 9 bytes, so a word meets at most two.
__global__ __launch_bounds__(256) void fasta_write_kernel(const uint64_t *roff, uint32_t n, const uint32_t *lengths, const uint32_t *names, const uint8_t *flags,
                                                          const uint64_t *seq_off, const uint8_t *seq_bytes, uint8_t *out, uint64_t n_bytes) {
    const uint64_t n_words = (n_bytes + 7u) / 8u;
    const WaveSpan sp = wave_span((n_words + 1u) / 2u, 64u);
    if (sp.begin >= sp.end) return;
    FastaRecord o;
    record_load(o, csr_owner(roff, n, sp.begin * 16u), roff, lengths, names, flags, seq_off, seq_bytes);
    for (uint64_t p = sp.begin + (threadIdx.x & 63u); p < sp.end; p += 64u) {
        uint64_t v[2] = {0ull, 0ull};
#pragma unroll
        for (uint32_t h = 0; h < 2u; h++) {
            const uint64_t at = 16u * p + 8u * h;
            if (at >= n_bytes) break;
            if (at >= o.hi) record_load(o, extract_next_owner(roff, n, o.r, at), roff, lengths, names, flags, seq_off, seq_bytes);
            const uint64_t k = at - o.lo;
            if (k >= o.header && k - o.header + 8u <= o.length) { v[h] = fasta_bases8(o.seq, k - o.header); continue; }
#pragma unroll
            for (uint32_t b = 0; b < 8u; b++) {
                if (at + b >= n_bytes) break;
                if (at + b >= o.hi) record_load(o, o.r + 1u, roff, lengths, names, flags, seq_off, seq_bytes);        // (no record is empty)
                v[h] |= (uint64_t)fasta_byte(o.name, o.flag, o.length, o.header, o.seq, at + b - o.lo) << (8u * b);
            }
        }
        const uint64_t at = 16u * p;
        if (at + 16u <= n_bytes) *reinterpret_cast<ulonglong2 *>(out + at) = make_ulonglong2(v[0], v[1]);
        else
            for (uint64_t b = at; b < n_bytes; b++) out[b] = (uint8_t)((b - at < 8u ? v[0] : v[1]) >> (8u * ((b - at) % 8u)));
    }
}

const StepKernel *stitch_step_kernels(uint32_t *n) {
    static const StepKernel k[] = {
        {"stitch_plan", reinterpret_cast<const void *>(stitch_plan_kernel), 256, 2},
        {"stitch_plan_ranges", reinterpret_cast<const void *>(stitch_plan_ranges_kernel), 256, 2},
        {"stitch_contigs", reinterpret_cast<const void *>(stitch_contigs_kernel), 256, 2},
        {"stitch_copy", reinterpret_cast<const void *>(stitch_copy_kernel), 256, 2},
        {"fasta_plan", reinterpret_cast<const void *>(fasta_plan_kernel), 256, 2},
        {"fasta_write", reinterpret_cast<const void *>(fasta_write_kernel), 256, 2},
    };
    *n = (uint32_t)(sizeof(k) / sizeof(k[0]));
    return k;
}

// Both entry points behind their argument checks: exactly one of pieces / ranges is set (both null: no piece at all).
static int stitch_run(mdbg_ctx *ctx, const char *who, const mdbg_reads *reads, const mdbg_spans *spans, const mdbg_stitch_piece *pieces, const mdbg_seq_range *ranges,
                      const uint64_t *piece_offsets, uint64_t n, int form, mdbg_sequences **out) {
    if (form != MDBG_SEQ_BITSET && form != MDBG_SEQ_ASCII) return set_error(ctx, MDBG_EINVAL, "%s: form %d is neither MDBG_SEQ_BITSET nor MDBG_SEQ_ASCII", who, form);
    if (n >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "%s: 2^32 contigs or more in one call", who);
    if (piece_offsets[0] != 0) return set_error(ctx, MDBG_EINVAL, "%s: piece_offsets[0] is %llu, not 0", who, (unsigned long long)piece_offsets[0]);
    for (uint64_t c = 0; c < n; c++)
        if (piece_offsets[c + 1] < piece_offsets[c])
            return set_error(ctx, MDBG_EINVAL, "%s: piece_offsets decrease behind contig %llu (%llu, then %llu)", who, (unsigned long long)c,
                             (unsigned long long)piece_offsets[c], (unsigned long long)piece_offsets[c + 1]);
    const uint64_t n_pieces = piece_offsets[n];
    if (n_pieces >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "%s: 2^32 pieces or more in one call", who);
    if (n_pieces && !pieces && !ranges) return set_error(ctx, MDBG_EINVAL, "%s: null argument", who);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_HIP_CHECK(ctx, reads_ready_on(ctx, reads));  // behind an asynchronous upload, on the device
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    std::unique_ptr<mdbg_sequences> sq(new mdbg_sequences());
    sq->n = n; sq->form = form;
    MDBG_TRY(sq->d_off.alloc(ctx, (size_t)n + 1));
    MDBG_TRY(sq->d_len.alloc(ctx, n));

    // ---- the plan: ranges, checks, the pieces' base offsets, the contigs' lengths and offsets ------------------------------------------
    DevBuf<uint8_t> d_in;                             // the pieces as given, 16 bytes each
    DevBuf<uint64_t> poff, pbase;                     // the contigs' first pieces (n + 1), the pieces' base offsets (n_pieces + 1)
    DevBuf<StitchRec> recs;
    DevBuf<uint32_t> plen, words;
    DevBuf<unsigned long long> status;                // [0] the checks' verdict, [1] the bytes in all, [2] the bases in all, [3] the first contig of 2^32 bases
    MDBG_TRY(d_in.alloc(ctx, (size_t)n_pieces * 16));
    MDBG_TRY(poff.alloc(ctx, (size_t)n + 1));
    MDBG_TRY(pbase.alloc(ctx, (size_t)n_pieces + 1));
    MDBG_TRY(recs.alloc(ctx, n_pieces));
    MDBG_TRY(plen.alloc(ctx, n_pieces));
    MDBG_TRY(words.alloc(ctx, n));
    MDBG_TRY(status.alloc(ctx, 4));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(status.p, 0xFF, 32, ctx->stream));
    if (n_pieces)
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d_in.p, pieces ? (const void *)pieces : (const void *)ranges, (size_t)n_pieces * 16, hipMemcpyHostToDevice, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(poff.p, piece_offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    {
        LaunchTimer timer(ctx, "stitch_plan");
        if (n_pieces && pieces)
            hipLaunchKernelGGL(stitch_plan_kernel, dim3(grid_for(n_pieces, 256, cap)), dim3(256), 0, ctx->stream, reinterpret_cast<const mdbg_stitch_piece *>(d_in.p),
                               n_pieces, reads->d_len.p, reads->n_reads, spans_view(spans), reads->d_word_off.p, recs.p, plen.p, status.p);
        else if (n_pieces)
            hipLaunchKernelGGL(stitch_plan_ranges_kernel, dim3(grid_for(n_pieces, 256, cap)), dim3(256), 0, ctx->stream, reinterpret_cast<const mdbg_seq_range *>(d_in.p),
                               n_pieces, reads->d_len.p, reads->n_reads, reads->d_word_off.p, recs.p, plen.p, status.p);
        MDBG_TRY(exclusive_scan_u32(ctx, plen.p, pbase.p, n_pieces));
        if (n)
            hipLaunchKernelGGL(stitch_contigs_kernel, dim3(grid_for(n, 256, cap)), dim3(256), 0, ctx->stream, pbase.p, poff.p, n, (uint32_t)form, sq->d_len.p, words.p,
                               status.p + 3);
        MDBG_TRY(exclusive_scan_u32(ctx, words.p, sq->d_off.p, n));
        extract_offsets_to_bytes(ctx, sq->d_off.p, n + 1);
    }
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(status.p + 1, sq->d_off.p + n, 8, hipMemcpyDeviceToDevice, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(status.p + 2, pbase.p + n_pieces, 8, hipMemcpyDeviceToDevice, ctx->stream));
    unsigned long long verdict[4] = {0, 0, 0, 0};
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, verdict, status.p, 32, hipMemcpyDeviceToHost));      // (the host's arrays have been read: the stream is idle)
    if (verdict[0] != EXTRACT_FINE) {
        const unsigned long long piece = verdict[0] >> 8;
        const unsigned long long contig = (unsigned long long)(std::upper_bound(piece_offsets, piece_offsets + n + 1, (uint64_t)piece) - piece_offsets) - 1u;
        return set_error(ctx, MDBG_EINVAL, "%s: piece %llu (piece %llu of contig %llu): %s", who, piece, piece - (unsigned long long)piece_offsets[contig], contig,
                         extract_why_text((uint32_t)(verdict[0] & 0xFFu)));
    }
    if (verdict[3] != ~0ull) return set_error(ctx, MDBG_ERANGE, "%s: contig %llu has 2^32 bases or more", who, verdict[3]);
    sq->n_bytes = verdict[1];
    sq->n_bases = verdict[2];

    // ---- the copy ----------------------------------------------------------------------------------------------------------------------
    MDBG_TRY(sq->d_bytes.alloc(ctx, sq->n_bytes));
    const uint64_t n_words = sq->n_bytes / 8u;
    if (n_words) {
        LaunchTimer timer(ctx, "stitch_copy");
        hipLaunchKernelGGL(stitch_copy_kernel, dim3(grid_for((n_words + 1u) / 2u, 256, cap)), dim3(256), 0, ctx->stream,
                           StitchGlobalSrc{reads->d_words.p, reads->has_invalid ? reads->d_invalid.p : nullptr}, recs.p, pbase.p, (uint32_t)n_pieces, poff.p, sq->d_off.p,
                           sq->d_len.p, (uint32_t)n, n_words, (uint32_t)form, reinterpret_cast<uint64_t *>(sq->d_bytes.p));
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    // the plan's buffers go back to the pool, which hands them to later work on the same stream only; the inputs must outlive the kernels
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = sq.release();
    return MDBG_OK;
}

}  // namespace mdbg

using namespace mdbg;

extern "C" int mdbg_spans_stitch(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_spans *spans, const mdbg_stitch_piece *pieces, const uint64_t *piece_offsets,
                                 uint64_t n_contigs, int form, mdbg_sequences **out) try {
    if (!ctx || !reads || !spans || !piece_offsets || !out || (piece_offsets[n_contigs] && !pieces)) return set_error(ctx, MDBG_EINVAL, "mdbg_spans_stitch: null argument");
    if (spans->n_reads != reads->n_reads)
        return set_error(ctx, MDBG_EINVAL, "mdbg_spans_stitch: %u reads but spans of %u (not these reads' spans)", reads->n_reads, spans->n_reads);
    return stitch_run(ctx, "mdbg_spans_stitch", reads, spans, pieces, nullptr, piece_offsets, n_contigs, form, out);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_reads_stitch_ranges(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_seq_range *ranges, const uint64_t *piece_offsets, uint64_t n_contigs, int form,
                                        mdbg_sequences **out) try {
    if (!ctx || !reads || !piece_offsets || !out || (piece_offsets[n_contigs] && !ranges)) return set_error(ctx, MDBG_EINVAL, "mdbg_reads_stitch_ranges: null argument");
    return stitch_run(ctx, "mdbg_reads_stitch_ranges", reads, nullptr, nullptr, ranges, piece_offsets, n_contigs, form, out);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_sequences_to_fasta_bytes(mdbg_ctx *ctx, const mdbg_sequences *seqs, const uint32_t *names, const uint8_t *circular, mdbg_bytes **out,
                                             uint64_t *n_bytes) try {
    if (!ctx || !seqs || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_sequences_to_fasta_bytes: null argument");
    if (seqs->form != MDBG_SEQ_BITSET) return set_error(ctx, MDBG_EINVAL, "mdbg_sequences_to_fasta_bytes: the sequences are not in MDBG_SEQ_BITSET form");
    const uint64_t n = seqs->n;
    if (circular)
        for (uint64_t i = 0; i < n; i++)
            if (circular[i] > 2) return set_error(ctx, MDBG_EINVAL, "mdbg_sequences_to_fasta_bytes: the flag of sequence %llu is %u, none of 0 (l), 1 (c), 2 (rc)", (unsigned long long)i, circular[i]);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    DevBuf<uint32_t> d_names;
    DevBuf<uint8_t> d_flags;
    DevBuf<uint64_t> rbytes, roff;
    MDBG_TRY(rbytes.alloc(ctx, n));
    MDBG_TRY(roff.alloc(ctx, (size_t)n + 1));
    if (names && n) {
        MDBG_TRY(d_names.alloc(ctx, n));
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d_names.p, names, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (circular && n) {
        MDBG_TRY(d_flags.alloc(ctx, n));
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d_flags.p, circular, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    }
    {
        LaunchTimer timer(ctx, "fasta_plan");
        if (n) hipLaunchKernelGGL(fasta_plan_kernel, dim3(grid_for(n, 256, cap)), dim3(256), 0, ctx->stream, seqs->d_len.p, d_names.p, d_flags.p, n, rbytes.p);
        MDBG_TRY(exclusive_scan_u64(ctx, rbytes.p, roff.p, n));
    }
    uint64_t total = 0;
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &total, roff.p + n, 8, hipMemcpyDeviceToHost));
    std::unique_ptr<mdbg_bytes> b(new mdbg_bytes());
    b->n = total;
    b->owner = ctx;
    MDBG_TRY(b->d.alloc(ctx, total));
    if (!ctx->upload_stream) MDBG_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking));     // (as mdbg_bytes_create leaves a buffer)
    if (total) {
        LaunchTimer timer(ctx, "fasta_write");
        hipLaunchKernelGGL(fasta_write_kernel, dim3(grid_for(((total + 7u) / 8u + 1u) / 2u, 256, cap)), dim3(256), 0, ctx->stream, roff.p, (uint32_t)n, seqs->d_len.p,
                           d_names.p, d_flags.p, seqs->d_off.p, seqs->d_bytes.p, b->d.p, total);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));       // the plan's buffers go back to the pool; the text is complete
    if (n_bytes) *n_bytes = total;
    *out = b.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)
