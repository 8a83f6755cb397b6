// extract.hip -- mdbg_spans_extract / mdbg_reads_extract_ranges: the oriented sequences of k-min-mers (or of any ranges) cut out of the
// packed reads on the device and packed as the reference keeps them -- ToBasespaceGfa::extractKminmerSequence (toBasespace/
// ToBasespaceGfa.hpp:1050-1103: memcpy, Utils::revcomp of a reversed window, substr for the left / right overhang) and DnaBitset2
// (utils/DnaBitset.hpp:118-242), the loop body of ExtractKminmerSequenceFunctor (:1177-1237) and LoadUnitigsFunctor's
// DnaBitset2(read._seq) (graph/GenerateGfa.hpp:418).
//
// Two steps:
//   the plan    one lane a request: its range (read, start, length, reversed) by extract_part_range, every check, the 64-bit words its
//               sequence takes, and a 16-byte record for the copy (where the read's words begin, the range); exclusive_scan_u32 over the
//               words gives the offsets.  One status word travels back before a base is read.
//   the copy    the OUTPUT WORDS of the whole batch are dealt to the waves in contiguous spans (wave_span), one lane an aligned pair of
//               words: each word is composed from at most two source words (extract_dev.hpp) and the pair is stored as 16 bytes --
//               padding included, so no byte is written twice and none is left unwritten.  A lane keeps the request it is inside of in
//               registers and loads nothing but source words while it stays there (a contig); when it leaves, it finds the next owner
//               by doubling steps from the old one (extract_next_owner).  A contig of 5 Mb and 100 000 ranges of 50 bases cost what their
//               bytes cost (profiles/kminmer_sequences.txt, which also has the first form: a search and three dependent loads per
//               word, 8-byte stores, two to three times slower).
// No LDS, no scratch; every buffer comes from the context's pool.  The result handle and a plan lane's range and checks are in
// extract_plan.hpp: stitch.hip, which puts contigs together from such ranges, shares them.
#include "extract_plan.hpp"

#include <memory>

namespace mdbg {

static_assert(sizeof(mdbg_seq_request) == 16 && sizeof(mdbg_seq_range) == 16 && sizeof(ExtractRange) == 16, "16 bytes a request");

// What the copy reads of a request, one 16-byte load: where its read's words begin (a word index below 2^63; bit 63 = reversed), and
// the range.
struct alignas(16) ExtractRec { uint64_t w0_rev; uint32_t start, length; };
constexpr uint64_t EXTRACT_REC_REVERSED = 1ull << 63;

// what a lane of the plan leaves behind: the record, the length and the words of the sequence; a refused request takes no room
__device__ __forceinline__ uint32_t plan_emit(uint64_t i, uint32_t why, ExtractRange rg, uint32_t form, const uint64_t *word_off, ExtractRec *recs,
                                              uint32_t *lengths, uint32_t *words, unsigned long long *status) {
    if (why) {
        atomicMin(status, ((unsigned long long)i << 8) | why);
        recs[i] = ExtractRec{0ull, 0u, 0u};
        lengths[i] = 0u;
        words[i] = 0u;
        return 0u;
    }
    recs[i] = ExtractRec{word_off[rg.read] | (rg.reversed ? EXTRACT_REC_REVERSED : 0ull), rg.start, rg.length};
    lengths[i] = rg.length;
    words[i] = extract_words(rg.length, form);
    return rg.length;
}

// (window, part) requests: the window's read by a search over the window offsets, the range by extract_part_range
__global__ __launch_bounds__(256) void extract_plan_kernel(const mdbg_seq_request *req, uint64_t n, uint32_t form, const uint32_t *read_len, uint32_t n_reads,
                                                           SpansView sp, const uint64_t *word_off, ExtractRec *recs, uint32_t *lengths, uint32_t *words,
                                                           unsigned long long *status) {
    unsigned long long bases = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const mdbg_seq_request q = req[i];
        ExtractRange rg{0u, 0u, 0u, 0u};
        uint32_t why = 0;
        if (q.part > EXTRACT_RIGHT) why = EXTRACT_BAD_PART;
        else if (q.reserved != 0u) why = EXTRACT_BAD_RESERVED;
        else why = extract_request_range(q.window, q.part, sp, read_len, n_reads, rg);
        bases += plan_emit(i, why, rg, form, word_off, recs, lengths, words, status);
    }
    plan_add_bases(bases, status + 2);
}

// ranges given by the caller
__global__ __launch_bounds__(256) void extract_plan_ranges_kernel(const mdbg_seq_range *in, uint64_t n, uint32_t form, const uint32_t *read_len, uint32_t n_reads,
                                                                  const uint64_t *word_off, ExtractRec *recs, uint32_t *lengths, uint32_t *words,
                                                                  unsigned long long *status) {
    unsigned long long bases = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const mdbg_seq_range q = in[i];
        const ExtractRange rg{q.read, q.start, q.length, q.reversed ? 1u : 0u};
        const uint32_t why = extract_given_range(q.read, q.start, q.length, read_len, n_reads);
        bases += plan_emit(i, why, rg, form, word_off, recs, lengths, words, status);
    }
    plan_add_bases(bases, status + 2);
}

// word offsets -> byte offsets, in place (n + 1 entries)
__global__ __launch_bounds__(256) void extract_offsets_kernel(uint64_t *off, uint64_t n1) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n1; i += (uint64_t)gridDim.x * 256u) off[i] *= 8u;
}
void extract_offsets_to_bytes(mdbg_ctx *ctx, uint64_t *d_off, uint64_t n1) {
    hipLaunchKernelGGL(extract_offsets_kernel, dim3(grid_for(n1, 256, (unsigned)ctx->n_cu * 32u)), dim3(256), 0, ctx->stream, d_off, n1);
}

// The request a lane is inside of: its index, its bytes [lo, hi) of the output, its record.
struct ExtractOwner { uint32_t r; uint64_t lo, hi; ExtractRec rec; };

__device__ __forceinline__ void owner_load(ExtractOwner &o, uint32_t r, const uint64_t *off, const ExtractRec *recs) {
    o.r = r;
    o.lo = off[r];
    o.hi = off[r + 1u];
    o.rec = recs[r];
}

// ... moved on to the request that owns byte `at` (off[o.r] <= at < off[n]): nothing is loaded while the lane stays inside its request
// -- a contig's words.
__device__ __forceinline__ void owner_advance(ExtractOwner &o, uint64_t at, const uint64_t *off, uint32_t n, const ExtractRec *recs) {
    if (at >= o.hi) owner_load(o, extract_next_owner(off, n, o.r, at), off, recs);
}

__device__ __forceinline__ uint64_t owner_word(const ExtractOwner &o, uint64_t g, const uint64_t *words, const uint32_t *inv, uint32_t form) {
    const uint64_t w0 = o.rec.w0_rev & ~EXTRACT_REC_REVERSED;
    return extract_word(words + w0, inv ? inv + w0 : nullptr, o.rec.start, o.rec.length, (o.rec.w0_rev & EXTRACT_REC_REVERSED) != 0ull,
                        (uint32_t)(g - o.lo / 8u), form);
}

// The copy, one lane an aligned PAIR of output words, stored as 16 bytes (8-byte stores run at 0.54 - 0.70 of the 16-byte rate).  off: byte
// offsets (multiples of 8), so word g belongs to the request that owns byte 8 g; the two words of a pair may belong to two requests.
__global__ __launch_bounds__(256) void extract_copy_kernel(const uint64_t *words, const uint32_t *inv, const ExtractRec *recs, const uint64_t *off, uint32_t n,
                                                           uint64_t n_words, uint32_t form, uint64_t *out) {
    const WaveSpan sp = wave_span((n_words + 1u) / 2u, 64u);
    if (sp.begin >= sp.end) return;
    ExtractOwner o;
    owner_load(o, csr_owner(off, n, sp.begin * 16u), off, recs);
    for (uint64_t p = sp.begin + (threadIdx.x & 63u); p < sp.end; p += 64u) {
        const uint64_t g = 2u * p;
        owner_advance(o, g * 8u, off, n, recs);
        const uint64_t a = owner_word(o, g, words, inv, form);
        if (g + 1u < n_words) {
            owner_advance(o, g * 8u + 8u, off, n, recs);
            const uint64_t b = owner_word(o, g + 1u, words, inv, form);
            *reinterpret_cast<ulonglong2 *>(out + g) = make_ulonglong2(a, b);
        } else {
            out[g] = a;
        }
    }
}

const StepKernel *extract_step_kernels(uint32_t *n) {
    static const StepKernel k[] = {
        {"extract_plan", reinterpret_cast<const void *>(extract_plan_kernel), 256, 2},
        {"extract_plan_ranges", reinterpret_cast<const void *>(extract_plan_ranges_kernel), 256, 2},
        {"extract_copy", reinterpret_cast<const void *>(extract_copy_kernel), 256, 2},
    };
    *n = (uint32_t)(sizeof(k) / sizeof(k[0]));
    return k;
}

const char *extract_why_text(uint32_t why) {
    switch (why) {
        case EXTRACT_BAD_PART: return "its part is none of MDBG_SEQ_ENTIRE / LEFT / RIGHT";
        case EXTRACT_BAD_RESERVED: return "its reserved field is not 0";
        case EXTRACT_BAD_WINDOW: return "its window index is not below the spans' number of windows";
        case EXTRACT_BAD_READ: return "its read index is not below the number of reads";
        case EXTRACT_BAD_READ_LENGTH: return "the spans record another length than its read has (not these reads' spans)";
        case EXTRACT_BAD_OVERHANG: return "seq_length_start or seq_length_end is larger than the window (not these reads' spans)";
        default: return "its range ends behind its read's last base";
    }
}

// Both entry points behind their argument checks: exactly one of req / in is set.
static int extract_run(mdbg_ctx *ctx, const char *who, const mdbg_reads *reads, const mdbg_spans *spans, const mdbg_seq_request *req, const mdbg_seq_range *in,
                       uint64_t n, int form, mdbg_sequences **out) {
    if (form != MDBG_SEQ_BITSET && form != MDBG_SEQ_ASCII) return set_error(ctx, MDBG_EINVAL, "%s: form %d is neither MDBG_SEQ_BITSET nor MDBG_SEQ_ASCII", who, form);
    if (n >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "%s: 2^32 requests or more in one call", who);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_HIP_CHECK(ctx, reads_ready_on(ctx, reads));  // behind an asynchronous upload, on the device
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    std::unique_ptr<mdbg_sequences> sq(new mdbg_sequences());
    sq->n = n; sq->form = form;
    MDBG_TRY(sq->d_off.alloc(ctx, (size_t)n + 1));
    MDBG_TRY(sq->d_len.alloc(ctx, n));

    // ---- the plan: ranges, checks, offsets ---------------------------------------------------------------------------------------------
    DevBuf<uint8_t> d_in;                             // the requests as given, 16 bytes each
    DevBuf<ExtractRec> recs;
    DevBuf<uint32_t> words;
    DevBuf<unsigned long long> status;                // [0] the checks' verdict, [1] the bytes in all, [2] the bases in all
    MDBG_TRY(d_in.alloc(ctx, (size_t)n * 16));
    MDBG_TRY(recs.alloc(ctx, n));
    MDBG_TRY(words.alloc(ctx, n));
    MDBG_TRY(status.alloc(ctx, 3));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(status.p, 0xFF, 8, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(status.p + 2, 0, 8, ctx->stream));
    if (n) MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d_in.p, req ? (const void *)req : (const void *)in, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
    {
        LaunchTimer timer(ctx, "extract_plan");
        if (n && req)
            hipLaunchKernelGGL(extract_plan_kernel, dim3(grid_for(n, 256, cap)), dim3(256), 0, ctx->stream, reinterpret_cast<const mdbg_seq_request *>(d_in.p), n,
                               (uint32_t)form, reads->d_len.p, reads->n_reads, spans_view(spans), reads->d_word_off.p, recs.p, sq->d_len.p, words.p, status.p);
        else if (n)
            hipLaunchKernelGGL(extract_plan_ranges_kernel, dim3(grid_for(n, 256, cap)), dim3(256), 0, ctx->stream, reinterpret_cast<const mdbg_seq_range *>(d_in.p), n,
                               (uint32_t)form, reads->d_len.p, reads->n_reads, reads->d_word_off.p, recs.p, sq->d_len.p, words.p, status.p);
        MDBG_TRY(exclusive_scan_u32(ctx, words.p, sq->d_off.p, n));
        extract_offsets_to_bytes(ctx, sq->d_off.p, n + 1);
    }
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(status.p + 1, sq->d_off.p + n, 8, hipMemcpyDeviceToDevice, ctx->stream));
    unsigned long long verdict[3] = {0, 0, 0};
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, verdict, status.p, 24, hipMemcpyDeviceToHost));
    if (verdict[0] != EXTRACT_FINE)
        return set_error(ctx, MDBG_EINVAL, "%s: request %llu: %s", who, verdict[0] >> 8, extract_why_text((uint32_t)(verdict[0] & 0xFFu)));
    sq->n_bytes = verdict[1];
    sq->n_bases = verdict[2];

    // ---- the copy ----------------------------------------------------------------------------------------------------------------------
    MDBG_TRY(sq->d_bytes.alloc(ctx, sq->n_bytes));
    const uint64_t n_words = sq->n_bytes / 8u;
    if (n_words) {
        LaunchTimer timer(ctx, "extract_copy");
        hipLaunchKernelGGL(extract_copy_kernel, dim3(grid_for((n_words + 1u) / 2u, 256, cap)), dim3(256), 0, ctx->stream, reads->d_words.p,
                           reads->has_invalid ? reads->d_invalid.p : nullptr, recs.p, sq->d_off.p, (uint32_t)n, n_words, (uint32_t)form,
                           reinterpret_cast<uint64_t *>(sq->d_bytes.p));
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    // the plan's buffers go back to the pool, which hands them to later work on the same stream only; the inputs must outlive the kernels
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = sq.release();
    return MDBG_OK;
}

}  // namespace mdbg

using namespace mdbg;

extern "C" int mdbg_spans_extract(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_spans *spans, const mdbg_seq_request *requests, uint64_t n, int form,
                                  mdbg_sequences **out) try {
    if (!ctx || !reads || !spans || !out || (n && !requests)) return set_error(ctx, MDBG_EINVAL, "mdbg_spans_extract: null argument");
    if (spans->n_reads != reads->n_reads)
        return set_error(ctx, MDBG_EINVAL, "mdbg_spans_extract: %u reads but spans of %u (not these reads' spans)", reads->n_reads, spans->n_reads);
    return extract_run(ctx, "mdbg_spans_extract", reads, spans, requests, nullptr, n, form, out);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_reads_extract_ranges(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_seq_range *ranges, uint64_t n, int form, mdbg_sequences **out) try {
    if (!ctx || !reads || !out || (n && !ranges)) return set_error(ctx, MDBG_EINVAL, "mdbg_reads_extract_ranges: null argument");
    return extract_run(ctx, "mdbg_reads_extract_ranges", reads, nullptr, nullptr, ranges, n, form, out);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_sequences_info(const mdbg_sequences *s, uint64_t *n, uint64_t *n_bases, uint64_t *n_bytes, int *form) {
    if (!s) return MDBG_EINVAL;
    if (n) *n = s->n;
    if (n_bases) *n_bases = s->n_bases;
    if (n_bytes) *n_bytes = s->n_bytes;
    if (form) *form = s->form;
    return MDBG_OK;
}

extern "C" int mdbg_sequences_to_host(mdbg_ctx *ctx, const mdbg_sequences *s, uint64_t *byte_offsets, uint32_t *lengths, uint8_t *bytes) try {
    if (!ctx || !s) return set_error(ctx, MDBG_EINVAL, "mdbg_sequences_to_host: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_HIP_CHECK(ctx, download_async(ctx, byte_offsets, s->d_off.p, (s->n + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, lengths, s->d_len.p, s->n * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, bytes, s->d_bytes.p, s->n_bytes));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_sequences_device_ptrs(const mdbg_sequences *s, const uint64_t **d_byte_offsets, const uint32_t **d_lengths, const uint8_t **d_bytes) {
    if (!s) return MDBG_EINVAL;
    if (d_byte_offsets) *d_byte_offsets = s->d_off.p;
    if (d_lengths) *d_lengths = s->d_len.p;
    if (d_bytes) *d_bytes = s->d_bytes.p;
    return MDBG_OK;
}

extern "C" void mdbg_sequences_free(mdbg_sequences *s) { delete s; }
