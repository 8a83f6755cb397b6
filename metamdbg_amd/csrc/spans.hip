// spans.hip -- mdbg_kminmer_spans: MDBG::getKminmers for a whole batch (Commons.hpp:5401-5526).  Reads and their scan output go in;
// per window of k minimizers the identity of the normalised window and the ReadKminmer fields come out -- where the k-min-mer starts
// and ends in the ORIGINAL read, how many bases its first and last step cover, whether it was reversed -- which is what the callers
// that re-scan raw reads or contigs cut bases out with (ToBasespaceGfa::ExtractKminmerSequenceFunctor, toBasespace/ToBasespaceGfa.hpp:
// 1177-1237; MappingContigToGraph, mapping/MappingContigToGraph.hpp:187-217; GenerateGfa::LoadUnitigsFunctor).
//
// Two steps:
//   the coordinate map   rle[j], the original coordinate of compressed position j (EncoderRLE::execute, Commons.hpp:4163-4203), for the
//                        two positions a minimizer asks for: S = rle[p] and E = rle[p + l].  The run starts of every 2048-base tile are
//                        counted once, one wave a tile (a word's offset inside its tile is kept, two bytes a word); the tiles of a read
//                        are summed; a query then finds its tile (binary search), its word (three rounds of three reads) and the
//                        j-th flag of that word's flag word (spans_dev.hpp).  Nothing depends on a read's length.  Without
//                        homopolymer compression rle is the identity and no base is read.
//   the windows          one thread a window: orientation and identity by kminmer_dev.hpp's window_hash*, the fields by spans_compose.
// Everything the two steps index with is checked on the device first (lengths, strictly increasing positions, p + l <= L'): a set of
// minimizers that is not these reads' scan is refused before any select runs.
#include "common.hpp"
#include "kminmer_dev.hpp"
#include "objects.hpp"
#include "spans_dev.hpp"

#include <memory>

namespace mdbg {

// what the checks found: (read << 8) | reason, the smallest wins; SPANS_FINE = nothing
constexpr unsigned long long SPANS_FINE = ~0ull;
constexpr uint32_t SPANS_BAD_LENGTH = 1, SPANS_BAD_ORDER = 2, SPANS_BAD_END = 3;

// per read: the tiles of its map, its windows, and the first check -- the scan recorded the length the reads have
__global__ __launch_bounds__(256) void spans_plan_kernel(const uint32_t *read_len, const uint32_t *scan_len, const uint64_t *off, uint32_t n_reads, uint32_t k,
                                                         int hpc, uint32_t *tiles, uint32_t *windows, unsigned long long *status) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * 256u) {
        const uint32_t L = read_len[r];
        if (scan_len[r] != L) atomicMin(status, ((unsigned long long)r << 8) | SPANS_BAD_LENGTH);
        tiles[r] = hpc ? (uint32_t)(((uint64_t)L + SPANS_TILE_BASES - 1u) / SPANS_TILE_BASES) : 0u;
        const uint64_t n = off[r + 1] - off[r];
        windows[r] = n >= k ? (uint32_t)(n - k + 1u) : 0u;
    }
}

// The run starts of every tile, one wave a tile: tile_runs[g] and, per word, the run starts of the tile in front of it (word_excl).
__global__ __launch_bounds__(256) void spans_tile_runs_kernel(const uint64_t *words, const uint64_t *word_off, const uint32_t *inv, const uint32_t *brk,
                                                              const uint32_t *len, uint32_t n_reads, const uint64_t *tile_off /* n_reads + 1 */,
                                                              uint32_t *tile_runs, uint16_t *word_excl) {
    const unsigned lane = threadIdx.x & 63u;
    const WaveSpan sp = wave_span(tile_off[n_reads], 1u);
    if (sp.begin >= sp.end) return;
    uint32_t r = csr_owner(tile_off, n_reads, sp.begin);
    for (uint64_t g = sp.begin; g < sp.end; g++) {
        r = csr_owner_from(tile_off, n_reads, g, r);
        const uint32_t L = len[r], t = (uint32_t)(g - tile_off[r]);
        const uint64_t w0 = word_off[r];
        const uint32_t nwords = (uint32_t)(((uint64_t)L + 31u) / 32u), wi = t * SPANS_TILE_WORDS + lane;
        uint32_t c = 0;
        if (wi < nwords) c = spans_count_flags(spans_read_word_flags(words + w0, inv ? inv + w0 : nullptr, brk ? brk + w0 : nullptr, L, wi));
        const uint32_t inc = wave_inclusive_sum_dpp(c);
        word_excl[g * SPANS_TILE_WORDS + lane] = (uint16_t)(inc - c);
        if (lane == 63u) tile_runs[g] = inc;
    }
}

// ... summed inside every read, one wave a read: tile_excl[g] = run starts of the read in front of tile g, comp_len[r] = L'.
__global__ __launch_bounds__(256) void spans_read_sums_kernel(uint32_t n_reads, const uint64_t *tile_off, const uint32_t *tile_runs, uint32_t *tile_excl,
                                                              uint32_t *comp_len) {
    const unsigned lane = threadIdx.x & 63u;
    for (uint64_t r = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; r < n_reads; r += ((uint64_t)gridDim.x * 256u) >> 6) {
        const uint64_t g0 = tile_off[r];
        const uint32_t nT = (uint32_t)(tile_off[r + 1] - g0);
        uint32_t carry = 0;
        for (uint32_t t0 = 0; t0 < nT; t0 += 64u) {
            const uint32_t t = t0 + lane, c = t < nT ? tile_runs[g0 + t] : 0u;
            const uint32_t inc = wave_inclusive_sum_dpp(c);
            if (t < nT) tile_excl[g0 + t] = carry + inc - c;
            carry += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        }
        if (lane == 0u) comp_len[r] = carry;
    }
}

// The checks, one lane a minimizer: positions strictly increasing inside a read, p + l inside the (compressed) read.
__global__ __launch_bounds__(256) void spans_check_kernel(const uint64_t *off, const uint32_t *pos, uint32_t n_reads, uint64_t n_min, uint32_t l,
                                                          const uint32_t *bound /* per read: L' (compression) or L */, unsigned long long *status) {
    const WaveSpan sp = wave_span(n_min, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t r0 = csr_owner(off, n_reads, sp.begin);
    for (uint64_t i = sp.begin + (threadIdx.x & 63u); i < sp.end; i += 64u) {
        const uint32_t r = csr_owner_from(off, n_reads, i, r0);
        r0 = r;
        const uint32_t p = pos[i];
        uint32_t why = 0;
        if ((uint64_t)p + l > bound[r]) why = SPANS_BAD_END;
        if (i > off[r] && pos[i - 1] >= p) why = SPANS_BAD_ORDER;
        if (why) atomicMin(status, ((unsigned long long)r << 8) | why);
    }
}

struct MapView {
    const uint64_t *words, *word_off;       // the reads
    const uint32_t *inv, *brk, *len;
    const uint64_t *tile_off;               // the map
    const uint32_t *tile_excl, *comp_len;
    const uint16_t *word_excl;
};

// one read's part of the map
__device__ __forceinline__ SpansReadMap spans_read_map(const MapView &v, uint32_t r) {
    const uint64_t w0 = v.word_off[r], g0 = v.tile_off[r];
    return SpansReadMap{v.words + w0, v.inv ? v.inv + w0 : nullptr, v.brk ? v.brk + w0 : nullptr, v.len[r], v.comp_len[r],
                        (uint32_t)(v.tile_off[r + 1] - g0), v.tile_excl + g0, v.word_excl + g0 * SPANS_TILE_WORDS};
}

// The map proper, one lane a minimizer: S = rle[p], E = rle[p + l].
__global__ __launch_bounds__(256) void spans_select_kernel(MapView v, const uint64_t *off, const uint32_t *pos, uint32_t n_reads, uint64_t n_min, uint32_t l,
                                                           int hpc, uint32_t *out_s, uint32_t *out_e) {
    const WaveSpan sp = wave_span(n_min, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t r0 = hpc ? csr_owner(off, n_reads, sp.begin) : 0u;
    for (uint64_t i = sp.begin + (threadIdx.x & 63u); i < sp.end; i += 64u) {
        const uint32_t p = pos[i];
        uint32_t s = p, e = p + l;
        if (hpc) {
            r0 = csr_owner_from(off, n_reads, i, r0);
            const SpansReadMap m = spans_read_map(v, r0);
            s = spans_rle(m, p);
            e = spans_rle(m, p + l);
        }
        out_s[i] = s;
        out_e[i] = e;
    }
}

// The windows, one lane a window.
__global__ __launch_bounds__(256) void spans_windows_kernel(const uint64_t *off, const uint64_t *woff, const uint32_t *mins, const uint32_t *s, const uint32_t *e,
                                                            uint32_t n_reads, uint64_t n_windows, uint32_t k, uint64_t *out_lo, uint64_t *out_hi, uint8_t *out_rev,
                                                            uint32_t *out_ps, uint32_t *out_pe, uint32_t *out_ls, uint32_t *out_le) {
    const WaveSpan sp = wave_span(n_windows, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t r = csr_owner(woff, n_reads, sp.begin);
    for (uint64_t g = sp.begin + (threadIdx.x & 63u); g < sp.end; g += 64u) {
        r = csr_owner_from(woff, n_reads, g, r);
        const uint64_t a = off[r] + (g - woff[r]);                  // the window's first minimizer
        uint64_t hi, lo;
        const bool reversed = window_hash_uniform(mins + a, k, hi, lo);
        const SpanFields f = spans_compose(s[a], s[a + 1], e[a + k - 2u], e[a + k - 1u], reversed);
        out_lo[g] = lo;
        out_hi[g] = hi;
        out_rev[g] = reversed ? 1 : 0;
        out_ps[g] = f.pos_start;
        out_pe[g] = f.pos_end;
        out_ls[g] = f.seq_length_start;
        out_le[g] = f.seq_length_end;
    }
}

}  // namespace mdbg

using namespace mdbg;

extern "C" int mdbg_kminmer_spans(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_minimizers *mins, uint32_t minimizer_size, int32_t hpc, uint32_t k,
                                  mdbg_spans **out) try {
    if (!ctx || !reads || !mins || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_kminmer_spans: null argument");
    if (k < 2) return set_error(ctx, MDBG_EINVAL, "mdbg_kminmer_spans: k must be at least 2 (a window's second minimizer is read)");
    if (minimizer_size < 1 || minimizer_size > 16) return set_error(ctx, MDBG_EINVAL, "mdbg_kminmer_spans: minimizer_size %u is outside 1 .. 16", minimizer_size);
    if (!mins->from_scan || !mins->d_pos.p || !mins->d_len.p)
        return set_error(ctx, MDBG_EINVAL, "mdbg_kminmer_spans: the minimizers carry no positions and read lengths (not an mdbg_scan output or a set made of such)");
    if (mins->n_reads != reads->n_reads)
        return set_error(ctx, MDBG_EINVAL, "mdbg_kminmer_spans: %u reads but minimizers of %u", reads->n_reads, mins->n_reads);
    if (mins->n_min >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_kminmer_spans: more than 2^32 minimizers in one batch");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_TRY(ensure_canonical(ctx, mins));            // a fresh scan output: into read order first
    MDBG_HIP_CHECK(ctx, reads_ready_on(ctx, reads));  // behind an asynchronous upload, on the device

    const uint32_t n = reads->n_reads, l = minimizer_size;
    const uint64_t n_min = mins->n_min;
    const bool comp = hpc != 0;
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    std::unique_ptr<mdbg_spans> sp(new mdbg_spans());
    sp->n_reads = n; sp->k = k; sp->n_min = n_min;
    MDBG_TRY(sp->d_woff.alloc(ctx, (size_t)n + 1));
    MDBG_TRY(sp->d_len.alloc(ctx, n));
    if (n) MDBG_HIP_CHECK(ctx, hipMemcpyAsync(sp->d_len.p, reads->d_len.p, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));

    // ---- the map's counts and the checks --------------------------------------------------------------------------------------
    const uint64_t tiles_bound = comp ? reads->n_words / SPANS_TILE_WORDS + n + 1u : 1u;     // sum of ceil(words / 64) over the reads
    DevBuf<uint32_t> tiles, wcnt, tile_runs, tile_excl, comp_len;
    DevBuf<uint64_t> tile_off;
    DevBuf<uint16_t> word_excl;
    DevBuf<unsigned long long> status;                // [0] the checks' verdict, [1] the windows in all
    MDBG_TRY(tiles.alloc(ctx, n));
    MDBG_TRY(wcnt.alloc(ctx, n));
    MDBG_TRY(tile_off.alloc(ctx, (size_t)n + 1));
    MDBG_TRY(status.alloc(ctx, 2));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(status.p, 0xFF, 8, ctx->stream));
    if (comp) {
        MDBG_TRY(tile_runs.alloc(ctx, tiles_bound));
        MDBG_TRY(tile_excl.alloc(ctx, tiles_bound));
        MDBG_TRY(word_excl.alloc(ctx, tiles_bound * SPANS_TILE_WORDS));
        MDBG_TRY(comp_len.alloc(ctx, n));
    }
    if (n)
        hipLaunchKernelGGL(spans_plan_kernel, dim3(grid_for(n, 256, cap)), dim3(256), 0, ctx->stream, reads->d_len.p, mins->d_len.p, mins->d_off.p, n, k,
                           comp ? 1 : 0, tiles.p, wcnt.p, status.p);
    MDBG_TRY(exclusive_scan_u32(ctx, wcnt.p, sp->d_woff.p, n));
    const uint32_t *inv = reads->has_invalid ? reads->d_invalid.p : nullptr, *brk = reads->has_break ? reads->d_break.p : nullptr;
    if (comp && n) {
        MDBG_TRY(exclusive_scan_u32(ctx, tiles.p, tile_off.p, n));
        LaunchTimer timer(ctx, "spans_map");
        hipLaunchKernelGGL(spans_tile_runs_kernel, dim3(grid_for(tiles_bound * 64u, 256, cap)), dim3(256), 0, ctx->stream, reads->d_words.p, reads->d_word_off.p,
                           inv, brk, reads->d_len.p, n, tile_off.p, tile_runs.p, word_excl.p);
        hipLaunchKernelGGL(spans_read_sums_kernel, dim3(grid_for((uint64_t)n * 64u, 256, cap)), dim3(256), 0, ctx->stream, n, tile_off.p, tile_runs.p,
                           tile_excl.p, comp_len.p);
    }
    if (n_min)
        hipLaunchKernelGGL(spans_check_kernel, dim3(grid_for(n_min, 256, cap)), dim3(256), 0, ctx->stream, mins->d_off.p, mins->d_pos.p, n, n_min, l,
                           comp ? comp_len.p : reads->d_len.p, status.p);
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(status.p + 1, sp->d_woff.p + n, 8, hipMemcpyDeviceToDevice, ctx->stream));
    unsigned long long verdict[2] = {0, 0};
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, verdict, status.p, 16, hipMemcpyDeviceToHost));
    if (verdict[0] != SPANS_FINE) {
        const unsigned long long r = verdict[0] >> 8;
        switch ((uint32_t)(verdict[0] & 0xFFu)) {
            case SPANS_BAD_LENGTH:
                return set_error(ctx, MDBG_EINVAL, "mdbg_kminmer_spans: read %llu: the minimizers record another length than the read has (not these reads' scan)", r);
            case SPANS_BAD_ORDER:
                return set_error(ctx, MDBG_EINVAL, "mdbg_kminmer_spans: read %llu: its positions are not strictly increasing", r);
            default:
                return set_error(ctx, MDBG_EINVAL, "mdbg_kminmer_spans: read %llu: a position + minimizer_size %u lies behind the %sread's end (not these reads' scan, "
                                 "or not its minimizer_size / hpc)", r, l, comp ? "compressed " : "");
        }
    }
    const uint64_t n_win = verdict[1];
    sp->n_windows = n_win;

    // ---- the map proper, then the windows ----------------------------------------------------------------------------------------
    MDBG_TRY(sp->d_s.alloc(ctx, n_min));
    MDBG_TRY(sp->d_e.alloc(ctx, n_min));
    MDBG_TRY(sp->d_lo.alloc(ctx, n_win));
    MDBG_TRY(sp->d_hi.alloc(ctx, n_win));
    MDBG_TRY(sp->d_rev.alloc(ctx, n_win));
    MDBG_TRY(sp->d_ps.alloc(ctx, n_win));
    MDBG_TRY(sp->d_pe.alloc(ctx, n_win));
    MDBG_TRY(sp->d_ls.alloc(ctx, n_win));
    MDBG_TRY(sp->d_le.alloc(ctx, n_win));
    if (n_min) {
        LaunchTimer timer(ctx, "spans_map");
        const MapView v{reads->d_words.p, reads->d_word_off.p, inv, brk, reads->d_len.p, tile_off.p, tile_excl.p, comp_len.p, word_excl.p};
        hipLaunchKernelGGL(spans_select_kernel, dim3(grid_for(n_min, 256, cap)), dim3(256), 0, ctx->stream, v, mins->d_off.p, mins->d_pos.p, n, n_min, l,
                           comp ? 1 : 0, sp->d_s.p, sp->d_e.p);
    }
    if (n_win) {
        LaunchTimer timer(ctx, "spans_windows");
        hipLaunchKernelGGL(spans_windows_kernel, dim3(grid_for(n_win, 256, cap)), dim3(256), 0, ctx->stream, mins->d_off.p, sp->d_woff.p, mins->d_min.p, sp->d_s.p,
                           sp->d_e.p, n, n_win, k, sp->d_lo.p, sp->d_hi.p, sp->d_rev.p, sp->d_ps.p, sp->d_pe.p, sp->d_ls.p, sp->d_le.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    // the map's working buffers go back to the context's pool, which hands them to later work on the same stream only; the inputs
    // must outlive the kernels: the stream is drained before the caller may free them
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = sp.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_spans_info(const mdbg_spans *s, uint32_t *n_reads, uint64_t *n_minimizers, uint64_t *n_windows, uint32_t *k) {
    if (!s) return MDBG_EINVAL;
    if (n_reads) *n_reads = s->n_reads;
    if (n_minimizers) *n_minimizers = s->n_min;
    if (n_windows) *n_windows = s->n_windows;
    if (k) *k = s->k;
    return MDBG_OK;
}

extern "C" int mdbg_spans_to_host(mdbg_ctx *ctx, const mdbg_spans *s, uint64_t *window_offsets, uint32_t *min_start, uint32_t *min_end, uint64_t *hash_lo,
                                  uint64_t *hash_hi, uint8_t *reversed, uint32_t *pos_start, uint32_t *pos_end, uint32_t *seq_length_start,
                                  uint32_t *seq_length_end) try {
    if (!ctx || !s) return set_error(ctx, MDBG_EINVAL, "mdbg_spans_to_host: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t n = s->n_reads, m = s->n_min, w = s->n_windows;
    MDBG_HIP_CHECK(ctx, download_async(ctx, window_offsets, s->d_woff.p, (n + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, min_start, s->d_s.p, m * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, min_end, s->d_e.p, m * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, hash_lo, s->d_lo.p, w * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, hash_hi, s->d_hi.p, w * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, reversed, s->d_rev.p, w));
    MDBG_HIP_CHECK(ctx, download_async(ctx, pos_start, s->d_ps.p, w * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, pos_end, s->d_pe.p, w * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, seq_length_start, s->d_ls.p, w * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, seq_length_end, s->d_le.p, w * 4));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_spans_device_ptrs(const mdbg_spans *s, const uint64_t **d_window_offsets, const uint64_t **d_hash_lo, const uint64_t **d_hash_hi,
                                      const uint32_t **d_pos_start, const uint32_t **d_pos_end) {
    if (!s) return MDBG_EINVAL;
    if (d_window_offsets) *d_window_offsets = s->d_woff.p;
    if (d_hash_lo) *d_hash_lo = s->d_lo.p;
    if (d_hash_hi) *d_hash_hi = s->d_hi.p;
    if (d_pos_start) *d_pos_start = s->d_ps.p;
    if (d_pos_end) *d_pos_end = s->d_pe.p;
    return MDBG_OK;
}

extern "C" void mdbg_spans_free(mdbg_spans *s) { delete s; }
