// gzip.hip -- an ordinary gzip file (gzip, pigz, zlib: one deflate stream per member, no index) inflated on the device
// (mdbg_bytes_inflate_gzip), and a device copy between two byte buffers (mdbg_bytes_copy).  Replaces gzread under the kseq loop
// (KSEQ_INIT(gzFile, gzread), Commons.hpp:82; the read loop, Commons.hpp:5842-5870) for the files inflate.hip does not take: gzip that
// is not BGZF.  The scheme is the two-pass one of host/gzip_parallel.hpp; finding the chunk starts stays with the caller.
//
//   gzip_decode_kernel     one wave per chunk, grid-stride.  Lane 0 runs the serial core (deflate_core.hpp, gz_step) over arrays in LDS
//                          and leaves up to 64 tokens; the wave resolves them into 16-bit SYMBOLS in global memory: a byte, or
//                          GZ_MARK + p for byte p of the unknown 32 KB in front of the chunk (that prologue is computed, not stored: a
//                          match source at symbol index s < 0 is the marker GZ_MARK + 32768 + s).  Member trailers inside a chunk are
//                          noted in the chunk's border list.  A chunk that needs more than 8 symbols per compressed byte reports
//                          GZ_E_OVERFLOW and is decoded once more at the format's maximum (one second launch over those chunks).
//   gzip_windows_kernel    one workgroup, the chunks in order: the last min(n, 32768) symbols of each chunk go to their place in the
//                          text; a marker reads the text this kernel wrote for the chunks before, or the stream's carried 32 KB.
//   gzip_translate_kernel  every other symbol to its byte, in parallel: 16-byte loads of symbols, 8-byte stores of text where the
//                          text address allows; markers read the windows.
//   gzip_crc_kernel        CRC-32 of the text by pieces of 16 KB that never straddle a member border: a wave a piece, its register
//                          multiplied by x^(8 * bytes behind the piece in its member) and XORed into the member's word.
//   gzip_carry_kernel      the last 32 KB of text into the stream's other window buffer (the buffers swap when the call succeeds).
//
//   LDS per wave of the decode kernel: the BGZF kernel's arrays (4576 bytes) and 112 bytes of state.
#include "common.hpp"
#include "objects.hpp"
#include "deflate_core.hpp"

#include <algorithm>
#include <vector>

struct mdbg_gzip_stream {
    mdbg_ctx *owner = nullptr;
    mdbg::DevBuf<uint8_t> carry[2];   // the last 32 KB of text, oldest byte first; carry[cur] is valid
    int cur = 0;
    bool member_open = false;         // the last call ended inside a member
    bool finished = false;            // the file's last member has ended
    uint32_t reg = 0xFFFFFFFFu;       // the open member's CRC register
    uint64_t member_len = 0;          // and the bytes of it produced so far
};

namespace mdbg {

int bytes_ready_on(mdbg_ctx *ctx, const mdbg_bytes *b);      // minimizers.hip

constexpr int GZ_THREADS = 256, GZ_WAVES = GZ_THREADS / 64;
constexpr uint32_t GZ_PIECE = 16384;                          // bytes of a CRC piece
constexpr int GZ_WIN_THREADS = 1024;

struct GzChunk {              // a chunk as the decode kernel sees it (checked by the host: the payload lies inside comp, the areas inside their buffers)
    uint64_t src;             // the byte of comp its first bit lies in
    uint64_t stop;            // bits from that byte on, or GZ_TO_END
    uint64_t sym, border;     // where its symbols and its borders start in their buffers
    uint32_t start_bit, csize, cap, border_cap, reach0, at_header, pad0, pad1;
};
struct GzResult { uint64_t end_bit; uint32_t n_sym, status, n_borders, ended; };
struct GzBorder { uint32_t at, crc, isize, pad; };
struct GzPlace {              // a decoded chunk as the text kernels see it
    const uint16_t *sym;
    uint64_t t0;              // its first byte's offset in the call's text
    int64_t mstart;           // offset of the first byte of the member open at its start (negative: in front of the call's text)
    uint32_t n, pad;
};
struct GzPiece { uint64_t at, behind; uint32_t len, seg; };
struct GzWave {
    gz_state st;
    alignas(4) uint8_t win[DFL_WIN];
    uint16_t lit_count[32], lit_sym[DFL_LIT_CAP], lit_fast[1u << DFL_LIT_ROOT];
    uint16_t dist_count[32], dist_sym[DFL_DIST_CAP], dist_fast[1u << DFL_DIST_ROOT];
    uint8_t lens[DFL_LENS];
    uint32_t tok[DFL_TOKENS];
};

// what the lanes of this wave stored to global memory is what they load from now on
__device__ __forceinline__ void gz_wave_global_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(GZ_THREADS) void gzip_decode_kernel(const uint8_t *comp, const GzChunk *chunks, uint64_t n_chunks, uint16_t *symbols, GzBorder *borders,
                                                                 GzResult *results) {
    __shared__ GzWave waves[GZ_WAVES];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    GzWave &W = waves[(tid >> 6) & (GZ_WAVES - 1)];
    dfl_mem m;
    m.win = W.win;
    m.lit_count = W.lit_count; m.lit_sym = W.lit_sym; m.lit_fast = W.lit_fast;
    m.dist_count = W.dist_count; m.dist_sym = W.dist_sym; m.dist_fast = W.dist_fast;
    m.lens = W.lens; m.tok = W.tok;
    const uint64_t wave = (uint64_t)blockIdx.x * GZ_WAVES + (tid >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * GZ_WAVES;
    for (uint64_t ci = wave; ci < n_chunks; ci += nwaves) {
        const GzChunk ch = chunks[ci];
        const uint8_t *payload = comp + ch.src;
        uint16_t *out = symbols + ch.sym;
        GzBorder *bord = borders + ch.border;
        const uint32_t csize = ch.csize <= GZ_MAX_SPAN ? ch.csize : 0u, cap = ch.cap;
        if (lane == 0) gz_begin(W.st, ch.start_bit & 7u, ch.stop, csize, cap, ch.reach0, ch.at_header != 0);
        wave_lds_sync();
        const uint64_t max_steps = gz_max_steps(csize);
        bool done = false;
        for (uint64_t step = 0; step < max_steps; step++) {
            const uint64_t bitpos = W.st.bitpos;
            const uint32_t wbase = W.st.wbase, filled = W.st.filled;
            if (dfl_window_stale(bitpos, wbase, csize, filled != 0)) {
                const uint32_t nb = dfl_window_base(payload, bitpos, csize);
                dfl_fill_lane(reinterpret_cast<uint32_t *>(W.win), payload, csize, nb, lane);
                if (lane == 0) { W.st.wbase = nb; W.st.filled = 1; }
            }
            wave_lds_sync();
            if (lane == 0) {
                gz_state s = W.st;
                gz_step(s, m);
                if (s.act == GZ_ACT_BORDER) {
                    const uint32_t bi = s.n_borders - 1u;
                    if (s.n_borders >= 1u && bi < ch.border_cap) { GzBorder b; b.at = s.out0; b.crc = s.border_crc; b.isize = s.border_isize; b.pad = 0; bord[bi] = b; }
                    else s.err = GZ_E_BORDERS;
                }
                W.st = s;
            }
            wave_lds_sync();
            const uint32_t act = W.st.act, out0 = W.st.out0;
            if (act == DFL_ACT_STORED) {
                const uint32_t at = W.st.stored_at, len = W.st.stored_len;          // len <= 65535
                for (uint32_t j = lane; j < len; j += 64) {
                    const uint64_t o = (uint64_t)out0 + j, s = (uint64_t)at + j;
                    if (o < cap && s < csize) out[o] = payload[s];
                }
            } else if (act == DFL_ACT_TOKENS) {
                const uint32_t ntok = W.st.n_tok < DFL_TOKENS ? W.st.n_tok : DFL_TOKENS;
                const uint32_t k = lane < ntok ? W.tok[lane] : 0u;
                const bool is_match = lane < ntok && (k & DFL_TOK_MATCH);
                const uint32_t mylen = lane < ntok ? (is_match ? ((k >> 16) & 511u) : 1u) : 0u;
                const uint32_t o = out0 + wave_inclusive_sum(mylen) - mylen;
                if (lane < ntok && !is_match && o < cap) out[o] = (uint16_t)(k & 255u);
                unsigned long long mask = __ballot(is_match);
                if (mask) gz_wave_global_sync();                   // the literals, and whatever earlier steps wrote
                int64_t dirty_lo = INT64_MAX;                      // this step's matches wrote [dirty_lo, here) since the last fence
                for (uint32_t guard = 0; mask && guard < DFL_TOKENS; guard++) {
                    const int t = __ffsll((long long)mask) - 1;
                    mask &= mask - 1ull;
                    const uint32_t kt = (uint32_t)__shfl((int)k, t, 64), ot = (uint32_t)__shfl((int)o, t, 64);
                    const uint32_t len = (kt >> 16) & 511u, dist = kt & 0xFFFFu;
                    if (dist == 0 || dist > GZ_REACH) continue;    // (the core emits no such token)
                    const int64_t src0 = (int64_t)ot - (int64_t)dist;      // >= -32768: in front of symbol 0 lies the computed prologue
                    if (src0 + (int64_t)(len < dist ? len : dist) > dirty_lo) { gz_wave_global_sync(); dirty_lo = INT64_MAX; }
                    for (uint32_t j = lane; j < len; j += 64) {
                        const uint64_t d = (uint64_t)ot + j;
                        const int64_t s = src0 + (int64_t)(j < dist ? j : j % dist);    // s < ot <= d
                        if (d < cap && s < (int64_t)d) out[d] = s < 0 ? (uint16_t)(GZ_MARK + (uint32_t)((int64_t)GZ_REACH + s)) : out[s];
                    }
                    if ((int64_t)ot < dirty_lo) dirty_lo = ot;
                }
            }
            if (gz_finished(W.st)) { done = true; break; }
        }
        if (lane == 0) {
            uint32_t err = W.st.err;
            if (err == DFL_OK && !done) err = DFL_E_INPUT;
            GzResult r;
            r.end_bit = W.st.bitpos; r.n_sym = W.st.out; r.status = err; r.n_borders = W.st.n_borders; r.ended = W.st.ended;
            results[ci] = r;
        }
        wave_lds_sync();                                           // the state is the next chunk's from here
    }
}

// byte of a symbol of the chunk `P`: a marker is the byte 32768 - p in front of the chunk's first text byte
__device__ __forceinline__ uint32_t gz_byte(const GzPlace &P, uint32_t v, const uint8_t *text, const uint8_t *carry, bool &bad) {
    if (!(v & GZ_MARK)) return v & 255u;
    const int64_t src = (int64_t)P.t0 - (int64_t)GZ_REACH + (int64_t)(v & (GZ_MARK - 1u));     // >= -32768, < t0
    if (src < P.mstart) { bad = true; return 0u; }
    return src < 0 ? carry[(int64_t)GZ_REACH + src] : text[src];
}

__global__ __launch_bounds__(GZ_WIN_THREADS) void gzip_windows_kernel(const GzPlace *places, uint64_t n_chunks, uint8_t *text, const uint8_t *carry, uint32_t *status) {
    const unsigned tid = threadIdx.x;
    for (uint64_t c = 0; c < n_chunks; c++) {
        const GzPlace P = places[c];
        const uint32_t tail = P.n < GZ_REACH ? P.n : GZ_REACH;
        bool bad = false;
        for (uint32_t k = P.n - tail + tid; k < P.n; k += GZ_WIN_THREADS) text[P.t0 + k] = (uint8_t)gz_byte(P, P.sym[k], text, carry, bad);
        if (bad) status[c] = GZ_E_BACKREF;
        __threadfence_block();
        __syncthreads();                                           // the next chunk's markers read these bytes
    }
}

// blockIdx.y strides the chunks, blockIdx.x the groups of 8 symbols in front of a chunk's last 32768
__global__ __launch_bounds__(256) void gzip_translate_kernel(const GzPlace *places, uint64_t n_chunks, uint8_t *text, const uint8_t *carry, uint32_t *status) {
    for (uint64_t c = blockIdx.y; c < n_chunks; c += gridDim.y) {
        const GzPlace P = places[c];
        const uint32_t n = P.n > GZ_REACH ? P.n - GZ_REACH : 0u;
        bool bad = false;
        for (uint64_t k = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 8; k < n; k += (uint64_t)gridDim.x * 256 * 8) {
            uint8_t *dst = text + P.t0 + k;
            if (k + 8 <= n) {
                const uint4 q = *reinterpret_cast<const uint4 *>(P.sym + k);    // (a chunk's symbols start at a multiple of 8)
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
                uint32_t b[8];
#pragma unroll
                for (int j = 0; j < 8; j++) b[j] = gz_byte(P, (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu, text, carry, bad);
                if ((reinterpret_cast<uintptr_t>(dst) & 7u) == 0) {
                    uint2 o;
                    o.x = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
                    o.y = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
                    *reinterpret_cast<uint2 *>(dst) = o;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; j++) dst[j] = (uint8_t)b[j];
                }
            } else {
                for (uint32_t j = 0; k + j < n; j++) dst[j] = (uint8_t)gz_byte(P, P.sym[k + j], text, carry, bad);
            }
        }
        if (bad) status[c] = GZ_E_BACKREF;
    }
}

__global__ __launch_bounds__(GZ_THREADS) void gzip_crc_kernel(const uint8_t *text, const GzPiece *pieces, uint64_t n_pieces, uint32_t *acc) {
    __shared__ uint32_t crc_table[256];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    crc_table[tid & 255u] = dfl_crc_table_entry(tid);
    __syncthreads();
    const uint64_t wave = (uint64_t)blockIdx.x * GZ_WAVES + (tid >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * GZ_WAVES;
    for (uint64_t pi = wave; pi < n_pieces; pi += nwaves) {
        const GzPiece pc = pieces[pi];
        const uint32_t len = pc.len <= GZ_PIECE ? pc.len : 0u;
        const uint8_t *p = text + pc.at;
        const uint32_t part = (len + 63u) / 64u;
        const uint32_t b0 = lane * part < len ? lane * part : len;
        const uint32_t e0 = b0 + part < len ? b0 + part : len;
        uint32_t reg = 0u;
        for (uint32_t i = b0; i < e0; i++) reg = dfl_crc_byte(crc_table, reg, p[i]);
        // bytes behind this lane's part in the member, modulo the order of x (2^32 - 1): members above 4 GB combine correctly
        const uint32_t behind = (uint32_t)((pc.behind + (len - e0)) % 0xFFFFFFFFull);
        uint32_t share = dfl_crc_mul(reg, dfl_crc_xpow8(behind));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) share ^= (uint32_t)__shfl_xor((int)share, d, 64);
        if (lane == 0) atomicXor(&acc[pc.seg], share);
    }
}

__global__ __launch_bounds__(256) void gzip_carry_kernel(const uint8_t *text, uint64_t total, const uint8_t *old_carry, uint8_t *new_carry) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= GZ_REACH) return;
    const int64_t src = (int64_t)total - (int64_t)GZ_REACH + j;
    new_carry[j] = src >= 0 ? text[src] : old_carry[(int64_t)GZ_REACH + src];
}

}  // namespace mdbg

using namespace mdbg;

extern "C" int mdbg_gzip_stream_create(mdbg_ctx *ctx, mdbg_gzip_stream **out) try {
    if (!ctx || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_gzip_stream_create: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<mdbg_gzip_stream> s(new mdbg_gzip_stream());
    s->owner = ctx;
    for (int i = 0; i < 2; i++) {
        MDBG_TRY(s->carry[i].alloc(ctx, GZ_REACH));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(s->carry[i].p, 0, GZ_REACH, ctx->stream));
    }
    *out = s.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" void mdbg_gzip_stream_free(mdbg_gzip_stream *s) { delete s; }

extern "C" int mdbg_bytes_copy(mdbg_ctx *ctx, mdbg_bytes *dst, uint64_t dst_at, const mdbg_bytes *src, uint64_t src_at, uint64_t n) try {
    if (!ctx || !dst || !src) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_copy: null argument");
    if (dst_at > dst->n || n > dst->n - dst_at)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_copy: [%llu, +%llu) lies outside the %llu bytes of the destination", (unsigned long long)dst_at, (unsigned long long)n,
                         (unsigned long long)dst->n);
    if (src_at > src->n || n > src->n - src_at)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_copy: [%llu, +%llu) lies outside the %llu bytes of the source", (unsigned long long)src_at, (unsigned long long)n,
                         (unsigned long long)src->n);
    if (dst == src && dst_at < src_at + n && src_at < dst_at + n && n)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_copy: [%llu, +%llu) and [%llu, +%llu) of one buffer overlap", (unsigned long long)dst_at, (unsigned long long)n,
                         (unsigned long long)src_at, (unsigned long long)n);
    if (n == 0) return MDBG_OK;
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_TRY(bytes_ready_on(ctx, src));
    MDBG_TRY(bytes_ready_on(ctx, dst));
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(dst->d.p + dst_at, src->d.p + src_at, n, hipMemcpyDeviceToDevice, ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

namespace {
struct GzSeg { uint64_t begin, end; uint32_t crc, isize, ended; uint64_t chunk; };

int gz_decode(mdbg_ctx *ctx, const mdbg_bytes *comp, const std::vector<GzChunk> &table, uint16_t *d_sym, GzBorder *d_borders, std::vector<GzResult> &res) {
    const uint64_t n = table.size();
    DevBuf<GzChunk> d_chunks;
    DevBuf<GzResult> d_res;
    MDBG_TRY(d_chunks.alloc(ctx, n));
    MDBG_TRY(d_res.alloc(ctx, n));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, d_chunks.p, table.data(), n * sizeof(GzChunk), hipMemcpyHostToDevice));
    {
        LaunchTimer timer(ctx, "gzip_decode");
        const unsigned grid = grid_for(n, GZ_WAVES, (unsigned)ctx->n_cu * 8u);
        hipLaunchKernelGGL(gzip_decode_kernel, dim3(grid), dim3(GZ_THREADS), 0, ctx->stream, comp->d.p, d_chunks.p, n, d_sym, d_borders, d_res.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    res.resize(n);
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, res.data(), d_res.p, n * sizeof(GzResult), hipMemcpyDeviceToHost));
    return MDBG_OK;
}
}  // namespace

extern "C" int mdbg_bytes_inflate_gzip(mdbg_ctx *ctx, mdbg_gzip_stream *s, const mdbg_bytes *comp, const mdbg_gzip_chunk *chunks, uint64_t n_chunks, mdbg_bytes *text,
                                       uint64_t text_at, uint64_t *n_text, uint64_t info[4]) try {
    if (!ctx || !s || !comp || !text || !n_text || (n_chunks && !chunks)) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_gzip: null argument");
    *n_text = 0;
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (s->owner != ctx) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_gzip: the stream belongs to another context");
    if (text_at > text->n)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_gzip: offset %llu lies outside the %llu bytes of the text buffer", (unsigned long long)text_at,
                         (unsigned long long)text->n);
    if (n_chunks == 0) return MDBG_OK;
    if (s->finished) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_gzip: the file's last member has ended on this stream");
    // ---- the chunk table ---------------------------------------------------------------------------------------------------------
    std::vector<GzChunk> table(n_chunks);
    uint64_t n_sym = 0, n_border = 0;
    for (uint64_t i = 0; i < n_chunks; i++) {
        const uint64_t start = chunks[i].start_bit, stop = chunks[i].stop_bit;
        if (i + 1 < n_chunks && (stop == MDBG_GZIP_TO_END || stop != chunks[i + 1].start_bit))
            return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_gzip: chunk %llu: its stop is not the next chunk's start", (unsigned long long)i);
        const uint64_t first = start >> 3;
        if (first >= comp->n || (stop != MDBG_GZIP_TO_END && (stop <= start || (stop + 7) / 8 > comp->n)))
            return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_gzip: chunk %llu: bits [%llu, %llu) are empty or lie outside the %llu compressed bytes", (unsigned long long)i,
                             (unsigned long long)start, (unsigned long long)stop, (unsigned long long)comp->n);
        if (i == 0 && !s->member_open && (start & 7u))
            return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_gzip: chunk 0: a member header starts at a whole byte, not at bit %llu", (unsigned long long)start);
        const uint64_t span = (stop == MDBG_GZIP_TO_END ? comp->n : (stop + 7) / 8) - first;
        if (span > GZ_MAX_SPAN)
            return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_gzip: chunk %llu: a span of %llu bytes is more than a chunk may have (%u)", (unsigned long long)i,
                             (unsigned long long)span, GZ_MAX_SPAN);
        GzChunk &c = table[i];
        c.src = first; c.stop = stop == MDBG_GZIP_TO_END ? GZ_TO_END : stop - first * 8;
        c.start_bit = (uint32_t)(start & 7u); c.csize = (uint32_t)span; c.cap = (uint32_t)span * 8u + 64u;
        c.border_cap = (uint32_t)span / 20u + 2u;
        c.reach0 = i == 0 ? (s->member_open ? (uint32_t)std::min<uint64_t>(s->member_len, GZ_REACH) : 0u) : GZ_REACH;
        c.at_header = i == 0 && !s->member_open ? 1u : 0u;
        c.pad0 = c.pad1 = 0;
        c.sym = n_sym; c.border = n_border;
        n_sym += ((uint64_t)c.cap + 7u) & ~7ull;
        n_border += c.border_cap;
    }
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DevBuf<uint16_t> d_sym, d_sym2;
    DevBuf<GzBorder> d_borders;
    MDBG_TRY(d_sym.alloc(ctx, n_sym));
    MDBG_TRY(d_borders.alloc(ctx, n_border));
    MDBG_TRY(bytes_ready_on(ctx, comp));                      // uploads still in flight: the kernels run behind them
    MDBG_TRY(bytes_ready_on(ctx, text));
    std::vector<GzResult> res;
    MDBG_TRY(gz_decode(ctx, comp, table, d_sym.p, d_borders.p, res));
    // ---- chunks that overflowed 8 symbols a byte: once more, at the format's maximum -----------------------------------------------
    std::vector<uint64_t> sym_at(n_chunks);                   // < n_sym: in d_sym; else n_sym + offset in d_sym2
    for (uint64_t i = 0; i < n_chunks; i++) sym_at[i] = table[i].sym;
    {
        std::vector<GzChunk> again;
        std::vector<uint64_t> which;
        uint64_t n2 = 0;
        for (uint64_t i = 0; i < n_chunks; i++) {
            if (res[i].status != GZ_E_OVERFLOW) continue;
            GzChunk c = table[i];
            c.cap = (uint32_t)gz_max_symbols(c.csize);
            c.sym = n2;
            n2 += ((uint64_t)c.cap + 7u) & ~7ull;
            again.push_back(c);
            which.push_back(i);
        }
        if (!again.empty()) {
            MDBG_TRY(d_sym2.alloc(ctx, n2));
            std::vector<GzResult> res2;
            MDBG_TRY(gz_decode(ctx, comp, again, d_sym2.p, d_borders.p, res2));
            for (size_t k = 0; k < which.size(); k++) { res[which[k]] = res2[k]; sym_at[which[k]] = n_sym + again[k].sym; }
        }
    }
    for (uint64_t i = 0; i < n_chunks; i++) {
        uint32_t st = res[i].status;
        if (st == DFL_OK && i + 1 < n_chunks && res[i].ended != GZ_END_STOP) st = GZ_E_STOP;     // a later chunk starts at a block header, inside a member
        if (st != DFL_OK)
            return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_gzip: chunk %llu does not decode: %s", (unsigned long long)i, dfl_reason(st));
    }
    // ---- places, in 64-bit arithmetic ------------------------------------------------------------------------------------------------
    std::vector<GzPlace> places(n_chunks);
    std::vector<GzSeg> segs;
    uint64_t total = 0, n_members = 0;
    {
        int64_t mstart = s->member_open ? -(int64_t)std::min<uint64_t>(s->member_len, (uint64_t)INT64_MAX) : 0;
        uint64_t seg_begin = 0;
        std::vector<GzBorder> hb;
        for (uint64_t i = 0; i < n_chunks; i++) {
            GzPlace &P = places[i];
            P.sym = sym_at[i] < n_sym ? d_sym.p + sym_at[i] : d_sym2.p + (sym_at[i] - n_sym);
            P.t0 = total; P.mstart = mstart; P.n = res[i].n_sym; P.pad = 0;
            if (res[i].n_borders) {
                if (res[i].n_borders > table[i].border_cap) return set_error(ctx, MDBG_EHIP, "mdbg_bytes_inflate_gzip: chunk %llu reports more borders than it has room for", (unsigned long long)i);
                hb.resize(res[i].n_borders);
                MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, hb.data(), d_borders.p + table[i].border, hb.size() * sizeof(GzBorder), hipMemcpyDeviceToHost));
                for (const GzBorder &b : hb) {
                    if (b.at > res[i].n_sym) return set_error(ctx, MDBG_EHIP, "mdbg_bytes_inflate_gzip: chunk %llu reports a border outside its symbols", (unsigned long long)i);
                    GzSeg g; g.begin = seg_begin; g.end = total + b.at; g.crc = b.crc; g.isize = b.isize; g.ended = 1; g.chunk = i;
                    segs.push_back(g);
                    seg_begin = g.end;
                    mstart = (int64_t)g.end;
                    n_members++;
                }
            }
            total += res[i].n_sym;
        }
        if (res[n_chunks - 1].ended == GZ_END_STOP) { GzSeg g; g.begin = seg_begin; g.end = total; g.crc = 0; g.isize = 0; g.ended = 0; g.chunk = n_chunks - 1; segs.push_back(g); }
    }
    if (total > text->n - text_at) {
        *n_text = total;
        return set_error(ctx, MDBG_ERANGE, "mdbg_bytes_inflate_gzip: the text is %llu bytes, the buffer has room for %llu behind offset %llu", (unsigned long long)total,
                         (unsigned long long)(text->n - text_at), (unsigned long long)text_at);
    }
    std::vector<GzPiece> pieces;
    for (size_t g = 0; g < segs.size(); g++)
        for (uint64_t at = segs[g].begin; at < segs[g].end; at += GZ_PIECE) {
            GzPiece p; p.at = at; p.len = (uint32_t)std::min<uint64_t>(GZ_PIECE, segs[g].end - at); p.seg = (uint32_t)g; p.behind = segs[g].end - (at + p.len);
            pieces.push_back(p);
        }
    // ---- symbols to text ---------------------------------------------------------------------------------------------------------------
    DevBuf<GzPlace> d_places;
    DevBuf<GzPiece> d_pieces;
    DevBuf<uint32_t> d_status, d_acc;
    MDBG_TRY(d_places.alloc(ctx, n_chunks));
    MDBG_TRY(d_pieces.alloc(ctx, pieces.size()));
    MDBG_TRY(d_status.alloc(ctx, n_chunks));
    MDBG_TRY(d_acc.alloc(ctx, segs.size()));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, d_places.p, places.data(), n_chunks * sizeof(GzPlace), hipMemcpyHostToDevice));
    if (!pieces.empty()) MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, d_pieces.p, pieces.data(), pieces.size() * sizeof(GzPiece), hipMemcpyHostToDevice));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(d_status.p, 0, n_chunks * 4, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(d_acc.p, 0, std::max<size_t>(segs.size(), 1) * 4, ctx->stream));
    uint8_t *d_text = text->d.p + text_at;
    const uint8_t *carry = s->carry[s->cur].p;
    uint8_t *next_carry = s->carry[s->cur ^ 1].p;
    {
        LaunchTimer timer(ctx, "gzip_windows");
        hipLaunchKernelGGL(gzip_windows_kernel, dim3(1), dim3(GZ_WIN_THREADS), 0, ctx->stream, d_places.p, n_chunks, d_text, carry, d_status.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    {
        LaunchTimer timer(ctx, "gzip_translate");
        const dim3 grid(16, (unsigned)std::min<uint64_t>(n_chunks, 4096));
        hipLaunchKernelGGL(gzip_translate_kernel, grid, dim3(256), 0, ctx->stream, d_places.p, n_chunks, d_text, carry, d_status.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    if (!pieces.empty()) {
        LaunchTimer timer(ctx, "gzip_crc");
        const unsigned grid = grid_for(pieces.size(), GZ_WAVES, (unsigned)ctx->n_cu * 8u);
        hipLaunchKernelGGL(gzip_crc_kernel, dim3(grid), dim3(GZ_THREADS), 0, ctx->stream, d_text, d_pieces.p, (uint64_t)pieces.size(), d_acc.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(gzip_carry_kernel, dim3(GZ_REACH / 256), dim3(256), 0, ctx->stream, d_text, total, carry, next_carry);
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    std::vector<uint32_t> status(n_chunks), acc(std::max<size_t>(segs.size(), 1));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, status.data(), d_status.p, n_chunks * 4, hipMemcpyDeviceToHost));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, acc.data(), d_acc.p, acc.size() * 4, hipMemcpyDeviceToHost));
    // ---- the verdicts: markers, then every member that ended against its trailer ------------------------------------------------------
    uint32_t open_reg = 0xFFFFFFFFu;
    for (size_t g = 0; g < segs.size(); g++) {
        const uint64_t len = segs[g].end - segs[g].begin;
        const uint32_t reg0 = g == 0 && s->member_open ? s->reg : 0xFFFFFFFFu;
        const uint32_t reg = acc[g] ^ dfl_crc_mul(reg0, dfl_crc_xpow8((uint32_t)(len % 0xFFFFFFFFull)));
        if (!segs[g].ended) { open_reg = reg; continue; }
        const uint64_t member = (g == 0 && s->member_open ? s->member_len : 0) + len;
        uint32_t &st = status[segs[g].chunk];
        if (st == DFL_OK && (uint32_t)member != segs[g].isize) st = GZ_E_ISIZE;
        if (st == DFL_OK && (reg ^ 0xFFFFFFFFu) != segs[g].crc) st = DFL_E_CRC;
    }
    for (uint64_t i = 0; i < n_chunks; i++)
        if (status[i] != DFL_OK)
            return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_gzip: chunk %llu does not decode: %s", (unsigned long long)i, dfl_reason(status[i]));
    // ---- the stream advances -----------------------------------------------------------------------------------------------------------
    const GzResult &last = res[n_chunks - 1];
    if (last.ended == GZ_END_STOP) {
        s->member_len = (segs.size() == 1 && s->member_open ? s->member_len : 0) + (segs.back().end - segs.back().begin);
        s->reg = open_reg;
        s->member_open = true;
    } else {
        s->member_open = false; s->member_len = 0; s->reg = 0xFFFFFFFFu;
        s->finished = last.ended == GZ_END_STREAM;
    }
    s->cur ^= 1;
    *n_text = total;
    if (info) { info[0] = total; info[1] = n_members; info[2] = s->finished ? 1 : 0; info[3] = table[n_chunks - 1].src * 8 + last.end_bit; }
    return MDBG_OK;
} MDBG_API_CATCH(ctx)
