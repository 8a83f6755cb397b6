// inflate.hip -- BGZF blocks inflated on the device (mdbg_bytes_inflate_bgzf), the text read back (mdbg_bytes_download) and cut at
// the end of its last whole record (mdbg_fastx_whole_records).  Replaces gzread under the kseq loop (KSEQ_INIT(gzFile, gzread),
// Commons.hpp:82; the read loop, Commons.hpp:5842-5870) for files that samtools, bam2fastq and bgzip write: independent gzip members
// of at most 64 KB that state their compressed and uncompressed sizes, so the block table comes from the headers and every block's
// place in the text is a prefix sum.
//
//   one wave per BGZF block, grid-stride over the blocks.  Lane 0 runs the serial core (deflate_core.hpp: bit reader, tables, symbol
//   decoder) over arrays in LDS and leaves up to 64 tokens; the wave resolves them: a prefix sum of their lengths, the literals stored
//   in parallel, the matches copied in token order with the lanes striding the copy (dist < len: source index j % dist).  The window
//   is the block: a match reads the text the wave itself wrote, in global memory, behind a workgroup-scope fence that is paid once in
//   every batch that holds a match, and again only when a match's source overlaps what an earlier match of the same batch wrote.  Stored blocks are a wave-wide copy.  The input reaches lane 0 through a 2 KB
//   window in LDS that the wave refills with aligned words.  Then the CRC-32: lanes over contiguous pieces with a 256-entry table in
//   LDS, joined by multiplying with x^(8 len) mod P.
//
//   LDS per wave: window 2048 + literal/length code 64 + 576 + 1024 + distance code 64 + 64 + 128 + lengths 352 + tokens 256 + state 72
//   = 4648 bytes; four waves a block and the CRC table: 19.6 KB, eight blocks a CU.
#include "common.hpp"
#include "objects.hpp"
#include "deflate_core.hpp"

#include <vector>

namespace mdbg {

int bytes_ready_on(mdbg_ctx *ctx, const mdbg_bytes *b);      // minimizers.hip

constexpr int INFL_THREADS = 256, INFL_WAVES = INFL_THREADS / 64;

struct InflBlock {            // a block as the kernel sees it (checked by the host: inside comp, inside text, isize <= 65536)
    uint64_t src, out;
    uint32_t csize, isize, crc, pad;
};
struct InflWave {
    dfl_state st;
    alignas(4) uint8_t win[DFL_WIN];
    uint16_t lit_count[32], lit_sym[DFL_LIT_CAP], lit_fast[1u << DFL_LIT_ROOT];
    uint16_t dist_count[32], dist_sym[DFL_DIST_CAP], dist_fast[1u << DFL_DIST_ROOT];
    uint8_t lens[DFL_LENS];
    uint32_t tok[DFL_TOKENS];
};

// what the lanes of this wave stored to global memory is what they load from now on
__device__ __forceinline__ void wave_global_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(INFL_THREADS) void inflate_bgzf_kernel(const uint8_t *comp, const InflBlock *blocks, uint64_t n_blocks, uint8_t *text,
                                                                    uint32_t *status) {
    __shared__ InflWave waves[INFL_WAVES];
    __shared__ uint32_t crc_table[256];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    crc_table[tid & 255u] = dfl_crc_table_entry(tid);
    __syncthreads();
    InflWave &W = waves[(tid >> 6) & (INFL_WAVES - 1)];
    dfl_mem m;
    m.win = W.win;
    m.lit_count = W.lit_count; m.lit_sym = W.lit_sym; m.lit_fast = W.lit_fast;
    m.dist_count = W.dist_count; m.dist_sym = W.dist_sym; m.dist_fast = W.dist_fast;
    m.lens = W.lens; m.tok = W.tok;
    const uint64_t wave = (uint64_t)blockIdx.x * INFL_WAVES + (tid >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * INFL_WAVES;
    for (uint64_t bi = wave; bi < n_blocks; bi += nwaves) {
        const InflBlock blk = blocks[bi];
        const uint8_t *payload = comp + blk.src;
        uint8_t *out = text + blk.out;
        const uint32_t csize = blk.csize, isize = blk.isize <= DFL_MAX_ISIZE ? blk.isize : 0u;
        if (lane == 0) dfl_begin(W.st, csize, isize);
        wave_lds_sync();
        const uint64_t max_steps = dfl_max_steps(csize);
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
                dfl_state s = W.st;
                dfl_step(s, m);
                W.st = s;
            }
            wave_lds_sync();
            const uint32_t act = W.st.act, out0 = W.st.out0;
            if (act == DFL_ACT_STORED) {
                const uint32_t at = W.st.stored_at, len = W.st.stored_len;          // len <= 65535
                for (uint32_t j = lane; j < len; j += 64) {
                    const uint64_t o = (uint64_t)out0 + j, s = (uint64_t)at + j;
                    if (o < isize && s < csize) out[o] = payload[s];
                }
            } else if (act == DFL_ACT_TOKENS) {
                const uint32_t ntok = W.st.n_tok < DFL_TOKENS ? W.st.n_tok : DFL_TOKENS;
                const uint32_t k = lane < ntok ? W.tok[lane] : 0u;
                const bool is_match = lane < ntok && (k & DFL_TOK_MATCH);
                const uint32_t mylen = lane < ntok ? (is_match ? ((k >> 16) & 511u) : 1u) : 0u;
                const uint32_t o = out0 + wave_inclusive_sum(mylen) - mylen;
                if (lane < ntok && !is_match && o < isize) out[o] = (uint8_t)k;
                unsigned long long mask = __ballot(is_match);
                if (mask) wave_global_sync();                      // the literals, and whatever earlier steps wrote
                uint32_t dirty_lo = 0xFFFFFFFFu;                   // this step's matches wrote [dirty_lo, here) since the last fence
                for (uint32_t guard = 0; mask && guard < DFL_TOKENS; guard++) {
                    const int t = __ffsll((long long)mask) - 1;
                    mask &= mask - 1ull;
                    const uint32_t kt = (uint32_t)__shfl((int)k, t, 64), ot = (uint32_t)__shfl((int)o, t, 64);
                    const uint32_t len = (kt >> 16) & 511u, dist = kt & 0xFFFFu;
                    if (dist == 0 || dist > ot) continue;          // (the core emits no such token)
                    const uint32_t src0 = ot - dist;
                    if (src0 + (len < dist ? len : dist) > dirty_lo) { wave_global_sync(); dirty_lo = 0xFFFFFFFFu; }
                    for (uint32_t j = lane; j < len; j += 64) {
                        const uint32_t d = ot + j;
                        const uint32_t s = src0 + (j < dist ? j : j % dist);        // s < ot <= d
                        if (d < isize && s < d) out[d] = out[s];
                    }
                    if (ot < dirty_lo) dirty_lo = ot;
                }
            }
            if (dfl_finished(W.st)) { done = true; break; }
        }
        uint32_t err = W.st.err;
        if (err == DFL_OK && !done) err = DFL_E_INPUT;
        if (err == DFL_OK && W.st.out != isize) err = DFL_E_SIZE;
        if (err == DFL_OK) {
            wave_global_sync();
            const uint32_t piece = (isize + 63u) / 64u;
            const uint32_t b0 = lane * piece < isize ? lane * piece : isize;
            const uint32_t e0 = b0 + piece < isize ? b0 + piece : isize;
            uint32_t reg = lane == 0 ? 0xFFFFFFFFu : 0u;
            for (uint32_t i = b0; i < e0; i++) reg = dfl_crc_byte(crc_table, reg, out[i]);
            uint32_t share = dfl_crc_mul(reg, dfl_crc_xpow8(isize - e0));
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) share ^= (uint32_t)__shfl_xor((int)share, d, 64);
            if ((share ^ 0xFFFFFFFFu) != blk.crc) err = DFL_E_CRC;
        }
        if (lane == 0) status[bi] = err;
        wave_lds_sync();                                           // the state is the next block's from here
    }
}

// ---- where the last whole record ends ------------------------------------------------------------------------------------------------
constexpr int WR_THREADS = 256;
constexpr uint64_t WR_TILE = (uint64_t)WR_THREADS * 64;       // a thread reads four pieces of 16 bytes
struct WrTile {
    uint64_t last_hdr;        // 1 + offset of the tile's last '>' that directly follows a '\n' (0: none)
    uint32_t n_nl, first;     // '\n' in the tile; tile 0: the range's first byte
};
// 16 bytes at the aligned offset `at` (the buffer holds 16 bytes more than its text): masks of '\n' and of '>' behind a '\n', in range
__device__ __forceinline__ void wr_load(const uint8_t *d, uint64_t at, uint64_t begin, uint64_t end, uint32_t &nl, uint32_t &hdr) {
    nl = hdr = 0;
    if (at >= end || at + 16 <= begin) return;
    const uint4 q = *reinterpret_cast<const uint4 *>(d + at);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    uint32_t gt = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 255u;
        if (at + j < begin || at + j >= end) continue;
        if (c == '\n') nl |= 1u << j;
        if (c == '>') gt |= 1u << j;
    }
    uint32_t prev_nl = 0;
    if (at > begin) prev_nl = d[at - 1] == '\n' ? 1u : 0u;
    hdr = gt & ((nl << 1) | prev_nl);
}
__global__ __launch_bounds__(WR_THREADS) void whole_records_count_kernel(const uint8_t *d, uint64_t begin, uint64_t end, uint64_t a0, WrTile *tiles) {
    __shared__ uint32_t cnt;
    __shared__ unsigned long long last;
    const unsigned tid = threadIdx.x;
    if (tid == 0) { cnt = 0; last = 0; }
    __syncthreads();
    uint32_t n = 0;
    unsigned long long mine = 0;
    for (int s = 0; s < 4; s++) {
        const uint64_t at = a0 + (uint64_t)blockIdx.x * WR_TILE + ((uint64_t)tid * 4 + s) * 16;
        uint32_t nl, hdr;
        wr_load(d, at, begin, end, nl, hdr);
        n += __popc(nl);
        if (hdr) mine = at + (31 - __clz((int)hdr)) + 1;
    }
    if (n) atomicAdd(&cnt, n);
    if (mine) atomicMax(&last, mine);
    __syncthreads();
    if (tid == 0) {
        WrTile t;
        t.last_hdr = last; t.n_nl = cnt; t.first = blockIdx.x == 0 ? d[begin] : 0u;
        tiles[blockIdx.x] = t;
    }
}
// one tile: 1 + offset of its `want`-th '\n' (1-based)
__global__ __launch_bounds__(WR_THREADS) void whole_records_find_kernel(const uint8_t *d, uint64_t begin, uint64_t end, uint64_t a0, uint64_t tile, uint32_t want,
                                                                        uint64_t *found) {
    __shared__ uint32_t wsum[WR_THREADS / 64];
    const unsigned tid = threadIdx.x, wave = tid >> 6;
    uint32_t nl[4], n = 0;
    for (int s = 0; s < 4; s++) {
        uint32_t hdr;
        wr_load(d, a0 + tile * WR_TILE + ((uint64_t)tid * 4 + s) * 16, begin, end, nl[s], hdr);
        n += __popc(nl[s]);
    }
    const uint32_t inc = wave_inclusive_sum(n);
    if ((tid & 63u) == 63u) wsum[wave] = inc;
    __syncthreads();
    uint32_t seen = inc - n;                                   // line ends in front of this thread's 64 bytes
    for (unsigned w = 0; w < wave; w++) seen += wsum[w];
    if (want <= seen || want > seen + n) return;
    for (int s = 0; s < 4; s++) {
        uint32_t mk = nl[s];
        while (mk) {
            const int j = __ffs((int)mk) - 1;
            mk &= mk - 1u;
            if (++seen == want) { *found = a0 + tile * WR_TILE + ((uint64_t)tid * 4 + s) * 16 + j + 1; return; }
        }
    }
}

}  // namespace mdbg

using namespace mdbg;

extern "C" int mdbg_bytes_inflate_bgzf(mdbg_ctx *ctx, const mdbg_bytes *comp, const mdbg_bgzf_block *blocks, uint64_t n_blocks, mdbg_bytes *text,
                                       uint64_t text_at, uint64_t *n_text) try {
    if (!ctx || !comp || !text || !n_text || (n_blocks && !blocks)) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_bgzf: null argument");
    *n_text = 0;
    if (text_at > text->n)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_bgzf: offset %llu lies outside the %llu bytes of the text buffer", (unsigned long long)text_at,
                         (unsigned long long)text->n);
    std::vector<InflBlock> table(n_blocks);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_blocks; i++) {
        const mdbg_bgzf_block &b = blocks[i];
        if (b.src > comp->n || b.csize > comp->n - b.src)
            return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_bgzf: block %llu: payload [%llu, +%u) lies outside the %llu compressed bytes", (unsigned long long)i,
                             (unsigned long long)b.src, b.csize, (unsigned long long)comp->n);
        if (b.csize > DFL_MAX_CSIZE)                           // (the kernel's loops are bounded by csize: a wave never sits on gigabytes)
            return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_bgzf: block %llu: csize %u is more than a BGZF block holds (65536)", (unsigned long long)i, b.csize);
        if (b.isize > DFL_MAX_ISIZE)
            return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_bgzf: block %llu: isize %u is more than a BGZF block holds (65536)", (unsigned long long)i, b.isize);
        table[i].src = b.src; table[i].out = total; table[i].csize = b.csize; table[i].isize = b.isize; table[i].crc = b.crc; table[i].pad = 0;
        total += b.isize;
        if (total > text->n - text_at)
            return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_bgzf: block %llu: the text up to its end is %llu bytes, the buffer has room for %llu behind offset %llu",
                             (unsigned long long)i, (unsigned long long)total, (unsigned long long)(text->n - text_at), (unsigned long long)text_at);
    }
    if (n_blocks == 0) return MDBG_OK;
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DevBuf<InflBlock> d_blocks;
    DevBuf<uint32_t> d_status;
    MDBG_TRY(d_blocks.alloc(ctx, n_blocks));
    MDBG_TRY(d_status.alloc(ctx, n_blocks));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, d_blocks.p, table.data(), n_blocks * sizeof(InflBlock), hipMemcpyHostToDevice));
    MDBG_TRY(bytes_ready_on(ctx, comp));                      // uploads still in flight: the kernel runs behind them
    MDBG_TRY(bytes_ready_on(ctx, text));
    {
        LaunchTimer timer(ctx, "inflate_bgzf");
        const unsigned grid = grid_for(n_blocks, INFL_WAVES, (unsigned)ctx->n_cu * 8u);
        hipLaunchKernelGGL(inflate_bgzf_kernel, dim3(grid), dim3(INFL_THREADS), 0, ctx->stream, comp->d.p, d_blocks.p, n_blocks, text->d.p + text_at, d_status.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    std::vector<uint32_t> status(n_blocks);
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, status.data(), d_status.p, n_blocks * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n_blocks; i++)
        if (status[i] != DFL_OK)
            return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_inflate_bgzf: block %llu does not decode: %s", (unsigned long long)i, dfl_reason(status[i]));
    *n_text = total;
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_bytes_download(mdbg_ctx *ctx, const mdbg_bytes *b, uint64_t at, void *host, uint64_t n) try {
    if (!ctx || !b || (n && !host)) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_download: null argument");
    if (at > b->n || n > b->n - at)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_download: [%llu, +%llu) lies outside the %llu bytes of the buffer", (unsigned long long)at, (unsigned long long)n,
                         (unsigned long long)b->n);
    if (n == 0) return MDBG_OK;
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_TRY(bytes_ready_on(ctx, b));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, host, b->d.p + at, n, hipMemcpyDeviceToHost));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_fastx_whole_records(mdbg_ctx *ctx, const mdbg_bytes *text, uint64_t begin, uint64_t end, uint64_t *cut, int *format) try {
    if (!ctx || !text || !cut || !format) return set_error(ctx, MDBG_EINVAL, "mdbg_fastx_whole_records: null argument");
    if (begin >= end || end > text->n)
        return set_error(ctx, MDBG_EINVAL, "mdbg_fastx_whole_records: [%llu, %llu) is empty or lies outside the %llu bytes of the buffer", (unsigned long long)begin,
                         (unsigned long long)end, (unsigned long long)text->n);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint8_t *d = text->d.p;
    const uint64_t a0 = begin & ~15ull;
    const uint64_t n_tiles = (end - a0 + WR_TILE - 1) / WR_TILE;
    if (n_tiles >= (1ull << 31)) return set_error(ctx, MDBG_ERANGE, "mdbg_fastx_whole_records: a range of %llu bytes is too long for one call", (unsigned long long)(end - begin));
    DevBuf<WrTile> d_tiles;
    DevBuf<uint64_t> d_found;
    MDBG_TRY(d_tiles.alloc(ctx, n_tiles));
    MDBG_TRY(d_found.alloc(ctx, 1));
    MDBG_TRY(bytes_ready_on(ctx, text));
    {
        LaunchTimer timer(ctx, "fastx_whole_records");
        hipLaunchKernelGGL(whole_records_count_kernel, dim3((unsigned)n_tiles), dim3(WR_THREADS), 0, ctx->stream, d, begin, end, a0, d_tiles.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    std::vector<WrTile> tiles(n_tiles);
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, tiles.data(), d_tiles.p, n_tiles * sizeof(WrTile), hipMemcpyDeviceToHost));
    const int first = (int)tiles[0].first;
    if (first != '>' && first != '@')
        return set_error(ctx, MDBG_EINVAL, "mdbg_fastx_whole_records: the text must begin with '>' or '@', not with byte 0x%02x", first);
    *format = first == '@' ? 1 : 0;
    *cut = begin;
    if (first == '>') {
        for (uint64_t t = n_tiles; t-- > 0;)
            if (tiles[t].last_hdr) { *cut = tiles[t].last_hdr - 1; break; }
        return MDBG_OK;
    }
    uint64_t n_nl = 0;
    for (uint64_t t = 0; t < n_tiles; t++) n_nl += tiles[t].n_nl;
    const uint64_t want = n_nl / 4 * 4;
    if (want == 0) return MDBG_OK;
    uint64_t run = 0, tile = 0;
    while (tile < n_tiles && run + tiles[tile].n_nl < want) run += tiles[tile++].n_nl;
    if (tile >= n_tiles) return set_error(ctx, MDBG_EHIP, "mdbg_fastx_whole_records: the tile counts do not add up");
    uint64_t found = 0;
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(d_found.p, 0, 8, ctx->stream));
    hipLaunchKernelGGL(whole_records_find_kernel, dim3(1), dim3(WR_THREADS), 0, ctx->stream, d, begin, end, a0, tile, (uint32_t)(want - run), d_found.p);
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &found, d_found.p, 8, hipMemcpyDeviceToHost));
    if (found <= begin || found > end) return set_error(ctx, MDBG_EHIP, "mdbg_fastx_whole_records: the search of tile %llu found nothing", (unsigned long long)tile);
    *cut = found;
    return MDBG_OK;
} MDBG_API_CATCH(ctx)
