// fastx.hip -- FASTA / FASTQ text taken apart on the device (mdbg_reads_from_fastx_bytes): the bytes of a plain file, uploaded as they
// are (mdbg_bytes_*), become an mdbg_reads without a host pass over the characters.  Record semantics: host/fastx.hpp (the kseq loop
// the reference parses with, Commons.hpp:82, :5827-5922), restated in metamdbg_amd/formats.py fastx_records.
//
//   classify   every tile of 16 KB counts its line starts, its header lines and the base characters of its lines; what a tile cannot
//              know alone -- the class of the line that is open where it begins -- is kept apart (FASTA: the characters in front of the
//              tile's first line start; FASTQ: the characters by line index modulo 4) and settled by one block that scans the tile sums.
//   records    the tiles again, now with what lies in front of them: every base character goes to its place in one contiguous run of
//              characters (its index is the count of base characters before it), every record start notes that count (the record's
//              base offset) and, FASTQ, every line its first byte.  Then one thread a record: length, words, the four-line rule.
//   pack       one wave per read over the contiguous characters: words, invalid bits, break bits, the per-read masked flag
//              (pack_ascii_kernel's rules); FASTQ: the quality lines copied device to device.
#include "common.hpp"
#include "objects.hpp"

#include <vector>

namespace mdbg {

int bytes_ready_on(mdbg_ctx *ctx, const mdbg_bytes *b);      // minimizers.hip

constexpr int FX_THREADS = 256;
constexpr int FX_SUB = 4;                                     // 16-byte loads per thread and tile
constexpr uint64_t FX_TILE = (uint64_t)FX_THREADS * 16 * FX_SUB;

struct FxTileSum {
    uint32_t nls;        // line starts in the tile
    uint32_t nhdr;       // of them FASTA headers
    uint32_t head;       // base characters in front of the tile's first line start
    uint32_t cnt[4];     // FASTA: [0] base characters of the non-header lines that start in the tile
                         // FASTQ: [k & 3] those of the tile's k-th line start (k = 1, 2, ...)
    uint32_t tail;       // FASTA: class of the last line that starts in the tile (1 sequence, 2 header)
    uint32_t lnb;        // FASTQ: 1 + local line index (0 = the open line) of the last byte that is neither \r nor \n; 0: none
};
struct FxTileCarry {
    uint64_t lines, hdrs, kept;   // line starts / headers / base characters in front of the tile
    uint32_t open, pad;           // FASTA: class of the line open at the tile's first byte
};
// totals: [0] lines, [1] headers, [2] base characters, [3] 1 + index of the last non-blank line, [4] first byte, [5] last byte is \n
constexpr int FX_TOTALS = 6;
// state: [0] first offending line << 3 | kind (atomicMin), [1] bit 0 invalid / bit 1 break seen | bit 8 a read too long, [2] longest read
constexpr uint64_t FX_NO_BAD = ~0ull;

template <typename T, bool MAX>
__device__ __forceinline__ T fx_block_excl(T v, T *total, T *lds /* 4 */) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(inc, d, 64);
        if (lane >= (unsigned)d) inc = MAX ? (t > inc ? t : inc) : inc + t;
    }
    T ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0;
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    const T w0 = lds[0], w1 = lds[1], w2 = lds[2], w3 = lds[3];
    T base = 0, tot = w0;
    if (MAX) {
        if (wave > 0) base = w0;
        if (wave > 1 && w1 > base) base = w1;
        if (wave > 2 && w2 > base) base = w2;
        if (w1 > tot) tot = w1;
        if (w2 > tot) tot = w2;
        if (w3 > tot) tot = w3;
    } else {
        base = (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0);
        tot = w0 + w1 + w2 + w3;
    }
    *total = tot;
    __syncthreads();
    return MAX ? (ex > base ? ex : base) : base + ex;
}

// 16 bytes of the text at the 16-byte aligned buffer offset `at`, as bit masks over the bytes that lie in [begin, end)
struct FxChunk {
    uint32_t w[4];
    uint32_t valid, nl, cr, ws, ls, gt, bad;   // in range, \n, \r, white space, line starts, line starts with '>', with '@' or '+'
    __device__ __forceinline__ uint32_t byte(int j) const { return (w[j >> 2] >> (8 * (j & 3))) & 255u; }
};
__device__ __forceinline__ void fx_load(const uint8_t *d, uint64_t at, uint64_t begin, uint64_t end, FxChunk &k) {
    k.valid = k.nl = k.cr = k.ws = k.ls = k.gt = k.bad = 0;
    k.w[0] = k.w[1] = k.w[2] = k.w[3] = 0;
    if (at >= end || at + 16 <= begin) return;
    const uint4 q = *reinterpret_cast<const uint4 *>(d + at);       // the buffer holds 16 bytes more than the text (mdbg_bytes_create)
    k.w[0] = q.x; k.w[1] = q.y; k.w[2] = q.z; k.w[3] = q.w;
    uint32_t gt = 0, bad = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t c = k.byte(j);
        const bool in = at + j >= begin && at + j < end;
        if (!in) continue;
        k.valid |= 1u << j;
        if (c == '\n') k.nl |= 1u << j;
        if (c == '\r') k.cr |= 1u << j;
        if (c == '\n' || c == '\r' || c == ' ' || c == '\t') k.ws |= 1u << j;
        if (c == '>') gt |= 1u << j;
        if (c == '@' || c == '+') bad |= 1u << j;
    }
    uint32_t prev_nl = 0;
    if (at > begin) prev_nl = d[at - 1] == '\n' ? 1u : 0u;
    k.ls = ((k.nl << 1) | prev_nl) & k.valid;
    if (begin >= at && begin < at + 16) k.ls |= 1u << (unsigned)(begin - at);      // the range's first byte starts a line
    k.gt = gt & k.ls;
    k.bad = bad & k.ls;
}
// the bytes of the chunk from line start `b` (a single bit of ls) up to the next line start
__device__ __forceinline__ uint32_t fx_piece(uint32_t ls, uint32_t b) {
    const uint32_t above = ls & ~(b | (b - 1u));
    const uint32_t next = above ? (above & (0u - above)) : 0x10000u;
    return (next - 1u) & ~(b - 1u);
}
__device__ __forceinline__ uint32_t fx_piece0(uint32_t ls) { return ls ? ((ls & (0u - ls)) - 1u) : 0xFFFFu; }

__global__ __launch_bounds__(FX_THREADS) void fastx_classify_kernel(const uint8_t *d, uint64_t begin, uint64_t end, uint64_t a0, FxTileSum *sums) {
    __shared__ uint64_t lds64[4];
    __shared__ uint32_t lds32[4];
    __shared__ uint32_t acc[8];             // head, cnt[4], lnb
    const bool fq = d[begin] == '@';
    const unsigned tid = threadIdx.x;
    if (tid < 8) acc[tid] = 0;
    __syncthreads();
    uint32_t run_ls = 0, run_hdr = 0, run_cls = 0, tail = 0;
    for (int s = 0; s < FX_SUB; s++) {
        const uint64_t at = a0 + (uint64_t)blockIdx.x * FX_TILE + ((uint64_t)s * FX_THREADS + tid) * 16;
        FxChunk k;
        fx_load(d, at, begin, end, k);
        const uint32_t nls = __popc(k.ls), nhdr = __popc(k.gt);
        uint64_t tot;
        const uint64_t ex = fx_block_excl<uint64_t, false>((uint64_t)nls | ((uint64_t)nhdr << 32), &tot, lds64);
        const uint32_t P = run_ls + (uint32_t)ex;                   // line starts of the tile in front of this chunk
        const uint32_t nonws = k.valid & ~k.ws;
        uint32_t head = 0, c[4] = {0, 0, 0, 0};
        if (fq) {
            const uint32_t p0 = __popc(nonws & fx_piece0(k.ls));
            if (P == 0) head += p0; else c[P & 3u] += p0;
            uint32_t m = k.ls, idx = P;
            while (m) {
                const uint32_t b = m & (0u - m);
                m ^= b;
                idx++;
                c[idx & 3u] += __popc(nonws & fx_piece(k.ls, b));
            }
            const uint32_t nb = k.valid & ~(k.nl | k.cr);
            if (nb) {
                const int j = 31 - __clz((int)nb);
                atomicMax(&acc[5], P + __popc(k.ls & ((2u << j) - 1u)) + 1u);
            }
        } else {
            const uint32_t mine = k.ls ? (((k.gt >> (31 - __clz((int)k.ls))) & 1u) ? 2u : 1u) : 0u;
            uint32_t totm;
            const uint32_t exm = fx_block_excl<uint32_t, true>(mine ? (((tid + 1u) << 2) | mine) : 0u, &totm, lds32);
            const uint32_t open = exm ? (exm & 3u) : run_cls;       // 0: the line began in front of the tile
            const uint32_t p0 = __popc(nonws & fx_piece0(k.ls));
            if (open == 0) head += p0; else if (open == 1) c[0] += p0;
            uint32_t m = k.ls & ~k.gt;
            while (m) {
                const uint32_t b = m & (0u - m);
                m ^= b;
                c[0] += __popc(nonws & fx_piece(k.ls, b));
            }
            if (totm) { run_cls = totm & 3u; tail = run_cls; }
        }
        if (head) atomicAdd(&acc[0], head);
#pragma unroll
        for (int i = 0; i < 4; i++) if (c[i]) atomicAdd(&acc[1 + i], c[i]);
        run_ls += (uint32_t)tot;
        run_hdr += (uint32_t)(tot >> 32);
    }
    __syncthreads();
    if (tid == 0) {
        FxTileSum t;
        t.nls = run_ls; t.nhdr = run_hdr; t.head = acc[0];
        t.cnt[0] = acc[1]; t.cnt[1] = acc[2]; t.cnt[2] = acc[3]; t.cnt[3] = acc[4];
        t.tail = tail; t.lnb = acc[5];
        sums[blockIdx.x] = t;
    }
}

// one block: what lies in front of every tile, and the totals
__global__ __launch_bounds__(FX_THREADS) void fastx_tiles_kernel(const uint8_t *d, uint64_t begin, uint64_t end, const FxTileSum *sums, uint64_t n_tiles,
                                                                 FxTileCarry *carries, uint64_t *totals) {
    __shared__ uint64_t lds64[4];
    __shared__ uint32_t lds32[4];
    const bool fq = d[begin] == '@';
    const unsigned tid = threadIdx.x;
    uint64_t run_lines = 0, run_hdrs = 0, run_kept = 0, run_lnb = 0;
    uint32_t run_cls = 1;
    for (uint64_t base = 0; base < n_tiles; base += FX_THREADS) {
        const uint64_t t = base + tid;
        FxTileSum s{};
        if (t < n_tiles) s = sums[t];
        uint64_t tot_l, tot_h, tot_k, tot_b;
        const uint64_t lb = run_lines + fx_block_excl<uint64_t, false>(s.nls, &tot_l, lds64);
        const uint64_t hb = run_hdrs + fx_block_excl<uint64_t, false>(s.nhdr, &tot_h, lds64);
        uint64_t kept;
        uint32_t open = 0;
        if (fq) {
            // the tile's k-th line start is line lb + k - 1 of the text; sequence lines are those with index 1 modulo 4
            kept = ((lb & 3u) == 2u ? s.head : 0u) + (uint64_t)s.cnt[(2u - (uint32_t)lb) & 3u];
        } else {
            uint32_t totm;
            const uint32_t exm = fx_block_excl<uint32_t, true>(s.nls ? (((tid + 1u) << 2) | s.tail) : 0u, &totm, lds32);
            open = exm ? (exm & 3u) : run_cls;
            kept = (open == 1u ? s.head : 0u) + (uint64_t)s.cnt[0];
            if (totm) run_cls = totm & 3u;
        }
        const uint64_t kb = run_kept + fx_block_excl<uint64_t, false>(kept, &tot_k, lds64);
        (void)fx_block_excl<uint64_t, true>(s.lnb ? lb + s.lnb - 1 : 0, &tot_b, lds64);
        if (tot_b > run_lnb) run_lnb = tot_b;
        if (t < n_tiles) {
            FxTileCarry c;
            c.lines = lb; c.hdrs = hb; c.kept = kb; c.open = open; c.pad = 0;
            carries[t] = c;
        }
        run_lines += tot_l; run_hdrs += tot_h; run_kept += tot_k;
    }
    if (tid == 0) {
        totals[0] = run_lines; totals[1] = run_hdrs; totals[2] = run_kept; totals[3] = run_lnb;
        totals[4] = d[begin]; totals[5] = d[end - 1] == '\n' ? 1 : 0;
    }
}

__global__ void fastx_init_kernel(uint64_t *boff, uint64_t n_rec, uint64_t n_kept, uint64_t *lstart, uint64_t n_lstart, uint64_t sentinel, uint64_t *state) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = i; j < n_lstart; j += step) lstart[j] = sentinel;
    if (i == 0) { boff[n_rec] = n_kept; state[0] = FX_NO_BAD; state[1] = 0; state[2] = 0; }
}

// The tiles again with their carries: base characters to asc[], record starts to boff[], FASTQ line starts to lstart[].
__global__ __launch_bounds__(FX_THREADS) void fastx_apply_kernel(const uint8_t *d, uint64_t begin, uint64_t end, uint64_t a0, const FxTileCarry *carries,
                                                                 uint64_t n_rec, uint64_t n_kept, uint8_t *asc, uint64_t *boff, uint64_t *lstart,
                                                                 uint64_t *state) {
    __shared__ uint64_t lds64[4];
    __shared__ uint32_t lds32[4];
    const bool fq = d[begin] == '@';
    const unsigned tid = threadIdx.x;
    const FxTileCarry cr = carries[blockIdx.x];
    uint64_t run_ls = cr.lines, run_hdr = cr.hdrs, run_kept = cr.kept;
    uint32_t run_cls = cr.open;
    for (int s = 0; s < FX_SUB; s++) {
        const uint64_t at = a0 + (uint64_t)blockIdx.x * FX_TILE + ((uint64_t)s * FX_THREADS + tid) * 16;
        FxChunk k;
        fx_load(d, at, begin, end, k);
        const uint32_t nls = __popc(k.ls), nhdr = __popc(k.gt);
        uint64_t tot;
        const uint64_t ex = fx_block_excl<uint64_t, false>((uint64_t)nls | ((uint64_t)nhdr << 32), &tot, lds64);
        const uint64_t P = run_ls + (uint32_t)ex;                   // line starts of the text in front of this chunk
        const uint64_t H = run_hdr + (uint32_t)(ex >> 32);
        const uint32_t nonws = k.valid & ~k.ws;
        uint32_t keep = 0;
        if (fq) {
            if (((P - 1) & 3u) == 1u) keep |= nonws & fx_piece0(k.ls);          // (P = 0: nothing lies in front of the first line start)
            uint32_t m = k.ls;
            uint64_t g = P;
            while (m) {
                const uint32_t b = m & (0u - m);
                m ^= b;
                if ((g & 3u) == 1u) keep |= nonws & fx_piece(k.ls, b);
                g++;
            }
        } else {
            const uint32_t mine = k.ls ? (((k.gt >> (31 - __clz((int)k.ls))) & 1u) ? 2u : 1u) : 0u;
            uint32_t totm;
            const uint32_t exm = fx_block_excl<uint32_t, true>(mine ? (((tid + 1u) << 2) | mine) : 0u, &totm, lds32);
            const uint32_t open = exm ? (exm & 3u) : run_cls;
            if (open == 1u) keep |= nonws & fx_piece0(k.ls);
            uint32_t m = k.ls & ~k.gt;
            while (m) {
                const uint32_t b = m & (0u - m);
                m ^= b;
                keep |= nonws & fx_piece(k.ls, b);
            }
            if (totm) run_cls = totm & 3u;
        }
        uint32_t totk;
        const uint64_t base = run_kept + fx_block_excl<uint32_t, false>((uint32_t)__popc(keep), &totk, lds32);
        // the characters
        {
            uint64_t o = base;
            uint32_t m = keep;
            while (m) {
                const int j = __ffs((int)m) - 1;
                m &= m - 1u;
                if (o < n_kept) asc[o] = (uint8_t)k.byte(j);
                o++;
            }
        }
        // the line starts
        {
            uint32_t m = k.ls;
            uint64_t g = P, h = H;
            while (m) {
                const int j = __ffs((int)m) - 1;
                const uint32_t b = 1u << j;
                m ^= b;
                const uint64_t at_base = base + (uint32_t)__popc(keep & (b - 1u));
                if (fq) {
                    if (g <= 4 * n_rec) lstart[g] = at + j;
                    if ((g & 3u) == 0 && (g >> 2) < n_rec) boff[g >> 2] = at_base;
                } else if (k.gt & b) {
                    if (h < n_rec) boff[h] = at_base;
                    h++;
                } else if (k.bad & b) {
                    atomicMin(reinterpret_cast<unsigned long long *>(&state[0]), (unsigned long long)((g << 3) | 1u));
                }
                g++;
            }
        }
        run_ls += (uint32_t)tot;
        run_hdr += (uint32_t)(tot >> 32);
        run_kept += totk;
    }
}

// bytes of line l without its \n and one trailing \r (lines past the text's last are empty)
__device__ __forceinline__ uint64_t fx_line_len(const uint8_t *d, const uint64_t *lstart, uint64_t l, uint64_t n_lines) {
    if (l >= n_lines) return 0;
    const uint64_t s = lstart[l], e = lstart[l + 1];
    uint64_t n = e > s ? e - s - 1 : 0;
    if (n && d[s + n - 1] == '\r') n--;
    return n;
}

__global__ __launch_bounds__(256) void fastx_records_kernel(const uint8_t *d, const uint64_t *boff, const uint64_t *lstart, uint64_t n_rec, uint64_t n_lines,
                                                            int fq, uint32_t *len, uint32_t *wcnt, uint64_t *state) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    const uint64_t L = boff[r + 1] - boff[r];
    uint32_t *flags = reinterpret_cast<uint32_t *>(&state[1]);
    if (L > 0xFFFFFFF0ull) {
        atomicOr(flags, 256u);
        atomicMin(reinterpret_cast<unsigned long long *>(&state[0]), (unsigned long long)((r << 3) | 5u));
        len[r] = 0; wcnt[r] = 0;
        return;
    }
    len[r] = (uint32_t)L;
    wcnt[r] = (uint32_t)(((L + 63) / 64) * 2);
    atomicMax(reinterpret_cast<uint32_t *>(&state[2]), (uint32_t)L);
    if (!fq) return;
    uint64_t bad = FX_NO_BAD;
    if (fx_line_len(d, lstart, 4 * r + 1, n_lines) != fx_line_len(d, lstart, 4 * r + 3, n_lines)) bad = ((4 * r + 3) << 3) | 4u;
    if (4 * r + 2 >= n_lines || d[lstart[4 * r + 2]] != '+') bad = ((4 * r + 2) << 3) | 3u;
    if (d[lstart[4 * r]] != '@') bad = ((4 * r) << 3) | 2u;
    if (bad != FX_NO_BAD) atomicMin(reinterpret_cast<unsigned long long *>(&state[0]), (unsigned long long)bad);
}

// One wave per read over the contiguous characters; a lane packs 32 of them from nine aligned words.  The bits are those of
// pack_ascii_kernel (reads.hip): code (c >> 1) & 3 (utils/kmer/Kmer.hpp:462), invalid = bit 3, break = another character with the same
// code and invalid bit as the one before it (Commons.hpp:4177-4178).  asc has 16 bytes in front of it and 64 behind.
__global__ __launch_bounds__(256) void fastx_pack_kernel(const uint8_t *asc, const uint64_t *boff, const uint64_t *word_off, uint32_t n_reads,
                                                         uint64_t *words, uint32_t *invalid, uint32_t *brk, uint32_t *any_flags, uint8_t *masked) {
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    uint32_t seen = 0, seen_brk = 0;
    for (uint64_t r = wave; r < n_reads; r += nwaves) {
        const uint64_t b_r = boff[r], L = boff[r + 1] - b_r;
        const uint64_t w0 = word_off[r], nw = word_off[r + 1] - w0;
        uint32_t mine = 0;
        for (uint64_t w = lane; w < nw; w += 64) {
            uint64_t x = 0;
            uint32_t inv = 0, bk = 0;
            const uint64_t b0 = w * 32;
            if (b0 < L) {
                const uintptr_t q = reinterpret_cast<uintptr_t>(asc + b_r + b0) - 1;      // the character in front of the word's first
                const uint32_t sh = (uint32_t)(q & 3u) * 8u;
                const uint32_t *p = reinterpret_cast<const uint32_t *>(q & ~(uintptr_t)3);
                uint32_t dw[10];
#pragma unroll
                for (int j = 0; j < 9; j++) dw[j] = p[j];
                dw[9] = 0;
                uint32_t e[9];
#pragma unroll
                for (int j = 0; j < 9; j++) e[j] = (uint32_t)((((uint64_t)dw[j + 1] << 32) | dw[j]) >> sh);
                const uint32_t nvalid = L - b0 < 32 ? (uint32_t)(L - b0) : 32u;
                uint32_t prev = e[0] & 255u;
#pragma unroll
                for (int i = 0; i < 32; i++) {
                    const uint32_t c = (e[(i + 1) >> 2] >> (8 * ((i + 1) & 3))) & 255u;
                    if ((uint32_t)i < nvalid) {
                        x |= (uint64_t)((c >> 1) & 3u) << (2 * i);
                        inv |= ((c >> 3) & 1u) << i;
                        if ((i > 0 || b0 > 0) && c != prev && ((c ^ prev) & 0x0Eu) == 0) bk |= 1u << i;
                        prev = c;
                    }
                }
            }
            words[w0 + w] = x;
            invalid[w0 + w] = inv;
            brk[w0 + w] = bk;
            seen |= inv;
            seen_brk |= bk;
            mine |= inv | bk;
        }
        const bool any = __ballot(mine != 0u) != 0ull;
        if (lane == 0) masked[r] = any ? 1 : 0;
    }
    if (seen) atomicOr(any_flags, 1u);
    if (seen_brk) atomicOr(any_flags, 2u);
}

// FASTQ: the quality line of every read to its place (the read's base offset); one wave per read.  A quality whose base character
// was stripped (space, tab, \r inside the sequence line) goes with it.
__global__ __launch_bounds__(256) void fastx_quality_kernel(const uint8_t *d, const uint64_t *boff, const uint64_t *lstart, uint32_t n_reads, uint64_t n_lines,
                                                            const uint64_t *state, uint8_t *qual) {
    if (state[0] != FX_NO_BAD) return;                       // a refused text: nothing is built
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = wave; r < n_reads; r += nwaves) {
        const uint64_t n = boff[r + 1] - boff[r];
        const uint64_t Ls = fx_line_len(d, lstart, 4 * r + 1, n_lines), Lq = fx_line_len(d, lstart, 4 * r + 3, n_lines);
        if (Ls != Lq || n > Ls || n == 0) continue;
        const uint8_t *src = d + lstart[4 * r + 3];
        uint8_t *dst = qual + boff[r];
        if (n == Ls) {
            for (uint64_t j = lane; j < n; j += 64) dst[j] = src[j];
        } else if (lane == 0) {
            const uint8_t *seq = d + lstart[4 * r + 1];
            uint64_t o = 0;
            for (uint64_t j = 0; j < Ls && o < n; j++) {
                const uint8_t c = seq[j];
                if (c != '\r' && c != ' ' && c != '\t') dst[o++] = src[j];
            }
        }
    }
}

}  // namespace mdbg

using namespace mdbg;

extern "C" int mdbg_reads_from_fastx_bytes(mdbg_ctx *ctx, const mdbg_bytes *text, uint64_t begin, uint64_t end, mdbg_reads **out, uint64_t info[4]) try {
    if (!ctx || !text || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_reads_from_fastx_bytes: null argument");
    if (begin > end || end > text->n)
        return set_error(ctx, MDBG_EINVAL, "mdbg_reads_from_fastx_bytes: [%llu, %llu) lies outside the %llu bytes of the buffer", (unsigned long long)begin,
                         (unsigned long long)end, (unsigned long long)text->n);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<mdbg_reads> r(new mdbg_reads());
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (begin == end) {
        MDBG_TRY(r->d_words.alloc(ctx, 0));
        MDBG_TRY(r->d_word_off.alloc(ctx, 1));
        MDBG_TRY(r->d_len.alloc(ctx, 0));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(r->d_word_off.p, 0, 8, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        *out = r.release();
        return MDBG_OK;
    }
    const uint8_t *d = text->d.p;
    const uint64_t a0 = begin & ~15ull;
    const uint64_t n_tiles = (end - a0 + FX_TILE - 1) / FX_TILE;
    if (n_tiles >= (1ull << 31)) return set_error(ctx, MDBG_ERANGE, "mdbg_reads_from_fastx_bytes: a range of %llu bytes is too long for one call", (unsigned long long)(end - begin));
    DevBuf<FxTileSum> d_sums;
    DevBuf<FxTileCarry> d_carries;
    DevBuf<uint64_t> d_totals, d_state;
    MDBG_TRY(d_sums.alloc(ctx, n_tiles));
    MDBG_TRY(d_carries.alloc(ctx, n_tiles));
    MDBG_TRY(d_totals.alloc(ctx, FX_TOTALS));
    MDBG_TRY(d_state.alloc(ctx, 4));
    MDBG_TRY(bytes_ready_on(ctx, text));                     // uploads still in flight: the kernels run behind them
    {
        LaunchTimer timer(ctx, "fastx_classify");
        hipLaunchKernelGGL(fastx_classify_kernel, dim3((unsigned)n_tiles), dim3(FX_THREADS), 0, ctx->stream, d, begin, end, a0, d_sums.p);
        hipLaunchKernelGGL(fastx_tiles_kernel, dim3(1), dim3(FX_THREADS), 0, ctx->stream, d, begin, end, d_sums.p, n_tiles, d_carries.p, d_totals.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    // the one copy that sizes everything: lines, records, base characters
    uint64_t tot[FX_TOTALS];
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, tot, d_totals.p, sizeof tot, hipMemcpyDeviceToHost));
    const int first = (int)tot[4];
    if (first != '>' && first != '@')
        return set_error(ctx, MDBG_EINVAL, "mdbg_reads_from_fastx_bytes: the text must begin with '>' or '@' (a whole number of records), not with byte 0x%02x", first);
    const bool fq = first == '@';
    const uint64_t n_lines = tot[0], n_kept = tot[2];
    const uint64_t n_rec = fq ? (tot[3] + 3) / 4 : tot[1];
    if (n_rec > 0xFFFFFFFFull) return set_error(ctx, MDBG_ERANGE, "mdbg_reads_from_fastx_bytes: %llu records in one call", (unsigned long long)n_rec);
    const uint32_t n_reads = (uint32_t)n_rec;
    const uint64_t words_bound = n_kept / 32 + 2 * n_rec + 2;      // words_for(L) <= L / 32 + 2
    const uint64_t n_lstart = fq ? 4 * n_rec + 2 : 0;
    DevBuf<uint64_t> d_boff, d_lstart;
    DevBuf<uint32_t> d_wcnt;
    DevBuf<uint8_t> d_asc;
    MDBG_TRY(d_boff.alloc(ctx, n_rec + 1));
    MDBG_TRY(d_lstart.alloc(ctx, n_lstart));
    MDBG_TRY(d_wcnt.alloc(ctx, n_rec));
    MDBG_TRY(d_asc.alloc(ctx, n_kept + 16 + 64));
    // words and side masks are allocated before the exact count is known: the buffers hold words_bound elements, of which the
    // first r->n_words are the reads' (a consumer goes by n_words and d_word_off, never by a buffer's size)
    MDBG_TRY(r->d_words.alloc(ctx, words_bound));
    MDBG_TRY(r->d_invalid.alloc(ctx, words_bound));
    MDBG_TRY(r->d_break.alloc(ctx, words_bound));
    MDBG_TRY(r->d_word_off.alloc(ctx, n_rec + 1));
    MDBG_TRY(r->d_len.alloc(ctx, n_rec));
    MDBG_TRY(r->d_masked.alloc(ctx, n_rec));
    uint8_t *asc = d_asc.p + 16;
    uint32_t *any_flags = reinterpret_cast<uint32_t *>(d_state.p + 1);
    {
        LaunchTimer timer(ctx, "fastx_records");
        // a line past the text's last starts where a \n after the last byte would put it
        hipLaunchKernelGGL(fastx_init_kernel, dim3(grid_for(n_lstart, 256, (unsigned)ctx->n_cu * 8u)), dim3(256), 0, ctx->stream, d_boff.p, n_rec, n_kept,
                           d_lstart.p, n_lstart, tot[5] ? end : end + 1, d_state.p);
        hipLaunchKernelGGL(fastx_apply_kernel, dim3((unsigned)n_tiles), dim3(FX_THREADS), 0, ctx->stream, d, begin, end, a0, d_carries.p, n_rec, n_kept, asc,
                           d_boff.p, d_lstart.p, d_state.p);
        if (n_rec)
            hipLaunchKernelGGL(fastx_records_kernel, dim3(grid_for(n_rec, 256)), dim3(256), 0, ctx->stream, d, d_boff.p, d_lstart.p, n_rec, n_lines, fq ? 1 : 0,
                               r->d_len.p, d_wcnt.p, d_state.p);
    }
    MDBG_TRY(exclusive_scan_u32(ctx, d_wcnt.p, r->d_word_off.p, n_rec));
    // (as mdbg_reads_from_ascii, which attaches qualities only when the batch holds a base: `if (quals && nb)`)
    const bool with_qual = fq && n_kept > 0;
    if (with_qual) {
        MDBG_TRY(r->d_qual.alloc(ctx, n_kept + 32));           // + 32: kernels read whole 16-byte pieces
        MDBG_TRY(r->d_qual_off.alloc(ctx, n_rec + 1));
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(r->d_qual_off.p, d_boff.p, (n_rec + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (n_rec) {
        const unsigned blocks = grid_for(n_rec * 64, 256, (unsigned)ctx->n_cu * 16u);
        LaunchTimer timer(ctx, "fastx_pack");
        hipLaunchKernelGGL(fastx_pack_kernel, dim3(blocks), dim3(256), 0, ctx->stream, asc, d_boff.p, r->d_word_off.p, n_reads, r->d_words.p, r->d_invalid.p,
                           r->d_break.p, any_flags, r->d_masked.p);
        if (with_qual)
            hipLaunchKernelGGL(fastx_quality_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d, d_boff.p, d_lstart.p, n_reads, n_lines, d_state.p, r->d_qual.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    uint64_t state[3] = {0, 0, 0}, n_words = 0;
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(state, d_state.p, sizeof state, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &n_words, r->d_word_off.p + n_rec, 8, hipMemcpyDeviceToHost));
    if (state[0] != FX_NO_BAD) {
        const unsigned long long where = (unsigned long long)(state[0] >> 3) + 1;
        switch ((int)(state[0] & 7u)) {
            case 1: return set_error(ctx, MDBG_EINVAL, "mdbg_reads_from_fastx_bytes: FASTA line %llu starts with '@' or '+' (a format switch inside the text is not guessed at)", where);
            case 2: return set_error(ctx, MDBG_EINVAL, "mdbg_reads_from_fastx_bytes: FASTQ line %llu should start a record with '@' (four lines per record; multi-line FASTQ is refused)", where);
            case 3: return set_error(ctx, MDBG_EINVAL, "mdbg_reads_from_fastx_bytes: FASTQ line %llu should start with '+' (four lines per record; multi-line or truncated FASTQ is refused)", where);
            case 4: return set_error(ctx, MDBG_EINVAL, "mdbg_reads_from_fastx_bytes: FASTQ line %llu: the quality line is not as long as the sequence line", where);
            default: return set_error(ctx, MDBG_ERANGE, "read %llu longer than 2^32 bases", where - 1);
        }
    }
    const uint32_t any = (uint32_t)state[1] & 3u;
    r->n_reads = n_reads;
    r->n_bases = n_kept;
    r->n_words = n_words;
    r->max_len = (uint32_t)state[2];
    r->has_qual = with_qual;
    r->has_break = (any & 2u) != 0;
    r->has_invalid = any != 0;
    if (!r->has_invalid) { r->d_invalid.release(); r->d_masked.release(); }
    if (!r->has_break) r->d_break.release();
    if (r->has_invalid) {                 // the ascending list of masked reads, from the flags as mdbg_reads_from_ascii builds it
        std::vector<uint8_t> flag(n_reads);
        MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, flag.data(), r->d_masked.p, n_reads, hipMemcpyDeviceToHost));
        std::vector<uint32_t> list;
        for (uint32_t i = 0; i < n_reads; i++) if (flag[i]) list.push_back(i);
        r->n_masked = (uint32_t)list.size();
        MDBG_TRY(r->d_masked_list.alloc(ctx, list.size()));
        if (!list.empty()) MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, r->d_masked_list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice));
    }
    if (info) { info[0] = fq ? 1 : 0; info[1] = n_reads; info[2] = n_kept; info[3] = r->n_masked; }
    *out = r.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)
