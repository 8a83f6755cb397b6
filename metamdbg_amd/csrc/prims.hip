// prims.hip -- small device-wide primitives: exclusive scan (reduce / scan / apply).
// Used for CSR offsets (minimizers per read, instances per read, flags -> output rows).
#include "common.hpp"
#include "objects.hpp"

#include <algorithm>

namespace mdbg {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

__device__ __forceinline__ uint64_t block_exclusive_sum(uint64_t v, uint64_t *total, uint64_t *lds /* 4 */) {
    // wave inclusive scan of 64-bit values, then combine the 4 waves through LDS
    unsigned lane = lane_id(), wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint64_t t = __shfl_up(inc, d, 64);
        if (lane >= (unsigned)d) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint64_t w0 = lds[0], w1 = lds[1], w2 = lds[2], w3 = lds[3];
    uint64_t base = (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0);
    *total = w0 + w1 + w2 + w3;
    __syncthreads();
    return base + inc - v;
}

// A block owns a tile of SCAN_TILE items and walks it in SCAN_SUB sub-tiles of 4 items per thread, so that every
// load is one 16-byte (u32 input) access per lane and every store two 16-byte accesses per lane: fully coalesced.
constexpr int SCAN_VEC = 4;
constexpr int SCAN_SUB = SCAN_ITEMS / SCAN_VEC;

template <typename Tin>
__device__ __forceinline__ void load_vec(const Tin *in, uint64_t idx, uint64_t n, uint64_t v[SCAN_VEC]) {
    if (idx + SCAN_VEC <= n && (reinterpret_cast<uintptr_t>(in + idx) & (sizeof(Tin) * SCAN_VEC - 1)) == 0) {
        if (sizeof(Tin) == 4) {
            const uint4 q = *reinterpret_cast<const uint4 *>(in + idx);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            const ulonglong2 q0 = *reinterpret_cast<const ulonglong2 *>(in + idx), q1 = *reinterpret_cast<const ulonglong2 *>(in + idx + 2);
            v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < SCAN_VEC; i++) v[i] = idx + i < n ? (uint64_t)in[idx + i] : 0ull;
    }
}

template <typename Tin>
__global__ __launch_bounds__(SCAN_THREADS) void scan_reduce_kernel(const Tin *in, uint64_t n, uint64_t *block_sums, uint32_t prio) {
    raise_wave_priority(prio);
    __shared__ uint64_t lds[4];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    uint64_t s = 0;
#pragma unroll
    for (int t = 0; t < SCAN_SUB; t++) {
        uint64_t v[SCAN_VEC];
        load_vec(in, base + ((uint64_t)t * SCAN_THREADS + threadIdx.x) * SCAN_VEC, n, v);
        s += v[0] + v[1] + v[2] + v[3];
    }
    uint64_t total;
    block_exclusive_sum(s, &total, lds);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// single block: exclusive scan of m <= arbitrary values, sequential over tiles
__global__ __launch_bounds__(SCAN_THREADS) void scan_small_kernel(uint64_t *vals, uint64_t m, uint32_t prio) {
    raise_wave_priority(prio);
    __shared__ uint64_t lds[4];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < m; base += SCAN_THREADS) {
        uint64_t idx = base + threadIdx.x;
        uint64_t v = idx < m ? vals[idx] : 0;
        uint64_t total;
        uint64_t ex = block_exclusive_sum(v, &total, lds);
        if (idx < m) vals[idx] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) vals[m] = carry;
}

template <typename Tin>
__global__ __launch_bounds__(SCAN_THREADS) void scan_apply_kernel(const Tin *in, uint64_t n, const uint64_t *block_offsets,
                                                                  uint64_t *out, uint32_t prio) {
    raise_wave_priority(prio);
    __shared__ uint64_t lds[4];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    uint64_t carry = block_offsets[blockIdx.x];
#pragma unroll
    for (int t = 0; t < SCAN_SUB; t++) {
        const uint64_t idx = base + ((uint64_t)t * SCAN_THREADS + threadIdx.x) * SCAN_VEC;
        uint64_t v[SCAN_VEC];
        load_vec(in, idx, n, v);
        uint64_t total;
        uint64_t ex = block_exclusive_sum(v[0] + v[1] + v[2] + v[3], &total, lds) + carry;
        if (idx + SCAN_VEC <= n) {                       // out is 8-byte aligned and idx a multiple of 4: 32-byte aligned stores
            ulonglong2 o0, o1;
            o0.x = ex; o0.y = ex + v[0]; o1.x = ex + v[0] + v[1]; o1.y = ex + v[0] + v[1] + v[2];
            if ((reinterpret_cast<uintptr_t>(out) & 15) == 0) {
                *reinterpret_cast<ulonglong2 *>(out + idx) = o0;
                *reinterpret_cast<ulonglong2 *>(out + idx + 2) = o1;
            } else { out[idx] = o0.x; out[idx + 1] = o0.y; out[idx + 2] = o1.x; out[idx + 3] = o1.y; }
        } else {
            uint64_t e = ex;
#pragma unroll
            for (int i = 0; i < SCAN_VEC; i++) { if (idx + i < n) out[idx + i] = e; e += v[i]; }
        }
        carry += total;
    }
    // the total: written by the block that owns item n-1, once its last sub-tile is done
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = carry;
}

template <typename Tin>
static int exclusive_scan_impl(mdbg_ctx *ctx, const Tin *d_in, uint64_t *d_out, uint64_t n) {
    if (n == 0) {
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(d_out, 0, sizeof(uint64_t), ctx->stream));
        return MDBG_OK;
    }
    uint64_t nblocks = (n + SCAN_TILE - 1) / SCAN_TILE;
    DevBuf<uint64_t> sums;
    MDBG_TRY(sums.alloc(ctx, nblocks + 1));
    LaunchTimer timer(ctx, "prefix_scan");
    const uint32_t prio = table_priority(ctx);
    hipLaunchKernelGGL(scan_reduce_kernel<Tin>, dim3((unsigned)nblocks), dim3(SCAN_THREADS), 0, ctx->stream, d_in, n, sums.p, prio);
    if (nblocks <= ctx->prefix_small_limit) {                // 65536 unless a test lowered it ("prefix_small_limit")
        hipLaunchKernelGGL(scan_small_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, sums.p, nblocks, prio);
    } else {
        // two-level: scan the block sums recursively (u64 input)
        DevBuf<uint64_t> tmp;
        MDBG_TRY(tmp.alloc(ctx, nblocks + 1));
        MDBG_TRY(exclusive_scan_impl<uint64_t>(ctx, sums.p, tmp.p, nblocks));
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(sums.p, tmp.p, (nblocks + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    hipLaunchKernelGGL(scan_apply_kernel<Tin>, dim3((unsigned)nblocks), dim3(SCAN_THREADS), 0, ctx->stream, d_in, n, sums.p, d_out, prio);
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    // no synchronisation: `sums` returns to the context's pool, whose blocks are only ever handed to later work on
    // the same stream, i.e. after the kernels above
    return MDBG_OK;
}

int exclusive_scan_u32(mdbg_ctx *ctx, const uint32_t *d_in, uint64_t *d_out, uint64_t n) {
    return exclusive_scan_impl<uint32_t>(ctx, d_in, d_out, n);
}

int exclusive_scan_u64(mdbg_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, uint64_t n) {
    return exclusive_scan_impl<uint64_t>(ctx, d_in, d_out, n);
}

// ---- sort_u64_pairs: stable least-significant-digit radix sort of 64-bit keys with a 32-bit value ------------------------------------
// Eight bits a pass.  A block owns a tile of SORT_TILE consecutive items, a wave a quarter of it, a lane item (round * 64 + lane) of its
// wave's quarter -- so "earlier in the input" is (block, wave, round, lane) order, and a pass keeps that order inside every digit:
//   the count     a block's 256-bin histogram in LDS, stored digit-major (hist[digit * blocks + block]);
//   the places    ONE device-wide exclusive scan over that array: digit-major order makes the scanned value the global place of the
//                 block's first key of the digit;
//   the scatter   a block counts again per wave, turns the four histograms into four rows of running places, and every wave walks its
//                 rounds in order: the lanes that hold one digit find each other by eight ballots, take consecutive places by lane
//                 order, and the last of them moves the row's place on.
// LDS atomics only (the counts; their order does not matter), no global atomics.  A digit in which all keys agree is skipped: the AND
// and the OR of all keys, reduced up front, differ in a byte exactly when some key differs there (a min / max pair would only find the
// constant HIGH digits).  The passes alternate between the caller's arrays and a pooled pair; an odd number ends with one copy back.
constexpr int SORT_THREADS = 256;
constexpr int SORT_ROUNDS = 16;
constexpr uint32_t SORT_WAVE_ITEMS = 64u * SORT_ROUNDS;
constexpr uint32_t SORT_TILE = 4u * SORT_WAVE_ITEMS;

__global__ __launch_bounds__(SORT_THREADS) void sort_bits_kernel(const uint64_t *keys, uint64_t n, uint64_t *partial) {
    __shared__ uint64_t lds[8];
    uint64_t all = ~0ull, any = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * SORT_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SORT_THREADS) {
        const uint64_t k = keys[i];
        all &= k; any |= k;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { all &= __shfl_xor(all, d, 64); any |= __shfl_xor(any, d, 64); }
    if (lane_id() == 0) { lds[threadIdx.x >> 6] = all; lds[4 + (threadIdx.x >> 6)] = any; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2u * blockIdx.x] = lds[0] & lds[1] & lds[2] & lds[3];
        partial[2u * blockIdx.x + 1u] = lds[4] | lds[5] | lds[6] | lds[7];
    }
}

// one block: the partial pairs of sort_bits_kernel folded into out[0] (AND), out[1] (OR)
__global__ __launch_bounds__(SORT_THREADS) void sort_bits_fold_kernel(const uint64_t *partial, uint32_t n_partial, uint64_t *out) {
    __shared__ uint64_t lds[8];
    uint64_t all = ~0ull, any = 0ull;
    for (uint32_t i = threadIdx.x; i < n_partial; i += SORT_THREADS) { all &= partial[2u * i]; any |= partial[2u * i + 1u]; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { all &= __shfl_xor(all, d, 64); any |= __shfl_xor(any, d, 64); }
    if (lane_id() == 0) { lds[threadIdx.x >> 6] = all; lds[4 + (threadIdx.x >> 6)] = any; }
    __syncthreads();
    if (threadIdx.x == 0) { out[0] = lds[0] & lds[1] & lds[2] & lds[3]; out[1] = lds[4] | lds[5] | lds[6] | lds[7]; }
}

__global__ __launch_bounds__(SORT_THREADS) void sort_hist_kernel(const uint64_t *keys, uint64_t n, uint32_t shift, uint32_t n_blocks, uint32_t *hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE;
#pragma unroll 4
    for (uint32_t t = 0; t < SORT_TILE / SORT_THREADS; t++) {
        const uint64_t i = base + (uint64_t)t * SORT_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * n_blocks + blockIdx.x] = h[threadIdx.x];
}

// places: the scan of sort_hist_kernel's counts (n < 2^32: a place fits 32 bits)
__global__ __launch_bounds__(SORT_THREADS) void sort_scatter_kernel(const uint64_t *keys_in, const uint32_t *vals_in, uint64_t n, uint32_t shift, uint32_t n_blocks,
                                                                    const uint64_t *places, uint64_t *keys_out, uint32_t *vals_out) {
    __shared__ uint32_t row[4][256];                  // per wave: its count of a digit, then the place of its next key of that digit
    const uint32_t wave = threadIdx.x >> 6, lane = lane_id();
#pragma unroll
    for (uint32_t w = 0; w < 4u; w++) row[w][threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE + (uint64_t)wave * SORT_WAVE_ITEMS;
    for (uint32_t t = 0; t < SORT_ROUNDS; t++) {
        const uint64_t i = base + t * 64u + lane;
        if (i < n) atomicAdd(&row[wave][(uint32_t)(keys_in[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    {
        uint32_t run = (uint32_t)places[(uint64_t)threadIdx.x * n_blocks + blockIdx.x];
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) { const uint32_t c = row[w][threadIdx.x]; row[w][threadIdx.x] = run; run += c; }
    }
    __syncthreads();
    for (uint32_t t = 0; t < SORT_ROUNDS; t++) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < n;
        const uint64_t key = valid ? keys_in[i] : 0ull;
        const uint32_t val = valid ? vals_in[i] : 0u;
        const uint32_t d = (uint32_t)(key >> shift) & 255u;
        unsigned long long same = __ballot(valid);    // the valid lanes of this round that hold the digit d
#pragma unroll
        for (uint32_t b = 0; b < 8u; b++) {
            const unsigned long long set = __ballot((d >> b) & 1u);
            same &= (d >> b) & 1u ? set : ~set;
        }
        const uint32_t rank = (uint32_t)__popcll(same & lanemask_lt()), count = (uint32_t)__popcll(same);
        const uint32_t place = valid ? row[wave][d] + rank : 0u;
        wave_lds_sync();
        if (valid && rank + 1u == count) row[wave][d] = place + 1u;
        wave_lds_sync();
        if (valid) { keys_out[place] = key; vals_out[place] = val; }
    }
}

int sort_u64_pairs(mdbg_ctx *ctx, uint64_t *d_keys, uint32_t *d_vals, uint64_t n, uint32_t passes[2]) {
    if (passes) passes[0] = passes[1] = 0u;
    if (n >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "sort_u64_pairs: 2^32 items or more in one sort");
    if (n < 2) { if (passes) passes[1] = 8u; return MDBG_OK; }
    const uint32_t n_blocks = (uint32_t)((n + SORT_TILE - 1u) / SORT_TILE);
    const uint32_t n_partial = std::min<uint32_t>(n_blocks, (uint32_t)ctx->n_cu * 8u);
    DevBuf<uint64_t> partial, bits, keys_tmp, places;
    DevBuf<uint32_t> vals_tmp, hist;
    MDBG_TRY(partial.alloc(ctx, 2u * (size_t)n_partial));
    MDBG_TRY(bits.alloc(ctx, 2));
    LaunchTimer timer(ctx, "radix_sort");
    hipLaunchKernelGGL(sort_bits_kernel, dim3(n_partial), dim3(SORT_THREADS), 0, ctx->stream, d_keys, n, partial.p);
    hipLaunchKernelGGL(sort_bits_fold_kernel, dim3(1), dim3(SORT_THREADS), 0, ctx->stream, partial.p, n_partial, bits.p);
    uint64_t h_bits[2] = {0, 0};
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, h_bits, bits.p, 16, hipMemcpyDeviceToHost));
    const uint64_t differ = h_bits[0] ^ h_bits[1];
    if (differ == 0) { if (passes) passes[1] = 8u; return MDBG_OK; }
    MDBG_TRY(keys_tmp.alloc(ctx, n));
    MDBG_TRY(vals_tmp.alloc(ctx, n));
    MDBG_TRY(hist.alloc(ctx, 256u * (size_t)n_blocks));
    MDBG_TRY(places.alloc(ctx, 256u * (size_t)n_blocks + 1u));
    uint64_t *kin = d_keys, *kout = keys_tmp.p;
    uint32_t *vin = d_vals, *vout = vals_tmp.p;
    for (uint32_t shift = 0; shift < 64u; shift += 8u) {
        if (((differ >> shift) & 255u) == 0) { if (passes) passes[1]++; continue; }
        hipLaunchKernelGGL(sort_hist_kernel, dim3(n_blocks), dim3(SORT_THREADS), 0, ctx->stream, kin, n, shift, n_blocks, hist.p);
        MDBG_TRY(exclusive_scan_u32(ctx, hist.p, places.p, 256u * (uint64_t)n_blocks));
        hipLaunchKernelGGL(sort_scatter_kernel, dim3(n_blocks), dim3(SORT_THREADS), 0, ctx->stream, kin, vin, n, shift, n_blocks, places.p, kout, vout);
        std::swap(kin, kout);
        std::swap(vin, vout);
        if (passes) passes[0]++;
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    if (kin != d_keys) {
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d_keys, kin, n * 8u, hipMemcpyDeviceToDevice, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d_vals, vin, n * 4u, hipMemcpyDeviceToDevice, ctx->stream));
    }
    // no synchronisation: the pooled buffers go to later work on the same stream only
    return MDBG_OK;
}

const StepKernel *prims_step_kernels(uint32_t *n) {
    static const StepKernel k[] = {
        {"prefix_reduce", reinterpret_cast<const void *>(scan_reduce_kernel<uint32_t>), SCAN_THREADS, 1},
        {"prefix_small", reinterpret_cast<const void *>(scan_small_kernel), SCAN_THREADS, 1},
        {"prefix_apply", reinterpret_cast<const void *>(scan_apply_kernel<uint32_t>), SCAN_THREADS, 1},
        {"sort_bits", reinterpret_cast<const void *>(sort_bits_kernel), SORT_THREADS, 2},
        {"sort_bits_fold", reinterpret_cast<const void *>(sort_bits_fold_kernel), SORT_THREADS, 2},
        {"sort_hist", reinterpret_cast<const void *>(sort_hist_kernel), SORT_THREADS, 2},
        {"sort_scatter", reinterpret_cast<const void *>(sort_scatter_kernel), SORT_THREADS, 2},
    };
    *n = (uint32_t)(sizeof(k) / sizeof(k[0]));
    return k;
}

int bytes_ready_on(mdbg_ctx *ctx, const mdbg_bytes *b);      // minimizers.hip

}  // namespace mdbg

using namespace mdbg;

extern "C" int mdbg_bytes_prefix_sum(mdbg_ctx *ctx, const mdbg_bytes *in, uint64_t in_at, int width, uint64_t n, mdbg_bytes *out, uint64_t out_at) try {
    if (!ctx || !in || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_prefix_sum: null argument");
    if (width != 4 && width != 8) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_prefix_sum: width %d is neither 4 nor 8", width);
    const uint64_t w = (uint64_t)width;
    if (in_at % w) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_prefix_sum: in_at %llu is no multiple of the width %d", (unsigned long long)in_at, width);
    if (out_at % 8) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_prefix_sum: out_at %llu is no multiple of 8", (unsigned long long)out_at);
    if (in_at > in->n || n > (in->n - in_at) / w)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_prefix_sum: %llu values of %d bytes from %llu lie outside the %llu bytes of the input", (unsigned long long)n, width,
                         (unsigned long long)in_at, (unsigned long long)in->n);
    if (out_at > out->n || (out->n - out_at) / 8 < 1 || n > (out->n - out_at) / 8 - 1)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_prefix_sum: %llu + 1 sums from %llu lie outside the %llu bytes of the output", (unsigned long long)n,
                         (unsigned long long)out_at, (unsigned long long)out->n);
    if (in == out && n && in_at < out_at + 8 * (n + 1) && out_at < in_at + w * n)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_prefix_sum: the values at [%llu, +%llu) and the sums at [%llu, +%llu) of one buffer overlap", (unsigned long long)in_at,
                         (unsigned long long)(w * n), (unsigned long long)out_at, (unsigned long long)(8 * (n + 1)));
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_TRY(bytes_ready_on(ctx, in));                        // uploads still in flight: the kernels run behind them
    MDBG_TRY(bytes_ready_on(ctx, out));
    uint64_t *d_out = reinterpret_cast<uint64_t *>(out->d.p + out_at);
    if (width == 4) return exclusive_scan_u32(ctx, reinterpret_cast<const uint32_t *>(in->d.p + in_at), d_out, n);
    return exclusive_scan_u64(ctx, reinterpret_cast<const uint64_t *>(in->d.p + in_at), d_out, n);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_bytes_sort_u64_pairs(mdbg_ctx *ctx, mdbg_bytes *keys, uint64_t keys_at, mdbg_bytes *values, uint64_t values_at, uint64_t n, uint64_t info[2]) try {
    if (!ctx || !keys || !values) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_sort_u64_pairs: null argument");
    if (keys_at % 8) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_sort_u64_pairs: keys_at %llu is no multiple of 8", (unsigned long long)keys_at);
    if (values_at % 4) return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_sort_u64_pairs: values_at %llu is no multiple of 4", (unsigned long long)values_at);
    if (keys_at > keys->n || n > (keys->n - keys_at) / 8)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_sort_u64_pairs: %llu keys from %llu lie outside the %llu bytes of their buffer", (unsigned long long)n,
                         (unsigned long long)keys_at, (unsigned long long)keys->n);
    if (values_at > values->n || n > (values->n - values_at) / 4)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_sort_u64_pairs: %llu values from %llu lie outside the %llu bytes of their buffer", (unsigned long long)n,
                         (unsigned long long)values_at, (unsigned long long)values->n);
    if (keys == values && n && keys_at < values_at + 4 * n && values_at < keys_at + 8 * n)
        return set_error(ctx, MDBG_EINVAL, "mdbg_bytes_sort_u64_pairs: the keys and the values of one buffer overlap");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_TRY(bytes_ready_on(ctx, keys));
    MDBG_TRY(bytes_ready_on(ctx, values));
    uint32_t passes[2] = {0u, 0u};
    MDBG_TRY(sort_u64_pairs(ctx, reinterpret_cast<uint64_t *>(keys->d.p + keys_at), reinterpret_cast<uint32_t *>(values->d.p + values_at), n, passes));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (info) { info[0] = passes[0]; info[1] = passes[1]; }
    return MDBG_OK;
} MDBG_API_CATCH(ctx)
