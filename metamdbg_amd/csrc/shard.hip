// shard.hip -- the sharded passes (reads split over several GPUs, one process each): a rank's rows grouped by owner, the owner's
// reduction, the replies back into the rank's table.  See include/mdbg_hip.h.
#include "common.hpp"
#include "murmur.hpp"
#include "objects.hpp"
#include "table.hpp"
#include "kminmer_dev.hpp"
#include "kminmer_host.hpp"

#include <vector>


// =====================================================================================================
// Sharded first pass (reads split over several GPUs, one process each).  See include/mdbg_hip.h.
// =====================================================================================================
namespace mdbg {

constexpr uint32_t SHARD_ROW_WORDS = 3;                 // [hash_lo, hash_hi, count]
constexpr uint64_t SHARD_EMIT_BIT = 1ull << 63;         // in a reply: "you list this key in your table"

__device__ __forceinline__ uint32_t owner_of(uint64_t hi, uint32_t n_ranks) {
    return (uint32_t)(((hi >> 32) * (uint64_t)n_ranks) >> 32);
}

__device__ __forceinline__ bool slot_read(const TableView &t, uint64_t cap, uint64_t s, uint64_t &lo, uint64_t &hi, uint32_t &v) {
    if (s < cap) {
        const uint4 *q = reinterpret_cast<const uint4 *>(t.slots + s);
        const uint4 key = q[0];
        lo = (uint64_t)key.x | ((uint64_t)key.y << 32);
        if (lo == 0ull) return false;
        hi = (uint64_t)key.z | ((uint64_t)key.w << 32);
        v = q[1].x;
        return true;
    }
    uint32_t i = (uint32_t)(s - cap);
    if (i >= *t.exc_n) return false;
    lo = t.exc_lo[i]; hi = t.exc_hi[i]; v = t.exc_val[i];
    return true;
}

// Rows are grouped by owner without a single global atomic (same-address device-scope atomics cost
// ~0.2 us each on this part, serialised): pass 1 writes one LDS histogram per block of SHARD_SPB slots
// to block_hist[owner][block]; an exclusive scan over that owner-major array gives every (owner, block)
// its first row; pass 2 hands out the places inside the block's range through LDS.
constexpr uint32_t SHARD_SPB = 2048;   // slots per block

__global__ __launch_bounds__(256) void owner_hist_kernel(TableView t, uint64_t cap, uint32_t n_ranks, uint32_t *block_hist) {
    __shared__ uint32_t h[64];
    if (threadIdx.x < 64) h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t s0 = (uint64_t)blockIdx.x * SHARD_SPB;
    for (uint32_t j = threadIdx.x; j < SHARD_SPB; j += 256) {
        uint64_t lo, hi; uint32_t v;
        if (s0 + j < cap + TABLE_EXC_CAP && slot_read(t, cap, s0 + j, lo, hi, v)) atomicAdd(&h[owner_of(hi, n_ranks)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < n_ranks) block_hist[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// write every occupied slot as a row [lo, hi, count] into its owner's range and remember its slot
__global__ __launch_bounds__(256) void owner_scatter_kernel(TableView t, uint64_t cap, uint32_t n_ranks, const uint64_t *block_base,
                                                            uint64_t *rows, uint32_t *row_slot) {
    __shared__ uint32_t h[64];
    if (threadIdx.x < 64) h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t s0 = (uint64_t)blockIdx.x * SHARD_SPB;
    for (uint32_t j = threadIdx.x; j < SHARD_SPB; j += 256) {
        const uint64_t s = s0 + j;
        uint64_t lo, hi; uint32_t v;
        if (!(s < cap + TABLE_EXC_CAP && slot_read(t, cap, s, lo, hi, v))) continue;
        const uint32_t own = owner_of(hi, n_ranks);
        const uint64_t row = block_base[(uint64_t)own * gridDim.x + blockIdx.x] + atomicAdd(&h[own], 1u);
        uint64_t *o = rows + row * SHARD_ROW_WORDS;
        o[0] = lo; o[1] = hi; o[2] = v;
        row_slot[row] = s < cap ? (uint32_t)s : (0x80000000u | (uint32_t)(s - cap));
    }
}

// The owner's table keys a row by (fmix64(hash_lo), hash_hi), not by the identity itself.  A slot's home is the TOP bits of
// lo ^ (hi >> 17) (table_home), of which the first 17 are hash_lo's alone; and this table is what takes the rows over when a bucket
// of part_owner_reduce outgrew its LDS table -- which is when more keys share the top bits of hash_lo than a table has slots.  With
// the identity as the key those very keys shared a handful of home slots here as well, and the hand-over ended in "hash table
// overflow" at any capacity.  fmix64 is a bijection that keeps 0 at 0: distinct keys stay distinct, a zero word stays a zero word
// (the side list), and the table belongs to this call alone (mdbg_shard_reduce drops it once the replies are written).
__device__ __forceinline__ uint64_t owner_key_lo(uint64_t lo) { return fmix64(lo); }

// owner: sum the received rows by key; rep = index of the received row that created the key -- its sender is the
// one rank that will list the key
__global__ __launch_bounds__(256) void rows_add_kernel(const uint64_t *rows, uint64_t n, TableView t) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t *r = rows + i * SHARD_ROW_WORDS;
    table_upsert_count(t, owner_key_lo(r[0]), r[1], (uint32_t)r[2], (uint32_t)i);
}

__global__ __launch_bounds__(256) void rows_reply_kernel(const uint64_t *rows, uint64_t n, TableView t, uint64_t *reply) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t *r = rows + i * SHARD_ROW_WORDS;
    const uint32_t slot = table_lookup_slot(t, owner_key_lo(r[0]), r[1]);
    uint64_t out = 0;
    if (slot != SLOT_NONE) out = (uint64_t)table_slot_val(t, slot) | (table_slot_rep(t, slot) == (uint32_t)i ? SHARD_EMIT_BIT : 0ull);
    reply[i] = out;
}

// global counts back into the local table (the slot of every sent row was remembered); the rows this rank
// was told to list and that are solid get their flag
__global__ __launch_bounds__(256) void apply_global_counts_kernel(const uint64_t *reply, const uint32_t *row_slot, uint64_t n, TableView t,
                                                                  uint64_t cap, uint32_t min_abundance, uint32_t *flag) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = row_slot[i], v = (uint32_t)reply[i];
    const bool emit = (reply[i] & SHARD_EMIT_BIT) != 0ull && v > 1u && !(v < min_abundance);
    if (s & 0x80000000u) { t.exc_val[s & 0x7FFFFFFFu] = v; flag[cap + (s & 0x7FFFFFFFu)] = emit ? 1u : 0u; }
    else { t.slots[s].val = v; flag[s] = emit ? 1u : 0u; }
}

// ---- the same grouping by owner for the rows of a finished local table (sharded k > firstK) ----
constexpr uint32_t SHARD_RPB = 2048;   // rows per block

__global__ __launch_bounds__(256) void table_owner_hist_kernel(const uint64_t *hi, uint64_t n, uint32_t n_ranks, uint32_t *block_hist) {
    __shared__ uint32_t h[64];
    if (threadIdx.x < 64) h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t r0 = (uint64_t)blockIdx.x * SHARD_RPB;
    for (uint32_t j = threadIdx.x; j < SHARD_RPB; j += 256)
        if (r0 + j < n) atomicAdd(&h[owner_of(hi[r0 + j], n_ranks)], 1u);
    __syncthreads();
    if (threadIdx.x < n_ranks) block_hist[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(256) void table_owner_scatter_kernel(const uint64_t *lo, const uint64_t *hi, const uint32_t *ab, uint64_t n,
                                                                  uint32_t n_ranks, const uint64_t *block_base, uint64_t *rows, uint32_t *row_index) {
    __shared__ uint32_t h[64];
    if (threadIdx.x < 64) h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t r0 = (uint64_t)blockIdx.x * SHARD_RPB;
    for (uint32_t j = threadIdx.x; j < SHARD_RPB; j += 256) {
        const uint64_t i = r0 + j;
        if (i >= n) continue;
        const uint32_t own = owner_of(hi[i], n_ranks);
        const uint64_t row = block_base[(uint64_t)own * gridDim.x + blockIdx.x] + atomicAdd(&h[own], 1u);
        uint64_t *o = rows + row * SHARD_ROW_WORDS;
        o[0] = lo[i]; o[1] = hi[i]; o[2] = ab[i];
        row_index[row] = (uint32_t)i;
    }
}

// the sharded first pass on the partitioned machinery: reply i belongs to local key row_index[i]
__global__ void replies_to_keys_kernel(const uint64_t *reply, const uint32_t *row_index, uint64_t n, uint32_t min_abundance, uint32_t *gcount, uint32_t *listed) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = (uint32_t)reply[i], key = row_index[i];
    gcount[key] = v;
    listed[key] = ((reply[i] & SHARD_EMIT_BIT) != 0ull && v > 1u && !(v < min_abundance)) ? 1u : 0u;
}

__global__ void keep_flag_kernel(const uint64_t *reply, const uint32_t *row_index, uint64_t n, uint32_t *flag) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[row_index[i]] = (reply[i] & SHARD_EMIT_BIT) ? 1u : 0u;
}

__global__ void keep_rows_kernel(const uint32_t *flag, const uint64_t *pos, uint64_t n, uint32_t k, const uint64_t *lo, const uint64_t *hi,
                                 const uint32_t *ab, const uint32_t *vec, uint64_t *olo, uint64_t *ohi, uint32_t *oab, uint32_t *ovec) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint64_t d = pos[i];
    olo[d] = lo[i]; ohi[d] = hi[i]; oab[d] = ab[i];
    if (vec) for (uint32_t j = 0; j < k; j++) ovec[d * k + j] = vec[i * k + j];
}

}  // namespace mdbg

using namespace mdbg;

struct mdbg_shard {
    uint32_t k = 0, n_ranks = 1;
    const mdbg_minimizers *reads = nullptr;
    const mdbg_table *table = nullptr;       // mdbg_shard_from_table: the local table whose rows are being deduplicated
    mdbg::DevBuf<uint32_t> row_index;        // ... and the table row every sent row came from
    mdbg::InstIndex ix;
    mdbg::DeviceTable local, owner;
    mdbg::DevBuf<uint32_t> inst_slot, row_slot;
    mdbg::DevBuf<uint64_t> rows, reply;
    mdbg::DevBuf<uint64_t> local_replies;    // mdbg_shard_exchange_local: the replies to this shard's rows
    uint64_t n_rows = 0;
    bool reduced = false;
    // the rank's share counted by the partitioned pass (csrc/partition.hip) instead of a local table: its distinct keys are the rows
    mdbg::PartLocal *part = nullptr;
    ~mdbg_shard() { if (part) mdbg::part_local_free(part); }
};

extern "C" uint32_t mdbg_row_words(uint32_t) { return mdbg::SHARD_ROW_WORDS; }

namespace mdbg {

// the rows every rank gets, from the scanned block histograms (owner-major, nb blocks an owner); returns the first row of every (owner, block)'s
// range on the device and the rows in all
static int owner_counts(mdbg_ctx *ctx, const DevBuf<uint32_t> &block_hist, unsigned nb, uint32_t n_ranks, DevBuf<uint64_t> &block_base, uint64_t *counts, uint64_t *total) {
    const uint64_t nh = (uint64_t)nb * n_ranks;
    MDBG_TRY(block_base.alloc(ctx, nh + 1));
    MDBG_TRY(exclusive_scan_u32(ctx, block_hist.p, block_base.p, nh));
    std::vector<uint64_t> base(nh + 1);
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, base.data(), block_base.p, (nh + 1) * 8, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < n_ranks; r++) counts[r] = base[(uint64_t)(r + 1) * nb] - base[(uint64_t)r * nb];
    *total = base[nh];
    return MDBG_OK;
}

// n rows (lo, hi, cnt) grouped by owner into sh->rows, the row each came from in sh->row_index; counts[r] = rows of rank r.  Synchronises.
static int group_rows_by_owner(mdbg_ctx *ctx, mdbg_shard *sh, const uint64_t *lo, const uint64_t *hi, const uint32_t *cnt, uint64_t n, uint64_t *counts) {
    const unsigned nb = grid_for(n, SHARD_RPB);
    DevBuf<uint32_t> block_hist;
    DevBuf<uint64_t> block_base;
    MDBG_TRY(block_hist.alloc(ctx, (uint64_t)nb * sh->n_ranks));
    {
        LaunchTimer timer(ctx, "shard_rows");
        hipLaunchKernelGGL(table_owner_hist_kernel, dim3(nb), dim3(256), 0, ctx->stream, hi, n, sh->n_ranks, block_hist.p);
    }
    uint64_t total = 0;
    MDBG_TRY(owner_counts(ctx, block_hist, nb, sh->n_ranks, block_base, counts, &total));
    MDBG_TRY(sh->rows.alloc(ctx, n * SHARD_ROW_WORDS));
    MDBG_TRY(sh->row_index.alloc(ctx, n));
    sh->n_rows = n;
    {
        LaunchTimer timer(ctx, "shard_rows");
        hipLaunchKernelGGL(table_owner_scatter_kernel, dim3(nb), dim3(256), 0, ctx->stream, lo, hi, cnt, n, sh->n_ranks, block_base.p, sh->rows.p, sh->row_index.p);
    }
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
}

}  // namespace mdbg

extern "C" int mdbg_shard_begin(mdbg_ctx *ctx, const mdbg_minimizers *reads, uint32_t k, uint32_t n_ranks,
                                mdbg_shard **out, const uint64_t **d_rows, uint64_t *counts) try {
    if (!ctx || !reads || !out || !d_rows || !counts || k < 2 || n_ranks < 1 || n_ranks > 64)
        return set_error(ctx, MDBG_EINVAL, "mdbg_shard_begin: bad argument");
    MDBG_TRY(check_seq(ctx, reads, "mdbg_shard_begin"));
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<mdbg_shard> sh(new mdbg_shard());
    sh->k = k; sh->n_ranks = n_ranks; sh->reads = reads;
    // the rank's share through the partitioned pass (as mdbg_kminmer_count_first chooses): its distinct keys with their local counts come out
    // bucket after bucket and are grouped by owner like the rows of a finished table (mdbg_shard_from_table)
    if (first_pass_partitioned(ctx, reads->n_min)) {
        bool done = false;
        MDBG_TRY(part_local_keys(ctx, reads, k, &sh->part, &done));
        if (done) {
            const uint64_t *klo, *khi; const uint32_t *kcnt; uint64_t n = 0, n_inst = 0;
            part_local_arrays(sh->part, &klo, &khi, &kcnt, &n, &n_inst);
            if (n >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "more than 2^32 distinct local keys");
            MDBG_TRY(group_rows_by_owner(ctx, sh.get(), klo, khi, kcnt, n, counts));
            update_key_hint(ctx, 3, n, n_inst);
            MDBG_DBG(ctx, "shard_begin (partitioned): %llu rows", (unsigned long long)n);
            *d_rows = sh->rows.p;
            *out = sh.release();
            return MDBG_OK;
        }
    }
    MDBG_TRY(build_inst_index(ctx, reads, k, sh->ix));
    const uint64_t I = sh->ix.total;
    MDBG_DBG(ctx, "shard_begin: %llu instances", (unsigned long long)I);
    MDBG_TRY(count_instances(ctx, make_view(reads, sh->ix), k, 3, sh->local, sh->inst_slot));
    TableView tv = sh->local.view();
    const uint64_t nslots = sh->local.cap + TABLE_EXC_CAP;
    const unsigned nb = grid_for(nslots, SHARD_SPB);
    DevBuf<uint32_t> block_hist;
    DevBuf<uint64_t> block_base;
    MDBG_TRY(block_hist.alloc(ctx, (uint64_t)nb * n_ranks));
    {
        LaunchTimer timer(ctx, "shard_rows");
        hipLaunchKernelGGL(owner_hist_kernel, dim3(nb), dim3(256), 0, ctx->stream, tv, sh->local.cap, n_ranks, block_hist.p);
    }
    uint64_t total = 0;
    MDBG_TRY(owner_counts(ctx, block_hist, nb, n_ranks, block_base, counts, &total));
    if (total >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "more than 2^32 distinct local keys");
    update_key_hint(ctx, 3, total, I);        // one row per distinct local key
    MDBG_TRY(sh->rows.alloc(ctx, total * SHARD_ROW_WORDS));
    MDBG_TRY(sh->row_slot.alloc(ctx, total));
    sh->n_rows = total;
    {
        LaunchTimer timer(ctx, "shard_rows");
        hipLaunchKernelGGL(owner_scatter_kernel, dim3(nb), dim3(256), 0, ctx->stream, tv, sh->local.cap, n_ranks, block_base.p,
                           sh->rows.p, sh->row_slot.p);
    }
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    MDBG_DBG(ctx, "shard_begin: %llu rows", (unsigned long long)total);
    *d_rows = sh->rows.p;
    *out = sh.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

__global__ void rows_zero_word_kernel(const uint64_t *rows, uint64_t n, unsigned long long *out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (rows[i * SHARD_ROW_WORDS] == 0ull || rows[i * SHARD_ROW_WORDS + 1] == 0ull)) atomicAdd(out, 1ull);
}

extern "C" int mdbg_shard_reduce(mdbg_ctx *ctx, mdbg_shard *sh, const uint64_t *d_recv, uint64_t n_recv, const uint64_t **d_reply) try {
    if (!ctx || !sh || !d_reply || (n_recv && !d_recv)) return set_error(ctx, MDBG_EINVAL, "mdbg_shard_reduce: bad argument");
    if (n_recv >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "more than 2^32 received rows");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // every key this rank owns arrives once from each rank that saw it: about n_recv / n_ranks distinct keys.  Sized for
    // that (+50 %), the table is n_ranks times smaller than one sized for the rows; it grows and refills if that was short.
    const uint64_t expected = n_recv / sh->n_ranks + n_recv / (2 * sh->n_ranks) + 1024;
    MDBG_DBG(ctx, "shard_reduce: %llu rows", (unsigned long long)n_recv);
    if (debug_on() && n_recv) {
        DevBuf<unsigned long long> z;
        MDBG_TRY(z.alloc(ctx, 1));
        (void)hipMemsetAsync(z.p, 0, 8, ctx->stream);
        hipLaunchKernelGGL(rows_zero_word_kernel, dim3(grid_for(n_recv, 256)), dim3(256), 0, ctx->stream, d_recv, n_recv, z.p);
        unsigned long long hz = 0;
        MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &hz, z.p, 8, hipMemcpyDeviceToHost));
        MDBG_DBG(ctx, "shard_reduce: %llu rows with a zero key word", hz);
    }
    if (ctx->first_pass_mode != 1) {          // the rows bucketed by key, every bucket summed in LDS (csrc/partition.hip)
        bool done = false;
        MDBG_TRY(sh->reply.alloc(ctx, n_recv));
        MDBG_TRY(part_owner_reduce(ctx, d_recv, n_recv, sh->reply.p, &done));
        if (done) {
            sh->reduced = true;
            *d_reply = sh->reply.p;
            return MDBG_OK;
        }
    }
    MDBG_TRY(build_table_adaptive(ctx, sh->owner, expected < n_recv ? expected : n_recv, n_recv, [&](TableView v) {
        if (n_recv) {
            LaunchTimer timer(ctx, "shard_reduce");
            hipLaunchKernelGGL(rows_add_kernel, dim3(grid_for(n_recv, 256)), dim3(256), 0, ctx->stream, d_recv, n_recv, v);
        }
        return MDBG_OK;
    }));
    TableView tv = sh->owner.view();
    MDBG_TRY(sh->reply.alloc(ctx, n_recv));
    if (n_recv) {
        LaunchTimer timer(ctx, "shard_reduce");
        hipLaunchKernelGGL(rows_reply_kernel, dim3(grid_for(n_recv, 256)), dim3(256), 0, ctx->stream, d_recv, n_recv, tv, sh->reply.p);
    }
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    MDBG_TRY(sh->owner.check_overflow(ctx));
    sh->owner = DeviceTable();      // only the replies are needed from here on
    sh->reduced = true;
    *d_reply = sh->reply.p;
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_shard_finish(mdbg_ctx *ctx, mdbg_shard *sh, const uint64_t *d_replies, uint32_t min_abundance, mdbg_table **out) try {
    if (!ctx || !sh || !out || (sh->n_rows && !d_replies)) return set_error(ctx, MDBG_EINVAL, "mdbg_shard_finish: bad argument");
    if (!sh->reduced) return set_error(ctx, MDBG_EINVAL, "mdbg_shard_finish: mdbg_shard_reduce has not run");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (sh->part) {
        // the replies, row by row, back to the order of the local keys: global count, and whether this rank lists the key
        DevBuf<uint32_t> gcount, listed;
        MDBG_TRY(gcount.alloc(ctx, sh->n_rows));
        MDBG_TRY(listed.alloc(ctx, sh->n_rows));
        if (sh->n_rows)
            hipLaunchKernelGGL(replies_to_keys_kernel, dim3(grid_for(sh->n_rows, 256)), dim3(256), 0, ctx->stream, d_replies, sh->row_index.p, sh->n_rows, min_abundance,
                               gcount.p, listed.p);
        return part_local_finish(ctx, sh->part, gcount.p, listed.p, min_abundance, out);
    }
    const uint64_t I = sh->ix.total;
    const uint64_t nslots = sh->local.cap + TABLE_EXC_CAP;
    DevBuf<uint32_t> sflag;
    MDBG_TRY(sflag.alloc(ctx, nslots));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(sflag.p, 0, nslots * 4, ctx->stream));
    if (sh->n_rows)
        hipLaunchKernelGGL(apply_global_counts_kernel, dim3(grid_for(sh->n_rows, 256)), dim3(256), 0, ctx->stream, d_replies, sh->row_slot.p,
                           sh->n_rows, sh->local.view(), sh->local.cap, min_abundance, sflag.p);
    // rescue over the local reads against the global counts now sitting in the local table
    SeqView sv = make_view(sh->reads, sh->ix), none{};
    RescuePlan plan;
    FlaggedRows how;
    how.timer = "kminmer_emit";
    how.extra_rows = [&](uint64_t, uint64_t &n_resc) {
        if (min_abundance <= 1 && I) MDBG_TRY(plan_rescue(ctx, sh->local, sh->ix, sv.n_reads, sh->inst_slot.p, plan));
        n_resc = plan.total;
        return MDBG_OK;
    };
    how.emit_extra = [&](const RowOut &ro, uint64_t n_solid) { if (plan.total) launch_emit_rescued(ctx, sv, sh->k, sh->inst_slot.p, plan, ro, n_solid); };
    std::unique_ptr<mdbg_table> t;
    MDBG_TRY(rows_from_flags(ctx, sh->local, sflag, sh->k, sv, none, true, how, t));
    t->st_minimizers = sv.n_min; t->st_instances = I; t->st_keys = sh->n_rows; t->st_slots = nslots;
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = t.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

// ---- sharded k > firstK -------------------------------------------------------------------------------------------
extern "C" int mdbg_shard_from_table(mdbg_ctx *ctx, const mdbg_table *local, uint32_t n_ranks, mdbg_shard **out, const uint64_t **d_rows,
                                     uint64_t *counts) try {
    if (!ctx || !local || !out || !d_rows || !counts || n_ranks < 1 || n_ranks > 64)
        return set_error(ctx, MDBG_EINVAL, "mdbg_shard_from_table: bad argument");
    if (local->n_records >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_shard_from_table: more than 2^32 rows");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<mdbg_shard> sh(new mdbg_shard());
    sh->k = local->k; sh->n_ranks = n_ranks; sh->table = local;
    MDBG_TRY(group_rows_by_owner(ctx, sh.get(), local->d_lo.p, local->d_hi.p, local->d_ab.p, local->n_records, counts));
    *d_rows = sh->rows.p;
    *out = sh.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_shard_keep(mdbg_ctx *ctx, mdbg_shard *sh, const uint64_t *d_replies, mdbg_table **out) try {
    if (!ctx || !sh || !out || !sh->table || (sh->n_rows && !d_replies)) return set_error(ctx, MDBG_EINVAL, "mdbg_shard_keep: bad argument");
    if (!sh->reduced) return set_error(ctx, MDBG_EINVAL, "mdbg_shard_keep: mdbg_shard_reduce has not run");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const mdbg_table *src = sh->table;
    const uint64_t n = sh->n_rows;
    DevBuf<uint32_t> flag;
    DevBuf<uint64_t> pos;
    MDBG_TRY(flag.alloc(ctx, n));
    MDBG_TRY(pos.alloc(ctx, n + 1));
    if (n) hipLaunchKernelGGL(keep_flag_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_replies, sh->row_index.p, n, flag.p);
    MDBG_TRY(exclusive_scan_u32(ctx, flag.p, pos.p, n));
    uint64_t kept = 0;
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &kept, pos.p + n, 8, hipMemcpyDeviceToHost));
    std::unique_ptr<mdbg_table> t(new mdbg_table());
    t->k = src->k;
    MDBG_TRY(alloc_rows(ctx, t.get(), kept, src->has_vectors));
    t->n_solid = kept;
    if (n) hipLaunchKernelGGL(keep_rows_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, flag.p, pos.p, n, src->k, src->d_lo.p, src->d_hi.p,
                              src->d_ab.p, src->has_vectors ? src->d_vec.p : nullptr, t->d_lo.p, t->d_hi.p, t->d_ab.p,
                              src->has_vectors ? t->d_vec.p : nullptr);
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = t.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

// Both all-to-alls of a sharded pass among shards that live on ONE device (a job checking itself, tests): device-to-device copies
// stand in for the wire, everything else -- mdbg_shard_reduce on every owner, the replies back in the order the rows were sent --
// is what mdbg_shard_exchange does between GPUs.
extern "C" int mdbg_shard_exchange_local(mdbg_ctx *ctx, mdbg_shard *const *shards, uint32_t n, const uint64_t *const *d_rows, const uint64_t *counts,
                                         const uint64_t **d_replies) try {
    if (!ctx || !shards || !d_rows || !counts || !d_replies || n < 1 || n > 64) return set_error(ctx, MDBG_EINVAL, "mdbg_shard_exchange_local: bad argument");
    for (uint32_t r = 0; r < n; r++)
        if (!shards[r] || shards[r]->n_ranks != n) return set_error(ctx, MDBG_EINVAL, "mdbg_shard_exchange_local: shard %u was not begun for %u ranks", r, n);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t rw = SHARD_ROW_WORDS;
    // soff[src][dst]: first row of src's rows for dst; roff[dst][src]: first received row on dst that came from src
    std::vector<uint64_t> soff((size_t)n * (n + 1), 0), roff((size_t)n * (n + 1), 0);
    for (uint32_t a = 0; a < n; a++)
        for (uint32_t b = 0; b < n; b++) {
            soff[(size_t)a * (n + 1) + b + 1] = soff[(size_t)a * (n + 1) + b] + counts[(size_t)a * n + b];
            roff[(size_t)a * (n + 1) + b + 1] = roff[(size_t)a * (n + 1) + b] + counts[(size_t)b * n + a];
        }
    std::vector<const uint64_t *> reply(n, nullptr);
    for (uint32_t dst = 0; dst < n; dst++) {
        const uint64_t n_recv = roff[(size_t)dst * (n + 1) + n];
        DevBuf<uint64_t> recv;
        MDBG_TRY(recv.alloc(ctx, n_recv * rw));
        for (uint32_t src = 0; src < n; src++) {
            const uint64_t c = counts[(size_t)src * n + dst];
            if (!c) continue;
            if (!d_rows[src]) return set_error(ctx, MDBG_EINVAL, "mdbg_shard_exchange_local: shard %u has rows but no row pointer", src);
            MDBG_HIP_CHECK(ctx, hipMemcpyAsync(recv.p + roff[(size_t)dst * (n + 1) + src] * rw, d_rows[src] + soff[(size_t)src * (n + 1) + dst] * rw, c * rw * 8,
                                               hipMemcpyDeviceToDevice, ctx->stream));
        }
        MDBG_TRY(mdbg_shard_reduce(ctx, shards[dst], recv.p, n_recv, &reply[dst]));   // (synchronises: recv may go)
    }
    for (uint32_t src = 0; src < n; src++) {
        MDBG_TRY(shards[src]->local_replies.alloc(ctx, soff[(size_t)src * (n + 1) + n]));
        for (uint32_t dst = 0; dst < n; dst++) {
            const uint64_t c = counts[(size_t)src * n + dst];
            if (c) MDBG_HIP_CHECK(ctx, hipMemcpyAsync(shards[src]->local_replies.p + soff[(size_t)src * (n + 1) + dst], reply[dst] + roff[(size_t)dst * (n + 1) + src],
                                                      c * 8, hipMemcpyDeviceToDevice, ctx->stream));
        }
        d_replies[src] = shards[src]->local_replies.p;
    }
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" void mdbg_shard_free(mdbg_shard *shard) { delete shard; }
