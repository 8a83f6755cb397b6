// tables.hip -- the table handle's own entry points: previous tables from abundance records and their unitig overlay, look-ups, rows back
// to the host, checksums, the small-contig test and the edge indexes.  The passes that build tables from sequences are kminmer.hip.
#include "common.hpp"
#include "murmur.hpp"
#include "objects.hpp"
#include "table.hpp"
#include "kminmer_dev.hpp"
#include "kminmer_host.hpp"

namespace mdbg {

// read owning global instance g: largest r with inst_off[r] <= g
__device__ __forceinline__ uint32_t find_read(const uint64_t *inst_off, uint32_t n_reads, uint64_t g) {
    uint32_t lo = 0, hi = n_reads;  // invariant: inst_off[lo] <= g < inst_off[hi]
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (inst_off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- prev tables ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rows_insert_kernel(const uint64_t *lo, const uint64_t *hi, const uint32_t *ab, uint64_t n,
                                                          int skip_one, TableView t) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (skip_one && ab[i] == 1u) return;   // graph/CreateMdbg.cpp:3445
    table_upsert_set(t, lo[i], hi[i], ab[i], 0u);
}

// (graph/CreateMdbg.cpp:3466-3507)
__global__ __launch_bounds__(256) void overlay_kernel(SeqView s, uint32_t kprev, const uint32_t *unitig_ab, TableView t) {
    uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= s.n_inst) return;
    uint32_t r = find_read(s.inst_off, s.n_reads, g);
    uint32_t a = unitig_ab[r];
    if (a == 0xFFFFFFFFu) return;   // unitig without refined abundance
    const uint32_t *m = s.mins + s.off[r] + (g - s.inst_off[r]);
    uint64_t hi, lo;
    window_hash(m, kprev, hi, lo);
    if (a == 1u) {
        // modify_if: set to 0 only when present
        if (lo == 0ull || hi == 0ull) { table_exc_upsert(t, lo, hi, 0, 0, true, 0, false); return; }
        uint32_t slot = table_find_or_insert(t, lo, hi, false);
        if (slot != SLOT_NONE) __hip_atomic_store(&t.slots[slot].val, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        table_upsert_set(t, lo, hi, a, 0u);
    }
}

__global__ __launch_bounds__(256) void lookup_kernel(TableView t, const uint64_t *lo, const uint64_t *hi, uint64_t n, uint32_t *out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t v;
    out[i] = table_lookup(t, lo[i], hi[i], v) ? v : 0u;
}

// small-contig test of IndexKminmerFunctor (graph/CreateMdbg.hpp:1330; getAbundance(0, .) :988-1010): one thread per unitig
__global__ __launch_bounds__(256) void small_contig_kernel(const uint64_t *off, uint32_t n_unitigs, const uint32_t *mins, uint32_t k,
                                                           uint32_t k_prev, TableView prev, uint8_t *flags) {
    uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_unitigs) return;
    const uint64_t b = off[u], n = off[u + 1] - b;
    uint8_t f = 0;
    if (n < k && n >= k_prev) {
        const uint32_t windows = (n - k_prev + 1) < 2 ? 1u : 2u;     // prev[0], or min(prev[0], prev[1])
        uint32_t a = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < windows; i++) {
            uint64_t hi, lo;
            window_hash(mins + b + i, k_prev, hi, lo);
            uint32_t v;
            if (!table_lookup(prev, lo, hi, v)) v = 1u;               // getPrevAbundances: missing => 1 (:1240-1265)
            a = v < a ? v : a;
        }
        f = a > 1u;
    }
    flags[u] = f;
}

// EdgeIndexer::partitionNode (graph/CreateMdbg.hpp:4083-4100): prefix and suffix identities of one node
__global__ __launch_bounds__(256) void edge_insert_kernel(const uint32_t *vecs, uint64_t n, uint32_t k, TableView t) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *v = vecs + i * k;
    uint64_t hi, lo;
    window_hash(v, k - 1, hi, lo);
    table_upsert_count(t, lo, hi, 0u, 0u);
    window_hash(v + 1, k - 1, hi, lo);
    table_upsert_count(t, lo, hi, 0u, 0u);
}

// UnitigEdgeIndexer::partitionUnitig (graph/CreateMdbg.hpp:4352-4389): the same two identities for the first and
// the last k-min-mer of every unitig (the last one skipped when it is the first).  The reference normalises the node
// before taking prefix and suffix; the pair {prefix, suffix} of a vector and of its reverse are each other's reverses,
// and every identity is taken on the normalised (k-1)-vector, so the orientation of the node does not matter.
__global__ __launch_bounds__(256) void unitig_edge_insert_kernel(const uint64_t *off, uint32_t n_unitigs, const uint32_t *mins, uint32_t k, TableView t) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_unitigs) return;
    const uint64_t f = off[i], n = off[i + 1] - f;
    if (n < k) return;
    uint64_t hi, lo;
    const uint32_t *v = mins + f;
    window_hash(v, k - 1, hi, lo);
    table_upsert_count(t, lo, hi, 0u, 0u);
    window_hash(v + 1, k - 1, hi, lo);
    table_upsert_count(t, lo, hi, 0u, 0u);
    if (n == k) return;
    v = mins + f + (n - k);
    window_hash(v, k - 1, hi, lo);
    table_upsert_count(t, lo, hi, 0u, 0u);
    window_hash(v + 1, k - 1, hi, lo);
    table_upsert_count(t, lo, hi, 0u, 0u);
}

__global__ __launch_bounds__(256) void sum_u64_kernel(const uint64_t *v, uint64_t n, unsigned long long *out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t x = i < n ? v[i] : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    if ((threadIdx.x & 63u) == 0 && x) atomicAdd(out, (unsigned long long)x);
}

// out[0] += sum abundance * lo (the reference's "Checksum kminmer abundance"), out[1] += sum abundance, out[2] += sum hi,
// out[3] += sum over rows with a vector of (v[0] + 3 v[1] + 5 v[2] ...) * (lo | 1): ties the vectors to their keys
__global__ __launch_bounds__(256) void table_checksum_kernel(const uint64_t *lo, const uint64_t *hi, const uint32_t *ab, const uint32_t *vec,
                                                             uint32_t k, uint64_t n, unsigned long long *out) {
    uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t l = lo[i], a = ab[i];
        s0 += a * l; s1 += a; s2 += hi[i];
        if (vec) {
            uint64_t w = 0;
            for (uint32_t j = 0; j < k; j++) w += (uint64_t)vec[i * k + j] * (2u * j + 1u);
            s3 += w * (l | 1ull);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s0 += __shfl_xor(s0, d, 64); s1 += __shfl_xor(s1, d, 64); s2 += __shfl_xor(s2, d, 64); s3 += __shfl_xor(s3, d, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(out + 0, (unsigned long long)s0); atomicAdd(out + 1, (unsigned long long)s1);
        atomicAdd(out + 2, (unsigned long long)s2); atomicAdd(out + 3, (unsigned long long)s3);
    }
}

__global__ void interleave_keys_kernel(const uint64_t *lo, const uint64_t *hi, uint64_t n, uint64_t *out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { out[2 * i] = lo[i]; out[2 * i + 1] = hi[i]; }
}

__global__ void unpack_records_kernel(const uint8_t *rec, uint64_t n, uint64_t *lo, uint64_t *hi, uint32_t *ab) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(rec) + 5 * i;      // (records are 20 bytes from a 256-byte aligned start)
    lo[i] = (uint64_t)p[0] | ((uint64_t)p[1] << 32); hi[i] = (uint64_t)p[2] | ((uint64_t)p[3] << 32); ab[i] = p[4];
}

__global__ void pack_records_kernel(const uint64_t *lo, const uint64_t *hi, const uint32_t *ab, uint64_t n, uint8_t *rec) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t *p = rec + 20 * i;
    uint64_t l = lo[i], h = hi[i]; uint32_t a = ab[i];
    for (int b = 0; b < 8; b++) { p[b] = (uint8_t)(l >> (8 * b)); p[8 + b] = (uint8_t)(h >> (8 * b)); }
    for (int b = 0; b < 4; b++) p[16 + b] = (uint8_t)(a >> (8 * b));
}

}  // namespace mdbg

using namespace mdbg;

int mdbg::ensure_lookup(mdbg_ctx *ctx, mdbg_table *t, bool skip_one) {
    if (t->lookup) return MDBG_OK;
    std::unique_ptr<DeviceTable> tab(new DeviceTable());
    MDBG_TRY(tab->init(ctx, table_slots_for(t->n_records)));
    if (t->n_records)
        hipLaunchKernelGGL(rows_insert_kernel, dim3(grid_for(t->n_records, 256)), dim3(256), 0, ctx->stream,
                           t->d_lo.p, t->d_hi.p, t->d_ab.p, t->n_records, skip_one ? 1 : 0, tab->view());
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    MDBG_TRY(tab->check_overflow(ctx));
    t->lookup = std::move(tab);
    return MDBG_OK;
}

// a previous table from n_records abundance records of 20 bytes on the device: the rows, and the look-up over them (abundance 1
// skipped, graph/CreateMdbg.cpp:3445) with headroom, since the unitig overlay may add keys that are not in the record file
static int prev_from_device_records(mdbg_ctx *ctx, const uint8_t *d_records, uint64_t n_records, mdbg_table **out) {
    std::unique_ptr<mdbg_table> t(new mdbg_table());
    MDBG_TRY(alloc_rows(ctx, t.get(), n_records, false));
    if (n_records)
        hipLaunchKernelGGL(unpack_records_kernel, dim3(grid_for(n_records, 256)), dim3(256), 0, ctx->stream, d_records, n_records,
                           t->d_lo.p, t->d_hi.p, t->d_ab.p);
    std::unique_ptr<DeviceTable> tab(new DeviceTable());
    MDBG_TRY(tab->init(ctx, table_slots_for(n_records + n_records / 4) + 4096));
    if (n_records)
        hipLaunchKernelGGL(rows_insert_kernel, dim3(grid_for(n_records, 256)), dim3(256), 0, ctx->stream,
                           t->d_lo.p, t->d_hi.p, t->d_ab.p, n_records, 1, tab->view());
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    MDBG_TRY(tab->check_overflow(ctx));
    t->lookup = std::move(tab);
    *out = t.release();
    return MDBG_OK;
}

extern "C" int mdbg_prev_from_records(mdbg_ctx *ctx, const uint8_t *records20, uint64_t n_records, mdbg_table **out) try {
    if (!ctx || !out || (n_records && !records20)) return set_error(ctx, MDBG_EINVAL, "mdbg_prev_from_records: bad argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DevBuf<uint8_t> d_rec;
    MDBG_TRY(d_rec.alloc(ctx, n_records * 20));
    if (n_records) MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d_rec.p, records20, n_records * 20, hipMemcpyHostToDevice, ctx->stream));
    return prev_from_device_records(ctx, d_rec.p, n_records, out);
} MDBG_API_CATCH(ctx)

namespace mdbg { int bytes_ready_on(mdbg_ctx *ctx, const mdbg_bytes *b); }

extern "C" int mdbg_prev_from_record_bytes(mdbg_ctx *ctx, const mdbg_bytes *records, uint64_t n_records, mdbg_table **out) try {
    if (!ctx || !out || !records) return set_error(ctx, MDBG_EINVAL, "mdbg_prev_from_record_bytes: bad argument");
    if (n_records * 20 != records->n) return set_error(ctx, MDBG_EINVAL, "mdbg_prev_from_record_bytes: %llu records are not the buffer's %llu bytes",
                                                       (unsigned long long)n_records, (unsigned long long)records->n);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_TRY(bytes_ready_on(ctx, records));
    return prev_from_device_records(ctx, records->d.p, n_records, out);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_prev_overlay_unitigs(mdbg_ctx *ctx, mdbg_table *prev, const mdbg_minimizers *unitigs,
                                         const uint32_t *abundance, uint32_t k_prev) try {
    if (!ctx || !prev || !prev->lookup || !abundance || k_prev < 2) return set_error(ctx, MDBG_EINVAL, "mdbg_prev_overlay_unitigs: bad argument");
    MDBG_TRY(check_seq(ctx, unitigs, "mdbg_prev_overlay_unitigs"));
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    InstIndex ix;
    MDBG_TRY(build_inst_index(ctx, unitigs, k_prev, ix));
    if (prev->lookup->cap < (prev->n_records + ix.total) * 3 / 2)
        return set_error(ctx, MDBG_ERANGE, "prev table too small for the unitig overlay (%llu windows)", (unsigned long long)ix.total);
    DevBuf<uint32_t> d_ab;
    MDBG_TRY(d_ab.alloc(ctx, unitigs->n_reads));
    if (unitigs->n_reads) MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d_ab.p, abundance, (size_t)unitigs->n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    SeqView sv = make_view(unitigs, ix);
    if (ix.total)
        hipLaunchKernelGGL(overlay_kernel, dim3(grid_for(ix.total, 256)), dim3(256), 0, ctx->stream, sv, k_prev, d_ab.p, prev->lookup->view());
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    prev->image.reset();                 // (made again, from the overlaid table, by the pass that reads it)
    return prev->lookup->check_overflow(ctx);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_table_info(const mdbg_table *t, uint32_t *k, uint64_t *n_records, uint64_t *n_solid, int *has_vectors) {
    if (!t) return MDBG_EINVAL;
    if (k) *k = t->k;
    if (n_records) *n_records = t->n_records;
    if (n_solid) *n_solid = t->n_solid;
    if (has_vectors) *has_vectors = t->has_vectors ? 1 : 0;
    return MDBG_OK;
}

extern "C" int mdbg_table_stats(const mdbg_table *t, uint64_t stats[4]) {
    if (!t || !stats) return MDBG_EINVAL;
    stats[0] = t->st_minimizers; stats[1] = t->st_instances; stats[2] = t->st_keys; stats[3] = t->st_slots;
    return MDBG_OK;
}

extern "C" int mdbg_table_checksum(mdbg_ctx *ctx, const mdbg_table *t, uint64_t sums[4]) try {
    if (!ctx || !t || !sums) return set_error(ctx, MDBG_EINVAL, "mdbg_table_checksum: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DevBuf<unsigned long long> acc;
    MDBG_TRY(acc.alloc(ctx, 4));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(acc.p, 0, 32, ctx->stream));
    if (t->n_records)
        hipLaunchKernelGGL(table_checksum_kernel, dim3(grid_for(t->n_records, 256 * 8, 4096)), dim3(256), 0, ctx->stream, t->d_lo.p, t->d_hi.p,
                           t->d_ab.p, t->has_vectors ? t->d_vec.p : nullptr, t->k, t->n_records, acc.p);
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, sums, acc.p, 32, hipMemcpyDeviceToHost));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_table_to_host(mdbg_ctx *ctx, const mdbg_table *t, uint8_t *records20, uint32_t *vectors) try {
    if (!ctx || !t) return set_error(ctx, MDBG_EINVAL, "mdbg_table_to_host: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (records20 && t->n_records) {
        DevBuf<uint8_t> d_rec;
        MDBG_TRY(d_rec.alloc(ctx, t->n_records * 20));
        hipLaunchKernelGGL(pack_records_kernel, dim3(grid_for(t->n_records, 256)), dim3(256), 0, ctx->stream,
                           t->d_lo.p, t->d_hi.p, t->d_ab.p, t->n_records, d_rec.p);
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(records20, d_rec.p, t->n_records * 20, hipMemcpyDeviceToHost, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (vectors) {
        if (!t->has_vectors) return set_error(ctx, MDBG_EINVAL, "mdbg_table_to_host: table has no vectors (k >= firstK+2)");
        if (t->n_records) MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, vectors, t->d_vec.p, t->n_records * t->k * 4, hipMemcpyDeviceToHost));
    }
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_table_to_host_range(mdbg_ctx *ctx, const mdbg_table *t, uint64_t first, uint64_t count, uint8_t *records20, uint32_t *vectors) try {
    if (!ctx || !t) return set_error(ctx, MDBG_EINVAL, "mdbg_table_to_host_range: null argument");
    if (first > t->n_records || count > t->n_records - first) return set_error(ctx, MDBG_EINVAL, "mdbg_table_to_host_range: rows [%llu, +%llu) of %llu",
                                                                               (unsigned long long)first, (unsigned long long)count, (unsigned long long)t->n_records);
    if (vectors && !t->has_vectors) return set_error(ctx, MDBG_EINVAL, "mdbg_table_to_host_range: table has no vectors (k >= firstK+2)");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (!count) return MDBG_OK;
    DevBuf<uint8_t> d_rec;
    if (records20) {
        MDBG_TRY(d_rec.alloc(ctx, count * 20));
        hipLaunchKernelGGL(pack_records_kernel, dim3(grid_for(count, 256)), dim3(256), 0, ctx->stream, t->d_lo.p + first, t->d_hi.p + first, t->d_ab.p + first,
                           count, d_rec.p);
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(records20, d_rec.p, count * 20, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (vectors) MDBG_HIP_CHECK(ctx, hipMemcpyAsync(vectors, t->d_vec.p + first * t->k, count * t->k * 4, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));      // one wait for both
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_table_lookup(mdbg_ctx *ctx, const mdbg_table *t, const uint64_t *hash_lo, const uint64_t *hash_hi,
                                 uint64_t n, uint32_t *abundance) try {
    if (!ctx || !t || (n && (!hash_lo || !hash_hi || !abundance))) return set_error(ctx, MDBG_EINVAL, "mdbg_table_lookup: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_TRY(ensure_lookup(ctx, const_cast<mdbg_table *>(t), false));
    if (!n) return MDBG_OK;
    DevBuf<uint64_t> dl, dh;
    DevBuf<uint32_t> dv;
    MDBG_TRY(dl.alloc(ctx, n));
    MDBG_TRY(dh.alloc(ctx, n));
    MDBG_TRY(dv.alloc(ctx, n));
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(dl.p, hash_lo, n * 8, hipMemcpyHostToDevice, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(dh.p, hash_hi, n * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(lookup_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, t->lookup->view(), dl.p, dh.p, n, dv.p);
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(abundance, dv.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_small_contigs(mdbg_ctx *ctx, const mdbg_minimizers *unitigs, uint32_t k, uint32_t k_prev, const mdbg_table *prev,
                                  uint8_t *flags) try {
    if (!ctx || !unitigs || k_prev < 1 || k <= k_prev) return set_error(ctx, MDBG_EINVAL, "mdbg_small_contigs: bad argument");
    MDBG_TRY(check_seq(ctx, unitigs, "mdbg_small_contigs"));
    if (unitigs->n_reads && !flags) return set_error(ctx, MDBG_EINVAL, "mdbg_small_contigs: flags is null");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    TableView pv;
    MDBG_TRY(prev_view(ctx, prev, pv));
    if (!unitigs->n_reads) return MDBG_OK;
    DevBuf<uint8_t> d_flags;
    MDBG_TRY(d_flags.alloc(ctx, unitigs->n_reads));
    hipLaunchKernelGGL(small_contig_kernel, dim3(grid_for(unitigs->n_reads, 256)), dim3(256), 0, ctx->stream, unitigs->d_off.p,
                       unitigs->n_reads, unitigs->d_min.p, k, k_prev, pv, d_flags.p);
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(flags, d_flags.p, unitigs->n_reads, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

// every occupied slot of `tab` becomes a key-only row of a new table of (k-1)-identities
static int edges_from_table(mdbg_ctx *ctx, DeviceTable &tab, uint32_t k_edge, mdbg_table **edges, uint64_t *checksum) {
    DevBuf<uint32_t> sflag;
    MDBG_TRY(flag_occupied_slots(ctx, tab, sflag));
    FlaggedRows how;      // (untimed)
    std::unique_ptr<mdbg_table> t;
    MDBG_TRY(rows_from_flags(ctx, tab, sflag, k_edge, SeqView{}, SeqView{}, false, how, t));
    if (checksum) {
        DevBuf<unsigned long long> acc;
        MDBG_TRY(acc.alloc(ctx, 1));
        (void)hipMemsetAsync(acc.p, 0, 8, ctx->stream);
        if (t->n_records) hipLaunchKernelGGL(sum_u64_kernel, dim3(grid_for(t->n_records, 256)), dim3(256), 0, ctx->stream, t->d_lo.p, t->n_records, acc.p);
        MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, checksum, acc.p, 8, hipMemcpyDeviceToHost));
    }
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *edges = t.release();
    return MDBG_OK;
}

extern "C" int mdbg_edge_index(mdbg_ctx *ctx, const mdbg_table *nodes, mdbg_table **edges, uint64_t *checksum) try {
    if (!ctx || !nodes || !edges) return set_error(ctx, MDBG_EINVAL, "mdbg_edge_index: null argument");
    if (!nodes->has_vectors || nodes->k < 3) return set_error(ctx, MDBG_EINVAL, "mdbg_edge_index: needs a table with vectors (k <= firstK+1)");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint64_t n = nodes->n_records;
    DeviceTable tab;
    MDBG_TRY(build_table_adaptive(ctx, tab, n, 2 * n, [&](TableView v) {
        if (n) {
            LaunchTimer timer(ctx, "edge_index");
            hipLaunchKernelGGL(edge_insert_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, nodes->d_vec.p, n, nodes->k, v);
        }
        return MDBG_OK;
    }));
    return edges_from_table(ctx, tab, nodes->k - 1, edges, checksum);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_unitig_edge_index(mdbg_ctx *ctx, const mdbg_minimizers *unitigs, uint32_t k, mdbg_table **edges, uint64_t *checksum) try {
    if (!ctx || !edges || k < 3) return set_error(ctx, MDBG_EINVAL, "mdbg_unitig_edge_index: bad argument");
    MDBG_TRY(check_seq(ctx, unitigs, "mdbg_unitig_edge_index"));
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint64_t n = unitigs->n_reads;
    DeviceTable tab;
    MDBG_TRY(build_table_adaptive(ctx, tab, 2 * n, 4 * n, [&](TableView v) {
        if (n) {
            LaunchTimer timer(ctx, "edge_index");
            hipLaunchKernelGGL(unitig_edge_insert_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, unitigs->d_off.p, (uint32_t)n,
                               unitigs->d_min.p, k, v);
        }
        return MDBG_OK;
    }));
    return edges_from_table(ctx, tab, k - 1, edges, checksum);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_table_keys_to_host(mdbg_ctx *ctx, const mdbg_table *t, uint64_t *keys_lo_hi) try {
    if (!ctx || !t || (t->n_records && !keys_lo_hi)) return set_error(ctx, MDBG_EINVAL, "mdbg_table_keys_to_host: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (!t->n_records) return MDBG_OK;
    DevBuf<uint64_t> tmp;
    MDBG_TRY(tmp.alloc(ctx, t->n_records * 2));
    hipLaunchKernelGGL(interleave_keys_kernel, dim3(grid_for(t->n_records, 256)), dim3(256), 0, ctx->stream, t->d_lo.p, t->d_hi.p, t->n_records, tmp.p);
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, keys_lo_hi, tmp.p, t->n_records * 16, hipMemcpyDeviceToHost));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" void mdbg_table_free(mdbg_table *t) { delete t; }
