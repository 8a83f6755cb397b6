// verify.hip -- mdbg_minimizers_attach_strands / mdbg_map_verify: which of a target's selected neighbours read correction keeps
// (ReadCorrectionFunctor::filterAlignments, readSelection/ReadCorrection.hpp:5006-5117).  Per selected row: the anchors of the two reads
// at correction density, their chain, its summary, the verdict.  The rules -- which neighbour indexes a target minimizer meets, the
// summary of a chain, kept or not, the identity's table -- are verify_dev.hpp, the chain's own are mapper_dev.hpp; this file deals the work
// and moves the rows.
//
//   the lookup   every read of `reads` may be a neighbour of many targets, so the lookup of a read is made ONCE a call, not once a row: one
//                sort_u64_pairs over the set's minimizers, key = read << 32 | minimizer, value = the index in the read.  Stable, so a read's
//                piece [off[r], off[r + 1]) holds its minimizers ascending and equal ones in ascending index.
//   the join     one wave a row.  The neighbour's piece of the lookup is staged in LDS up to CHAIN_LDS_ANCHORS minimizers; a longer
//                neighbour is read where it lies -- the same code over another pointer.  The target's indexes are walked 64 a trip, a lane
//                binary-searches its minimizer's run.  count: the runs' lengths summed over the wave; an exclusive scan places the rows'
//                anchors.  fill: the same walk, a prefix sum over the trip's lanes gives every lane its place: anchors leave in (ri, qi)
//                order, which is the reference's sorted order.  No sort of anchors, no atomic.
//   the chains   one wave a row, rows drawn from a device counter (wave_draw); the dynamic programme is the mapper's, chain_wave
//                (chain_wave.hpp).  Lane 0 walks the parents twice -- length and root, then the gaps -- and writes the row: no match list
//                leaves the kernel.
//   the rows     one lane a row: the four tests, the identity by table; the kept rows are compacted behind a scan.
#include "common.hpp"
#include "objects.hpp"
#include "chain_wave.hpp"
#include "verify_dev.hpp"
#include "verify_join.hpp"
#include "realign_dev.hpp"

#include <algorithm>
#include <memory>
#include <vector>

namespace mdbg {

static_assert(sizeof(mdbg_verified) == 64, "a verified row is 64 bytes");
static_assert(sizeof(mdbg_verify_params) == 32, "mdbg_verify_params is 32 bytes");

// ---- the lookup ---------------------------------------------------------------------------------------------------------------------------
// one lane a minimizer of the set: the sort's key and value
__global__ __launch_bounds__(256) void verify_keys_kernel(const uint64_t *off, const uint32_t *mins, uint32_t n_reads, uint64_t n_min, uint64_t *keys, uint32_t *vals) {
    const WaveSpan sp = wave_span(n_min, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t r = csr_owner(off, n_reads, sp.begin);
    for (uint64_t x = sp.begin + (threadIdx.x & 63u); x < sp.end; x += 64u) {
        r = csr_owner_from(off, n_reads, x, r);
        keys[x] = ((uint64_t)r << 32) | mins[x];
        vals[x] = (uint32_t)(x - off[r]);
    }
}

// behind the sort: the minimizers alone (what a lane searches), and the longest read
__global__ __launch_bounds__(256) void verify_sorted_kernel(const uint64_t *keys, uint64_t n_min, uint32_t *sorted) {
    for (uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x; x < n_min; x += (uint64_t)gridDim.x * 256u) sorted[x] = (uint32_t)keys[x];
}

__global__ __launch_bounds__(256) void verify_longest_read_kernel(const uint64_t *off, uint32_t n_reads, unsigned long long *longest) {
    unsigned long long m = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * 256u) m = max(m, (unsigned long long)(off[r + 1u] - off[r]));
    m = wave_max_u64(m);
    if (lane_id() == 0 && m) atomicMax(longest, m);
}

// ---- the rows' reads ----------------------------------------------------------------------------------------------------------------------
// one lane a row: the target's and the neighbour's number in `reads`, or VERIFY_NO_READ
__global__ __launch_bounds__(256) void verify_row_reads_kernel(const uint64_t *sel_off, uint32_t n_targets, const mdbg_selected *sel, uint64_t n_rows, uint32_t target_first,
                                                               uint32_t reads_first, uint32_t n_reads, uint32_t *row_t, uint32_t *row_q) {
    const WaveSpan sp = wave_span(n_rows, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t t = csr_owner(sel_off, n_targets, sp.begin);
    for (uint64_t s = sp.begin + (threadIdx.x & 63u); s < sp.end; s += 64u) {
        t = csr_owner_from(sel_off, n_targets, s, t);
        row_t[s] = verify_local_read((uint64_t)target_first + t, reads_first, n_reads);
        row_q[s] = verify_local_read(sel[s].ref_read, reads_first, n_reads);
    }
}

// ---- the join -----------------------------------------------------------------------------------------------------------------------------
// One wave a row.  sorted / sorted_idx: the lookup.  FILL false: n_anchors[row] = the row's anchors (cut to 32 bits), placed[row] = those that
// are chained at all (verify_placed_anchors), *longest = the largest placed.  FILL true: the anchors of the rows with a_off[row + 1] >
// a_off[row], from a_off[row] on, in (ri, qi) order.  ORIENTED (mdbg_map_realign; the verifier's own form is compiled without it): the
// neighbour of a row with row_rev[row] set is seen reverse-complemented -- its run walked backwards, index, position and direction by
// realign_dev.hpp's oriented view -- so the anchors still leave in (ri, qi) order of the ORIENTED read.
template <bool FILL, bool ORIENTED>
__global__ __launch_bounds__(256) void verify_join_kernel(VerifyReads rd, const uint32_t *sorted, const uint32_t *sorted_idx, const uint32_t *row_t, const uint32_t *row_q,
                                                          uint64_t n_rows, uint32_t *n_anchors, uint32_t *placed, unsigned long long *longest, const uint64_t *a_off,
                                                          VerifyAnchors out, const uint8_t *row_rev) {
    __shared__ uint32_t s_key[4][CHAIN_LDS_ANCHORS];
    __shared__ uint32_t s_idx[4][CHAIN_LDS_ANCHORS];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * 256u) >> 6;
    for (uint64_t row = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; row < n_rows; row += n_waves) {
        // every turn begins at a point all lanes pass together (the last row's lanes have read the staged lookup before it is overwritten),
        // and what decides a row's path is the same in every lane (common.hpp, wave_draw)
        wave_lds_sync();
        const uint32_t tl = wave_uniform_u32(row_t[row]), ql = wave_uniform_u32(row_q[row]);
        const bool present = tl != VERIFY_NO_READ && ql != VERIFY_NO_READ;
        uint64_t base = 0, end = 0;
        if (FILL) { base = a_off[row]; end = a_off[row + 1u]; }
        const bool work = FILL ? end > base : present;
        uint64_t acc = 0;
        if (work) {
            const uint64_t t0 = rd.off[tl], q0 = rd.off[ql];
            const uint32_t n_t = wave_uniform_u32((uint32_t)(rd.off[tl + 1u] - t0)), n_q = wave_uniform_u32((uint32_t)(rd.off[ql + 1u] - q0));
            const bool in_lds = n_q <= CHAIN_LDS_ANCHORS;
            const uint32_t turned = ORIENTED ? wave_uniform_u32(row_rev[row]) : 0u, len_q = ORIENTED ? wave_uniform_u32(rd.len[ql]) : 0u;
            if (in_lds) {
                for (uint32_t k = lane; k < n_q; k += 64u) { s_key[wave][k] = sorted[q0 + k]; s_idx[wave][k] = sorted_idx[q0 + k]; }
                wave_lds_sync();
            }
            const uint32_t *keys = in_lds ? s_key[wave] : sorted + q0;
            const uint32_t *idx = in_lds ? s_idx[wave] : sorted_idx + q0;
            for (uint32_t i0 = 0; i0 < n_t; i0 += 64u) {
                const uint32_t i = i0 + lane;
                VerifyRun run{0u, 0u};
                if (i < n_t) run = verify_run(keys, n_q, rd.mins[t0 + i]);
                if (!FILL) { acc += run.count; continue; }
                const uint32_t incl = wave_inclusive_sum(run.count);
                const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
                uint64_t at = base + (incl - run.count);
                for (uint32_t k = 0; k < run.count; k++, at++) {
                    if (at >= end) break;                                        // (never, for counts this walk produced: nothing outside the row's room)
                    if (ORIENTED) {
                        const uint32_t j = idx[realign_run_entry(run.begin, run.count, k, turned)];
                        out.ri[at] = i; out.qi[at] = realign_oriented_index(j, n_q, turned); out.rpos[at] = rd.pos[t0 + i];
                        out.qpos[at] = realign_oriented_position(rd.pos[q0 + j], len_q, turned);
                        out.rev[at] = (uint8_t)map_anchor_reversed(rd.dir[t0 + i], realign_oriented_direction(rd.dir[q0 + j], turned));
                        continue;
                    }
                    const uint32_t j = idx[run.begin + k];
                    out.ri[at] = i; out.qi[at] = j; out.rpos[at] = rd.pos[t0 + i]; out.qpos[at] = rd.pos[q0 + j];
                    out.rev[at] = (uint8_t)map_anchor_reversed(rd.dir[t0 + i], rd.dir[q0 + j]);
                }
                base += total;
            }
        }
        if (!FILL) {
            acc = wave_sum_u64(acc);
            if (lane == 0) {
                const uint32_t p = verify_placed_anchors(acc);
                n_anchors[row] = acc > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)acc;
                placed[row] = p;
                if (p) atomicMax(longest, (unsigned long long)p);
            }
        }
    }
}

// ---- the chains ---------------------------------------------------------------------------------------------------------------------------
// One wave a row.  g_score / g_parent: as many as there are anchors, for the rows above CHAIN_LDS_ANCHORS (null when there is none).
// counters: [0] the next row, [1] chains found.  Every row is written, by lane 0: flags MDBG_VERIFY_CHAIN and the summary, or
// MDBG_VERIFY_ABSENT / MDBG_VERIFY_TOO_LONG / 0 and zero fields (n_anchors stays for a row without a chain).
__global__ __launch_bounds__(256) void verify_chain_kernel(VerifyReads rd, const mdbg_selected *sel, const uint32_t *row_t, const uint32_t *row_q, const uint32_t *n_anchors,
                                                           const uint64_t *a_off, uint64_t n_rows, const uint32_t *a_ri, const uint32_t *a_qi, const uint32_t *a_rpos,
                                                           const uint32_t *a_qpos, const uint8_t *a_rev, uint32_t band, unsigned long long *counters, int32_t *g_score,
                                                           uint32_t *g_parent, mdbg_verified *rows) {
    __shared__ int32_t s_score[4][CHAIN_LDS_ANCHORS];
    __shared__ uint32_t s_parent[4][CHAIN_LDS_ANCHORS];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    for (;;) {
        wave_lds_sync();          // the turn's common start, one path to its end (wave_draw); lane 0 has walked the last row's parents before they are overwritten
        const uint64_t p = wave_draw(counters);
        if (p >= n_rows) break;
        const uint64_t a0 = a_off[p];
        const uint32_t n = wave_uniform_u32((uint32_t)(a_off[p + 1u] - a0));     // 0: absent, fewer than 3 anchors, or too long -- not chained
        const bool in_lds = n <= CHAIN_LDS_ANCHORS;
        int32_t *score = in_lds ? s_score[wave] : g_score + a0;
        uint32_t *parent = in_lds ? s_parent[wave] : g_parent + a0;
        const ChainEnd end = chain_wave(n, a_rpos + a0, a_qpos + a0, a_rev + a0, band, score, parent, in_lds);
        if (lane == 0) {
            const uint32_t best_i = end.i;
            const uint32_t tl = row_t[p], ql = row_q[p], na = n_anchors[p];
            mdbg_verified row;
            row.neighbour = sel[p].ref_read;
            row.flags = tl == VERIFY_NO_READ || ql == VERIFY_NO_READ ? MDBG_VERIFY_ABSENT : na >= VERIFY_TOO_LONG_FROM ? MDBG_VERIFY_TOO_LONG : 0u;
            row.n_anchors = row.flags ? 0u : na;
            row.query_reversed = 0u; row.n_matches = row.n_mismatches = row.n_deletions = row.n_insertions = 0;
            row.overhang_start = row.overhang_end = row.align_length = row.n_seeds = row.reference_start = row.reference_end = row.query_start = row.query_end = 0u;
            uint32_t root = best_i;
            const uint32_t len = n ? map_chain_walk(parent, best_i, &root) : 0u;
            if (len >= VERIFY_MIN_CHAIN) {
                const uint32_t *ri = a_ri + a0, *qi = a_qi + a0;
                const uint32_t reversed = verify_query_reversed(qi[root], qi[best_i]);
                VerifyGaps gaps{0, 0, 0};
                for (uint32_t b = best_i, a = parent[b]; a != MAP_NO_PARENT; b = a, a = parent[a]) verify_gap(ri[a], qi[a], ri[b], qi[b], reversed, gaps);
                const uint64_t t0 = rd.off[tl], q0 = rd.off[ql];
                const VerifySummary s = verify_summary(len, gaps, ri[root], qi[root], ri[best_i], qi[best_i], rd.pos + t0, rd.pos + q0, (uint32_t)(rd.off[tl + 1u] - t0),
                                                       (uint32_t)(rd.off[ql + 1u] - q0), rd.len[tl], rd.len[ql]);
                row.flags = MDBG_VERIFY_CHAIN; row.query_reversed = s.query_reversed; row.n_matches = s.n_matches; row.n_mismatches = s.n_mismatches;
                row.n_deletions = s.n_deletions; row.n_insertions = s.n_insertions; row.overhang_start = s.overhang_start; row.overhang_end = s.overhang_end;
                row.align_length = s.align_length; row.n_seeds = s.n_seeds; row.reference_start = s.reference_start; row.reference_end = s.reference_end;
                row.query_start = s.query_start; row.query_end = s.query_end;
                atomicAdd(counters + 1, 1ull);
            }
            rows[p] = row;
        }
    }
}

// ---- the rows -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void verify_rows_kernel(mdbg_verified *rows, uint64_t n_rows, uint32_t max_overhang, uint32_t min_overlap_length, const uint32_t *min_matches,
                                                          uint32_t table_n, uint32_t *keep) {
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n_rows; s += (uint64_t)gridDim.x * 256u) {
        const mdbg_verified row = rows[s];
        const bool kept = (row.flags & MDBG_VERIFY_CHAIN) &&
                          verify_kept(row.overhang_start, row.overhang_end, row.align_length, row.n_matches, row.n_seeds, max_overhang, min_overlap_length, min_matches, table_n);
        if (kept) rows[s].flags = row.flags | MDBG_VERIFY_KEPT;
        keep[s] = kept ? 1u : 0u;
    }
}

// the kept rows behind the scan, and kept_offsets[t] = kept rows of the targets below t
__global__ __launch_bounds__(256) void verify_kept_kernel(const mdbg_verified *rows, const uint32_t *keep, const uint64_t *kpos, uint64_t n_rows, const uint64_t *row_off,
                                                          uint64_t n_targets, uint64_t *kept_off, uint32_t *kept_neighbour, uint8_t *kept_reversed) {
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n_rows; s += (uint64_t)gridDim.x * 256u) {
        if (!keep[s]) continue;
        kept_neighbour[kpos[s]] = rows[s].neighbour;
        kept_reversed[kpos[s]] = (uint8_t)rows[s].query_reversed;
    }
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t <= n_targets; t += (uint64_t)gridDim.x * 256u) kept_off[t] = kpos[row_off[t]];
}

const StepKernel *verify_step_kernels(uint32_t *n) {
    static const StepKernel k[] = {
        {"verify_keys", reinterpret_cast<const void *>(verify_keys_kernel), 256, 2},
        {"verify_sorted", reinterpret_cast<const void *>(verify_sorted_kernel), 256, 2},
        {"verify_longest_read", reinterpret_cast<const void *>(verify_longest_read_kernel), 256, 2},
        {"verify_row_reads", reinterpret_cast<const void *>(verify_row_reads_kernel), 256, 2},
        {"verify_join_count", reinterpret_cast<const void *>(verify_join_kernel<false, false>), 256, 2},
        {"verify_join_fill", reinterpret_cast<const void *>(verify_join_kernel<true, false>), 256, 2},
        {"verify_chain", reinterpret_cast<const void *>(verify_chain_kernel), 256, 2},
        {"verify_rows", reinterpret_cast<const void *>(verify_rows_kernel), 256, 2},
        {"verify_kept", reinterpret_cast<const void *>(verify_kept_kernel), 256, 2},
    };
    *n = (uint32_t)(sizeof(k) / sizeof(k[0]));
    return k;
}

int verify_lookup(mdbg_ctx *ctx, const char *timer, const VerifyReads &rd, uint64_t n_min, uint64_t *keys, uint32_t *sorted, uint32_t *sorted_idx) {
    if (!n_min) return MDBG_OK;
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    {
        LaunchTimer t(ctx, timer);
        hipLaunchKernelGGL(verify_keys_kernel, dim3(grid_for(n_min, 256, cap)), dim3(256), 0, ctx->stream, rd.off, rd.mins, rd.n_reads, n_min, keys, sorted_idx);
    }
    MDBG_TRY(sort_u64_pairs(ctx, keys, sorted_idx, n_min, nullptr));
    LaunchTimer t(ctx, timer);
    hipLaunchKernelGGL(verify_sorted_kernel, dim3(grid_for(n_min, 256, cap)), dim3(256), 0, ctx->stream, keys, n_min, sorted);
    return MDBG_OK;
}

void verify_join_count(mdbg_ctx *ctx, const VerifyReads &rd, const uint32_t *sorted, const uint32_t *sorted_idx, const uint32_t *row_t, const uint32_t *row_q, uint64_t n_rows,
                       uint32_t *n_anchors, uint32_t *placed, unsigned long long *longest) {
    hipLaunchKernelGGL((verify_join_kernel<false, false>), dim3(grid_for(n_rows, 4, (unsigned)ctx->n_cu * 4u)), dim3(256), 0, ctx->stream, rd, sorted, sorted_idx, row_t, row_q, n_rows,
                       n_anchors, placed, longest, nullptr, VerifyAnchors{nullptr, nullptr, nullptr, nullptr, nullptr}, nullptr);
}

const void *verify_join_fill_oriented_kernel() { return reinterpret_cast<const void *>(verify_join_kernel<true, true>); }

void verify_join_fill_oriented(mdbg_ctx *ctx, const VerifyReads &rd, const uint32_t *sorted, const uint32_t *sorted_idx, const uint32_t *row_t, const uint32_t *row_q,
                               const uint8_t *row_reversed, uint64_t n_rows, const uint64_t *a_off, const VerifyAnchors &out) {
    hipLaunchKernelGGL((verify_join_kernel<true, true>), dim3(grid_for(n_rows, 4, (unsigned)ctx->n_cu * 4u)), dim3(256), 0, ctx->stream, rd, sorted, sorted_idx, row_t, row_q, n_rows,
                       nullptr, nullptr, nullptr, a_off, out, row_reversed);
}

// a set mdbg_map_verify can read: positions, directions and read lengths present, CSR order
static int verify_set_ready(mdbg_ctx *ctx, const mdbg_minimizers *m) {
    if (!m->d_pos.p || !m->d_dir.p || !m->d_len.p)
        return set_error(ctx, MDBG_EINVAL, "mdbg_map_verify: the reads carry no %s (a scan output, its concat or thresholded form, or mdbg_minimizers_attach_positions + mdbg_minimizers_attach_strands; a slice carries values only)",
                         !m->d_pos.p ? "positions" : "directions and read lengths");
    return ensure_canonical(ctx, m);
}

static int verify_params_ok(mdbg_ctx *ctx, const char *who, const mdbg_verify_params *p) {
    if (p->max_chaining_band == 0) return set_error(ctx, MDBG_EINVAL, "%s: max_chaining_band is 0", who);
    if (p->minimizer_size == 0) return set_error(ctx, MDBG_EINVAL, "%s: minimizer_size is 0", who);
    if (p->min_identity != p->min_identity) return set_error(ctx, MDBG_EINVAL, "%s: min_identity is not a number", who);      // (it would pass every row: `identity < NaN` is false)
    return MDBG_OK;
}

}  // namespace mdbg

using namespace mdbg;

extern "C" uint32_t mdbg_verify_lds_anchors(void) { return CHAIN_LDS_ANCHORS; }

extern "C" int mdbg_verify_min_matches(const mdbg_verify_params *p, uint32_t n_seeds_max, uint32_t *min_matches) {
    if (!p || !min_matches || p->minimizer_size == 0 || p->min_identity != p->min_identity || n_seeds_max == 0xFFFFFFFFu) return MDBG_EINVAL;      // (2^32 - 1: s <= n_seeds_max would never end)
    for (uint32_t s = 0; s <= n_seeds_max; s++) min_matches[s] = verify_min_matches_search(s, p->minimizer_size, p->min_identity);
    return MDBG_OK;
}

extern "C" int mdbg_minimizers_attach_strands(mdbg_ctx *ctx, mdbg_minimizers *m, const uint8_t *directions, const uint32_t *read_lengths) try {
    if (!ctx || !m || (m->n_min && !directions) || (m->n_reads && !read_lengths)) return set_error(ctx, MDBG_EINVAL, "mdbg_minimizers_attach_strands: null argument");
    if (m->scattered || m->from_scan) return set_error(ctx, MDBG_EINVAL, "mdbg_minimizers_attach_strands: a scan output has its directions and read lengths");
    if (!m->d_pos.p) return set_error(ctx, MDBG_EINVAL, "mdbg_minimizers_attach_strands: the set carries no positions (mdbg_minimizers_attach_positions comes first)");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> off((size_t)m->n_reads + 1);
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, off.data(), m->d_off.p, off.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < m->n_reads; r++)
        for (uint64_t i = off[r]; i < off[r + 1]; i++)
            if (directions[i] > 1u)
                return set_error(ctx, MDBG_EINVAL, "mdbg_minimizers_attach_strands: read %u, minimizer %llu: direction %u is neither 0 nor 1", r,
                                 (unsigned long long)(i - off[r]), (unsigned)directions[i]);
    DevBuf<uint8_t> d;
    DevBuf<uint32_t> l;
    MDBG_TRY(d.alloc(ctx, m->n_min)); MDBG_TRY(l.alloc(ctx, m->n_reads));
    if (m->n_min) MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d.p, directions, m->n_min, hipMemcpyHostToDevice, ctx->stream));
    if (m->n_reads) MDBG_HIP_CHECK(ctx, hipMemcpyAsync(l.p, read_lengths, (size_t)m->n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    m->d_dir = std::move(d);
    m->d_len = std::move(l);
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_map_verify(mdbg_ctx *ctx, const mdbg_selection *sel, uint32_t target_first_read, const mdbg_minimizers *reads, uint32_t reads_first_read,
                               const mdbg_verify_params *p, mdbg_verification **out) try {
    if (!ctx || !sel || !reads || !p || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_map_verify: null argument");
    MDBG_TRY(verify_params_ok(ctx, "mdbg_map_verify", p));
    if ((uint64_t)target_first_read + sel->n_queries > (1ull << 32))
        return set_error(ctx, MDBG_EINVAL, "mdbg_map_verify: %llu targets from read %u leave the 32-bit read numbers", (unsigned long long)sel->n_queries, target_first_read);
    if ((uint64_t)reads_first_read + reads->n_reads > (1ull << 32))
        return set_error(ctx, MDBG_EINVAL, "mdbg_map_verify: %u reads from read %u leave the 32-bit read numbers", reads->n_reads, reads_first_read);
    if (sel->n_queries >= (1ull << 32) || sel->n_selected >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_map_verify: 2^32 targets or rows, or more");
    if (reads->n_min >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_map_verify: the reads have %llu minimizers, 2^32 or more", (unsigned long long)reads->n_min);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_TRY(verify_set_ready(ctx, reads));
    const unsigned cap = (unsigned)ctx->n_cu * 32u, wave_cap = (unsigned)ctx->n_cu * 4u;
    const uint64_t nt = sel->n_queries, nr = sel->n_selected, n_min = reads->n_min;
    const uint32_t n_reads = reads->n_reads;
    std::unique_ptr<mdbg_verification> v(new mdbg_verification());
    v->n_targets = nt; v->n_rows = nr;
    MDBG_TRY(v->d_row_off.alloc(ctx, (size_t)nt + 1)); MDBG_TRY(v->d_rows.alloc(ctx, nr)); MDBG_TRY(v->d_kept_off.alloc(ctx, (size_t)nt + 1));
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(v->d_row_off.p, sel->d_sel_off.p, ((size_t)nt + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (nr == 0) {
        MDBG_TRY(v->d_kept_neighbour.alloc(ctx, 0)); MDBG_TRY(v->d_kept_reversed.alloc(ctx, 0));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(v->d_kept_off.p, 0, ((size_t)nt + 1) * 8, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        *out = v.release();
        return MDBG_OK;
    }
    const VerifyReads rd{reads->d_off.p, reads->d_min.p, reads->d_pos.p, reads->d_dir.p, reads->d_len.p, n_reads, reads_first_read};

    // ---- the lookup, the rows' reads, the count: the totals that size the anchors are the first host wait --------------------------------
    DevBuf<uint64_t> keys, a_off;
    DevBuf<uint32_t> sorted, sorted_idx, row_t, row_q, n_anchors, placed;
    DevBuf<unsigned long long> longest;       // [0] the longest row, [1] the longest read
    MDBG_TRY(keys.alloc(ctx, n_min)); MDBG_TRY(sorted.alloc(ctx, n_min)); MDBG_TRY(sorted_idx.alloc(ctx, n_min));
    MDBG_TRY(row_t.alloc(ctx, nr)); MDBG_TRY(row_q.alloc(ctx, nr)); MDBG_TRY(n_anchors.alloc(ctx, nr)); MDBG_TRY(placed.alloc(ctx, nr));
    MDBG_TRY(a_off.alloc(ctx, (size_t)nr + 1)); MDBG_TRY(longest.alloc(ctx, 2));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(longest.p, 0, 16, ctx->stream));
    if (n_min) {
        {
            LaunchTimer timer(ctx, "verify_join");
            hipLaunchKernelGGL(verify_keys_kernel, dim3(grid_for(n_min, 256, cap)), dim3(256), 0, ctx->stream, rd.off, rd.mins, n_reads, n_min, keys.p, sorted_idx.p);
        }
        MDBG_TRY(sort_u64_pairs(ctx, keys.p, sorted_idx.p, n_min, nullptr));
    }
    const VerifyAnchors none{nullptr, nullptr, nullptr, nullptr, nullptr};
    {
        LaunchTimer timer(ctx, "verify_join");
        if (n_min) hipLaunchKernelGGL(verify_sorted_kernel, dim3(grid_for(n_min, 256, cap)), dim3(256), 0, ctx->stream, keys.p, n_min, sorted.p);
        if (n_reads) hipLaunchKernelGGL(verify_longest_read_kernel, dim3(grid_for(n_reads, 256, cap)), dim3(256), 0, ctx->stream, rd.off, n_reads, longest.p + 1);
        hipLaunchKernelGGL(verify_row_reads_kernel, dim3(grid_for(nr, 256, cap)), dim3(256), 0, ctx->stream, sel->d_sel_off.p, (uint32_t)nt, sel->d_rows.p, nr, target_first_read,
                           reads_first_read, n_reads, row_t.p, row_q.p);
        hipLaunchKernelGGL((verify_join_kernel<false, false>), dim3(grid_for(nr, 4, wave_cap)), dim3(256), 0, ctx->stream, rd, sorted.p, sorted_idx.p, row_t.p, row_q.p, nr,
                           n_anchors.p, placed.p, longest.p, nullptr, none, nullptr);
        MDBG_TRY(exclusive_scan_u32(ctx, placed.p, a_off.p, nr));
    }
    uint64_t total = 0;
    unsigned long long h_longest[2] = {0, 0};
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(h_longest, longest.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &total, a_off.p + nr, 8, hipMemcpyDeviceToHost));
    if (total >= (1ull << 32))
        return set_error(ctx, MDBG_ERANGE, "mdbg_map_verify: the %llu rows would produce %llu anchors, 2^32 or more; verify fewer targets in one call", (unsigned long long)nr,
                         (unsigned long long)total);

    // ---- fill ----------------------------------------------------------------------------------------------------------------------------
    DevBuf<uint32_t> a_ri, a_qi, a_rpos, a_qpos, g_parent, min_matches, keep;
    DevBuf<uint8_t> a_rev;
    DevBuf<int32_t> g_score;
    DevBuf<unsigned long long> counters;
    DevBuf<uint64_t> kpos;
    MDBG_TRY(a_ri.alloc(ctx, total)); MDBG_TRY(a_qi.alloc(ctx, total)); MDBG_TRY(a_rpos.alloc(ctx, total)); MDBG_TRY(a_qpos.alloc(ctx, total)); MDBG_TRY(a_rev.alloc(ctx, total));
    const bool spill = h_longest[0] > CHAIN_LDS_ANCHORS;      // some row's scores and parents do not fit LDS
    if (spill) { MDBG_TRY(g_score.alloc(ctx, total)); MDBG_TRY(g_parent.alloc(ctx, total)); }
    MDBG_TRY(counters.alloc(ctx, 2)); MDBG_TRY(keep.alloc(ctx, nr)); MDBG_TRY(kpos.alloc(ctx, (size_t)nr + 1));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(counters.p, 0, 16, ctx->stream));
    // the identity's table: n_seeds never exceeds the shorter read's minimizers (it is a count of one read's minimizers inside the alignment)
    const uint32_t table_n = (uint32_t)std::min<unsigned long long>(h_longest[1], 0xFFFFFFFEull) + 1u;
    std::vector<uint32_t> h_table(table_n);
    for (uint32_t s = 0; s < table_n; s++) h_table[s] = verify_min_matches_search(s, p->minimizer_size, p->min_identity);
    MDBG_TRY(min_matches.alloc(ctx, table_n));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, min_matches.p, h_table.data(), (size_t)table_n * 4, hipMemcpyHostToDevice));      // (the host table may go when this returns)
    if (total) {
        LaunchTimer timer(ctx, "verify_join");
        hipLaunchKernelGGL((verify_join_kernel<true, false>), dim3(grid_for(nr, 4, wave_cap)), dim3(256), 0, ctx->stream, rd, sorted.p, sorted_idx.p, row_t.p, row_q.p, nr, nullptr,
                           nullptr, nullptr, a_off.p, VerifyAnchors{a_ri.p, a_qi.p, a_rpos.p, a_qpos.p, a_rev.p}, nullptr);
    }
    // ---- chains, rows: the kept rows' count is the second host wait -----------------------------------------------------------------------
    {
        LaunchTimer timer(ctx, "verify_chains");
        hipLaunchKernelGGL(verify_chain_kernel, dim3(grid_for(nr, 4, wave_cap)), dim3(256), 0, ctx->stream, rd, sel->d_rows.p, row_t.p, row_q.p, n_anchors.p, a_off.p, nr, a_ri.p,
                           a_qi.p, a_rpos.p, a_qpos.p, a_rev.p, p->max_chaining_band, counters.p, spill ? g_score.p : nullptr, spill ? g_parent.p : nullptr, v->d_rows.p);
    }
    {
        LaunchTimer timer(ctx, "verify_rows");
        hipLaunchKernelGGL(verify_rows_kernel, dim3(grid_for(nr, 256, cap)), dim3(256), 0, ctx->stream, v->d_rows.p, nr, p->max_overhang, p->min_overlap_length, min_matches.p,
                           table_n, keep.p);
        MDBG_TRY(exclusive_scan_u32(ctx, keep.p, kpos.p, nr));
    }
    unsigned long long h_counters[2] = {0, 0};
    uint64_t n_kept = 0;
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(h_counters, counters.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &n_kept, kpos.p + nr, 8, hipMemcpyDeviceToHost));
    v->n_chains = h_counters[1]; v->n_kept = n_kept;
    MDBG_TRY(v->d_kept_neighbour.alloc(ctx, n_kept)); MDBG_TRY(v->d_kept_reversed.alloc(ctx, n_kept));
    {
        LaunchTimer timer(ctx, "verify_rows");
        hipLaunchKernelGGL(verify_kept_kernel, dim3(grid_for(std::max(nr, nt + 1), 256, cap)), dim3(256), 0, ctx->stream, v->d_rows.p, keep.p, kpos.p, nr, v->d_row_off.p, nt,
                           v->d_kept_off.p, v->d_kept_neighbour.p, v->d_kept_reversed.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));       // the transient buffers go back to the pool; the inputs must outlive the kernels
    *out = v.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_verification_info(const mdbg_verification *v, uint64_t info[4]) {
    if (!v || !info) return MDBG_EINVAL;
    info[0] = v->n_targets; info[1] = v->n_rows; info[2] = v->n_chains; info[3] = v->n_kept;
    return MDBG_OK;
}

extern "C" int mdbg_verification_to_host(mdbg_ctx *ctx, const mdbg_verification *v, uint64_t *row_offsets, mdbg_verified *rows, uint64_t *kept_offsets, uint32_t *kept_neighbour,
                                         uint8_t *kept_reversed) try {
    if (!ctx || !v) return set_error(ctx, MDBG_EINVAL, "mdbg_verification_to_host: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_HIP_CHECK(ctx, download_async(ctx, row_offsets, v->d_row_off.p, ((size_t)v->n_targets + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, rows, v->d_rows.p, (size_t)v->n_rows * sizeof(mdbg_verified)));
    MDBG_HIP_CHECK(ctx, download_async(ctx, kept_offsets, v->d_kept_off.p, ((size_t)v->n_targets + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, kept_neighbour, v->d_kept_neighbour.p, (size_t)v->n_kept * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, kept_reversed, v->d_kept_reversed.p, (size_t)v->n_kept));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_verification_device_ptrs(const mdbg_verification *v, const void *d_ptrs[5]) {
    if (!v || !d_ptrs) return MDBG_EINVAL;
    d_ptrs[0] = v->d_row_off.p; d_ptrs[1] = v->d_rows.p; d_ptrs[2] = v->d_kept_off.p; d_ptrs[3] = v->d_kept_neighbour.p; d_ptrs[4] = v->d_kept_reversed.p;
    return MDBG_OK;
}

extern "C" void mdbg_verification_free(mdbg_verification *v) { delete v; }
