// realign.hip -- mdbg_minimizers_attach_qualities / mdbg_map_realign: the kept (target, neighbour) pairs realigned at assembly density, as far
// as the POA graph (the first half of ReadCorrectionFunctor::performPoaCorrection4, readSelection/ReadCorrection.hpp:5217-5285).  Per kept
// row: both reads thinned, the neighbour turned round if the row says so, the anchors, their chain, the list _alignments, normalizeAlignment,
// and what Graph::addAlignment2 reads of every entry.  The rules are realign_dev.hpp (the oriented view, a link's entries, the runs at both
// ends, the normalisation step, the entry kind), verify_dev.hpp and mapper_dev.hpp; this file deals the work.
//
//   thin         the whole set once a call: mdbg_apply_density_threshold's flag, scan and compaction (density_thin), positions, directions
//                and qualities going along.  The backbone arrays are a gather of the listed targets out of it.
//   lookup/join  the verifier's (verify_join.hpp) over the thinned set; the fill sees the neighbour through the row's orientation.
//   the chains   one wave a row, chain_wave unchanged.  Lane 0 walks the parents twice: length and root, then the gaps -- and writes the row,
//                the chain's anchors (ri, qi) in ascending order where the row's anchors lie, and the raw length of its list.
//   the lists    one wave a row.  fill: the wave across the chain's links, 64 a trip, a prefix sum over their lengths gives every lane its
//                place; the runs at both ends lane-strided.  normalise: lane 0, serial, in LDS up to REALIGN_LDS_ENTRIES entries and in the
//                raw buffer above -- the same code over another pointer.  The survivors are counted; behind a scan a second kernel compacts
//                them into the final arrays and fills kind / minimizer / quality in the same pass.
#include "common.hpp"
#include "objects.hpp"
#include "chain_wave.hpp"
#include "verify_join.hpp"
#include "realign_dev.hpp"

#include <algorithm>
#include <memory>
#include <vector>

struct mdbg_realignment {
    uint64_t n_targets = 0, n_rows = 0, n_chains = 0, n_entries = 0, n_backbone = 0;
    mdbg::DevBuf<uint64_t> d_row_off;         // n_targets + 1
    mdbg::DevBuf<mdbg_realigned> d_rows;      // n_rows
    mdbg::DevBuf<uint64_t> d_entry_off;       // n_rows + 1
    mdbg::DevBuf<uint32_t> d_ref_index, d_query_index, d_query_min;      // n_entries
    mdbg::DevBuf<uint8_t> d_query_qual, d_kind;                          // n_entries
    mdbg::DevBuf<uint64_t> d_target_off;      // n_targets + 1
    mdbg::DevBuf<uint32_t> d_target_min;      // n_backbone
    mdbg::DevBuf<uint8_t> d_target_qual;      // n_backbone
};

namespace mdbg {

static_assert(sizeof(mdbg_realigned) == 48, "a realigned row is 48 bytes");
static_assert(sizeof(mdbg_realign_params) == 32, "mdbg_realign_params is 32 bytes");
static_assert(sizeof(RealignEntry) == 8, "an entry is two 32-bit indexes");

struct RealignThin { const uint64_t *off; const uint32_t *mins; const uint8_t *qual; };

// what lane 0 wrote (or the lanes, for lane 0) is seen by the wave's other lanes: LDS, or the wave's own piece of global memory
__device__ __forceinline__ void realign_wave_sync(bool in_lds) {
    if (in_lds) wave_lds_sync(); else { __threadfence_block(); __builtin_amdgcn_wave_barrier(); }
}

// ---- the rows' reads, the backbone -----------------------------------------------------------------------------------------------------------
// one lane a row: the target's and the neighbour's number in `reads` -- both VERIFY_NO_READ for a row that is not joined -- and why not
__global__ __launch_bounds__(256) void realign_row_reads_kernel(const uint64_t *kept_off, uint32_t n_targets, const uint32_t *kept_neighbour, uint64_t n_rows,
                                                                uint32_t target_first, uint32_t reads_first, uint32_t n_reads, const uint64_t *thin_off, uint32_t min_minimizers,
                                                                uint32_t *row_t, uint32_t *row_q, uint32_t *row_state) {
    const WaveSpan sp = wave_span(n_rows, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t t = csr_owner(kept_off, n_targets, sp.begin);
    for (uint64_t s = sp.begin + (threadIdx.x & 63u); s < sp.end; s += 64u) {
        t = csr_owner_from(kept_off, n_targets, s, t);
        const uint32_t tl = verify_local_read((uint64_t)target_first + t, reads_first, n_reads), ql = verify_local_read(kept_neighbour[s], reads_first, n_reads);
        uint32_t state = 0;
        if (tl == VERIFY_NO_READ || ql == VERIFY_NO_READ) state = MDBG_REALIGN_ABSENT;
        else if (realign_neighbour_short(thin_off[ql + 1u] - thin_off[ql], min_minimizers)) state = MDBG_REALIGN_SHORT;
        row_t[s] = state ? VERIFY_NO_READ : tl;
        row_q[s] = state ? VERIFY_NO_READ : ql;
        row_state[s] = state;
    }
}

__global__ __launch_bounds__(256) void realign_backbone_count_kernel(uint64_t n_targets, uint32_t target_first, uint32_t reads_first, uint32_t n_reads, const uint64_t *thin_off,
                                                                     uint32_t *count) {
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < n_targets; t += (uint64_t)gridDim.x * 256u) {
        const uint32_t tl = verify_local_read((uint64_t)target_first + t, reads_first, n_reads);
        count[t] = tl == VERIFY_NO_READ ? 0u : (uint32_t)(thin_off[tl + 1u] - thin_off[tl]);
    }
}

// one wave a target: T' out of the thinned set
__global__ __launch_bounds__(256) void realign_backbone_gather_kernel(uint64_t n_targets, uint32_t target_first, uint32_t reads_first, uint32_t n_reads, RealignThin thin,
                                                                      const uint64_t *target_off, uint32_t *target_min, uint8_t *target_qual) {
    const uint32_t lane = lane_id();
    const uint64_t n_waves = ((uint64_t)gridDim.x * 256u) >> 6;
    for (uint64_t t = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; t < n_targets; t += n_waves) {
        const uint32_t tl = verify_local_read((uint64_t)target_first + t, reads_first, n_reads);
        if (tl == VERIFY_NO_READ) continue;
        const uint64_t from = thin.off[tl], to = target_off[t];
        const uint64_t n = target_off[t + 1u] - to;
        for (uint64_t k = lane; k < n; k += 64u) { target_min[to + k] = thin.mins[from + k]; target_qual[to + k] = thin.qual[from + k]; }
    }
}

// ---- the chains -----------------------------------------------------------------------------------------------------------------------------
// One wave a row, as verify_chain_kernel.  counters: [0] the next row, [1] chains found.  Every row is written by lane 0; for a chain also
// c_ri / c_qi [a_off[p], a_off[p] + c_len[p]): its anchors, root first, and raw_len[p]: the length of its list before normalisation.
__global__ __launch_bounds__(256) void realign_chain_kernel(const uint64_t *thin_off, const uint32_t *kept_neighbour, const uint8_t *kept_reversed, const uint32_t *row_t,
                                                            const uint32_t *row_q, const uint32_t *row_state, const uint32_t *n_anchors, const uint64_t *a_off, uint64_t n_rows,
                                                            const uint32_t *a_ri, const uint32_t *a_qi, const uint32_t *a_rpos, const uint32_t *a_qpos, const uint8_t *a_rev,
                                                            uint32_t band, unsigned long long *counters, int32_t *g_score, uint32_t *g_parent, uint32_t *c_ri, uint32_t *c_qi,
                                                            uint32_t *c_len, uint32_t *raw_len, mdbg_realigned *rows) {
    __shared__ int32_t s_score[4][CHAIN_LDS_ANCHORS];
    __shared__ uint32_t s_parent[4][CHAIN_LDS_ANCHORS];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    for (;;) {
        wave_lds_sync();          // the turn's common start, one path to its end (wave_draw)
        const uint64_t p = wave_draw(counters);
        if (p >= n_rows) break;
        const uint64_t a0 = a_off[p];
        const uint32_t n = wave_uniform_u32((uint32_t)(a_off[p + 1u] - a0));     // 0: not joined, fewer than 3 anchors, or too long -- not chained
        const bool in_lds = n <= CHAIN_LDS_ANCHORS;
        int32_t *score = in_lds ? s_score[wave] : g_score + a0;
        uint32_t *parent = in_lds ? s_parent[wave] : g_parent + a0;
        const ChainEnd end = chain_wave(n, a_rpos + a0, a_qpos + a0, a_rev + a0, band, score, parent, in_lds);
        if (lane == 0) {
            const uint32_t best_i = end.i, state = row_state[p], na = n_anchors[p];
            mdbg_realigned row;
            row.neighbour = kept_neighbour[p];
            row.flags = state ? state : na >= VERIFY_TOO_LONG_FROM ? MDBG_REALIGN_TOO_LONG : 0u;
            row.oriented_reversed = row.flags ? 0u : kept_reversed[p];
            row.n_anchors = row.flags ? 0u : na;
            row.chain_reversed = 0u; row.n_entries = 0u; row.n_matches = row.n_mismatches = row.n_deletions = row.n_insertions = 0;
            row.reference_start_index = row.reference_end_index = 0u;
            uint32_t root = best_i, raw = 0u, kept_len = 0u;
            const uint32_t len = n ? map_chain_walk(parent, best_i, &root) : 0u;
            if (len >= VERIFY_MIN_CHAIN) {
                const uint32_t *ri = a_ri + a0, *qi = a_qi + a0;
                const uint32_t reversed = verify_query_reversed(qi[root], qi[best_i]);
                VerifyGaps gaps{0, 0, 0};
                uint64_t links = 0;
                uint32_t at = len - 1u;
                c_ri[a0 + at] = ri[best_i]; c_qi[a0 + at] = qi[best_i];
                for (uint32_t b = best_i, a = parent[b]; a != MAP_NO_PARENT; b = a, a = parent[a]) {
                    verify_gap(ri[a], qi[a], ri[b], qi[b], reversed, gaps);
                    links += realign_link_length(realign_link(ri[a], qi[a], ri[b], qi[b], reversed));
                    at--;
                    c_ri[a0 + at] = ri[a]; c_qi[a0 + at] = qi[a];
                }
                const uint32_t tl = row_t[p], ql = row_q[p];
                const VerifyEdges edge = verify_edge_mismatches(reversed, ri[root], qi[root], ri[best_i], qi[best_i], (uint32_t)(thin_off[tl + 1u] - thin_off[tl]),
                                                                (uint32_t)(thin_off[ql + 1u] - thin_off[ql]));
                row.flags = MDBG_REALIGN_CHAIN; row.chain_reversed = reversed; row.n_matches = (int32_t)len;
                row.n_mismatches = (int32_t)edge.start_mis + gaps.mismatches + (int32_t)edge.end_mis;
                row.n_deletions = gaps.deletions; row.n_insertions = gaps.insertions;
                row.reference_start_index = ri[root]; row.reference_end_index = ri[best_i];
                raw = (uint32_t)realign_raw_length((uint64_t)edge.start_mis, links, (uint64_t)edge.end_mis);
                kept_len = len;
                atomicAdd(counters + 1, 1ull);
            }
            c_len[p] = kept_len;
            raw_len[p] = raw;
            rows[p] = row;
        }
    }
}

// ---- the lists ------------------------------------------------------------------------------------------------------------------------------
// One wave a row with a chain: the raw list into LDS (raw_off[p + 1] - raw_off[p] <= REALIGN_LDS_ENTRIES) or into g_raw where it lies,
// normalised by lane 0, left in g_raw with its tombstones; n_final[p] and the row's n_entries: the survivors.
__global__ __launch_bounds__(256) void realign_lists_kernel(RealignThin thin, const uint8_t *kept_reversed, const uint32_t *row_t, const uint32_t *row_q, const uint64_t *a_off,
                                                            const uint32_t *c_ri, const uint32_t *c_qi, const uint32_t *c_len, const uint64_t *raw_off, uint64_t n_rows,
                                                            RealignEntry *g_raw, uint32_t *n_final, mdbg_realigned *rows) {
    __shared__ RealignEntry s_list[4][REALIGN_LDS_ENTRIES];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * 256u) >> 6;
    for (uint64_t p = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; p < n_rows; p += n_waves) {
        wave_lds_sync();          // the last row's lanes have read the list before it is overwritten
        const uint64_t raw0 = raw_off[p];
        const uint32_t n_raw = wave_uniform_u32((uint32_t)(raw_off[p + 1u] - raw0));
        uint32_t alive = 0;
        if (n_raw) {
            const bool in_lds = n_raw <= REALIGN_LDS_ENTRIES;
            RealignEntry *list = in_lds ? s_list[wave] : g_raw + raw0;
            const uint32_t tl = wave_uniform_u32(row_t[p]), ql = wave_uniform_u32(row_q[p]), clen = wave_uniform_u32(c_len[p]);
            const uint64_t t0 = thin.off[tl], q0 = thin.off[ql];
            const uint32_t n_t = (uint32_t)(thin.off[tl + 1u] - t0), n_q = (uint32_t)(thin.off[ql + 1u] - q0);
            const uint32_t *ri = c_ri + a_off[p], *qi = c_qi + a_off[p];
            const uint32_t f_ri = ri[0], f_qi = qi[0], l_ri = ri[clen - 1u], l_qi = qi[clen - 1u];
            const uint32_t crev = verify_query_reversed(f_qi, l_qi);
            const VerifyEdges edge = verify_edge_mismatches(crev, f_ri, f_qi, l_ri, l_qi, n_t, n_q);
            const uint32_t start_mis = (uint32_t)edge.start_mis, end_mis = (uint32_t)edge.end_mis;
            // every store is held inside the row's room [0, n_raw): nothing is written outside it
            for (uint32_t k = lane; k < start_mis; k += 64u)
                if (k < n_raw) list[k] = realign_start_entry(f_ri, f_qi, start_mis, crev, k);
            uint32_t base = start_mis;
            for (uint32_t k0 = 0; k0 + 1u < clen; k0 += 64u) {
                const uint32_t k = k0 + lane;
                const bool mine = k + 1u < clen;
                RealignLink link{0u, 0u};
                uint32_t a_r = 0, a_q = 0;
                if (mine) { a_r = ri[k]; a_q = qi[k]; link = realign_link(a_r, a_q, ri[k + 1u], qi[k + 1u], crev); }
                const uint32_t mine_len = mine ? realign_link_length(link) : 0u;
                const uint32_t incl = wave_inclusive_sum(mine_len);
                const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
                const uint32_t at = base + (incl - mine_len);
                for (uint32_t e = 0; e < mine_len; e++)
                    if (at + e < n_raw) list[at + e] = realign_link_entry(a_r, a_q, link, crev, e);
                base += total;
            }
            for (uint32_t k = lane; k <= end_mis; k += 64u)
                if (base + k < n_raw) list[base + k] = realign_end_entry(l_ri, l_qi, crev, k);
            realign_wave_sync(in_lds);
            if (lane == 0) {
                const RealignQuery q{thin.mins + q0, thin.qual + q0, n_q, (uint32_t)kept_reversed[p]};
                realign_normalize(list, n_raw, thin.mins + t0, q);
            }
            realign_wave_sync(in_lds);
            for (uint32_t k = lane; k < n_raw; k += 64u) {
                const RealignEntry e = list[k];
                if (in_lds) g_raw[raw0 + k] = e;
                alive += realign_tombstone(e) ? 0u : 1u;
            }
        }
        alive = (uint32_t)wave_sum_u64(alive);
        if (lane == 0) {
            n_final[p] = alive;
            if (n_raw) rows[p].n_entries = alive;
        }
    }
}

// One wave a row: the survivors of g_raw behind entry_off[p], in order, with what addAlignment2 reads of each.
__global__ __launch_bounds__(256) void realign_compact_kernel(RealignThin thin, const uint8_t *kept_reversed, const uint32_t *row_t, const uint32_t *row_q, const uint64_t *raw_off,
                                                              const RealignEntry *g_raw, const uint64_t *entry_off, uint64_t n_rows, uint32_t *ref_index, uint32_t *query_index,
                                                              uint32_t *query_min, uint8_t *query_qual, uint8_t *kind) {
    const uint32_t lane = lane_id();
    const uint64_t n_waves = ((uint64_t)gridDim.x * 256u) >> 6;
    for (uint64_t p = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; p < n_rows; p += n_waves) {
        const uint64_t raw0 = raw_off[p], e0 = entry_off[p], e1 = entry_off[p + 1u];
        const uint32_t n_raw = wave_uniform_u32((uint32_t)(raw_off[p + 1u] - raw0));
        if (!n_raw) continue;
        const uint32_t tl = wave_uniform_u32(row_t[p]), ql = wave_uniform_u32(row_q[p]);
        const uint64_t t0 = thin.off[tl], q0 = thin.off[ql];
        const RealignQuery q{thin.mins + q0, thin.qual + q0, (uint32_t)(thin.off[ql + 1u] - q0), (uint32_t)kept_reversed[p]};
        uint64_t base = e0;
        for (uint32_t k0 = 0; k0 < n_raw; k0 += 64u) {
            const uint32_t k = k0 + lane;
            RealignEntry e{REALIGN_NONE, REALIGN_NONE};
            if (k < n_raw) e = g_raw[raw0 + k];
            const uint32_t keep = realign_tombstone(e) ? 0u : 1u;
            const uint32_t incl = wave_inclusive_sum(keep);
            const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
            const uint64_t at = base + (incl - keep);
            if (keep && at < e1) {
                const bool has_q = e.q != REALIGN_NONE;
                ref_index[at] = e.r; query_index[at] = e.q;
                query_min[at] = has_q ? realign_query_minimizer(q, e.q) : 0u;
                query_qual[at] = has_q ? realign_query_quality(q, e.q) : (uint8_t)0;
                kind[at] = realign_kind(e, thin.mins + t0, q);
            }
            base += total;
        }
    }
}

const StepKernel *realign_step_kernels(uint32_t *n) {
    static const StepKernel k[] = {
        {"realign_join_fill", verify_join_fill_oriented_kernel(), 256, 2},
        {"realign_row_reads", reinterpret_cast<const void *>(realign_row_reads_kernel), 256, 2},
        {"realign_backbone_count", reinterpret_cast<const void *>(realign_backbone_count_kernel), 256, 2},
        {"realign_backbone_gather", reinterpret_cast<const void *>(realign_backbone_gather_kernel), 256, 2},
        {"realign_chain", reinterpret_cast<const void *>(realign_chain_kernel), 256, 2},
        {"realign_lists", reinterpret_cast<const void *>(realign_lists_kernel), 256, 2},
        {"realign_compact", reinterpret_cast<const void *>(realign_compact_kernel), 256, 2},
    };
    *n = (uint32_t)(sizeof(k) / sizeof(k[0]));
    return k;
}

// The call behind both entry points.  d_kept_*: the kept lists on the device (nt + 1 offsets, nr rows).
static int realign_run(mdbg_ctx *ctx, const char *who, uint64_t nt, uint64_t nr, const uint64_t *d_kept_off, const uint32_t *d_kept_neighbour, const uint8_t *d_kept_reversed,
                       uint32_t target_first_read, const mdbg_minimizers *reads, uint32_t reads_first_read, const mdbg_realign_params *p, mdbg_realignment **out) {
    if (p->max_chaining_band == 0) return set_error(ctx, MDBG_EINVAL, "%s: max_chaining_band is 0", who);
    if (!(p->assembly_density > 0.0f)) return set_error(ctx, MDBG_EINVAL, "%s: assembly_density must be > 0", who);
    if (p->min_minimizers == 0) return set_error(ctx, MDBG_EINVAL, "%s: min_minimizers is 0", who);
    if (nt >= (1ull << 32) || nr >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "%s: 2^32 targets or rows, or more", who);
    if ((uint64_t)target_first_read + nt > (1ull << 32))
        return set_error(ctx, MDBG_EINVAL, "%s: %llu targets from read %u leave the 32-bit read numbers", who, (unsigned long long)nt, target_first_read);
    if ((uint64_t)reads_first_read + reads->n_reads > (1ull << 32))
        return set_error(ctx, MDBG_EINVAL, "%s: %u reads from read %u leave the 32-bit read numbers", who, reads->n_reads, reads_first_read);
    if (reads->n_min >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "%s: the reads have %llu minimizers, 2^32 or more", who, (unsigned long long)reads->n_min);
    if (!reads->d_pos.p || !reads->d_dir.p || !reads->d_len.p)
        return set_error(ctx, MDBG_EINVAL, "%s: the reads carry no %s (a scan output, its concat or thresholded form, or mdbg_minimizers_attach_positions + mdbg_minimizers_attach_strands; a slice carries values only)",
                         who, !reads->d_pos.p ? "positions" : "directions and read lengths");
    MDBG_TRY(ensure_canonical(ctx, reads));
    const unsigned cap = (unsigned)ctx->n_cu * 32u, wave_cap = (unsigned)ctx->n_cu * 4u;
    const uint32_t n_reads = reads->n_reads;
    std::unique_ptr<mdbg_realignment> r(new mdbg_realignment());
    r->n_targets = nt; r->n_rows = nr;
    MDBG_TRY(r->d_row_off.alloc(ctx, (size_t)nt + 1)); MDBG_TRY(r->d_rows.alloc(ctx, nr)); MDBG_TRY(r->d_entry_off.alloc(ctx, (size_t)nr + 1));
    MDBG_TRY(r->d_target_off.alloc(ctx, (size_t)nt + 1));
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(r->d_row_off.p, d_kept_off, ((size_t)nt + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));

    // ---- thin: the set at assembly density, positions, directions and qualities going along (the kept count is its host wait) ---------------
    DevBuf<uint8_t> no_qual;
    const uint8_t *qual = reads->d_mqual.p;
    if (!qual) {
        MDBG_TRY(no_qual.alloc(ctx, reads->n_min));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(no_qual.p, 0, std::max<size_t>(reads->n_min, 1), ctx->stream));
        qual = no_qual.p;
    }
    mdbg_minimizers thinned;
    MDBG_TRY(density_thin(ctx, reads, p->assembly_density, reads->d_pos.p, reads->d_dir.p, qual, "realign_thin", &thinned));
    const uint64_t n_min = thinned.n_min;
    const RealignThin thin{thinned.d_off.p, thinned.d_min.p, thinned.d_mqual.p};
    const VerifyReads rd{thinned.d_off.p, thinned.d_min.p, thinned.d_pos.p, thinned.d_dir.p, reads->d_len.p, n_reads, reads_first_read};

    // ---- the backbone's sizes; the lookup, the rows' reads, the count: the totals that size the anchors are the next host wait ------------------
    DevBuf<uint32_t> t_count;
    MDBG_TRY(t_count.alloc(ctx, nt));
    {
        LaunchTimer timer(ctx, "realign_thin");
        if (nt) hipLaunchKernelGGL(realign_backbone_count_kernel, dim3(grid_for(nt, 256, cap)), dim3(256), 0, ctx->stream, nt, target_first_read, reads_first_read, n_reads,
                                   thin.off, t_count.p);
        MDBG_TRY(exclusive_scan_u32(ctx, t_count.p, r->d_target_off.p, nt));
    }
    DevBuf<uint64_t> keys, a_off;
    DevBuf<uint32_t> sorted, sorted_idx, row_t, row_q, row_state, n_anchors, placed;
    DevBuf<unsigned long long> longest;
    uint64_t total = 0;
    unsigned long long h_longest = 0;
    if (nr) {
        MDBG_TRY(keys.alloc(ctx, n_min)); MDBG_TRY(sorted.alloc(ctx, n_min)); MDBG_TRY(sorted_idx.alloc(ctx, n_min));
        MDBG_TRY(row_t.alloc(ctx, nr)); MDBG_TRY(row_q.alloc(ctx, nr)); MDBG_TRY(row_state.alloc(ctx, nr)); MDBG_TRY(n_anchors.alloc(ctx, nr)); MDBG_TRY(placed.alloc(ctx, nr));
        MDBG_TRY(a_off.alloc(ctx, (size_t)nr + 1)); MDBG_TRY(longest.alloc(ctx, 1));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(longest.p, 0, 8, ctx->stream));
        MDBG_TRY(verify_lookup(ctx, "realign_join", rd, n_min, keys.p, sorted.p, sorted_idx.p));
        LaunchTimer timer(ctx, "realign_join");
        hipLaunchKernelGGL(realign_row_reads_kernel, dim3(grid_for(nr, 256, cap)), dim3(256), 0, ctx->stream, d_kept_off, (uint32_t)nt, d_kept_neighbour, nr, target_first_read,
                           reads_first_read, n_reads, thin.off, p->min_minimizers, row_t.p, row_q.p, row_state.p);
        verify_join_count(ctx, rd, sorted.p, sorted_idx.p, row_t.p, row_q.p, nr, n_anchors.p, placed.p, longest.p);
        MDBG_TRY(exclusive_scan_u32(ctx, placed.p, a_off.p, nr));
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(&h_longest, longest.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(&total, a_off.p + nr, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &r->n_backbone, r->d_target_off.p + nt, 8, hipMemcpyDeviceToHost));
    if (total >= (1ull << 32))
        return set_error(ctx, MDBG_ERANGE, "%s: the %llu rows would produce %llu anchors, 2^32 or more; realign fewer targets in one call", who, (unsigned long long)nr,
                         (unsigned long long)total);
    MDBG_TRY(r->d_target_min.alloc(ctx, r->n_backbone)); MDBG_TRY(r->d_target_qual.alloc(ctx, r->n_backbone));
    if (r->n_backbone) {
        LaunchTimer timer(ctx, "realign_thin");
        hipLaunchKernelGGL(realign_backbone_gather_kernel, dim3(grid_for(nt, 4, wave_cap)), dim3(256), 0, ctx->stream, nt, target_first_read, reads_first_read, n_reads, thin,
                           r->d_target_off.p, r->d_target_min.p, r->d_target_qual.p);
    }
    if (nr == 0) {
        MDBG_TRY(r->d_ref_index.alloc(ctx, 0)); MDBG_TRY(r->d_query_index.alloc(ctx, 0)); MDBG_TRY(r->d_query_min.alloc(ctx, 0));
        MDBG_TRY(r->d_query_qual.alloc(ctx, 0)); MDBG_TRY(r->d_kind.alloc(ctx, 0));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(r->d_entry_off.p, 0, 8, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipGetLastError());
        MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        *out = r.release();
        return MDBG_OK;
    }

    // ---- fill, chains: the raw entries' total is the next host wait ---------------------------------------------------------------------------
    DevBuf<uint32_t> a_ri, a_qi, a_rpos, a_qpos, g_parent, c_ri, c_qi, c_len, raw_len, n_final;
    DevBuf<uint8_t> a_rev;
    DevBuf<int32_t> g_score;
    DevBuf<unsigned long long> counters;
    DevBuf<uint64_t> raw_off;
    MDBG_TRY(a_ri.alloc(ctx, total)); MDBG_TRY(a_qi.alloc(ctx, total)); MDBG_TRY(a_rpos.alloc(ctx, total)); MDBG_TRY(a_qpos.alloc(ctx, total)); MDBG_TRY(a_rev.alloc(ctx, total));
    MDBG_TRY(c_ri.alloc(ctx, total)); MDBG_TRY(c_qi.alloc(ctx, total));
    const bool spill = h_longest > CHAIN_LDS_ANCHORS;
    if (spill) { MDBG_TRY(g_score.alloc(ctx, total)); MDBG_TRY(g_parent.alloc(ctx, total)); }
    MDBG_TRY(counters.alloc(ctx, 2)); MDBG_TRY(c_len.alloc(ctx, nr)); MDBG_TRY(raw_len.alloc(ctx, nr)); MDBG_TRY(n_final.alloc(ctx, nr)); MDBG_TRY(raw_off.alloc(ctx, (size_t)nr + 1));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(counters.p, 0, 16, ctx->stream));
    if (total) {
        LaunchTimer timer(ctx, "realign_join");
        verify_join_fill_oriented(ctx, rd, sorted.p, sorted_idx.p, row_t.p, row_q.p, d_kept_reversed, nr, a_off.p, VerifyAnchors{a_ri.p, a_qi.p, a_rpos.p, a_qpos.p, a_rev.p});
    }
    {
        LaunchTimer timer(ctx, "realign_chains");
        hipLaunchKernelGGL(realign_chain_kernel, dim3(grid_for(nr, 4, wave_cap)), dim3(256), 0, ctx->stream, thin.off, d_kept_neighbour, d_kept_reversed, row_t.p, row_q.p, row_state.p,
                           n_anchors.p, a_off.p, nr, a_ri.p, a_qi.p, a_rpos.p, a_qpos.p, a_rev.p, p->max_chaining_band, counters.p, spill ? g_score.p : nullptr,
                           spill ? g_parent.p : nullptr, c_ri.p, c_qi.p, c_len.p, raw_len.p, r->d_rows.p);
        MDBG_TRY(exclusive_scan_u32(ctx, raw_len.p, raw_off.p, nr));
    }
    unsigned long long h_counters[2] = {0, 0};
    uint64_t raw_total = 0;
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(h_counters, counters.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &raw_total, raw_off.p + nr, 8, hipMemcpyDeviceToHost));
    r->n_chains = h_counters[1];
    if (raw_total >= (1ull << 32))
        return set_error(ctx, MDBG_ERANGE, "%s: the %llu rows would produce %llu entries, 2^32 or more; realign fewer targets in one call", who, (unsigned long long)nr,
                         (unsigned long long)raw_total);

    // ---- lists: the survivors' total is the last host wait ------------------------------------------------------------------------------------
    DevBuf<RealignEntry> g_raw;
    MDBG_TRY(g_raw.alloc(ctx, raw_total));
    {
        LaunchTimer timer(ctx, "realign_lists");
        hipLaunchKernelGGL(realign_lists_kernel, dim3(grid_for(nr, 4, wave_cap)), dim3(256), 0, ctx->stream, thin, d_kept_reversed, row_t.p, row_q.p, a_off.p, c_ri.p, c_qi.p, c_len.p,
                           raw_off.p, nr, g_raw.p, n_final.p, r->d_rows.p);
        MDBG_TRY(exclusive_scan_u32(ctx, n_final.p, r->d_entry_off.p, nr));
    }
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &r->n_entries, r->d_entry_off.p + nr, 8, hipMemcpyDeviceToHost));
    MDBG_TRY(r->d_ref_index.alloc(ctx, r->n_entries)); MDBG_TRY(r->d_query_index.alloc(ctx, r->n_entries)); MDBG_TRY(r->d_query_min.alloc(ctx, r->n_entries));
    MDBG_TRY(r->d_query_qual.alloc(ctx, r->n_entries)); MDBG_TRY(r->d_kind.alloc(ctx, r->n_entries));
    if (r->n_entries) {
        LaunchTimer timer(ctx, "realign_lists");
        hipLaunchKernelGGL(realign_compact_kernel, dim3(grid_for(nr, 4, wave_cap)), dim3(256), 0, ctx->stream, thin, d_kept_reversed, row_t.p, row_q.p, raw_off.p, g_raw.p,
                           r->d_entry_off.p, nr, r->d_ref_index.p, r->d_query_index.p, r->d_query_min.p, r->d_query_qual.p, r->d_kind.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));       // the transient buffers go back to the pool; the inputs must outlive the kernels
    *out = r.release();
    return MDBG_OK;
}

}  // namespace mdbg

using namespace mdbg;

extern "C" uint32_t mdbg_realign_lds_entries(void) { return REALIGN_LDS_ENTRIES; }

extern "C" int mdbg_minimizers_attach_qualities(mdbg_ctx *ctx, mdbg_minimizers *m, const uint8_t *qualities) try {
    if (!ctx || !m || (m->n_min && !qualities)) return set_error(ctx, MDBG_EINVAL, "mdbg_minimizers_attach_qualities: null argument");
    if (m->scattered || m->from_scan) return set_error(ctx, MDBG_EINVAL, "mdbg_minimizers_attach_qualities: a scan output has its qualities");
    if (!m->d_pos.p) return set_error(ctx, MDBG_EINVAL, "mdbg_minimizers_attach_qualities: the set carries no positions (mdbg_minimizers_attach_positions comes first)");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DevBuf<uint8_t> q;
    MDBG_TRY(q.alloc(ctx, m->n_min));
    if (m->n_min) MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, q.p, qualities, m->n_min, hipMemcpyHostToDevice));
    m->d_mqual = std::move(q);
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_map_realign(mdbg_ctx *ctx, const mdbg_verification *v, uint32_t target_first_read, const mdbg_minimizers *reads, uint32_t reads_first_read,
                                const mdbg_realign_params *p, mdbg_realignment **out) try {
    if (!ctx || !v || !reads || !p || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_map_realign: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return realign_run(ctx, "mdbg_map_realign", v->n_targets, v->n_kept, v->d_kept_off.p, v->d_kept_neighbour.p, v->d_kept_reversed.p, target_first_read, reads, reads_first_read, p,
                       out);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_map_realign_pairs(mdbg_ctx *ctx, uint64_t n_targets, const uint64_t *kept_offsets, const uint32_t *kept_neighbour, const uint8_t *kept_reversed,
                                      uint32_t target_first_read, const mdbg_minimizers *reads, uint32_t reads_first_read, const mdbg_realign_params *p,
                                      mdbg_realignment **out) try {
    if (!ctx || !kept_offsets || !reads || !p || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_map_realign_pairs: null argument");
    if (n_targets >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_map_realign_pairs: 2^32 targets or more");
    if (kept_offsets[0] != 0) return set_error(ctx, MDBG_EINVAL, "mdbg_map_realign_pairs: kept_offsets[0] is not 0");
    for (uint64_t t = 0; t < n_targets; t++)
        if (kept_offsets[t + 1] < kept_offsets[t]) return set_error(ctx, MDBG_EINVAL, "mdbg_map_realign_pairs: kept_offsets fall at target %llu", (unsigned long long)t);
    const uint64_t nr = kept_offsets[n_targets];
    if (nr >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_map_realign_pairs: 2^32 rows or more");
    if (nr && (!kept_neighbour || !kept_reversed)) return set_error(ctx, MDBG_EINVAL, "mdbg_map_realign_pairs: null argument");
    for (uint64_t s = 0; s < nr; s++)
        if (kept_reversed[s] > 1u) return set_error(ctx, MDBG_EINVAL, "mdbg_map_realign_pairs: row %llu: kept_reversed %u is neither 0 nor 1", (unsigned long long)s, (unsigned)kept_reversed[s]);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DevBuf<uint64_t> d_off;
    DevBuf<uint32_t> d_nb;
    DevBuf<uint8_t> d_rev;
    MDBG_TRY(d_off.alloc(ctx, (size_t)n_targets + 1)); MDBG_TRY(d_nb.alloc(ctx, nr)); MDBG_TRY(d_rev.alloc(ctx, nr));
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d_off.p, kept_offsets, ((size_t)n_targets + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (nr) {
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d_nb.p, kept_neighbour, (size_t)nr * 4, hipMemcpyHostToDevice, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipMemcpyAsync(d_rev.p, kept_reversed, (size_t)nr, hipMemcpyHostToDevice, ctx->stream));
    }
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));       // (the host arrays may go when this returns)
    return realign_run(ctx, "mdbg_map_realign_pairs", n_targets, nr, d_off.p, d_nb.p, d_rev.p, target_first_read, reads, reads_first_read, p, out);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_realignment_info(const mdbg_realignment *r, uint64_t info[4]) {
    if (!r || !info) return MDBG_EINVAL;
    info[0] = r->n_targets; info[1] = r->n_rows; info[2] = r->n_chains; info[3] = r->n_entries;
    return MDBG_OK;
}

extern "C" int mdbg_realignment_to_host(mdbg_ctx *ctx, const mdbg_realignment *r, uint64_t *row_offsets, mdbg_realigned *rows, uint64_t *entry_offsets, uint32_t *ref_index,
                                        uint32_t *query_index, uint32_t *query_minimizer, uint8_t *query_quality, uint8_t *kind, uint64_t *target_offsets,
                                        uint32_t *target_minimizer, uint8_t *target_quality) try {
    if (!ctx || !r) return set_error(ctx, MDBG_EINVAL, "mdbg_realignment_to_host: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_HIP_CHECK(ctx, download_async(ctx, row_offsets, r->d_row_off.p, ((size_t)r->n_targets + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, rows, r->d_rows.p, (size_t)r->n_rows * sizeof(mdbg_realigned)));
    MDBG_HIP_CHECK(ctx, download_async(ctx, entry_offsets, r->d_entry_off.p, ((size_t)r->n_rows + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, ref_index, r->d_ref_index.p, (size_t)r->n_entries * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, query_index, r->d_query_index.p, (size_t)r->n_entries * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, query_minimizer, r->d_query_min.p, (size_t)r->n_entries * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, query_quality, r->d_query_qual.p, (size_t)r->n_entries));
    MDBG_HIP_CHECK(ctx, download_async(ctx, kind, r->d_kind.p, (size_t)r->n_entries));
    MDBG_HIP_CHECK(ctx, download_async(ctx, target_offsets, r->d_target_off.p, ((size_t)r->n_targets + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, target_minimizer, r->d_target_min.p, (size_t)r->n_backbone * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, target_quality, r->d_target_qual.p, (size_t)r->n_backbone));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_realignment_device_ptrs(const mdbg_realignment *r, const void *d_ptrs[11]) {
    if (!r || !d_ptrs) return MDBG_EINVAL;
    d_ptrs[0] = r->d_row_off.p; d_ptrs[1] = r->d_rows.p; d_ptrs[2] = r->d_entry_off.p; d_ptrs[3] = r->d_ref_index.p; d_ptrs[4] = r->d_query_index.p;
    d_ptrs[5] = r->d_query_min.p; d_ptrs[6] = r->d_query_qual.p; d_ptrs[7] = r->d_kind.p; d_ptrs[8] = r->d_target_off.p; d_ptrs[9] = r->d_target_min.p;
    d_ptrs[10] = r->d_target_qual.p;
    return MDBG_OK;
}

extern "C" void mdbg_realignment_free(mdbg_realignment *r) { delete r; }
