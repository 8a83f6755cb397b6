// select.hip -- mdbg_map_select / mdbg_selection_from_host / mdbg_map_select_merge / mdbg_selection_to_alignment_bytes: which of a query's
// chains ReadCorrection gets to see.  The reference keeps a heap of `coverage` alignments per query position (addAlignmentScore,
// ReadMapper.hpp:1233-1313) and applies the same rule again over the chunks' results (mergeAlignmentPartition, :228-363); the rules are
// select_dev.hpp, this file deals the work and moves the rows.
//
//   the view     the candidates of all queries as one CSR (cand_off), per candidate its read, score, list and list length.  From an
//                mdbg_chains: the rows with MDBG_CHAIN_FOUND, compacted behind a scan.  From parts: the parts' rows of a query one behind the
//                other (offsets are the sums of the parts' offsets), with one compare per row that the reads still ascend.
//   the rank     one sort_u64_pairs: key = query << 32 | the score turned round, value = the candidate's number.  Stable, and the candidates
//                are made in read order: equal scores stay in ascending read index.
//   the select   one wave a query, queries drawn from a device counter.  A byte per query position -- in LDS up to SELECT_LDS_POSITIONS
//                positions, above in the query's own piece of a pooled global buffer -- counts how often the position was taken.  The wave
//                walks the query's candidates in rank order ONE AFTER THE OTHER, the lanes take a candidate's matches 64 a trip: a lane whose
//                position stands below `coverage` raises it and marks the candidate.  The positions of one list differ, so a trip needs no
//                atomic, and the first `coverage` candidates of a position in rank order are exactly those that find it below `coverage`.
//   the compact  the marks are scanned; rows, sel_offsets and the match lists (dealt by output element) follow.
#include "common.hpp"
#include "objects.hpp"
#include "select_dev.hpp"

#include <algorithm>
#include <memory>

namespace mdbg {

static_assert(sizeof(mdbg_selected) == 24, "a selected row is 24 bytes");
static_assert(SELECT_LDS_POSITIONS % 4u == 0, "the counters are zeroed a word at a time");

// what the select kernel reads: the queries' candidates as a CSR, the rank order inside it, the lists
struct SelectView {
    const uint64_t *cand_off;                 // n_queries + 1
    const uint32_t *order;                    // n_candidates: slot cand_off[q] + k holds the k-th candidate of q in rank order
    const int32_t *score;                     // per candidate
    const uint32_t *const *list;              //   where its match list begins
    const uint32_t *len;                      //   and how long it is
    const unsigned long long *extent;         // n_queries: 1 + the largest position of the query's lists
    const uint64_t *spill_off;                // n_queries + 1: the query's piece of the pooled counters (extent > SELECT_LDS_POSITIONS)
};
struct SelectCands { uint32_t *ref_read; int32_t *score; uint32_t *len; uint32_t *part; uint64_t *pair; const uint32_t **list; };
struct SelectPart { const uint64_t *sel_off; const mdbg_selected *rows; const uint64_t *match_off; const uint32_t *matches; };

// ---- the view of an mdbg_chains ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void select_chain_flags_kernel(const mdbg_chain *chains, uint64_t n_pairs, uint32_t *flag) {
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * 256u) flag[p] = chains[p].flags == MDBG_CHAIN_FOUND ? 1u : 0u;
}

// out[i] = pos[at[i]], i < n: a CSR's offsets carried through a scan (candidates of the pairs, rows of the candidates)
__global__ __launch_bounds__(256) void select_offsets_kernel(const uint64_t *at, const uint64_t *pos, uint64_t n, uint64_t *out) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) out[i] = pos[at[i]];
}

// the pairs dealt to the waves; a pair that takes part becomes candidate cpos[p] of its query
__global__ __launch_bounds__(256) void select_from_chains_kernel(const uint64_t *pair_off, uint32_t n_queries, const mdbg_chain *chains, const uint64_t *match_off,
                                                                 const uint32_t *matches, uint64_t n_pairs, const uint32_t *flag, const uint64_t *cpos, SelectCands c,
                                                                 uint64_t *keys, uint32_t *vals, unsigned long long *extent) {
    const WaveSpan sp = wave_span(n_pairs, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t q = csr_owner(pair_off, n_queries, sp.begin);
    for (uint64_t p = sp.begin + (threadIdx.x & 63u); p < sp.end; p += 64u) {
        q = csr_owner_from(pair_off, n_queries, p, q);
        if (!flag[p]) continue;
        const uint64_t k = cpos[p];
        const uint32_t n = chains[p].n_matches;
        const uint32_t *list = matches + match_off[p];
        const int32_t score = (int32_t)chains[p].alignment_score;
        c.ref_read[k] = chains[p].ref_read; c.score[k] = score; c.len[k] = n; c.part[k] = 0u; c.pair[k] = p; c.list[k] = list;
        keys[k] = select_rank_key(q, score);
        vals[k] = (uint32_t)k;
        if (n) atomicMax(extent + q, (unsigned long long)list[n - 1u] + 1ull);
    }
}

// ---- the view of several parts ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void select_merge_offsets_kernel(const SelectPart *parts, uint32_t n_parts, uint64_t n, uint64_t *cand_off) {
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < n; q += (uint64_t)gridDim.x * 256u) {
        uint64_t sum = 0;
        for (uint32_t i = 0; i < n_parts; i++) sum += parts[i].sel_off[q];
        cand_off[q] = sum;
    }
}

// the candidates dealt to the waves: candidate k of query q is row k of the parts' rows of q laid one behind the other
__global__ __launch_bounds__(256) void select_concat_kernel(const SelectPart *parts, uint32_t n_parts, const uint64_t *cand_off, uint32_t n_queries, uint64_t n_cand,
                                                            SelectCands c, uint64_t *keys, uint32_t *vals, unsigned long long *extent) {
    const WaveSpan sp = wave_span(n_cand, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t q = csr_owner(cand_off, n_queries, sp.begin);
    for (uint64_t k = sp.begin + (threadIdx.x & 63u); k < sp.end; k += 64u) {
        q = csr_owner_from(cand_off, n_queries, k, q);
        uint64_t local = k - cand_off[q];
        for (uint32_t i = 0; i < n_parts; i++) {
            const uint64_t r0 = parts[i].sel_off[q], cnt = parts[i].sel_off[q + 1u] - r0;
            if (local >= cnt) { local -= cnt; continue; }
            const mdbg_selected row = parts[i].rows[r0 + local];
            const uint32_t *list = parts[i].matches + parts[i].match_off[r0 + local];
            c.ref_read[k] = row.ref_read; c.score[k] = row.score; c.len[k] = row.n_matches; c.part[k] = i; c.pair[k] = row.pair; c.list[k] = list;
            keys[k] = select_rank_key(q, row.score);
            vals[k] = (uint32_t)k;
            if (row.n_matches) atomicMax(extent + q, (unsigned long long)list[row.n_matches - 1u] + 1ull);
            break;
        }
    }
}

// one compare per row: the reads of a query ascend strictly across the parts; bad = the lowest query in which they do not
__global__ __launch_bounds__(256) void select_ascending_kernel(const uint64_t *cand_off, uint32_t n_queries, const uint32_t *ref_read, uint64_t n_cand,
                                                               unsigned long long *bad) {
    const WaveSpan sp = wave_span(n_cand, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t q = csr_owner(cand_off, n_queries, sp.begin);
    for (uint64_t k = sp.begin + (threadIdx.x & 63u); k < sp.end; k += 64u) {
        q = csr_owner_from(cand_off, n_queries, k, q);
        if (k > cand_off[q] && ref_read[k] <= ref_read[k - 1u]) atomicMin(bad, (unsigned long long)q);
    }
}

// ---- the select ---------------------------------------------------------------------------------------------------------------------------
// a query longer than the LDS share counts in global memory: 8-byte pieces of one pooled buffer
__global__ __launch_bounds__(256) void select_spill_need_kernel(const unsigned long long *extent, uint64_t n_queries, uint64_t *need) {
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < n_queries; q += (uint64_t)gridDim.x * 256u)
        need[q] = extent[q] > SELECT_LDS_POSITIONS ? (extent[q] + 7ull) & ~7ull : 0ull;
}

// One wave a query.  g_count: the pooled counters, zeroed by the caller (null when no query spills).  mark / mark_len: per candidate, 1 and
// its list's length when some position took it, else 0 and 0 -- written for EVERY candidate, by lane 0.  counter: the next query.
__global__ __launch_bounds__(256) void select_kernel(SelectView v, uint64_t n_queries, uint32_t coverage, unsigned long long *counter, uint8_t *g_count, uint32_t *mark,
                                                     uint32_t *mark_len) {
    __shared__ uint32_t s_words[4][SELECT_LDS_POSITIONS / 4u];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    for (;;) {
        wave_lds_sync();          // the turn's common start, one path to its end (wave_draw)
        const uint64_t q = wave_draw(counter);
        if (q >= n_queries) break;
        const uint64_t c0 = v.cand_off[q];
        const uint32_t n = wave_uniform_u32((uint32_t)(v.cand_off[q + 1u] - c0));
        const uint64_t extent = v.extent[q];
        const bool in_lds = extent <= SELECT_LDS_POSITIONS;                    // the same in every lane
        uint8_t *count = in_lds ? reinterpret_cast<uint8_t *>(s_words[wave]) : g_count + v.spill_off[q];
        if (in_lds) {
            for (uint32_t w = lane; w < ((uint32_t)extent + 3u) / 4u; w += 64u) s_words[wave][w] = 0u;
            wave_lds_sync();
        }
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t c = wave_uniform_u32(v.order[c0 + k]);
            const uint32_t len = wave_uniform_u32(v.len[c]);
            const uint32_t *list = v.list[c];
            bool taken = false;
            for (uint32_t base = 0; base < len; base += 64u) {
                const uint32_t t = base + lane;
                if (t < len) {
                    const uint32_t pos = list[t];
                    if (pos < extent) {                                         // (always, for lists that ascend: nothing outside the counters)
                        const uint32_t cnt = count[pos];
                        if (select_takes(cnt, coverage)) { count[pos] = (uint8_t)(cnt + 1u); taken = true; }
                    }
                }
            }
            const bool any = __ballot(taken) != 0ull;
            if (lane == 0) { mark[c] = any ? 1u : 0u; mark_len[c] = any ? len : 0u; }
            if (in_lds) wave_lds_sync(); else __threadfence_block();           // (the next candidate's lanes read what this one's wrote)
        }
    }
}

// ---- the compact --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void select_rows_kernel(const uint32_t *mark, const uint64_t *spos, const uint64_t *mpos, uint64_t n_cand, SelectCands c,
                                                          mdbg_selected *rows, uint64_t *match_off, const uint32_t **src) {
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < n_cand; k += (uint64_t)gridDim.x * 256u) {
        if (!mark[k]) continue;
        const uint64_t s = spos[k];
        mdbg_selected row;
        row.ref_read = c.ref_read[k]; row.score = c.score[k]; row.n_matches = c.len[k]; row.part = c.part[k]; row.pair = c.pair[k];
        rows[s] = row;
        match_off[s] = mpos[k];
        src[s] = c.list[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) match_off[spos[n_cand]] = mpos[n_cand];
}

// the match lists dealt by output element
__global__ __launch_bounds__(256) void select_matches_kernel(const uint64_t *match_off, uint32_t n_rows, uint64_t total, const uint32_t *const *src, uint32_t *matches) {
    const WaveSpan sp = wave_span(total, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t s = csr_owner(match_off, n_rows, sp.begin);
    for (uint64_t x = sp.begin + (threadIdx.x & 63u); x < sp.end; x += 64u) {
        s = csr_owner_from(match_off, n_rows, x, s);
        matches[x] = src[s][x - match_off[s]];
    }
}

// ---- the alignment file -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void select_nonempty_kernel(const uint64_t *sel_off, uint64_t n_queries, uint32_t *nonempty) {
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < n_queries; q += (uint64_t)gridDim.x * 256u) nonempty[q] = sel_off[q + 1u] > sel_off[q] ? 1u : 0u;
}

// every word exactly once: a query's lane writes the record's two head words, a row's lane its read
__global__ __launch_bounds__(256) void select_alignment_write_kernel(const uint64_t *sel_off, const uint64_t *before, uint32_t n_queries, const mdbg_selected *rows,
                                                                     uint64_t n_rows, uint32_t first_read, uint8_t *out, uint64_t n_bytes) {
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < n_queries; q += (uint64_t)gridDim.x * 256u) {
        const uint64_t r0 = sel_off[q], n = sel_off[q + 1u] - r0;
        const uint64_t at = select_record_start(before[q], r0);
        if (n == 0 || at + 8u > n_bytes) continue;
        *reinterpret_cast<uint32_t *>(out + at) = first_read + (uint32_t)q;
        *reinterpret_cast<uint32_t *>(out + at + 4u) = (uint32_t)n;
    }
    const WaveSpan sp = wave_span(n_rows, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t q = csr_owner(sel_off, n_queries, sp.begin);
    for (uint64_t s = sp.begin + (threadIdx.x & 63u); s < sp.end; s += 64u) {
        q = csr_owner_from(sel_off, n_queries, s, q);
        const uint64_t at = select_record_start(before[q], sel_off[q]) + 8u + 4u * (s - sel_off[q]);
        if (at + 4u > n_bytes) continue;                                        // (offsets that are not this selection's: nothing outside the buffer)
        *reinterpret_cast<uint32_t *>(out + at) = rows[s].ref_read;
    }
}

const StepKernel *select_step_kernels(uint32_t *n) {
    static const StepKernel k[] = {
        {"select_chain_flags", reinterpret_cast<const void *>(select_chain_flags_kernel), 256, 2},
        {"select_offsets", reinterpret_cast<const void *>(select_offsets_kernel), 256, 2},
        {"select_from_chains", reinterpret_cast<const void *>(select_from_chains_kernel), 256, 2},
        {"select_merge_offsets", reinterpret_cast<const void *>(select_merge_offsets_kernel), 256, 2},
        {"select_concat", reinterpret_cast<const void *>(select_concat_kernel), 256, 2},
        {"select_ascending", reinterpret_cast<const void *>(select_ascending_kernel), 256, 2},
        {"select_spill_need", reinterpret_cast<const void *>(select_spill_need_kernel), 256, 2},
        {"select", reinterpret_cast<const void *>(select_kernel), 256, 2},
        {"select_rows", reinterpret_cast<const void *>(select_rows_kernel), 256, 2},
        {"select_matches", reinterpret_cast<const void *>(select_matches_kernel), 256, 2},
        {"select_nonempty", reinterpret_cast<const void *>(select_nonempty_kernel), 256, 2},
        {"select_alignment_write", reinterpret_cast<const void *>(select_alignment_write_kernel), 256, 2},
    };
    *n = (uint32_t)(sizeof(k) / sizeof(k[0]));
    return k;
}

// the candidates' arrays, the sort's pairs and the queries' extents: what either view fills
struct SelectWork {
    DevBuf<uint64_t> cand_off, keys, pair;
    DevBuf<uint32_t> vals, ref_read, len, part;
    DevBuf<int32_t> score;
    DevBuf<const uint32_t *> list;
    DevBuf<unsigned long long> extent, bad;
    int alloc(mdbg_ctx *ctx, uint64_t nq, uint64_t n_cand) {
        MDBG_TRY(cand_off.alloc(ctx, (size_t)nq + 1)); MDBG_TRY(keys.alloc(ctx, n_cand)); MDBG_TRY(pair.alloc(ctx, n_cand)); MDBG_TRY(vals.alloc(ctx, n_cand));
        MDBG_TRY(ref_read.alloc(ctx, n_cand)); MDBG_TRY(len.alloc(ctx, n_cand)); MDBG_TRY(part.alloc(ctx, n_cand)); MDBG_TRY(score.alloc(ctx, n_cand));
        MDBG_TRY(list.alloc(ctx, n_cand)); MDBG_TRY(extent.alloc(ctx, nq)); MDBG_TRY(bad.alloc(ctx, 1));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(extent.p, 0, (size_t)std::max<uint64_t>(nq, 1) * 8, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(bad.p, 0xFF, 8, ctx->stream));
        return MDBG_OK;
    }
    SelectCands cands() { return SelectCands{ref_read.p, score.p, len.p, part.p, pair.p, list.p}; }
};

static int selection_empty(mdbg_ctx *ctx, uint64_t nq, std::unique_ptr<mdbg_selection> &sel) {
    MDBG_TRY(sel->d_sel_off.alloc(ctx, (size_t)nq + 1)); MDBG_TRY(sel->d_rows.alloc(ctx, 0)); MDBG_TRY(sel->d_match_off.alloc(ctx, 1)); MDBG_TRY(sel->d_matches.alloc(ctx, 0));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(sel->d_sel_off.p, 0, ((size_t)nq + 1) * 8, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(sel->d_match_off.p, 0, 8, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
}

// rank, select, compact: the view is filled (w), its kernels are queued.  check_bad: the ascending check ran (the merge).
static int select_run(mdbg_ctx *ctx, const char *who, SelectWork &w, uint64_t nq, uint64_t n_cand, uint32_t coverage, bool check_bad, mdbg_selection **out) {
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    std::unique_ptr<mdbg_selection> sel(new mdbg_selection());
    sel->n_queries = nq; sel->n_candidates = n_cand;
    // ---- the pooled counters of the queries that do not fit LDS: their total is the first host wait -----------------------------------
    DevBuf<uint64_t> need, spill_off;
    MDBG_TRY(need.alloc(ctx, nq)); MDBG_TRY(spill_off.alloc(ctx, (size_t)nq + 1));
    uint64_t spill = 0;
    unsigned long long h_bad = ~0ull;
    {
        LaunchTimer timer(ctx, "map_select");
        hipLaunchKernelGGL(select_spill_need_kernel, dim3(grid_for(nq, 256, cap)), dim3(256), 0, ctx->stream, w.extent.p, nq, need.p);
        MDBG_TRY(exclusive_scan_u64(ctx, need.p, spill_off.p, nq));
    }
    if (check_bad) MDBG_HIP_CHECK(ctx, hipMemcpyAsync(&h_bad, w.bad.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &spill, spill_off.p + nq, 8, hipMemcpyDeviceToHost));
    if (h_bad != ~0ull)
        return set_error(ctx, MDBG_EINVAL, "%s: query %llu: the reads do not ascend strictly across the parts (parts must be in chunk order)", who, h_bad);
    DevBuf<uint8_t> g_count;
    if (spill) {
        MDBG_TRY(g_count.alloc(ctx, spill));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(g_count.p, 0, spill, ctx->stream));
    }
    // ---- rank ----------------------------------------------------------------------------------------------------------------------------
    MDBG_TRY(sort_u64_pairs(ctx, w.keys.p, w.vals.p, n_cand, nullptr));
    // ---- select --------------------------------------------------------------------------------------------------------------------------
    DevBuf<uint32_t> mark, mark_len;
    DevBuf<uint64_t> spos, mpos;
    DevBuf<unsigned long long> counter;
    MDBG_TRY(mark.alloc(ctx, n_cand)); MDBG_TRY(mark_len.alloc(ctx, n_cand)); MDBG_TRY(spos.alloc(ctx, (size_t)n_cand + 1)); MDBG_TRY(mpos.alloc(ctx, (size_t)n_cand + 1));
    MDBG_TRY(counter.alloc(ctx, 1));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(counter.p, 0, 8, ctx->stream));
    const SelectView v{w.cand_off.p, w.vals.p, w.score.p, w.list.p, w.len.p, w.extent.p, spill_off.p};
    {
        LaunchTimer timer(ctx, "map_select");
        hipLaunchKernelGGL(select_kernel, dim3(grid_for(nq, 4, (unsigned)ctx->n_cu * 4u)), dim3(256), 0, ctx->stream, v, nq, coverage, counter.p, spill ? g_count.p : nullptr,
                           mark.p, mark_len.p);
        MDBG_TRY(exclusive_scan_u32(ctx, mark.p, spos.p, n_cand));
        MDBG_TRY(exclusive_scan_u32(ctx, mark_len.p, mpos.p, n_cand));
    }
    // ---- compact: the totals that size the result are the second host wait -------------------------------------------------------------
    uint64_t n_sel = 0, n_matches = 0;
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(&n_sel, spos.p + n_cand, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &n_matches, mpos.p + n_cand, 8, hipMemcpyDeviceToHost));
    sel->n_selected = n_sel; sel->n_matches = n_matches;
    MDBG_TRY(sel->d_sel_off.alloc(ctx, (size_t)nq + 1)); MDBG_TRY(sel->d_rows.alloc(ctx, n_sel)); MDBG_TRY(sel->d_match_off.alloc(ctx, (size_t)n_sel + 1));
    MDBG_TRY(sel->d_matches.alloc(ctx, n_matches));
    DevBuf<const uint32_t *> src;
    MDBG_TRY(src.alloc(ctx, n_sel));
    {
        LaunchTimer timer(ctx, "map_select");
        hipLaunchKernelGGL(select_offsets_kernel, dim3(grid_for(nq + 1, 256, cap)), dim3(256), 0, ctx->stream, w.cand_off.p, spos.p, nq + 1, sel->d_sel_off.p);
        hipLaunchKernelGGL(select_rows_kernel, dim3(grid_for(n_cand, 256, cap)), dim3(256), 0, ctx->stream, mark.p, spos.p, mpos.p, n_cand, w.cands(), sel->d_rows.p,
                           sel->d_match_off.p, src.p);
        if (n_matches)
            hipLaunchKernelGGL(select_matches_kernel, dim3(grid_for(n_matches, 256, cap)), dim3(256), 0, ctx->stream, sel->d_match_off.p, (uint32_t)n_sel, n_matches, src.p,
                               sel->d_matches.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));       // the transient buffers go back to the pool; the inputs must outlive the kernels
    *out = sel.release();
    return MDBG_OK;
}

}  // namespace mdbg

using namespace mdbg;

extern "C" uint32_t mdbg_select_lds_positions(void) { return SELECT_LDS_POSITIONS; }

extern "C" int mdbg_map_select(mdbg_ctx *ctx, const mdbg_chains *chains, uint32_t coverage, mdbg_selection **out) try {
    if (!ctx || !chains || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_map_select: null argument");
    if (coverage < 1u || coverage > SELECT_MAX_COVERAGE) return set_error(ctx, MDBG_EINVAL, "mdbg_map_select: coverage %u is not in 1 ... %u", coverage, SELECT_MAX_COVERAGE);
    if (chains->n_queries >= (1ull << 32) || chains->n_pairs >= (1ull << 32))
        return set_error(ctx, MDBG_ERANGE, "mdbg_map_select: 2^32 queries or pairs, or more");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    const uint64_t nq = chains->n_queries, np = chains->n_pairs, n_cand = chains->n_found;
    if (n_cand == 0) {
        std::unique_ptr<mdbg_selection> sel(new mdbg_selection());
        sel->n_queries = nq;
        MDBG_TRY(selection_empty(ctx, nq, sel));
        *out = sel.release();
        return MDBG_OK;
    }
    SelectWork w;
    MDBG_TRY(w.alloc(ctx, nq, n_cand));
    DevBuf<uint32_t> flag;
    DevBuf<uint64_t> cpos;
    MDBG_TRY(flag.alloc(ctx, np)); MDBG_TRY(cpos.alloc(ctx, (size_t)np + 1));
    {
        LaunchTimer timer(ctx, "map_select");
        hipLaunchKernelGGL(select_chain_flags_kernel, dim3(grid_for(np, 256, cap)), dim3(256), 0, ctx->stream, chains->d_chain.p, np, flag.p);
        MDBG_TRY(exclusive_scan_u32(ctx, flag.p, cpos.p, np));
        hipLaunchKernelGGL(select_offsets_kernel, dim3(grid_for(nq + 1, 256, cap)), dim3(256), 0, ctx->stream, chains->d_pair_off.p, cpos.p, nq + 1, w.cand_off.p);
        hipLaunchKernelGGL(select_from_chains_kernel, dim3(grid_for(np, 256, cap)), dim3(256), 0, ctx->stream, chains->d_pair_off.p, (uint32_t)nq, chains->d_chain.p,
                           chains->d_match_off.p, chains->d_matches.p, np, flag.p, cpos.p, w.cands(), w.keys.p, w.vals.p, w.extent.p);
    }
    return select_run(ctx, "mdbg_map_select", w, nq, n_cand, coverage, false, out);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_selection_from_host(mdbg_ctx *ctx, uint64_t n_queries, const uint64_t *sel_offsets, const uint32_t *ref_read, const uint64_t *match_offsets,
                                        const uint32_t *matches, mdbg_selection **out) try {
    if (!ctx || !out || !sel_offsets) return set_error(ctx, MDBG_EINVAL, "mdbg_selection_from_host: null argument");
    if (n_queries >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_selection_from_host: 2^32 queries or more");
    if (sel_offsets[0] != 0) return set_error(ctx, MDBG_EINVAL, "mdbg_selection_from_host: sel_offsets does not start at 0");
    for (uint64_t q = 0; q < n_queries; q++)
        if (sel_offsets[q + 1] < sel_offsets[q]) return set_error(ctx, MDBG_EINVAL, "mdbg_selection_from_host: query %llu: sel_offsets does not ascend", (unsigned long long)q);
    const uint64_t n = sel_offsets[n_queries];
    if (n >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_selection_from_host: 2^32 rows or more");
    if (n && (!ref_read || !match_offsets || !matches)) return set_error(ctx, MDBG_EINVAL, "mdbg_selection_from_host: null argument");
    if (n && match_offsets[0] != 0) return set_error(ctx, MDBG_EINVAL, "mdbg_selection_from_host: match_offsets does not start at 0");
    std::vector<mdbg_selected> rows((size_t)n);
    for (uint64_t q = 0; q < n_queries; q++)
        for (uint64_t s = sel_offsets[q]; s < sel_offsets[q + 1]; s++) {
            if (s > sel_offsets[q] && ref_read[s] <= ref_read[s - 1])
                return set_error(ctx, MDBG_EINVAL, "mdbg_selection_from_host: query %llu: read %u does not lie above the one before it (%u)", (unsigned long long)q, ref_read[s],
                                 ref_read[s - 1]);
            const uint64_t m0 = match_offsets[s], m1 = match_offsets[s + 1];
            if (m1 < m0) return set_error(ctx, MDBG_EINVAL, "mdbg_selection_from_host: query %llu: match_offsets does not ascend at row %llu", (unsigned long long)q, (unsigned long long)s);
            if (m1 == m0) return set_error(ctx, MDBG_EINVAL, "mdbg_selection_from_host: query %llu: the match list of read %u is empty", (unsigned long long)q, ref_read[s]);
            if (m1 - m0 >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_selection_from_host: query %llu: a match list of 2^32 elements or more", (unsigned long long)q);
            for (uint64_t i = m0 + 1; i < m1; i++)
                if (matches[i] <= matches[i - 1])
                    return set_error(ctx, MDBG_EINVAL, "mdbg_selection_from_host: query %llu: the match list of read %u does not ascend strictly (%u behind %u)",
                                     (unsigned long long)q, ref_read[s], matches[i], matches[i - 1]);
            mdbg_selected &row = rows[(size_t)s];
            row.ref_read = ref_read[s]; row.score = select_list_score((uint32_t)(m1 - m0), matches[m0], matches[m1 - 1]); row.n_matches = (uint32_t)(m1 - m0);
            row.part = 0u; row.pair = s;
        }
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint64_t n_matches = n ? match_offsets[n] : 0;
    std::unique_ptr<mdbg_selection> sel(new mdbg_selection());
    sel->n_queries = n_queries; sel->n_selected = n; sel->n_matches = n_matches; sel->n_candidates = n;
    MDBG_TRY(sel->d_sel_off.alloc(ctx, (size_t)n_queries + 1)); MDBG_TRY(sel->d_rows.alloc(ctx, n)); MDBG_TRY(sel->d_match_off.alloc(ctx, (size_t)n + 1));
    MDBG_TRY(sel->d_matches.alloc(ctx, n_matches));
    const uint64_t zero = 0;
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(sel->d_sel_off.p, sel_offsets, ((size_t)n_queries + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n) MDBG_HIP_CHECK(ctx, hipMemcpyAsync(sel->d_rows.p, rows.data(), (size_t)n * sizeof(mdbg_selected), hipMemcpyHostToDevice, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(sel->d_match_off.p, n ? match_offsets : &zero, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n_matches) MDBG_HIP_CHECK(ctx, hipMemcpyAsync(sel->d_matches.p, matches, (size_t)n_matches * 4, hipMemcpyHostToDevice, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = sel.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_map_select_merge(mdbg_ctx *ctx, const mdbg_selection *const *parts, uint32_t n_parts, uint32_t coverage, mdbg_selection **out) try {
    if (!ctx || !parts || !out || n_parts == 0) return set_error(ctx, MDBG_EINVAL, "mdbg_map_select_merge: null argument or no part");
    if (coverage < 1u || coverage > SELECT_MAX_COVERAGE)
        return set_error(ctx, MDBG_EINVAL, "mdbg_map_select_merge: coverage %u is not in 1 ... %u", coverage, SELECT_MAX_COVERAGE);
    uint64_t n_cand = 0;
    for (uint32_t i = 0; i < n_parts; i++) {
        if (!parts[i]) return set_error(ctx, MDBG_EINVAL, "mdbg_map_select_merge: part %u is null", i);
        if (parts[i]->n_queries != parts[0]->n_queries)
            return set_error(ctx, MDBG_EINVAL, "mdbg_map_select_merge: part %u has %llu queries, part 0 has %llu", i, (unsigned long long)parts[i]->n_queries,
                             (unsigned long long)parts[0]->n_queries);
        n_cand += parts[i]->n_selected;
    }
    const uint64_t nq = parts[0]->n_queries;
    if (n_cand >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_map_select_merge: the parts have %llu rows, 2^32 or more", (unsigned long long)n_cand);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    if (n_cand == 0) {
        std::unique_ptr<mdbg_selection> sel(new mdbg_selection());
        sel->n_queries = nq;
        MDBG_TRY(selection_empty(ctx, nq, sel));
        *out = sel.release();
        return MDBG_OK;
    }
    std::vector<SelectPart> h_parts(n_parts);
    for (uint32_t i = 0; i < n_parts; i++) h_parts[i] = SelectPart{parts[i]->d_sel_off.p, parts[i]->d_rows.p, parts[i]->d_match_off.p, parts[i]->d_matches.p};
    DevBuf<SelectPart> d_parts;
    MDBG_TRY(d_parts.alloc(ctx, n_parts));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, d_parts.p, h_parts.data(), (size_t)n_parts * sizeof(SelectPart), hipMemcpyHostToDevice));
    SelectWork w;
    MDBG_TRY(w.alloc(ctx, nq, n_cand));
    {
        LaunchTimer timer(ctx, "map_select");
        hipLaunchKernelGGL(select_merge_offsets_kernel, dim3(grid_for(nq + 1, 256, cap)), dim3(256), 0, ctx->stream, d_parts.p, n_parts, nq + 1, w.cand_off.p);
        hipLaunchKernelGGL(select_concat_kernel, dim3(grid_for(n_cand, 256, cap)), dim3(256), 0, ctx->stream, d_parts.p, n_parts, w.cand_off.p, (uint32_t)nq, n_cand, w.cands(),
                           w.keys.p, w.vals.p, w.extent.p);
        hipLaunchKernelGGL(select_ascending_kernel, dim3(grid_for(n_cand, 256, cap)), dim3(256), 0, ctx->stream, w.cand_off.p, (uint32_t)nq, w.ref_read.p, n_cand, w.bad.p);
    }
    return select_run(ctx, "mdbg_map_select_merge", w, nq, n_cand, coverage, true, out);
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_selection_to_alignment_bytes(mdbg_ctx *ctx, const mdbg_selection *sel, uint32_t query_first_read, mdbg_bytes **out, uint64_t *n_bytes) try {
    if (!ctx || !sel || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_selection_to_alignment_bytes: null argument");
    if ((uint64_t)query_first_read + sel->n_queries > (1ull << 32))
        return set_error(ctx, MDBG_EINVAL, "mdbg_selection_to_alignment_bytes: %llu queries from read %u leave the 32-bit read numbers", (unsigned long long)sel->n_queries,
                         query_first_read);
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    const uint64_t nq = sel->n_queries, n = sel->n_selected;
    DevBuf<uint32_t> nonempty;
    DevBuf<uint64_t> before;
    MDBG_TRY(nonempty.alloc(ctx, nq)); MDBG_TRY(before.alloc(ctx, (size_t)nq + 1));
    {
        LaunchTimer timer(ctx, "select_alignment_write");
        hipLaunchKernelGGL(select_nonempty_kernel, dim3(grid_for(nq, 256, cap)), dim3(256), 0, ctx->stream, sel->d_sel_off.p, nq, nonempty.p);
        MDBG_TRY(exclusive_scan_u32(ctx, nonempty.p, before.p, nq));
    }
    uint64_t n_nonempty = 0;
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &n_nonempty, before.p + nq, 8, hipMemcpyDeviceToHost));
    const uint64_t total = select_record_start(n_nonempty, n);
    std::unique_ptr<mdbg_bytes> b(new mdbg_bytes());
    b->n = total;
    b->owner = ctx;
    MDBG_TRY(b->d.alloc(ctx, total + 16));
    if (!ctx->upload_stream) MDBG_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking));     // (as mdbg_bytes_create leaves a buffer)
    if (n) {
        LaunchTimer timer(ctx, "select_alignment_write");
        hipLaunchKernelGGL(select_alignment_write_kernel, dim3(grid_for(std::max(nq, n), 256, cap)), dim3(256), 0, ctx->stream, sel->d_sel_off.p, before.p, (uint32_t)nq,
                           sel->d_rows.p, n, query_first_read, b->d.p, total);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));       // (the scanned counts go back to the pool)
    if (n_bytes) *n_bytes = total;
    *out = b.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_selection_info(const mdbg_selection *s, uint64_t info[4]) {
    if (!s || !info) return MDBG_EINVAL;
    info[0] = s->n_queries; info[1] = s->n_selected; info[2] = s->n_matches; info[3] = s->n_candidates;
    return MDBG_OK;
}

extern "C" int mdbg_selection_to_host(mdbg_ctx *ctx, const mdbg_selection *s, uint64_t *sel_offsets, mdbg_selected *rows, uint64_t *match_offsets, uint32_t *matches) try {
    if (!ctx || !s) return set_error(ctx, MDBG_EINVAL, "mdbg_selection_to_host: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_HIP_CHECK(ctx, download_async(ctx, sel_offsets, s->d_sel_off.p, ((size_t)s->n_queries + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, rows, s->d_rows.p, (size_t)s->n_selected * sizeof(mdbg_selected)));
    MDBG_HIP_CHECK(ctx, download_async(ctx, match_offsets, s->d_match_off.p, ((size_t)s->n_selected + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, matches, s->d_matches.p, (size_t)s->n_matches * 4));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_selection_device_ptrs(const mdbg_selection *s, const void *d_ptrs[4]) {
    if (!s || !d_ptrs) return MDBG_EINVAL;
    d_ptrs[0] = s->d_sel_off.p; d_ptrs[1] = s->d_rows.p; d_ptrs[2] = s->d_match_off.p; d_ptrs[3] = s->d_matches.p;
    return MDBG_OK;
}

extern "C" void mdbg_selection_free(mdbg_selection *s) { delete s; }
