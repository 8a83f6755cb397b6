// mapper.hip -- mdbg_map_index_build / mdbg_map_anchors / mdbg_map_chains: the read-against-read mapper of read correction
// (readSelection/ReadMapper.hpp) in minimizer space.  A join of every read's windows of two minimizers against an index of a chunk's
// windows, a regrouping by (query, reference read), and a banded dynamic programme per group.  The rules themselves -- the window, which
// index entries a query window takes, the predecessor test and its score, the two tie rules, the fields of a chain -- are mapper_dev.hpp;
// this file deals the work and moves the rows.
//
//   the index    one lane a window of the chunk (wave_span over the windows): key = the pair, value = the window's number.  One
//                sort_u64_pairs; stable, so a pair's entries stay in (read, index) order.  The entries' fields are gathered behind the sort,
//                run heads are marked and scanned, and a compact array of the distinct pairs with their run starts is the lookup: a query
//                binary-searches it (twenty-odd dependent loads at a million pairs, against a hash table's one or two -- the simpler of the
//                two, built first; the join's time is the anchors', not the lookups').
//   the anchors  count: one lane a query minimizer; a window's count is its pair's run minus the query's own entries, which are one block
//                of the run (two more binary searches).  An exclusive scan places them.  fill: the OUTPUT anchors are dealt to the waves in
//                contiguous spans, a lane finds its window from the scanned counts -- a window that hits a run of 100 000 entries is
//                spread over many waves.  Generation order is (query, query index); one sort_u64_pairs by (query << 32 | the reference
//                window's number) gives (query, ref_read, ref_position, query_position): a read's windows are numbered in position order,
//                and equal keys keep the generation order.  Group heads, sizes, the min_anchors filter and the final rows follow.
//   the chains   one wave a pair, pairs drawn in order from a device counter (wave_draw); the dynamic programme is chain_wave
//                (chain_wave.hpp), which the verifier runs too.  Lane 0 walks the parents and writes the row and the pair's match list
//                into a staging array (a list is no longer than its pair); the lists are compacted behind a scan, dealt by output element.
#include "common.hpp"
#include "objects.hpp"
#include "chain_wave.hpp"

#include <algorithm>
#include <memory>

struct mdbg_map_index {
    uint32_t n_reads = 0, first_read = 0;
    uint64_t n_entries = 0, n_pairs = 0, longest = 0;
    mdbg::DevBuf<uint64_t> d_pair;            // n_entries: the entries' pairs, ascending
    mdbg::DevBuf<uint32_t> d_win;             // n_entries: the window's number in the chunk (ascending inside a pair)
    mdbg::DevBuf<uint32_t> d_read, d_pos, d_idx;   // n_entries: global read, position, index
    mdbg::DevBuf<uint8_t> d_rev;              // n_entries
    mdbg::DevBuf<uint64_t> d_distinct;        // n_pairs
    mdbg::DevBuf<uint32_t> d_run;             // n_pairs + 1: where a pair's entries begin
};

struct mdbg_anchors {
    uint64_t n_queries = 0, n_pairs = 0, n_anchors = 0, longest = 0;
    mdbg::DevBuf<uint64_t> d_pair_off;        // n_queries + 1
    mdbg::DevBuf<uint32_t> d_pair_ref;        // n_pairs
    mdbg::DevBuf<uint64_t> d_anchor_off;      // n_pairs + 1
    mdbg::DevBuf<uint32_t> d_ref_read, d_ref_pos, d_ref_idx, d_q_pos, d_q_idx;   // n_anchors
    mdbg::DevBuf<uint8_t> d_rev;              // n_anchors
};

namespace mdbg {

static_assert(sizeof(mdbg_chain) == 80, "a chain row is 80 bytes");
static_assert(sizeof(mdbg_map_params) == 32, "mdbg_map_params is 32 bytes");

// ---- the index ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void map_window_counts_kernel(const uint64_t *off, uint32_t n_reads, uint32_t *wcount) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * 256u) wcount[r] = map_read_windows(off[r + 1u] - off[r]);
}

// one lane a window: the sort's key and value, and the entry's fields by window number
__global__ __launch_bounds__(256) void map_windows_kernel(const uint64_t *off, const uint32_t *mins, const uint32_t *pos, const uint64_t *woff, uint32_t n_reads,
                                                          uint64_t n_windows, uint32_t first_read, uint64_t *keys, uint32_t *vals, uint32_t *w_read, uint32_t *w_pos,
                                                          uint32_t *w_idx, uint8_t *w_rev) {
    const WaveSpan sp = wave_span(n_windows, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t r = csr_owner(woff, n_reads, sp.begin);
    for (uint64_t w = sp.begin + (threadIdx.x & 63u); w < sp.end; w += 64u) {
        r = csr_owner_from(woff, n_reads, w, r);
        const uint32_t i = (uint32_t)(w - woff[r]);
        const uint64_t at = off[r] + i;
        const MapWindow mw = map_window(mins[at], mins[at + 1u], pos[at], pos[at + 1u]);
        keys[w] = mw.pair;
        vals[w] = (uint32_t)w;
        w_read[w] = first_read + r;
        w_pos[w] = mw.position;
        w_idx[w] = i;
        w_rev[w] = (uint8_t)mw.reversed;
    }
}

// behind the sort: entry e is window vals[e]; a run head is an entry whose pair differs from the one before it
__global__ __launch_bounds__(256) void map_entries_kernel(const uint64_t *keys, const uint32_t *vals, const uint32_t *w_read, const uint32_t *w_pos, const uint32_t *w_idx,
                                                          const uint8_t *w_rev, uint64_t n, uint32_t *e_read, uint32_t *e_pos, uint32_t *e_idx, uint8_t *e_rev,
                                                          uint32_t *head) {
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256u) {
        const uint32_t w = vals[e];
        e_read[e] = w_read[w];
        e_pos[e] = w_pos[w];
        e_idx[e] = w_idx[w];
        e_rev[e] = w_rev[w];
        head[e] = e == 0 || keys[e] != keys[e - 1u] ? 1u : 0u;
    }
}

// heads -> the compact rows: what[k] (optional) and start[k] of the k-th head, start[total heads] = n
__global__ __launch_bounds__(256) void map_compact_heads_kernel(const uint64_t *keys, uint32_t key_shift, const uint32_t *head, const uint64_t *hpos, uint64_t n,
                                                                uint64_t *what, uint32_t *start) {
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256u) {
        if (!head[e]) continue;
        const uint64_t k = hpos[e];
        if (what) what[k] = keys[e] >> key_shift;
        start[k] = (uint32_t)e;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) start[hpos[n]] = (uint32_t)n;
}

// the largest of start[k + 1] - start[k]: a maximum per wave, one atomic a wave
__global__ __launch_bounds__(256) void map_longest_kernel(const uint32_t *start, uint64_t n, unsigned long long *longest) {
    uint32_t m = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256u) m = max(m, start[k + 1u] - start[k]);
    m = wave_max_u32(m);
    if (lane_id() == 0 && m) atomicMax(longest, (unsigned long long)m);
}

// ---- the anchors -------------------------------------------------------------------------------------------------------------------------
struct MapIndexView { const uint64_t *distinct; const uint32_t *run; uint64_t n_pairs; const uint32_t *e_read, *e_pos, *e_idx, *e_win; const uint8_t *e_rev; };
struct MapQueryView { const uint64_t *off; const uint32_t *mins, *pos; uint32_t n_reads, first_read, begin; uint64_t m0; };

// the pair's number among the distinct pairs, or n_pairs
__device__ __forceinline__ uint64_t map_find_pair(const uint64_t *distinct, uint64_t n_pairs, uint64_t pair) {
    uint64_t lo = 0, hi = n_pairs;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (distinct[mid] < pair) lo = mid + 1u; else hi = mid;
    }
    return lo < n_pairs && distinct[lo] == pair ? lo : n_pairs;
}

// one lane a query minimizer t (flat number m0 + t): the anchors of the window that starts there, and where its run lies
__global__ __launch_bounds__(256) void map_count_kernel(MapQueryView q, MapIndexView ix, uint64_t n_items, uint32_t *cnt, uint32_t *q_read, uint32_t *q_begin,
                                                        uint32_t *q_self, uint32_t *q_selfn) {
    const WaveSpan sp = wave_span(n_items, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t r = csr_owner(q.off, q.n_reads, q.m0 + sp.begin);
    for (uint64_t t = sp.begin + (threadIdx.x & 63u); t < sp.end; t += 64u) {
        const uint64_t at = q.m0 + t;
        r = csr_owner_from(q.off, q.n_reads, at, r);
        const uint64_t r0 = q.off[r], r1 = q.off[r + 1u];
        MapRun run{0u, 0u, 0u, 0u};
        if (at + 1u < r1 && map_query_asks(r1 - r0)) {
            const MapWindow mw = map_window(q.mins[at], q.mins[at + 1u], q.pos[at], q.pos[at + 1u]);
            const uint64_t k = map_find_pair(ix.distinct, ix.n_pairs, mw.pair);
            if (k < ix.n_pairs) run = map_run(ix.e_read, ix.run[k], ix.run[k + 1u], q.first_read + r);
        }
        cnt[t] = run.count;
        q_read[t] = r;
        q_begin[t] = run.begin;
        q_self[t] = run.self_begin;
        q_selfn[t] = run.self_count;
    }
}

// how many reads from `begin` stay below 2^32 anchors (the refusal's message): aoff at a read's last minimizer is the sum through that read
__global__ __launch_bounds__(256) void map_fit_kernel(const uint64_t *off, uint32_t begin, uint32_t end, uint64_t m0, const uint64_t *aoff, unsigned long long *fit) {
    for (uint64_t r = (uint64_t)begin + (uint64_t)blockIdx.x * 256u + threadIdx.x; r < end; r += (uint64_t)gridDim.x * 256u)
        if (aoff[off[r + 1u] - m0] < (1ull << 32)) atomicMax(fit, (unsigned long long)(r + 1u - begin));
}

// the OUTPUT anchors dealt to the waves: anchor a belongs to query minimizer t = the owner of a among the scanned counts
__global__ __launch_bounds__(256) void map_fill_kernel(const uint64_t *aoff, uint64_t n_items, uint64_t total, const uint32_t *q_read, const uint32_t *q_begin,
                                                       const uint32_t *q_self, const uint32_t *q_selfn, const uint32_t *e_win, uint32_t query_begin, uint64_t *keys,
                                                       uint32_t *vals, uint32_t *gen_e, uint32_t *gen_t) {
    const WaveSpan sp = wave_span(total, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t t = csr_owner(aoff, (uint32_t)n_items, sp.begin);
    for (uint64_t a = sp.begin + (threadIdx.x & 63u); a < sp.end; a += 64u) {
        t = csr_owner_from(aoff, (uint32_t)n_items, a, t);
        const uint32_t e = map_run_entry(q_begin[t], q_self[t], q_selfn[t], (uint32_t)(a - aoff[t]));
        keys[a] = ((uint64_t)(q_read[t] - query_begin) << 32) | e_win[e];
        vals[a] = (uint32_t)a;
        gen_e[a] = e;
        gen_t[a] = t;
    }
}

// behind the sort: slot s holds generated anchor vals[s]; a group head is a slot whose (query, reference read) differs from the one before it
__global__ __launch_bounds__(256) void map_group_heads_kernel(const uint64_t *keys, const uint32_t *vals, const uint32_t *gen_e, const uint32_t *e_read, uint64_t n,
                                                              uint32_t *head) {
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n; s += (uint64_t)gridDim.x * 256u)
        head[s] = s == 0 || (keys[s] >> 32) != (keys[s - 1u] >> 32) || e_read[gen_e[vals[s]]] != e_read[gen_e[vals[s - 1u]]] ? 1u : 0u;
}

// a group stays when it has min_anchors anchors: its size (or 0) and a flag for the two scans; the longest kept group
__global__ __launch_bounds__(256) void map_group_sizes_kernel(const uint32_t *gstart, uint64_t n_groups, uint32_t min_anchors, uint32_t *ksize, uint32_t *kflag,
                                                              unsigned long long *longest) {
    uint32_t m = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * 256u) {
        const uint32_t size = gstart[g + 1u] - gstart[g];
        const bool keep = size >= min_anchors;
        ksize[g] = keep ? size : 0u;
        kflag[g] = keep ? 1u : 0u;
        if (keep) m = max(m, size);
    }
    m = wave_max_u32(m);
    if (lane_id() == 0 && m) atomicMax(longest, (unsigned long long)m);
}

// the kept groups' rows: reference read and first anchor
__global__ __launch_bounds__(256) void map_pairs_kernel(const uint32_t *gstart, const uint32_t *kflag, const uint64_t *kidx, const uint64_t *knew, uint64_t n_groups,
                                                        const uint32_t *vals, const uint32_t *gen_e, const uint32_t *e_read, uint32_t *pair_ref, uint64_t *anchor_off) {
    for (uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * 256u) {
        if (!kflag[g]) continue;
        const uint64_t p = kidx[g];
        pair_ref[p] = e_read[gen_e[vals[gstart[g]]]];
        anchor_off[p] = knew[g];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) anchor_off[kidx[n_groups]] = knew[n_groups];
}

// pair_offsets[qi] = kept groups of the queries below qi (gquery ascending)
__global__ __launch_bounds__(256) void map_pair_offsets_kernel(const uint64_t *gquery, uint64_t n_groups, const uint64_t *kidx, uint64_t n_queries, uint64_t *pair_off) {
    for (uint64_t qi = (uint64_t)blockIdx.x * 256u + threadIdx.x; qi <= n_queries; qi += (uint64_t)gridDim.x * 256u) {
        uint64_t lo = 0, hi = n_groups;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2u;
            if (gquery[mid] < qi) lo = mid + 1u; else hi = mid;
        }
        pair_off[qi] = kidx[lo];
    }
}

struct MapAnchorRows { uint32_t *ref_read, *ref_pos, *ref_idx, *q_pos, *q_idx; uint8_t *rev; };

// the final rows: sorted slot s of a kept group moves to the group's new place
__global__ __launch_bounds__(256) void map_emit_kernel(const uint32_t *vals, const uint32_t *head, const uint64_t *gpos, const uint32_t *gstart, const uint32_t *kflag,
                                                       const uint64_t *knew, uint64_t n, const uint32_t *gen_e, const uint32_t *gen_t, const uint32_t *q_read,
                                                       MapQueryView q, MapIndexView ix, MapAnchorRows out) {
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n; s += (uint64_t)gridDim.x * 256u) {
        const uint64_t g = gpos[s] + head[s] - 1u;
        if (!kflag[g]) continue;
        const uint64_t dst = knew[g] + (s - gstart[g]);
        const uint32_t a = vals[s], e = gen_e[a], t = gen_t[a];
        const uint64_t at = q.m0 + t;
        const MapWindow mw = map_window(q.mins[at], q.mins[at + 1u], q.pos[at], q.pos[at + 1u]);
        out.ref_read[dst] = ix.e_read[e];
        out.ref_pos[dst] = ix.e_pos[e];
        out.ref_idx[dst] = ix.e_idx[e];
        out.q_pos[dst] = mw.position;
        out.q_idx[dst] = (uint32_t)(at - q.off[q_read[t]]);
        out.rev[dst] = (uint8_t)map_anchor_reversed(ix.e_rev[e], mw.reversed);
    }
}

// ---- the chains --------------------------------------------------------------------------------------------------------------------------
// One wave a pair.  g_score / g_parent: n_anchors each, for the pairs above CHAIN_LDS_ANCHORS (null when there is none).  staged: n_anchors,
// the pair's match list from its first anchor's place on.  counters: [0] the next pair, [1] chains found.
__global__ __launch_bounds__(256) void map_chain_kernel(const uint64_t *anchor_off, const uint32_t *pair_ref, uint64_t n_pairs, const uint32_t *ref_pos,
                                                        const uint32_t *ref_idx, const uint32_t *q_pos, const uint32_t *q_idx, const uint8_t *rev, uint32_t band,
                                                        unsigned long long *counters, int32_t *g_score, uint32_t *g_parent, mdbg_chain *chains, uint32_t *n_matches,
                                                        uint32_t *staged) {
    __shared__ int32_t s_score[4][CHAIN_LDS_ANCHORS];
    __shared__ uint32_t s_parent[4][CHAIN_LDS_ANCHORS];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    for (;;) {
        wave_lds_sync();          // the turn's common start, one path to its end (wave_draw); lane 0 has walked the last pair's parents before they are overwritten
        const uint64_t p = wave_draw(counters);
        if (p >= n_pairs) break;
        const uint64_t a0 = anchor_off[p];
        const uint32_t n = (uint32_t)(anchor_off[p + 1u] - a0);
        const bool chained = n != 0u && n < MAP_CHAIN_TOO_LONG_FROM;      // the same in every lane
        const bool in_lds = n <= CHAIN_LDS_ANCHORS;
        int32_t *score = in_lds ? s_score[wave] : g_score + a0;
        uint32_t *parent = in_lds ? s_parent[wave] : g_parent + a0;
        const uint32_t *rp = ref_pos + a0;
        const ChainEnd end = chain_wave(chained ? n : 0u, rp, q_pos + a0, rev + a0, band, score, parent, in_lds);
        if (lane == 0) {
            const uint32_t best_i = end.i;
            mdbg_chain row;
            row.ref_read = pair_ref[p]; row.flags = n && !chained ? MDBG_CHAIN_TOO_LONG : 0u; row.score = 0; row.n_matches = 0u; row.query_reversed = 0u; row.reserved = 0u;
            row.n_diff_query = row.n_diff_reference = row.query_start = row.query_end = row.reference_start = row.reference_end = row.alignment_score = 0;
            // map_chain_walk, written out: through the helper this kernel's map_chains timer read 1.2 % above the parent's in every one of
            // eleven alternating runs, written out it reads the parent's (profiles/chain_shared_bench_alternating.txt); the verifier calls it
            uint32_t len = 0, root = best_i;
            if (chained)
                for (uint32_t at = best_i; at != MAP_NO_PARENT; at = parent[at]) { root = at; len++; }
            if (len >= MAP_MIN_CHAIN) {
                const MapChain c = map_chain_fields(end.score, len, q_idx[a0 + best_i], q_idx[a0 + root], ref_idx[a0 + best_i], ref_idx[a0 + root], rp[best_i], rp[root]);
                row.flags = MDBG_CHAIN_FOUND; row.score = c.score; row.n_matches = c.n_matches; row.query_reversed = c.query_reversed;
                row.n_diff_query = c.n_diff_query; row.n_diff_reference = c.n_diff_reference; row.query_start = c.query_start; row.query_end = c.query_end;
                row.reference_start = c.reference_start; row.reference_end = c.reference_end; row.alignment_score = c.alignment_score;
                uint32_t k = 0;              // best anchor -> root, turned round when query_reversed (:1017-1034)
                for (uint32_t at = best_i; at != MAP_NO_PARENT; at = parent[at], k++) staged[a0 + (c.query_reversed ? len - 1u - k : k)] = q_idx[a0 + at];
                atomicAdd(counters + 1, 1ull);
            }
            chains[p] = row;
            n_matches[p] = row.n_matches;
        }
    }
}

// the match lists dealt by output element
__global__ __launch_bounds__(256) void map_matches_kernel(const uint64_t *match_off, const uint64_t *anchor_off, uint32_t n_pairs, uint64_t total, const uint32_t *staged,
                                                          uint32_t *matches) {
    const WaveSpan sp = wave_span(total, 64u);
    if (sp.begin >= sp.end) return;
    uint32_t p = csr_owner(match_off, n_pairs, sp.begin);
    for (uint64_t x = sp.begin + (threadIdx.x & 63u); x < sp.end; x += 64u) {
        p = csr_owner_from(match_off, n_pairs, x, p);
        matches[x] = staged[anchor_off[p] + (x - match_off[p])];
    }
}

const StepKernel *mapper_step_kernels(uint32_t *n) {
    static const StepKernel k[] = {
        {"map_window_counts", reinterpret_cast<const void *>(map_window_counts_kernel), 256, 2},
        {"map_windows", reinterpret_cast<const void *>(map_windows_kernel), 256, 2},
        {"map_entries", reinterpret_cast<const void *>(map_entries_kernel), 256, 2},
        {"map_compact_heads", reinterpret_cast<const void *>(map_compact_heads_kernel), 256, 2},
        {"map_longest", reinterpret_cast<const void *>(map_longest_kernel), 256, 2},
        {"map_count", reinterpret_cast<const void *>(map_count_kernel), 256, 2},
        {"map_fit", reinterpret_cast<const void *>(map_fit_kernel), 256, 2},
        {"map_fill", reinterpret_cast<const void *>(map_fill_kernel), 256, 2},
        {"map_group_heads", reinterpret_cast<const void *>(map_group_heads_kernel), 256, 2},
        {"map_group_sizes", reinterpret_cast<const void *>(map_group_sizes_kernel), 256, 2},
        {"map_pairs", reinterpret_cast<const void *>(map_pairs_kernel), 256, 2},
        {"map_pair_offsets", reinterpret_cast<const void *>(map_pair_offsets_kernel), 256, 2},
        {"map_emit", reinterpret_cast<const void *>(map_emit_kernel), 256, 2},
        {"map_chain", reinterpret_cast<const void *>(map_chain_kernel), 256, 2},
        {"map_matches", reinterpret_cast<const void *>(map_matches_kernel), 256, 2},
    };
    *n = (uint32_t)(sizeof(k) / sizeof(k[0]));
    return k;
}

// a set the mapper can read: positions present, CSR order
static int map_set_ready(mdbg_ctx *ctx, const char *who, const char *what, const mdbg_minimizers *m) {
    if (!m->d_pos.p) return set_error(ctx, MDBG_EINVAL, "%s: the %s carry no positions (a scan output, or mdbg_minimizers_attach_positions)", who, what);
    return ensure_canonical(ctx, m);
}

}  // namespace mdbg

using namespace mdbg;

extern "C" int mdbg_minimizers_attach_positions(mdbg_ctx *ctx, mdbg_minimizers *m, const uint32_t *positions) try {
    if (!ctx || !m || (m->n_min && !positions)) return set_error(ctx, MDBG_EINVAL, "mdbg_minimizers_attach_positions: null argument");
    if (m->scattered) return set_error(ctx, MDBG_EINVAL, "mdbg_minimizers_attach_positions: a scan output has its positions");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> off((size_t)m->n_reads + 1);
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, off.data(), m->d_off.p, off.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < m->n_reads; r++)
        for (uint64_t i = off[r]; i < off[r + 1]; i++) {
            if (positions[i] >= (1u << 31))
                return set_error(ctx, MDBG_EINVAL, "mdbg_minimizers_attach_positions: read %u, minimizer %llu: position %u is 2^31 or more", r,
                                 (unsigned long long)(i - off[r]), positions[i]);
            if (i > off[r] && positions[i] <= positions[i - 1])
                return set_error(ctx, MDBG_EINVAL, "mdbg_minimizers_attach_positions: read %u, minimizer %llu: position %u does not lie above the one before it (%u)", r,
                                 (unsigned long long)(i - off[r]), positions[i], positions[i - 1]);
        }
    DevBuf<uint32_t> d;
    MDBG_TRY(d.alloc(ctx, m->n_min));
    if (m->n_min) MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, d.p, positions, m->n_min * 4, hipMemcpyHostToDevice));
    m->d_pos = std::move(d);
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_map_index_build(mdbg_ctx *ctx, const mdbg_minimizers *chunk, uint32_t chunk_first_read, mdbg_map_index **out) try {
    if (!ctx || !chunk || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_map_index_build: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_TRY(map_set_ready(ctx, "mdbg_map_index_build", "chunk's reads", chunk));
    if ((uint64_t)chunk_first_read + chunk->n_reads > (1ull << 32))
        return set_error(ctx, MDBG_EINVAL, "mdbg_map_index_build: %u reads from read %u leave the 32-bit read numbers", chunk->n_reads, chunk_first_read);
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    const uint32_t n_reads = chunk->n_reads;
    std::unique_ptr<mdbg_map_index> ix(new mdbg_map_index());
    ix->n_reads = n_reads; ix->first_read = chunk_first_read;
    LaunchTimer timer(ctx, "map_index");
    DevBuf<uint32_t> wcount;
    DevBuf<uint64_t> woff;
    MDBG_TRY(wcount.alloc(ctx, n_reads));
    MDBG_TRY(woff.alloc(ctx, (size_t)n_reads + 1));
    if (n_reads) hipLaunchKernelGGL(map_window_counts_kernel, dim3(grid_for(n_reads, 256, cap)), dim3(256), 0, ctx->stream, chunk->d_off.p, n_reads, wcount.p);
    MDBG_TRY(exclusive_scan_u32(ctx, wcount.p, woff.p, n_reads));
    uint64_t n = 0;
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &n, woff.p + n_reads, 8, hipMemcpyDeviceToHost));
    if (n >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_map_index_build: the chunk has %llu windows, 2^32 index entries or more", (unsigned long long)n);
    ix->n_entries = n;
    MDBG_TRY(ix->d_pair.alloc(ctx, n)); MDBG_TRY(ix->d_win.alloc(ctx, n));
    MDBG_TRY(ix->d_read.alloc(ctx, n)); MDBG_TRY(ix->d_pos.alloc(ctx, n)); MDBG_TRY(ix->d_idx.alloc(ctx, n)); MDBG_TRY(ix->d_rev.alloc(ctx, n));
    if (n == 0) {
        MDBG_TRY(ix->d_distinct.alloc(ctx, 0)); MDBG_TRY(ix->d_run.alloc(ctx, 1));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(ix->d_run.p, 0, 4, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        *out = ix.release();
        return MDBG_OK;
    }
    DevBuf<uint32_t> w_read, w_pos, w_idx, head;
    DevBuf<uint8_t> w_rev;
    DevBuf<uint64_t> hpos;
    DevBuf<unsigned long long> longest;
    MDBG_TRY(w_read.alloc(ctx, n)); MDBG_TRY(w_pos.alloc(ctx, n)); MDBG_TRY(w_idx.alloc(ctx, n)); MDBG_TRY(w_rev.alloc(ctx, n));
    MDBG_TRY(head.alloc(ctx, n)); MDBG_TRY(hpos.alloc(ctx, (size_t)n + 1)); MDBG_TRY(longest.alloc(ctx, 1));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(longest.p, 0, 8, ctx->stream));
    hipLaunchKernelGGL(map_windows_kernel, dim3(grid_for(n, 256, cap)), dim3(256), 0, ctx->stream, chunk->d_off.p, chunk->d_min.p, chunk->d_pos.p, woff.p, n_reads, n,
                       chunk_first_read, ix->d_pair.p, ix->d_win.p, w_read.p, w_pos.p, w_idx.p, w_rev.p);
    MDBG_TRY(sort_u64_pairs(ctx, ix->d_pair.p, ix->d_win.p, n, nullptr));
    hipLaunchKernelGGL(map_entries_kernel, dim3(grid_for(n, 256, cap)), dim3(256), 0, ctx->stream, ix->d_pair.p, ix->d_win.p, w_read.p, w_pos.p, w_idx.p, w_rev.p, n,
                       ix->d_read.p, ix->d_pos.p, ix->d_idx.p, ix->d_rev.p, head.p);
    MDBG_TRY(exclusive_scan_u32(ctx, head.p, hpos.p, n));
    uint64_t n_pairs = 0;
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &n_pairs, hpos.p + n, 8, hipMemcpyDeviceToHost));
    ix->n_pairs = n_pairs;
    MDBG_TRY(ix->d_distinct.alloc(ctx, n_pairs)); MDBG_TRY(ix->d_run.alloc(ctx, (size_t)n_pairs + 1));
    hipLaunchKernelGGL(map_compact_heads_kernel, dim3(grid_for(n, 256, cap)), dim3(256), 0, ctx->stream, ix->d_pair.p, 0u, head.p, hpos.p, n, ix->d_distinct.p, ix->d_run.p);
    hipLaunchKernelGGL(map_longest_kernel, dim3(grid_for(n_pairs, 256, cap)), dim3(256), 0, ctx->stream, ix->d_run.p, n_pairs, longest.p);
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    unsigned long long h_longest = 0;
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &h_longest, longest.p, 8, hipMemcpyDeviceToHost));      // (and the transient buffers may go back to the pool)
    ix->longest = h_longest;
    *out = ix.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_map_index_info(const mdbg_map_index *ix, uint64_t info[4]) {
    if (!ix || !info) return MDBG_EINVAL;
    info[0] = ix->n_entries; info[1] = ix->n_pairs; info[2] = ix->longest; info[3] = ix->n_reads;
    return MDBG_OK;
}

extern "C" int mdbg_map_index_to_host(mdbg_ctx *ctx, const mdbg_map_index *ix, uint64_t *pairs, uint32_t *reads, uint32_t *positions, uint32_t *indexes,
                                      uint8_t *reversed) try {
    if (!ctx || !ix) return set_error(ctx, MDBG_EINVAL, "mdbg_map_index_to_host: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t n = ix->n_entries;
    MDBG_HIP_CHECK(ctx, download_async(ctx, pairs, ix->d_pair.p, n * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, reads, ix->d_read.p, n * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, positions, ix->d_pos.p, n * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, indexes, ix->d_idx.p, n * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, reversed, ix->d_rev.p, n));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" void mdbg_map_index_free(mdbg_map_index *ix) { delete ix; }

extern "C" int mdbg_map_anchors(mdbg_ctx *ctx, const mdbg_map_index *ix, const mdbg_minimizers *queries, uint32_t query_first_read, const mdbg_map_params *p,
                                mdbg_anchors **out) try {
    if (!ctx || !ix || !queries || !p || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_map_anchors: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_TRY(map_set_ready(ctx, "mdbg_map_anchors", "queries", queries));
    uint32_t qb = p->query_begin, qe = p->query_end;
    if (qb == 0 && qe == 0) qe = queries->n_reads;
    if (qb > qe || qe > queries->n_reads)
        return set_error(ctx, MDBG_EINVAL, "mdbg_map_anchors: the query reads [%u, %u) lie outside the set's %u reads", qb, qe, queries->n_reads);
    if ((uint64_t)query_first_read + queries->n_reads > (1ull << 32))
        return set_error(ctx, MDBG_EINVAL, "mdbg_map_anchors: %u reads from read %u leave the 32-bit read numbers", queries->n_reads, query_first_read);
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    const uint64_t nq = qe - qb;
    std::unique_ptr<mdbg_anchors> an(new mdbg_anchors());
    an->n_queries = nq;
    MDBG_TRY(an->d_pair_off.alloc(ctx, (size_t)nq + 1));
    auto finish_empty = [&]() -> int {
        MDBG_TRY(an->d_pair_ref.alloc(ctx, 0)); MDBG_TRY(an->d_anchor_off.alloc(ctx, 1));
        MDBG_TRY(an->d_ref_read.alloc(ctx, 0)); MDBG_TRY(an->d_ref_pos.alloc(ctx, 0)); MDBG_TRY(an->d_ref_idx.alloc(ctx, 0));
        MDBG_TRY(an->d_q_pos.alloc(ctx, 0)); MDBG_TRY(an->d_q_idx.alloc(ctx, 0)); MDBG_TRY(an->d_rev.alloc(ctx, 0));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(an->d_pair_off.p, 0, ((size_t)nq + 1) * 8, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(an->d_anchor_off.p, 0, 8, ctx->stream));
        MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        *out = an.release();
        return MDBG_OK;
    };
    uint64_t m01[2] = {0, 0};
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(&m01[0], queries->d_off.p + qb, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &m01[1], queries->d_off.p + qe, 8, hipMemcpyDeviceToHost));
    const uint64_t m0 = m01[0], n_items = m01[1] - m01[0];
    if (n_items >= (1ull << 32)) return set_error(ctx, MDBG_ERANGE, "mdbg_map_anchors: the query reads [%u, %u) have 2^32 minimizers or more", qb, qe);
    if (n_items == 0 || ix->n_entries == 0) return finish_empty();

    const MapQueryView q{queries->d_off.p, queries->d_min.p, queries->d_pos.p, queries->n_reads, query_first_read, qb, m0};
    const MapIndexView iv{ix->d_distinct.p, ix->d_run.p, ix->n_pairs, ix->d_read.p, ix->d_pos.p, ix->d_idx.p, ix->d_win.p, ix->d_rev.p};
    // ---- count: the anchors of every query window, their places, the total -------------------------------------------------------------
    DevBuf<uint32_t> cnt, q_read, q_begin, q_self, q_selfn;
    DevBuf<uint64_t> aoff;
    MDBG_TRY(cnt.alloc(ctx, n_items)); MDBG_TRY(q_read.alloc(ctx, n_items)); MDBG_TRY(q_begin.alloc(ctx, n_items));
    MDBG_TRY(q_self.alloc(ctx, n_items)); MDBG_TRY(q_selfn.alloc(ctx, n_items)); MDBG_TRY(aoff.alloc(ctx, (size_t)n_items + 1));
    {
        LaunchTimer timer(ctx, "map_count");
        hipLaunchKernelGGL(map_count_kernel, dim3(grid_for(n_items, 256, cap)), dim3(256), 0, ctx->stream, q, iv, n_items, cnt.p, q_read.p, q_begin.p, q_self.p, q_selfn.p);
        MDBG_TRY(exclusive_scan_u32(ctx, cnt.p, aoff.p, n_items));
    }
    uint64_t total = 0;
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &total, aoff.p + n_items, 8, hipMemcpyDeviceToHost));
    if (total >= (1ull << 32)) {
        DevBuf<unsigned long long> fit;
        MDBG_TRY(fit.alloc(ctx, 1));
        MDBG_HIP_CHECK(ctx, hipMemsetAsync(fit.p, 0, 8, ctx->stream));
        hipLaunchKernelGGL(map_fit_kernel, dim3(grid_for(nq, 256, cap)), dim3(256), 0, ctx->stream, queries->d_off.p, qb, qe, m0, aoff.p, fit.p);
        unsigned long long h_fit = 0;
        MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &h_fit, fit.p, 8, hipMemcpyDeviceToHost));
        return set_error(ctx, MDBG_ERANGE, "mdbg_map_anchors: the query reads [%u, %u) would produce %llu anchors, 2^32 or more; %llu query reads from %u fit in one call", qb,
                         qe, (unsigned long long)total, h_fit, qb);
    }
    if (total == 0) return finish_empty();

    // ---- fill and regroup ----------------------------------------------------------------------------------------------------------------
    DevBuf<uint64_t> keys, gpos;
    DevBuf<uint32_t> vals, gen_e, gen_t, head;
    MDBG_TRY(keys.alloc(ctx, total)); MDBG_TRY(vals.alloc(ctx, total)); MDBG_TRY(gen_e.alloc(ctx, total)); MDBG_TRY(gen_t.alloc(ctx, total));
    MDBG_TRY(head.alloc(ctx, total)); MDBG_TRY(gpos.alloc(ctx, (size_t)total + 1));
    {
        LaunchTimer timer(ctx, "map_fill");
        hipLaunchKernelGGL(map_fill_kernel, dim3(grid_for(total, 256, cap)), dim3(256), 0, ctx->stream, aoff.p, n_items, total, q_read.p, q_begin.p, q_self.p, q_selfn.p,
                           ix->d_win.p, qb, keys.p, vals.p, gen_e.p, gen_t.p);
    }
    MDBG_TRY(sort_u64_pairs(ctx, keys.p, vals.p, total, nullptr));
    uint64_t n_groups = 0;
    {
        LaunchTimer timer(ctx, "map_group");
        hipLaunchKernelGGL(map_group_heads_kernel, dim3(grid_for(total, 256, cap)), dim3(256), 0, ctx->stream, keys.p, vals.p, gen_e.p, ix->d_read.p, total, head.p);
        MDBG_TRY(exclusive_scan_u32(ctx, head.p, gpos.p, total));
    }
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &n_groups, gpos.p + total, 8, hipMemcpyDeviceToHost));
    DevBuf<uint64_t> gquery, knew, kidx;
    DevBuf<uint32_t> gstart, ksize, kflag;
    DevBuf<unsigned long long> longest;
    MDBG_TRY(gquery.alloc(ctx, n_groups)); MDBG_TRY(gstart.alloc(ctx, (size_t)n_groups + 1)); MDBG_TRY(ksize.alloc(ctx, n_groups)); MDBG_TRY(kflag.alloc(ctx, n_groups));
    MDBG_TRY(knew.alloc(ctx, (size_t)n_groups + 1)); MDBG_TRY(kidx.alloc(ctx, (size_t)n_groups + 1)); MDBG_TRY(longest.alloc(ctx, 1));
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(longest.p, 0, 8, ctx->stream));
    {
        LaunchTimer timer(ctx, "map_group");
        hipLaunchKernelGGL(map_compact_heads_kernel, dim3(grid_for(total, 256, cap)), dim3(256), 0, ctx->stream, keys.p, 32u, head.p, gpos.p, total, gquery.p, gstart.p);
        hipLaunchKernelGGL(map_group_sizes_kernel, dim3(grid_for(n_groups, 256, cap)), dim3(256), 0, ctx->stream, gstart.p, n_groups, p->min_anchors, ksize.p, kflag.p,
                           longest.p);
        MDBG_TRY(exclusive_scan_u32(ctx, ksize.p, knew.p, n_groups));
        MDBG_TRY(exclusive_scan_u32(ctx, kflag.p, kidx.p, n_groups));
    }
    uint64_t n_pairs = 0, n_anchors = 0;
    unsigned long long h_longest = 0;
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(&n_pairs, kidx.p + n_groups, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(&n_anchors, knew.p + n_groups, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &h_longest, longest.p, 8, hipMemcpyDeviceToHost));
    an->n_pairs = n_pairs; an->n_anchors = n_anchors; an->longest = h_longest;
    MDBG_TRY(an->d_pair_ref.alloc(ctx, n_pairs)); MDBG_TRY(an->d_anchor_off.alloc(ctx, (size_t)n_pairs + 1));
    MDBG_TRY(an->d_ref_read.alloc(ctx, n_anchors)); MDBG_TRY(an->d_ref_pos.alloc(ctx, n_anchors)); MDBG_TRY(an->d_ref_idx.alloc(ctx, n_anchors));
    MDBG_TRY(an->d_q_pos.alloc(ctx, n_anchors)); MDBG_TRY(an->d_q_idx.alloc(ctx, n_anchors)); MDBG_TRY(an->d_rev.alloc(ctx, n_anchors));
    {
        LaunchTimer timer(ctx, "map_group");
        hipLaunchKernelGGL(map_pairs_kernel, dim3(grid_for(n_groups, 256, cap)), dim3(256), 0, ctx->stream, gstart.p, kflag.p, kidx.p, knew.p, n_groups, vals.p, gen_e.p,
                           ix->d_read.p, an->d_pair_ref.p, an->d_anchor_off.p);
        hipLaunchKernelGGL(map_pair_offsets_kernel, dim3(grid_for(nq + 1, 256, cap)), dim3(256), 0, ctx->stream, gquery.p, n_groups, kidx.p, nq, an->d_pair_off.p);
        hipLaunchKernelGGL(map_emit_kernel, dim3(grid_for(total, 256, cap)), dim3(256), 0, ctx->stream, vals.p, head.p, gpos.p, gstart.p, kflag.p, knew.p, total, gen_e.p,
                           gen_t.p, q_read.p, q, iv,
                           MapAnchorRows{an->d_ref_read.p, an->d_ref_pos.p, an->d_ref_idx.p, an->d_q_pos.p, an->d_q_idx.p, an->d_rev.p});
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));       // the transient buffers go back to the pool; the inputs must outlive the kernels
    *out = an.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_anchors_info(const mdbg_anchors *a, uint64_t info[4]) {
    if (!a || !info) return MDBG_EINVAL;
    info[0] = a->n_queries; info[1] = a->n_pairs; info[2] = a->n_anchors; info[3] = a->longest;
    return MDBG_OK;
}

extern "C" int mdbg_anchors_to_host(mdbg_ctx *ctx, const mdbg_anchors *a, uint64_t *pair_offsets, uint32_t *pair_ref_read, uint64_t *anchor_offsets, uint32_t *ref_read,
                                    uint32_t *ref_position, uint32_t *ref_index, uint32_t *query_position, uint32_t *query_index, uint8_t *reversed) try {
    if (!ctx || !a) return set_error(ctx, MDBG_EINVAL, "mdbg_anchors_to_host: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t n = a->n_anchors;
    MDBG_HIP_CHECK(ctx, download_async(ctx, pair_offsets, a->d_pair_off.p, ((size_t)a->n_queries + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, pair_ref_read, a->d_pair_ref.p, (size_t)a->n_pairs * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, anchor_offsets, a->d_anchor_off.p, ((size_t)a->n_pairs + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, ref_read, a->d_ref_read.p, n * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, ref_position, a->d_ref_pos.p, n * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, ref_index, a->d_ref_idx.p, n * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, query_position, a->d_q_pos.p, n * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, query_index, a->d_q_idx.p, n * 4));
    MDBG_HIP_CHECK(ctx, download_async(ctx, reversed, a->d_rev.p, n));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_anchors_device_ptrs(const mdbg_anchors *a, const void *d_ptrs[9]) {
    if (!a || !d_ptrs) return MDBG_EINVAL;
    const void *p[9] = {a->d_pair_off.p, a->d_pair_ref.p, a->d_anchor_off.p, a->d_ref_read.p, a->d_ref_pos.p, a->d_ref_idx.p, a->d_q_pos.p, a->d_q_idx.p, a->d_rev.p};
    for (int i = 0; i < 9; i++) d_ptrs[i] = p[i];
    return MDBG_OK;
}

extern "C" void mdbg_anchors_free(mdbg_anchors *a) { delete a; }

extern "C" int mdbg_map_chains(mdbg_ctx *ctx, const mdbg_anchors *a, const mdbg_map_params *p, mdbg_chains **out) try {
    if (!ctx || !a || !p || !out) return set_error(ctx, MDBG_EINVAL, "mdbg_map_chains: null argument");
    if (p->max_chaining_band == 0) return set_error(ctx, MDBG_EINVAL, "mdbg_map_chains: max_chaining_band is 0");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const unsigned cap = (unsigned)ctx->n_cu * 32u;
    const uint64_t np = a->n_pairs, na = a->n_anchors;
    std::unique_ptr<mdbg_chains> ch(new mdbg_chains());
    ch->n_queries = a->n_queries; ch->n_pairs = np;
    MDBG_TRY(ch->d_pair_off.alloc(ctx, (size_t)a->n_queries + 1));
    MDBG_TRY(ch->d_chain.alloc(ctx, np));
    MDBG_TRY(ch->d_match_off.alloc(ctx, (size_t)np + 1));
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(ch->d_pair_off.p, a->d_pair_off.p, ((size_t)a->n_queries + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    DevBuf<unsigned long long> counters;
    DevBuf<uint32_t> n_matches, staged, g_parent;
    DevBuf<int32_t> g_score;
    MDBG_TRY(counters.alloc(ctx, 2)); MDBG_TRY(n_matches.alloc(ctx, np)); MDBG_TRY(staged.alloc(ctx, na));
    const bool spill = a->longest > CHAIN_LDS_ANCHORS;          // some pair's scores and parents do not fit LDS
    if (spill) { MDBG_TRY(g_score.alloc(ctx, na)); MDBG_TRY(g_parent.alloc(ctx, na)); }
    MDBG_HIP_CHECK(ctx, hipMemsetAsync(counters.p, 0, 16, ctx->stream));
    {
        LaunchTimer timer(ctx, "map_chains");
        if (np)
            hipLaunchKernelGGL(map_chain_kernel, dim3(grid_for(np, 4, (unsigned)ctx->n_cu * 4u)), dim3(256), 0, ctx->stream, a->d_anchor_off.p, a->d_pair_ref.p, np,
                               a->d_ref_pos.p, a->d_ref_idx.p, a->d_q_pos.p, a->d_q_idx.p, a->d_rev.p, p->max_chaining_band, counters.p, spill ? g_score.p : nullptr,
                               spill ? g_parent.p : nullptr, ch->d_chain.p, n_matches.p, staged.p);
        MDBG_TRY(exclusive_scan_u32(ctx, n_matches.p, ch->d_match_off.p, np));
    }
    unsigned long long h_counters[2] = {0, 0};
    uint64_t total = 0;
    MDBG_HIP_CHECK(ctx, hipMemcpyAsync(h_counters, counters.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    MDBG_HIP_CHECK(ctx, memcpy_sync(ctx, &total, ch->d_match_off.p + np, 8, hipMemcpyDeviceToHost));
    ch->n_found = h_counters[1]; ch->n_matches = total;
    MDBG_TRY(ch->d_matches.alloc(ctx, total));
    if (total) {
        LaunchTimer timer(ctx, "map_matches");
        hipLaunchKernelGGL(map_matches_kernel, dim3(grid_for(total, 256, cap)), dim3(256), 0, ctx->stream, ch->d_match_off.p, a->d_anchor_off.p, (uint32_t)np, total, staged.p,
                           ch->d_matches.p);
    }
    MDBG_HIP_CHECK(ctx, hipGetLastError());
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = ch.release();
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_chains_info(const mdbg_chains *c, uint64_t info[4]) {
    if (!c || !info) return MDBG_EINVAL;
    info[0] = c->n_queries; info[1] = c->n_pairs; info[2] = c->n_found; info[3] = c->n_matches;
    return MDBG_OK;
}

extern "C" int mdbg_chains_to_host(mdbg_ctx *ctx, const mdbg_chains *c, uint64_t *pair_offsets, mdbg_chain *chains, uint64_t *match_offsets, uint32_t *matches) try {
    if (!ctx || !c) return set_error(ctx, MDBG_EINVAL, "mdbg_chains_to_host: null argument");
    MDBG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MDBG_HIP_CHECK(ctx, download_async(ctx, pair_offsets, c->d_pair_off.p, ((size_t)c->n_queries + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, chains, c->d_chain.p, (size_t)c->n_pairs * sizeof(mdbg_chain)));
    MDBG_HIP_CHECK(ctx, download_async(ctx, match_offsets, c->d_match_off.p, ((size_t)c->n_pairs + 1) * 8));
    MDBG_HIP_CHECK(ctx, download_async(ctx, matches, c->d_matches.p, (size_t)c->n_matches * 4));
    MDBG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return MDBG_OK;
} MDBG_API_CATCH(ctx)

extern "C" int mdbg_chains_device_ptrs(const mdbg_chains *c, const void *d_ptrs[4]) {
    if (!c || !d_ptrs) return MDBG_EINVAL;
    d_ptrs[0] = c->d_pair_off.p; d_ptrs[1] = c->d_chain.p; d_ptrs[2] = c->d_match_off.p; d_ptrs[3] = c->d_matches.p;
    return MDBG_OK;
}

extern "C" void mdbg_chains_free(mdbg_chains *c) { delete c; }
