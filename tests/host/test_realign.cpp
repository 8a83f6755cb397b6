// test_realign.cpp -- metamdbg_amd/csrc/realign_dev.hpp on the host, behind serial copies of the lane loops of realign.hip's chain kernel
// (lane 0's raw length), lists kernel (the fill across the links, 64 a trip behind a prefix sum; the runs at both ends; lane 0's
// normalisation over tombstones) and compact kernel, and of the oriented fill of verify.hip's join -- against a transcription of
// MinimizerChainer::computeChainingAlignment's list (MinimizerChainer.hpp:330-569) and normalizeAlignment (:1015-1111) written in our own
// words with two running counters and std::vector::erase, and against a plain reverse-complement copy of a read (Commons.hpp:1042-1079).
// Built plain and with -fsanitize=address,undefined by tests/test_realign_host.py; prints its counts, which that test holds above zero,
// and the smallest case in which a robbed anchor is re-matched later in the same pass (a cascade).
//
//   test_realign <most minimizers of a pair together>
//
// Cases: every pair (T', N') of reads over the alphabet {1, 2, 3} with at most 7 minimizers each and at most <argument> together, and a seeded
// sample of the pairs of 5 - 7 minimizers each (all of them would be 10^7 pairs of some hundred chains each); for every pair EVERY chain of two or
// more equal-minimizer pairs rising in both indexes (forward) and rising in the target and falling in the neighbour (reversed).  The runs
// at both ends are what the chain's ends and the reads' lengths make them: present and absent are both counted.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/realign_dev.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <utility>
#include <vector>

using namespace mdbg;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

typedef std::vector<uint32_t> Read;
typedef std::pair<uint32_t, uint32_t> Pair;           // (ri, qi) of a chain anchor; (first, second) of a list entry
struct Counts {
    uint64_t pairs = 0, chains = 0, reversed_chains = 0, start_runs = 0, no_start_runs = 0, end_runs = 0, no_end_runs = 0, entries = 0, moves = 0, erased = 0, cascades = 0,
             trips_above_one = 0, oriented_reads = 0, oriented_anchors = 0, mirrored_runs = 0;
} g;
struct Cascade { bool found = false; Read t, n; std::vector<Pair> chain, raw, fin; } g_cascade;

// ---- the transcription: our own words, the reference's shape ------------------------------------------------------------------------------
static const uint32_t NO = 0xFFFFFFFFu;
static std::vector<Pair> list_by_counters(const Read &t, const Read &n, const std::vector<Pair> &chain, bool &has_start, bool &has_end) {
    const Pair f = chain.front(), l = chain.back();
    const bool rev = f.second > l.second;
    int64_t start_mis, end_mis;
    if (rev) { start_mis = std::min<int64_t>(f.first, (int64_t)n.size() - f.second - 1); end_mis = std::min<int64_t>((int64_t)t.size() - l.first - 1, l.second); }
    else { start_mis = std::min<int64_t>(f.first, f.second); end_mis = std::min<int64_t>((int64_t)t.size() - l.first - 1, (int64_t)n.size() - l.second - 1); }
    has_start = start_mis > 0; has_end = end_mis > 0;
    uint32_t r = f.first - (uint32_t)start_mis, q = rev ? f.second + (uint32_t)start_mis : f.second - (uint32_t)start_mis;
    auto step = [&]() { if (rev) q--; else q++; };
    std::vector<Pair> out;
    for (int64_t k = 0; k < start_mis; k++) { out.push_back(Pair(r, q)); r++; step(); }
    for (size_t c = 0; c + 1 < chain.size(); c++) {
        const Pair a = chain[c], b = chain[c + 1];
        const int rg = (int)b.first - (int)a.first - 1, qg = rev ? (int)a.second - (int)b.second - 1 : (int)b.second - (int)a.second - 1;
        const int mis = std::min(rg, qg), del = rg > qg ? rg - mis : 0, ins = rg > qg ? 0 : qg - mis;
        CHECK(r == a.first && q == a.second);
        out.push_back(Pair(r, q)); r++; step();
        for (int k = 0; k < mis + del; k++) { out.push_back(Pair(r, NO)); r++; }
        for (int k = 0; k < mis + ins; k++) { out.push_back(Pair(NO, q)); step(); }
    }
    CHECK(r == l.first && q == l.second);
    out.push_back(Pair(r, q)); r++; step();
    for (int64_t k = 0; k < end_mis; k++) { out.push_back(Pair(r, q)); r++; step(); }
    return out;
}

// one forward pass, in-place edits, erase; robbed[i]: entry i has lost an index to an earlier entry.  Returns whether a robbed entry took one.
static bool normalize_by_erase(std::vector<Pair> &a, const Read &t, const Read &n) {
    std::vector<char> robbed(a.size(), 0);
    bool cascade = false;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i].first == NO) {
            size_t j = i;
            while (j < a.size() && a[j].first == NO) j++;
            if (j == a.size()) continue;
            if (t[a[j].first] == n[a[i].second]) { a[i].first = a[j].first; a[j].first = NO; g.moves++; cascade |= robbed[i] != 0; robbed[j] = 1; }
            if (a[j].first == NO && a[j].second == NO) { a.erase(a.begin() + j); robbed.erase(robbed.begin() + j); g.erased++; }
        } else if (a[i].second == NO) {
            size_t j = i;
            while (j < a.size() && a[j].second == NO) j++;
            if (j == a.size()) continue;
            if (t[a[i].first] == n[a[j].second]) { a[i].second = a[j].second; a[j].second = NO; g.moves++; cascade |= robbed[i] != 0; robbed[j] = 1; }
            if (a[j].first == NO && a[j].second == NO) { a.erase(a.begin() + j); robbed.erase(robbed.begin() + j); g.erased++; }
        }
    }
    return cascade;
}

// ---- serial copies of the kernels' lane loops -----------------------------------------------------------------------------------------------
// `stored` is the neighbour as it lies in memory: n itself, or its reverse when the row is `turned` (then N' = n is seen through the view)
static void ours(const Read &t, const Read &stored, uint32_t turned, const std::vector<Pair> &chain, std::vector<Pair> &raw_out, std::vector<Pair> &final_out,
                 std::vector<uint8_t> &kind_out) {
    const uint32_t clen = (uint32_t)chain.size(), n_t = (uint32_t)t.size(), n_q = (uint32_t)stored.size();
    std::vector<uint32_t> ri(clen), qi(clen);
    for (uint32_t k = 0; k < clen; k++) { ri[k] = chain[k].first; qi[k] = chain[k].second; }
    const uint32_t crev = verify_query_reversed(qi[0], qi[clen - 1]);
    // realign_chain_kernel, lane 0: the raw length from the links walked backwards
    uint64_t links = 0;
    for (uint32_t b = clen - 1; b > 0; b--) links += realign_link_length(realign_link(ri[b - 1], qi[b - 1], ri[b], qi[b], crev));
    const VerifyEdges edge = verify_edge_mismatches(crev, ri[0], qi[0], ri[clen - 1], qi[clen - 1], n_t, n_q);
    const uint32_t n_raw = (uint32_t)realign_raw_length((uint64_t)edge.start_mis, links, (uint64_t)edge.end_mis);
    // realign_lists_kernel: the row's room is exactly n_raw entries (the sanitizer stands at both ends); every entry written exactly once
    std::vector<RealignEntry> list(n_raw, RealignEntry{0xDEADBEEFu, 0xDEADBEEFu});
    std::vector<uint32_t> written(n_raw, 0);
    auto put = [&](uint32_t at, RealignEntry e) { CHECK(at < n_raw); list[at] = e; written[at]++; };
    const uint32_t start_mis = (uint32_t)edge.start_mis, end_mis = (uint32_t)edge.end_mis;
    for (uint32_t lane = 0; lane < 64u; lane++)
        for (uint32_t k = lane; k < start_mis; k += 64u) put(k, realign_start_entry(ri[0], qi[0], start_mis, crev, k));
    uint32_t base = start_mis;
    for (uint32_t k0 = 0; k0 + 1u < clen; k0 += 64u) {
        if (k0) g.trips_above_one++;
        RealignLink link[64];
        uint32_t len[64], incl[64], sum = 0;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            const uint32_t k = k0 + lane;
            const bool mine = k + 1u < clen;
            link[lane] = mine ? realign_link(ri[k], qi[k], ri[k + 1u], qi[k + 1u], crev) : RealignLink{0u, 0u};
            len[lane] = mine ? realign_link_length(link[lane]) : 0u;
            sum += len[lane]; incl[lane] = sum;                         // wave_inclusive_sum
        }
        for (uint32_t lane = 0; lane < 64u; lane++) {
            const uint32_t k = k0 + lane, at = base + (incl[lane] - len[lane]);
            for (uint32_t e = 0; e < len[lane]; e++) put(at + e, realign_link_entry(ri[k], qi[k], link[lane], crev, e));
        }
        base += sum;
    }
    for (uint32_t lane = 0; lane < 64u; lane++)
        for (uint32_t k = lane; k <= end_mis; k += 64u) put(base + k, realign_end_entry(ri[clen - 1], qi[clen - 1], crev, k));
    for (uint32_t k = 0; k < n_raw; k++) CHECK(written[k] == 1u);
    raw_out.clear();
    for (const RealignEntry &e : list) raw_out.push_back(Pair(e.r, e.q));
    // lane 0: the pass over tombstones
    std::vector<uint8_t> no_quality(n_q, 0);
    const RealignQuery q{stored.data(), no_quality.data(), n_q, turned};
    realign_normalize(list.data(), n_raw, t.data(), q);
    // realign_compact_kernel: the survivors behind a prefix sum, 64 a trip
    uint32_t alive = 0;
    for (const RealignEntry &e : list) alive += realign_tombstone(e) ? 0u : 1u;
    final_out.assign(alive, Pair(0xDEADBEEFu, 0xDEADBEEFu));
    kind_out.assign(alive, 0xFF);
    uint32_t out_base = 0;
    for (uint32_t k0 = 0; k0 < n_raw; k0 += 64u) {
        uint32_t incl[64], keep[64], sum = 0;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            const uint32_t k = k0 + lane;
            keep[lane] = k < n_raw && !realign_tombstone(list[k]) ? 1u : 0u;
            sum += keep[lane]; incl[lane] = sum;
        }
        for (uint32_t lane = 0; lane < 64u; lane++) {
            if (!keep[lane]) continue;
            const uint32_t at = out_base + (incl[lane] - keep[lane]);
            CHECK(at < alive && kind_out[at] == 0xFF);
            final_out[at] = Pair(list[k0 + lane].r, list[k0 + lane].q);
            kind_out[at] = realign_kind(list[k0 + lane], t.data(), q);
        }
        out_base += sum;
    }
    CHECK(out_base == alive);
}

static void one_chain(const Read &t, const Read &n, const Read &n_reversed, uint32_t turned, const std::vector<Pair> &chain) {
    bool has_start = false, has_end = false;
    std::vector<Pair> ref = list_by_counters(t, n, chain, has_start, has_end);
    const std::vector<Pair> raw_ref = ref;
    const bool cascade = normalize_by_erase(ref, t, n);
    std::vector<Pair> raw, fin;
    std::vector<uint8_t> kind;
    ours(t, turned ? n_reversed : n, turned, chain, raw, fin, kind);
    CHECK(raw == raw_ref);
    CHECK(fin == ref);                                    // tombstones and one compaction are the reference's erase
    for (size_t k = 0; k < ref.size(); k++) {
        const uint8_t want = ref[k].first == NO ? REALIGN_INSERTION : ref[k].second == NO ? REALIGN_DELETION : t[ref[k].first] == n[ref[k].second] ? REALIGN_MATCH : REALIGN_MISMATCH;
        CHECK(kind[k] == want);
        CHECK(!(ref[k].first == NO && ref[k].second == NO));
    }
    g.chains++; g.entries += ref.size();
    g.reversed_chains += chain.front().second > chain.back().second;
    (has_start ? g.start_runs : g.no_start_runs)++;
    (has_end ? g.end_runs : g.no_end_runs)++;
    if (cascade) {
        g.cascades++;
        const size_t size = t.size() + n.size(), best = g_cascade.t.size() + g_cascade.n.size();
        // the smallest with a chain the kernels would keep (4 anchors or more), forward: what the GPU test plants
        if (chain.size() >= 4 && chain.front().second < chain.back().second && (!g_cascade.found || size < best || (size == best && raw_ref.size() < g_cascade.raw.size()))) {
            g_cascade.found = true; g_cascade.t = t; g_cascade.n = n; g_cascade.chain = chain; g_cascade.raw = raw_ref; g_cascade.fin = ref;
        }
    }
}

// every chain of two or more equal-minimizer pairs: ri rising, qi rising (dir = +1) or falling (dir = -1)
static void chains_from(const Read &t, const Read &n, const Read &n_reversed, uint32_t turned, int dir, std::vector<Pair> &chain) {
    if (chain.size() >= 2) one_chain(t, n, n_reversed, turned, chain);
    const uint32_t i0 = chain.empty() ? 0u : chain.back().first + 1u;
    for (uint32_t i = i0; i < t.size(); i++)
        for (uint32_t j = 0; j < n.size(); j++) {
            if (t[i] != n[j]) continue;
            if (!chain.empty() && (dir > 0 ? j <= chain.back().second : j >= chain.back().second)) continue;
            chain.push_back(Pair(i, j));
            chains_from(t, n, n_reversed, turned, dir, chain);
            chain.pop_back();
        }
}

static void one_pair(const Read &t, const Read &n) {
    Read n_reversed(n.rbegin(), n.rend());
    const uint32_t turned = (uint32_t)(g.pairs & 1u);               // every other pair's neighbour lies reversed in memory and is seen through the view
    g.pairs++;
    std::vector<Pair> chain;
    chains_from(t, n, n_reversed, turned, +1, chain);
    chains_from(t, n, n_reversed, turned, -1, chain);
}

static Read read_of(uint32_t code, uint32_t len) {
    Read r(len);
    for (uint32_t k = 0; k < len; k++) { r[k] = 1u + code % 3u; code /= 3u; }
    return r;
}
static uint32_t pow3(uint32_t n) { uint32_t p = 1; while (n--) p *= 3u; return p; }

// ---- the oriented view and the join's mirrored walk against a plain reverse-complement copy ---------------------------------------------------
struct Full { Read m, pos; std::vector<uint8_t> dir, qual; uint32_t len = 0; };
static Full reverse_complement(const Full &r) {
    Full o = r;
    std::reverse(o.m.begin(), o.m.end()); std::reverse(o.pos.begin(), o.pos.end()); std::reverse(o.dir.begin(), o.dir.end()); std::reverse(o.qual.begin(), o.qual.end());
    for (size_t i = 0; i < o.m.size(); i++) { o.dir[i] = !o.dir[i]; o.pos[i] = o.len - o.pos[i]; }
    return o;
}
static Full draw(std::mt19937 &rng, uint32_t n, uint32_t alphabet) {
    Full r;
    uint32_t pos = rng() % 50u;
    for (uint32_t i = 0; i < n; i++) { r.m.push_back(1u + rng() % alphabet); r.pos.push_back(pos); pos += 1u + rng() % 40u; r.dir.push_back(rng() & 1u); r.qual.push_back(rng() % 41u); }
    r.len = pos + rng() % 100u;
    return r;
}
struct Anchor { uint32_t ri, qi, rpos, qpos, rev; bool operator==(const Anchor &o) const { return ri == o.ri && qi == o.qi && rpos == o.rpos && qpos == o.qpos && rev == o.rev; } };

static void oriented_join(const Full &t, const Full &stored, uint32_t turned) {
    const Full view = turned ? reverse_complement(stored) : stored;
    const uint32_t n_q = (uint32_t)stored.m.size();
    const RealignQuery q{stored.m.data(), stored.qual.data(), n_q, turned};
    for (uint32_t j = 0; j < n_q; j++) {
        const uint32_t s = realign_oriented_index(j, n_q, turned);
        CHECK(s < n_q && realign_oriented_index(s, n_q, turned) == j);
        CHECK(realign_query_minimizer(q, j) == view.m[j] && realign_query_quality(q, j) == view.qual[j]);
        CHECK(realign_oriented_position(stored.pos[s], stored.len, turned) == view.pos[j] && realign_oriented_direction(stored.dir[s], turned) == view.dir[j]);
    }
    g.oriented_reads++;
    // the lookup of the STORED read, the fill's walk (verify_join_kernel<true, true>), lane after lane
    std::vector<uint32_t> idx(n_q), keys(n_q);
    for (uint32_t j = 0; j < n_q; j++) idx[j] = j;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return stored.m[a] < stored.m[b]; });
    for (uint32_t k = 0; k < n_q; k++) keys[k] = stored.m[idx[k]];
    std::vector<Anchor> got, want;
    for (uint32_t i = 0; i < t.m.size(); i++) {
        const VerifyRun run = verify_run(keys.data(), n_q, t.m[i]);
        if (run.count > 1 && turned) g.mirrored_runs++;
        for (uint32_t k = 0; k < run.count; k++) {
            const uint32_t e = realign_run_entry(run.begin, run.count, k, turned);
            CHECK(e >= run.begin && e < run.begin + run.count);
            const uint32_t j = idx[e];
            got.push_back(Anchor{i, realign_oriented_index(j, n_q, turned), t.pos[i], realign_oriented_position(stored.pos[j], stored.len, turned),
                                 map_anchor_reversed(t.dir[i], realign_oriented_direction(stored.dir[j], turned))});
        }
    }
    // the reference's: every equal pair of T' and the plain copy, sorted by (ref_position, query_position)
    for (uint32_t j = 0; j < n_q; j++)
        for (uint32_t i = 0; i < t.m.size(); i++)
            if (t.m[i] == view.m[j]) want.push_back(Anchor{i, j, t.pos[i], view.pos[j], (uint32_t)(t.dir[i] != view.dir[j])});
    std::sort(want.begin(), want.end(), [](const Anchor &a, const Anchor &b) { return a.rpos == b.rpos ? a.qpos < b.qpos : a.rpos < b.rpos; });
    CHECK(got == want);
    g.oriented_anchors += got.size();
}

int main(int argc, char **argv) {
    const uint32_t together = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 9u;
    // every pair of at most 7 minimizers each and at most `together` together
    for (uint32_t n_t = 1; n_t <= 7; n_t++)
        for (uint32_t n_q = 1; n_q <= 7 && n_t + n_q <= together; n_q++)
            for (uint32_t a = 0; a < pow3(n_t); a++)
                for (uint32_t b = 0; b < pow3(n_q); b++) one_pair(read_of(a, n_t), read_of(b, n_q));
    // a seeded sample of the longer pairs
    std::mt19937 rng(8100);
    for (int k = 0; k < 1200; k++) {
        const uint32_t n_t = 5u + rng() % 3u, n_q = 5u + rng() % 3u;
        one_pair(read_of(rng() % pow3(n_t), n_t), read_of(rng() % pow3(n_q), n_q));
    }
    // chains of more links than a wave has lanes: identical reads of 150 minimizers, every other one dropped from the neighbour here and there
    for (int k = 0; k < 20; k++) {
        Read t, n;
        std::vector<Pair> chain;
        for (uint32_t i = 0; i < 150; i++) {
            t.push_back(1u + rng() % 3u);
            if (rng() % 7u) { chain.push_back(Pair(i, (uint32_t)n.size())); n.push_back(t.back()); }
            if (rng() % 9u == 0) n.push_back(1u + rng() % 3u);
        }
        Read n_reversed(n.rbegin(), n.rend());
        g.pairs++;
        one_chain(t, n, n_reversed, (uint32_t)(k & 1), chain);
        std::vector<Pair> back;                                   // ... and the same chain falling in the neighbour
        for (const Pair &p : chain) back.push_back(Pair(p.first, (uint32_t)n.size() - 1u - p.second));
        one_chain(t, n_reversed, n, (uint32_t)(k & 1), back);
    }
    // the oriented view
    for (int k = 0; k < 400; k++) {
        const Full t = draw(rng, rng() % 60u, 2u + rng() % 12u), q = draw(rng, rng() % 60u, 2u + rng() % 12u);
        oriented_join(t, q, 0u);
        oriented_join(t, q, 1u);
    }
    if (g_cascade.found) {
        auto show = [](const char *name, const std::vector<Pair> &l) {
            std::printf("%s", name);
            for (const Pair &p : l) std::printf(" (%d,%d)", (int)p.first, (int)p.second);
            std::printf("\n");
        };
        std::printf("cascade: target");
        for (uint32_t v : g_cascade.t) std::printf(" %u", v);
        std::printf(" | neighbour");
        for (uint32_t v : g_cascade.n) std::printf(" %u", v);
        std::printf("\n");
        show("cascade chain:", g_cascade.chain); show("cascade raw:", g_cascade.raw); show("cascade final:", g_cascade.fin);
    }
    std::printf("ok: %llu pairs, %llu chains, %llu reversed chains, %llu/%llu with/without a start run, %llu/%llu with/without an end run, %llu entries, %llu moves, %llu erased, "
                "%llu cascades, %llu trips above one, %llu oriented reads, %llu oriented anchors, %llu mirrored runs\n",
                (unsigned long long)g.pairs, (unsigned long long)g.chains, (unsigned long long)g.reversed_chains, (unsigned long long)g.start_runs,
                (unsigned long long)g.no_start_runs, (unsigned long long)g.end_runs, (unsigned long long)g.no_end_runs, (unsigned long long)g.entries, (unsigned long long)g.moves,
                (unsigned long long)g.erased, (unsigned long long)g.cascades, (unsigned long long)g.trips_above_one, (unsigned long long)g.oriented_reads,
                (unsigned long long)g.oriented_anchors, (unsigned long long)g.mirrored_runs);
    return 0;
}
