// test_mapper.cpp -- metamdbg_amd/csrc/mapper_dev.hpp on the host, behind serial copies of the lane loops of mapper.hip's count and fill
// kernels and the chain's own lane routine (map_lane_best, map_chain_walk) run lane by lane, against a brute-force transcription of ReadMapper.hpp (the join of AlignReadsLowDensityFunctor::operator(), :726-742;
// argmaxPosition and chainAnchors, :887-1230, with the reference's own types: float scores, int64 positions, int32 differences).
// Built with -fsanitize=address,undefined by tests/test_mapper_host.py; prints its counts, which that test holds above zero.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/mapper_dev.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace mdbg;

struct Anchor { uint32_t rpos, qpos, ridx, qidx, rev; };
struct Counts { uint64_t windows = 0, runs = 0, self_blocks = 0, pairs = 0, anchors = 0, ties = 0, end_ties = 0, band_cuts = 0, trips_above_one = 0, chains = 0, reversed_chains = 0; } g;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// ---- the window rule against KmerVec::normalize + packPair ------------------------------------------------------------------------------
static void check_windows(std::mt19937_64 &rng) {
    for (int it = 0; it < 20000; it++) {
        uint32_t a = (uint32_t)rng(), b = it % 7 == 0 ? a : (uint32_t)rng();
        if (it % 11 == 0) b = a + 1u;
        const uint32_t pa = (uint32_t)(rng() % ((1u << 31) - 101u)), pb = pa + 1u + (uint32_t)(rng() % 100);
        const MapWindow w = map_window(a, b, pa, pb);
        // normalize: the vector is kept when it is smaller than its reverse, else reversed -- the equal case falls through to reversed
        const bool keep = a < b;
        const uint32_t lo = keep ? a : b, hi = keep ? b : a;
        CHECK(w.reversed == (keep ? 0u : 1u));
        CHECK(w.pair == (((uint64_t)lo << 32) | hi));
        CHECK(w.position == (uint32_t)(pa + pb) / 2u);
        g.windows++;
    }
    CHECK(map_read_windows(0) == 0 && map_read_windows(1) == 0 && map_read_windows(2) == 1 && map_read_windows(250) == 249);
    CHECK(!map_query_asks(9) && map_query_asks(10));
    for (uint32_t r = 0; r < 2; r++) for (uint32_t q = 0; q < 2; q++) CHECK(map_anchor_reversed(r, q) == (r != q ? 1u : 0u));        // both windows' flags (:738)
}

// ---- count and fill: a run of index entries against "every entry whose read is not the query's" -----------------------------------------
static void check_runs(std::mt19937_64 &rng) {
    for (int it = 0; it < 4000; it++) {
        const uint32_t before = (uint32_t)(rng() % 5), n = (uint32_t)(rng() % 40), after = (uint32_t)(rng() % 5);
        std::vector<uint32_t> reads(before + n + after);
        const uint32_t top = it % 9 == 0 ? 0xFFFFFFFFu : 30u;
        for (auto &r : reads) r = top == 30u ? (uint32_t)(rng() % 12) : 0xFFFFFFF0u + (uint32_t)(rng() % 16);
        std::sort(reads.begin() + before, reads.begin() + before + n);          // (the neighbours' entries are other pairs': any reads)
        const uint32_t query = n && rng() % 3 ? reads[before + rng() % n] : top == 30u ? (uint32_t)(rng() % 14) : 0xFFFFFFF0u + (uint32_t)(rng() % 16);
        const MapRun run = map_run(reads.data(), before, before + n, query);
        std::vector<uint32_t> want;
        for (uint32_t e = before; e < before + n; e++) if (reads[e] != query) want.push_back(e);
        CHECK(run.count == want.size());
        for (uint32_t j = 0; j < run.count; j++) CHECK(map_run_entry(run.begin, run.self_begin, run.self_count, j) == want[j]);      // the fill's lane j
        g.runs++;
        g.self_blocks += run.self_count > 0;
    }
}

// ---- chains -------------------------------------------------------------------------------------------------------------------------------
struct Result { std::vector<int32_t> score; std::vector<uint32_t> parent; uint32_t best = 0; bool found = false; MapChain c{}; std::vector<uint32_t> matches; };

// chain_wave (chain_wave.hpp) with its 64 lanes in turn: the kernels' own map_lane_best per lane, one max, lane 0's store; then lane 0's walk
static Result chain_lanes(const std::vector<Anchor> &a, uint32_t band) {
    Result r;
    const uint32_t n = (uint32_t)a.size();
    r.score.assign(n, 0); r.parent.assign(n, 0);
    std::vector<uint32_t> rp(n), qp(n);
    std::vector<uint8_t> rv(n);
    for (uint32_t i = 0; i < n; i++) { rp[i] = a[i].rpos; qp[i] = a[i].qpos; rv[i] = (uint8_t)a[i].rev; }
    int32_t best_score = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t cnt = map_band_count(i, band);
        g.trips_above_one += cnt ? (cnt - 1u) / 64u : 0u;
        uint64_t best = 0;
        for (uint32_t lane = 0; lane < 64u; lane++) best = std::max(best, map_lane_best(r.score.data(), rp.data(), qp.data(), rv.data(), i, band, lane));
        uint32_t at_best = 0;
        for (uint32_t t = 0; t < cnt && best; t++) {       // (counted, not used: how many predecessors reach the winning score)
            const uint32_t j = i - 1u - t;
            const uint64_t c = map_candidate(r.score[j], map_pred_gap(a[i].rpos, a[i].qpos, a[i].rev, a[j].rpos, a[j].qpos, a[j].rev), j);
            at_best += c && (c >> 32) == (best >> 32);
        }
        g.ties += at_best > 1;
        r.score[i] = map_candidate_score(best);
        r.parent[i] = map_candidate_parent(best);
        if (map_better_end(r.score[i], best_score)) { best_score = r.score[i]; r.best = i; }
    }
    if (!n) return r;
    uint32_t root = r.best;
    const uint32_t len = map_chain_walk(r.parent.data(), r.best, &root);
    if (len < MAP_MIN_CHAIN) return r;
    r.found = true;
    r.c = map_chain_fields(best_score, len, a[r.best].qidx, a[root].qidx, a[r.best].ridx, a[root].ridx, a[r.best].rpos, a[root].rpos);
    r.matches.assign(len, 0);
    uint32_t k = 0;
    for (uint32_t at = r.best; at != MAP_NO_PARENT; at = r.parent[at], k++) r.matches[r.c.query_reversed ? len - 1u - k : k] = a[at].qidx;
    return r;
}

// the transcription: argmaxPosition's loop and chainAnchors' bookkeeping with the reference's types.  band < 0: unlimited.
struct Brute { std::vector<float> score; std::vector<size_t> parent; size_t best = (size_t)-1; float max_score = 0; bool found = false;
               int64_t n_matches = 0, ndq = 0, ndr = 0, qs = 0, qe = 0, rs = 0, re = 0; bool qrev = false; std::vector<uint32_t> matches; };
static Brute chain_brute(const std::vector<Anchor> &a, int64_t band) {
    Brute b;
    const float w = 20;
    b.score.assign(a.size(), 0); b.parent.assign(a.size(), 0);
    for (size_t i = 0; i < a.size(); i++) {
        float bestScore = 0;
        size_t bestPrev = i;
        const int64_t ri = a[i].rpos, qi = a[i].qpos;
        for (int64_t j = (int64_t)i - 1; j >= 0; j--) {
            if (band >= 0 && (int64_t)i - j > band) break;
            const int64_t rj = a[j].rpos, qj = a[j].qpos;
            if (a[i].rev != a[j].rev) continue;
            if (ri == rj || qi == qj) continue;
            int32_t d_q = a[i].rev ? (int32_t)(qj - qi) : (int32_t)(qi - qj);
            int32_t d_r = (int32_t)(ri - rj);
            if (d_q > 5000 || d_r > 5000) continue;
            if (d_r <= 0) continue;
            int32_t gap = std::abs(d_r - d_q);
            if (gap > 100) continue;
            if (a[i].rev) { if (qi > qj) continue; } else { if (qi < qj) continue; }
            float new_score = b.score[j] + (w - gap);
            if (new_score > bestScore) { bestScore = new_score; bestPrev = (size_t)j; }
        }
        if (bestPrev != i) { b.score[i] = bestScore; b.parent[i] = bestPrev; } else { b.score[i] = w; b.parent[i] = (size_t)-1; }
    }
    for (size_t i = 0; i < a.size(); i++) if (b.score[i] > b.max_score) { b.max_score = b.score[i]; b.best = i; }
    std::vector<size_t> interval;
    for (size_t at = b.best; at != (size_t)-1; at = b.parent[at]) interval.push_back(at);
    if (interval.size() < 3) return b;
    b.found = true;
    for (size_t at : interval) b.matches.push_back(a[at].qidx);
    b.n_matches = (int64_t)interval.size();
    const Anchor &first = a[interval[0]], &last = a[interval.back()];
    b.qrev = first.qidx > last.qidx;
    if (b.qrev) { b.ndq = (first.qidx - last.qidx + 1) - b.n_matches; b.qs = last.qidx; b.qe = first.qidx; std::reverse(b.matches.begin(), b.matches.end()); }
    else { b.ndq = (last.qidx - first.qidx + 1) - b.n_matches; b.qs = first.qidx; b.qe = last.qidx; }
    b.ndr = (first.ridx - last.ridx + 1) - b.n_matches;
    b.rs = first.rpos; b.re = last.rpos;
    return b;
}

static void check_pair(const std::vector<Anchor> &a, uint32_t band) {
    const Result r = chain_lanes(a, band);
    const Brute b = chain_brute(a, band);
    for (size_t i = 0; i < a.size(); i++) {
        CHECK((float)r.score[i] == b.score[i]);
        CHECK((r.parent[i] == MAP_NO_PARENT ? (size_t)-1 : (size_t)r.parent[i]) == b.parent[i]);
    }
    g.pairs++;
    g.anchors += a.size();
    if (a.empty()) return;
    CHECK(r.best == b.best);
    size_t at_max = 0;
    for (float s : b.score) at_max += s == b.max_score;
    g.end_ties += at_max > 1;
    CHECK(r.found == b.found);
    if (r.found) {
        CHECK((float)r.c.score == b.max_score && r.c.n_matches == b.n_matches && (r.c.query_reversed != 0) == b.qrev && r.c.n_diff_query == b.ndq &&
              r.c.n_diff_reference == b.ndr && r.c.query_start == b.qs && r.c.query_end == b.qe && r.c.reference_start == b.rs && r.c.reference_end == b.re &&
              r.c.alignment_score == b.n_matches - b.ndq);
        CHECK(r.matches == b.matches);
        g.chains++;
        g.reversed_chains += r.c.query_reversed;
    }
    const Brute freeb = chain_brute(a, -1);
    g.band_cuts += freeb.max_score != b.max_score || freeb.best != b.best;
}

// every pair of up to 6 anchors over a small grid: ref position x query position x strand, in the sorted order the mapper leaves
static void check_small_pairs() {
    std::vector<Anchor> types;
    const uint32_t rgrid[3] = {100, 130, 240}, qgrid[3] = {50, 80, 190};
    for (uint32_t ri = 0; ri < 3; ri++) for (uint32_t qi = 0; qi < 3; qi++) for (uint32_t rev = 0; rev < 2; rev++) types.push_back({rgrid[ri], qgrid[qi], ri, qi, rev});
    std::vector<uint32_t> pick;
    std::vector<Anchor> a;
    // non-decreasing sequences of types: (ref position, query position) ascending, an anchor possibly twice
    auto walk = [&](auto &&self, uint32_t from, uint32_t left) -> void {
        a.clear();
        for (uint32_t t : pick) a.push_back(types[t]);
        for (uint32_t band : {1u, 2u, 5u}) check_pair(a, band);
        if (!left) return;
        for (uint32_t t = from; t < types.size(); t++) { pick.push_back(t); self(self, t, left - 1u); pick.pop_back(); }
    };
    walk(walk, 0, 6);
}

// seeded pairs of 1 - 300 anchors: colinear stretches on either strand with indels, strays, repeats at one reference position
static void check_seeded_pairs(std::mt19937_64 &rng) {
    const uint32_t bands[6] = {1, 5, 62, 64, 65, 130};
    for (int it = 0; it < 360; it++) {
        const uint32_t n = it < 6 ? 1u + (uint32_t)it : 1u + (uint32_t)(rng() % 300);
        std::vector<Anchor> a;
        uint32_t r = 1000, q = 100000, ridx = 10, qidx = 5000;
        uint32_t rev = (uint32_t)(rng() % 2);
        const uint32_t step = it % 4 == 0 ? 40u : 0u;      // every fourth pair: exact spacing, so that scores tie
        while (a.size() < n) {
            const uint32_t kind = (uint32_t)(rng() % 100);
            const uint32_t dr = step ? step : 20u + (uint32_t)(rng() % 40), dq = step ? step : dr + (uint32_t)(rng() % 7) - 3u;
            r += dr; ridx++;
            if (rev) { q -= dq; qidx--; } else { q += dq; qidx++; }
            if (kind < 4) { rev ^= 1u; continue; }                                             // the match changes strand
            if (kind < 10) { q += rev ? -150 : 150; continue; }                                // an indel above the gap limit
            if (kind < 16) { a.push_back({r, (uint32_t)(q + 3000u + rng() % 4000), ridx, (uint32_t)(qidx + 80), (uint32_t)(rng() % 2)}); }      // a stray
            if (kind < 30 && step) for (uint32_t k = 1; k < 1u + rng() % 70 && a.size() < n; k++)                 // a repeat: many query places at one reference place
                a.push_back({r, q + k * step * (rev ? -1 : 1), ridx, qidx + (rev ? 0u - k : k), (uint32_t)((k + rev) % 2 ? rev ^ 1u : rev)});
            a.push_back({r, q, ridx, qidx, rev});
        }
        a.resize(n);
        std::stable_sort(a.begin(), a.end(), [](const Anchor &x, const Anchor &y) { return x.rpos != y.rpos ? x.rpos < y.rpos : x.qpos < y.qpos; });
        for (uint32_t band : bands) check_pair(a, band);
    }
}

int main() {
    std::mt19937_64 rng(20240607);
    check_windows(rng);
    check_runs(rng);
    check_small_pairs();
    check_seeded_pairs(rng);
    // a wrapped index difference, as the reference's u_int32_t arithmetic leaves it (:1031-1044)
    const MapChain c = map_chain_fields(60, 3, 5, 9, 4, 8, 100, 20);
    CHECK(c.query_reversed == 0 && c.n_diff_query == 2 && c.n_diff_reference == (int64_t)(uint32_t)(4u - 8u + 1u) - 3);
    std::printf("ok: %llu windows, %llu runs, %llu with a self block, %llu pairs, %llu anchors, %llu chains, %llu reversed chains, %llu ties met, %llu end ties, "
                "%llu band cuts that mattered, %llu trips above one\n", (unsigned long long)g.windows, (unsigned long long)g.runs, (unsigned long long)g.self_blocks,
                (unsigned long long)g.pairs, (unsigned long long)g.anchors, (unsigned long long)g.chains, (unsigned long long)g.reversed_chains,
                (unsigned long long)g.ties, (unsigned long long)g.end_ties, (unsigned long long)g.band_cuts, (unsigned long long)g.trips_above_one);
    return 0;
}
