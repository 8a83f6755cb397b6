// test_verify.cpp -- metamdbg_amd/csrc/verify_dev.hpp (and the chain rules of mapper_dev.hpp it reuses) on the host, behind serial copies of
// the lane loops of verify.hip's count and fill kernels and of lane 0's second walk, and the chain's own map_lane_best lane by lane, against a brute-force transcription of
// filterAlignments' join (ReadCorrection.hpp:5051-5069) and MinimizerChainer.hpp (the sort :154-159, chainAnchors / argmaxPosition :735-961
// with float scores, the summary :274-673 with the reference's own loops).  Built with -fsanitize=address,undefined by
// tests/test_verify_host.py; prints its counts, which that test holds above zero.
//
//   test_verify [file of `minimizer_size n_matches n_seeds identity_bits` lines: the fixture's _identity floats]
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/verify_dev.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

using namespace mdbg;

struct Anchor { uint32_t rpos, qpos, ri, qi, rev; };
struct Read { std::vector<uint32_t> m, pos; std::vector<uint8_t> dir; uint32_t len = 0; };
struct Counts { uint64_t pairs = 0, anchors = 0, multi = 0, chains = 0, reversed_chains = 0, ties = 0, end_ties = 0, band_cuts = 0, trips_above_one = 0, tables = 0, identities = 0; } g;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// ---- serial copies of the kernels' lane loops ---------------------------------------------------------------------------------------------
// the lookup of a neighbour: its minimizers sorted by (value, index), as one stable sort by value leaves them
static void lookup(const Read &q, std::vector<uint32_t> &keys, std::vector<uint32_t> &idx) {
    idx.resize(q.m.size());
    for (uint32_t j = 0; j < idx.size(); j++) idx[j] = j;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return q.m[a] < q.m[b]; });
    keys.resize(idx.size());
    for (size_t k = 0; k < idx.size(); k++) keys[k] = q.m[idx[k]];
}

// verify_join_kernel<false>: 64 target indexes a trip, a lane sums its runs
static uint64_t count_anchors(const Read &t, const std::vector<uint32_t> &keys) {
    uint64_t lanes[64] = {0};
    for (uint32_t i0 = 0; i0 < t.m.size(); i0 += 64u)
        for (uint32_t lane = 0; lane < 64u; lane++) {
            const uint32_t i = i0 + lane;
            if (i < t.m.size()) lanes[lane] += verify_run(keys.data(), (uint32_t)keys.size(), t.m[i]).count;
        }
    uint64_t sum = 0;
    for (uint64_t v : lanes) sum += v;
    return sum;
}

// verify_join_kernel<true>: a prefix sum over the trip's lanes gives every lane its place
static std::vector<Anchor> fill_anchors(const Read &t, const Read &q, const std::vector<uint32_t> &keys, const std::vector<uint32_t> &idx, uint64_t total) {
    std::vector<Anchor> out((size_t)total);
    uint64_t base = 0;
    for (uint32_t i0 = 0; i0 < t.m.size(); i0 += 64u) {
        VerifyRun run[64];
        uint32_t incl[64], sum = 0;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            const uint32_t i = i0 + lane;
            run[lane] = i < t.m.size() ? verify_run(keys.data(), (uint32_t)keys.size(), t.m[i]) : VerifyRun{0u, 0u};
            sum += run[lane].count;
            incl[lane] = sum;
        }
        for (uint32_t lane = 0; lane < 64u; lane++) {
            const uint32_t i = i0 + lane;
            uint64_t at = base + (incl[lane] - run[lane].count);
            for (uint32_t k = 0; k < run[lane].count; k++, at++) {
                CHECK(at < total);
                const uint32_t j = idx[run[lane].begin + k];
                out[(size_t)at] = Anchor{t.pos[i], q.pos[j], i, j, map_anchor_reversed(t.dir[i], q.dir[j])};
            }
            g.multi += run[lane].count > 1;
        }
        base += incl[63];
    }
    CHECK(base == total);
    return out;
}

// chain_wave (chain_wave.hpp), its 64 lanes in turn: the kernels' own map_lane_best, one max, lane 0's store; then map_chain_walk.  Root first.
static std::vector<uint32_t> chain_lanes(const std::vector<Anchor> &a, uint32_t band) {
    const uint32_t n = (uint32_t)a.size();
    std::vector<int32_t> score(n);
    std::vector<uint32_t> parent(n), rp(n), qp(n);
    std::vector<uint8_t> rv(n);
    for (uint32_t i = 0; i < n; i++) { rp[i] = a[i].rpos; qp[i] = a[i].qpos; rv[i] = (uint8_t)a[i].rev; }
    int32_t best_score = 0;
    uint32_t best_i = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t cnt = map_band_count(i, band);
        g.trips_above_one += cnt ? (cnt - 1u) / 64u : 0u;
        uint64_t best = 0;
        for (uint32_t lane = 0; lane < 64u; lane++) best = std::max(best, map_lane_best(score.data(), rp.data(), qp.data(), rv.data(), i, band, lane));
        score[i] = map_candidate_score(best);
        parent[i] = map_candidate_parent(best);
        if (map_better_end(score[i], best_score)) { best_score = score[i]; best_i = i; }
    }
    std::vector<uint32_t> walk;
    if (!n) return walk;
    uint32_t root = best_i;
    walk.resize(map_chain_walk(parent.data(), best_i, &root));
    for (uint32_t k = (uint32_t)walk.size(), at = best_i; k > 0; at = parent[at]) walk[--k] = at;
    CHECK(walk.front() == root && parent[root] == MAP_NO_PARENT);
    return walk;
}

// lane 0's second walk and the summary
static VerifySummary summary_lanes(const std::vector<Anchor> &a, const std::vector<uint32_t> &walk, const Read &t, const Read &q) {
    const uint32_t root = walk.front(), best = walk.back();
    const uint32_t reversed = verify_query_reversed(a[root].qi, a[best].qi);
    VerifyGaps gaps{0, 0, 0};
    for (size_t k = walk.size() - 1; k > 0; k--) verify_gap(a[walk[k - 1]].ri, a[walk[k - 1]].qi, a[walk[k]].ri, a[walk[k]].qi, reversed, gaps);
    // the index invariants of a chain of 4 strictly monotone anchors: no `- 1` leaves its read
    CHECK(a[best].ri >= 3u && a[best].ri < t.m.size() && a[root].ri < t.m.size());
    if (reversed) CHECK(a[root].qi >= 3u && a[root].qi < q.m.size()); else CHECK(a[best].qi >= 3u && a[best].qi < q.m.size());
    for (size_t k = 1; k < walk.size(); k++) {
        CHECK(a[walk[k]].ri > a[walk[k - 1]].ri && a[walk[k]].rev == a[root].rev && a[root].rev == reversed);
        if (reversed) CHECK(a[walk[k]].qi < a[walk[k - 1]].qi); else CHECK(a[walk[k]].qi > a[walk[k - 1]].qi);
    }
    return verify_summary((uint32_t)walk.size(), gaps, a[root].ri, a[root].qi, a[best].ri, a[best].qi, t.pos.data(), q.pos.data(), (uint32_t)t.m.size(), (uint32_t)q.m.size(), t.len,
                          q.len);
}

// ---- the brute force: the reference's own order of work and types -------------------------------------------------------------------------
static std::vector<Anchor> brute_anchors(const Read &t, const Read &q) {
    std::map<uint32_t, std::vector<uint32_t>> where;
    for (uint32_t i = 0; i < t.m.size(); i++) where[t.m[i]].push_back(i);
    std::vector<Anchor> a;
    for (uint32_t j = 0; j < q.m.size(); j++) {
        auto hit = where.find(q.m[j]);
        if (hit == where.end()) continue;
        for (uint32_t i : hit->second) a.push_back(Anchor{t.pos[i], q.pos[j], i, j, (uint32_t)(t.dir[i] != q.dir[j])});
    }
    std::sort(a.begin(), a.end(), [](const Anchor &x, const Anchor &y) { return x.rpos == y.rpos ? x.qpos < y.qpos : x.rpos < y.rpos; });
    return a;
}

static std::vector<uint32_t> brute_chain(const std::vector<Anchor> &a, int64_t band) {       // band < 0: unlimited
    const size_t n = a.size();
    std::vector<float> scores(n, 0);
    std::vector<size_t> parents(n, 0);
    const float w = 20;
    for (size_t i = 0; i < n; i++) {
        float bestScore = 0;
        size_t bestPrev = i;
        int ties = 0;
        for (int64_t j = (int64_t)i - 1; j >= 0; j--) {
            if (band >= 0 && (int64_t)i - j > band) break;
            if (a[i].rev != a[j].rev) continue;
            if (a[i].rpos == a[j].rpos || a[i].qpos == a[j].qpos) continue;
            const int32_t d_q = a[i].rev ? (int32_t)a[j].qpos - (int32_t)a[i].qpos : (int32_t)a[i].qpos - (int32_t)a[j].qpos;
            const int32_t d_r = (int32_t)a[i].rpos - (int32_t)a[j].rpos;
            if (d_q > 5000 || d_r > 5000) continue;
            if (d_r <= 0) continue;
            const int32_t gap = std::abs(d_r - d_q);
            if (gap > 100) continue;
            if (a[i].rev ? a[i].qpos > a[j].qpos : a[i].qpos < a[j].qpos) continue;
            const float s = scores[j] + (w - gap);
            if (s > bestScore) { bestScore = s; bestPrev = (size_t)j; ties = 0; } else if (s == bestScore) ties++;
        }
        g.ties += ties > 0;
        if (bestPrev != i) { scores[i] = bestScore; parents[i] = bestPrev; } else { scores[i] = w; parents[i] = (size_t)-1; }
    }
    float maxScore = 0;
    size_t bestIndex = (size_t)-1;
    int end_ties = 0;
    for (size_t i = 0; i < n; i++) {
        if (scores[i] > maxScore) { maxScore = scores[i]; bestIndex = i; end_ties = 0; } else if (scores[i] == maxScore) end_ties++;
    }
    g.end_ties += end_ties > 0;
    std::vector<uint32_t> walk;
    for (size_t at = bestIndex; at != (size_t)-1; at = parents[at]) walk.push_back((uint32_t)at);
    std::reverse(walk.begin(), walk.end());
    return walk;
}

static VerifySummary brute_summary(const std::vector<Anchor> &a, const std::vector<uint32_t> &walk, const Read &t, const Read &q) {
    const Anchor &f = a[walk.front()], &l = a[walk.back()];
    const bool rev = f.qi > l.qi;
    const int64_t Lt = t.len, Lq = q.len;
    int64_t os, oe;
    int32_t sm, em;
    if (rev) {
        os = std::min((int64_t)t.pos[f.ri], Lq - (int64_t)q.pos[f.qi - 1]);
        sm = std::min((int32_t)f.ri, (int32_t)q.m.size() - (int32_t)f.qi - 1);
        oe = std::min(Lt - (int64_t)t.pos[l.ri - 1], (int64_t)q.pos[l.qi]);
        em = std::min((int32_t)t.m.size() - (int32_t)l.ri - 1, (int32_t)l.qi);
    } else {
        os = std::min((int64_t)t.pos[f.ri], (int64_t)q.pos[f.qi]);
        sm = std::min((int32_t)f.ri, (int32_t)f.qi);
        oe = std::min(Lt - (int64_t)t.pos[l.ri - 1], Lq - (int64_t)q.pos[l.qi - 1]);
        em = (int32_t)std::min(t.m.size() - l.ri - 1, q.m.size() - l.qi - 1);
    }
    VerifySummary s{};
    s.n_mismatches = sm;
    for (size_t k = 0; k + 1 < walk.size(); k++) {
        const Anchor &c = a[walk[k]], &x = a[walk[k + 1]];
        const int rg = (int)x.ri - (int)c.ri - 1;
        const int qg = rev ? (int)c.qi - (int)x.qi - 1 : (int)x.qi - (int)c.qi - 1;
        const int mis = std::min(rg, qg);
        int ins = 0, del = 0;
        if (rg > qg) del = rg - mis; else ins = qg - mis;
        s.n_matches += 1; s.n_mismatches += mis; s.n_deletions += del; s.n_insertions += ins;
    }
    s.n_matches += 1;
    s.n_mismatches += em;
    s.query_reversed = rev;
    s.overhang_start = (uint32_t)os; s.overhang_end = (uint32_t)oe;
    const uint64_t rs = (uint64_t)(s.n_matches + s.n_mismatches + s.n_deletions), qs = (uint64_t)(s.n_matches + s.n_mismatches + s.n_insertions);
    s.n_seeds = (uint32_t)std::min(rs, qs);
    s.align_length = l.rpos - f.rpos;
    s.reference_start = f.rpos; s.reference_end = l.rpos;
    s.query_start = rev ? l.qpos : f.qpos; s.query_end = rev ? f.qpos : l.qpos;
    return s;
}

static bool same(const VerifySummary &x, const VerifySummary &y) {
    return x.query_reversed == y.query_reversed && x.n_matches == y.n_matches && x.n_mismatches == y.n_mismatches && x.n_deletions == y.n_deletions &&
           x.n_insertions == y.n_insertions && x.overhang_start == y.overhang_start && x.overhang_end == y.overhang_end && x.align_length == y.align_length &&
           x.n_seeds == y.n_seeds && x.reference_start == y.reference_start && x.reference_end == y.reference_end && x.query_start == y.query_start &&
           x.query_end == y.query_end;
}

// ---- every multiset of up to 5 anchors over a 3 x 3 grid of positions and both strands ----------------------------------------------------
static void check_multisets(uint32_t band) {
    const uint32_t pos[3] = {0u, 50u, 200u};
    std::vector<Anchor> types;
    for (uint32_t r = 0; r < 3; r++) for (uint32_t q = 0; q < 3; q++) for (uint32_t v = 0; v < 2; v++) types.push_back(Anchor{pos[r], pos[q], r, q, v});
    std::vector<uint32_t> pick;
    auto run = [&]() {
        std::vector<Anchor> a;
        for (uint32_t k : pick) a.push_back(types[k]);            // types ascend in (rpos, qpos): a multiset taken in order is sorted
        CHECK(chain_lanes(a, band) == brute_chain(a, band));
        g.pairs++;
    };
    for (uint32_t n = 1; n <= 5; n++) {
        pick.assign(n, 0);
        for (;;) {
            run();
            int k = (int)n - 1;
            while (k >= 0 && pick[k] == types.size() - 1) k--;
            if (k < 0) break;
            const uint32_t v = pick[k] + 1;
            for (uint32_t x = (uint32_t)k; x < n; x++) pick[x] = v;
        }
    }
}

// ---- seeded pairs of reads -----------------------------------------------------------------------------------------------------------------
static Read noisy_copy(std::mt19937_64 &rng, const std::vector<uint32_t> &gm, const std::vector<uint32_t> &gap, const std::vector<uint8_t> &strand, size_t start, size_t n, bool reverse,
                       double rate) {
    Read r;
    uint32_t p = (uint32_t)(rng() % 150);
    for (size_t k = start; k < start + n && k < gm.size(); k++) {
        const double u = (double)(rng() % 10000) / 10000.0;
        if (u >= rate) { r.m.push_back(u < 2 * rate ? (uint32_t)rng() : gm[k]); r.pos.push_back(p); r.dir.push_back(strand[k]); }
        p += gap[k] + (uint32_t)(rng() % 5);
    }
    r.len = p + 20u + (uint32_t)(rng() % 100);
    if (reverse) {
        std::reverse(r.m.begin(), r.m.end()); std::reverse(r.pos.begin(), r.pos.end()); std::reverse(r.dir.begin(), r.dir.end());
        for (auto &x : r.pos) x = r.len - 1u - x;
        for (auto &d : r.dir) d = (uint8_t)(1u - d);
    }
    return r;
}

static void check_pairs(std::mt19937_64 &rng, uint32_t band) {
    for (int it = 0; it < 360; it++) {
        const size_t glen = 20 + rng() % 400;
        std::vector<uint32_t> gm(glen), gap(glen);
        std::vector<uint8_t> strand(glen);
        const uint32_t alphabet = it % 5 == 0 ? 6u : it % 5 == 1 ? 40u : 0u;          // small alphabets: a minimizer meets several indexes
        for (size_t k = 0; k < glen; k++) { gm[k] = alphabet ? 1u + (uint32_t)(rng() % alphabet) : (uint32_t)rng(); gap[k] = 20u + (uint32_t)(rng() % 40); strand[k] = (uint8_t)(rng() & 1u); }
        if (it % 7 == 0) for (size_t k = glen / 3; k < glen / 3 + 12 && k + 1 < glen; k++) gm[k] = gm[glen / 3 + (k & 1u)];      // a tandem repeat
        if (alphabet == 6u) { gm.resize(std::min<size_t>(glen, 24)); }
        const size_t n = gm.size();
        const Read t = noisy_copy(rng, gm, gap, strand, rng() % (n / 2 + 1), 1 + rng() % n, false, it % 3 ? 0.03 : 0.2);
        const Read q = noisy_copy(rng, gm, gap, strand, rng() % (n / 2 + 1), 1 + rng() % n, it % 2 == 1, it % 4 ? 0.03 : 0.25);
        std::vector<uint32_t> keys, idx;
        lookup(q, keys, idx);
        const uint64_t total = count_anchors(t, keys);
        const std::vector<Anchor> a = fill_anchors(t, q, keys, idx, total), want = brute_anchors(t, q);
        CHECK(a.size() == want.size());
        for (size_t k = 0; k < a.size(); k++) CHECK(a[k].rpos == want[k].rpos && a[k].qpos == want[k].qpos && a[k].ri == want[k].ri && a[k].qi == want[k].qi && a[k].rev == want[k].rev);
        CHECK(verify_placed_anchors(total) == (total >= 3 ? total : 0));
        g.pairs++; g.anchors += total;
        if (total < 1 || total > 400) continue;                                         // (the anchors were checked; the chains of 1 - 400 are)
        const std::vector<uint32_t> walk = chain_lanes(a, band), bw = brute_chain(a, band);
        CHECK(walk == bw);
        g.band_cuts += brute_chain(a, -1) != bw;
        if (total < VERIFY_MIN_ANCHORS || walk.size() < VERIFY_MIN_CHAIN) continue;
        const VerifySummary s = summary_lanes(a, walk, t, q);
        CHECK(same(s, brute_summary(a, bw, t, q)));
        g.chains++; g.reversed_chains += s.query_reversed;
    }
}

// ---- the identity's table ------------------------------------------------------------------------------------------------------------------
static void check_tables() {
    const uint32_t sizes[3] = {13u, 15u, 16u};
    const float idents[4] = {0.9f, 0.96f, 1.0f, 1.5f};
    for (uint32_t size : sizes) for (float ident : idents) {
        for (uint32_t s = 0; s <= 600u; s++) {
            const uint32_t a = verify_min_matches_search(s, size, ident);
            CHECK(a == verify_min_matches_scan(s, size, ident));
            if (ident > 1.0f) CHECK(a == s + 1u);
            if (ident == 1.0f) CHECK(a == s);
            uint32_t table[1] = {a};
            if (a <= s) CHECK(verify_kept(0, 0, 1000, (int32_t)a, 0, 1000, 1000, table, 1) && (a == 0 || !verify_kept(0, 0, 1000, (int32_t)a - 1, 0, 1000, 1000, table, 1)));
        }
        g.tables++;
    }
    uint32_t one[1] = {0};
    CHECK(!verify_kept(1001, 0, 1000, 5, 0, 1000, 1000, one, 1) && !verify_kept(0, 1001, 1000, 5, 0, 1000, 1000, one, 1) && !verify_kept(0, 0, 999, 5, 0, 1000, 1000, one, 1));
    CHECK(verify_kept(1000, 1000, 1000, 5, 0, 1000, 1000, one, 1) && !verify_kept(0, 0, 1000, 5, 1, 1000, 1000, one, 1));
    CHECK(verify_local_read(5, 5, 1) == 0 && verify_local_read(4, 5, 1) == VERIFY_NO_READ && verify_local_read(6, 5, 1) == VERIFY_NO_READ && verify_local_read(0xFFFFFFFFull, 0xFFFFFFFFu, 1) == 0);
}

static void check_fixture_identities(const char *path) {
    FILE *f = std::fopen(path, "r");
    CHECK(f);
    unsigned size, m, s, bits;
    while (std::fscanf(f, "%u %u %u %u", &size, &m, &s, &bits) == 4) {
        const float mine = verify_identity(m, s, size);
        uint32_t b = 0;
        std::memcpy(&b, &mine, 4);
        CHECK(b == bits);
        g.identities++;
    }
    std::fclose(f);
}

int main(int argc, char **argv) {
    std::mt19937_64 rng(20261021);
    for (uint32_t band : {1u, 2u, 5u}) check_multisets(band);
    for (uint32_t band : {1u, 5u, 62u, 64u, 65u, 130u}) check_pairs(rng, band);
    check_tables();
    if (argc > 1) check_fixture_identities(argv[1]);
    std::printf("ok: %llu pairs, %llu anchors, %llu minimizers meeting several, %llu chains, %llu reversed chains, %llu ties met, %llu end ties, %llu band cuts that mattered, "
                "%llu trips above one, %llu tables, %llu fixture identities\n",
                (unsigned long long)g.pairs, (unsigned long long)g.anchors, (unsigned long long)g.multi, (unsigned long long)g.chains, (unsigned long long)g.reversed_chains,
                (unsigned long long)g.ties, (unsigned long long)g.end_ties, (unsigned long long)g.band_cuts, (unsigned long long)g.trips_above_one, (unsigned long long)g.tables,
                (unsigned long long)g.identities);
    return 0;
}
