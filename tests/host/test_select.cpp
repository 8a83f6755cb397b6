// test_select.cpp -- metamdbg_amd/csrc/select_dev.hpp on the host, behind a serial copy of the lane loop of select.hip's select_kernel
// (the rank by one stable sort of select_rank_key, then the candidates one after the other, their matches 64 a trip, one byte a
// position), against a transcription of the reference's heap procedure (ReadMapper.hpp: AlignmentScoreComparator :90-97, the push /
// replace rule of addAlignmentScore :1259-1310, the drain :809-820), fed in ascending read index.  The closed form "the first K under
// (score descending, read ascending)" is what the lane loop implements; this program does not assume it, it compares the two.
// Built plain and with -fsanitize=address,undefined by tests/test_select_host.py; prints its counts, which that test holds above zero.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/select_dev.hpp"
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <random>
#include <set>
#include <vector>

using namespace mdbg;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Cand { uint32_t read; int32_t score; std::vector<uint32_t> list; };      // list: strictly ascending positions
struct Counts { uint64_t cases = 0, candidates = 0, selected = 0, evicted_everywhere = 0, ties_at_the_cut = 0, saturated = 0, partial_trips = 0, trips_above_one = 0; } g;

// ---- the reference: one heap a position ----------------------------------------------------------------------------------------------------
struct AlignmentScore { uint32_t read; int32_t score; };
struct AlignmentScoreComparator {
    bool operator()(AlignmentScore const &a, AlignmentScore const &b) const {
        if (a.score == b.score) return a.read < b.read;
        return a.score > b.score;
    }
};
typedef std::priority_queue<AlignmentScore, std::vector<AlignmentScore>, AlignmentScoreComparator> Queue;

static std::vector<uint8_t> by_heaps(const std::vector<Cand> &cands, uint32_t coverage, uint32_t extent) {
    std::vector<Queue> queues(extent);
    std::set<uint32_t> pushed;
    for (const Cand &c : cands) {                       // ascending read index
        const AlignmentScore cur{c.read, c.score};
        for (uint32_t p : c.list) {
            Queue &queue = queues[p];
            if (queue.size() < coverage) { queue.push(cur); pushed.insert(c.read); continue; }
            const AlignmentScore &worse = queue.top();
            if (cur.score < worse.score) continue;
            if (cur.score == worse.score) {
                g.ties_at_the_cut++;
                if (cur.read > worse.read) continue;
            }
            queue.pop();
            queue.push(cur);
            pushed.insert(c.read);
        }
    }
    std::set<uint32_t> left;
    for (Queue &queue : queues)
        while (!queue.empty()) { left.insert(queue.top().read); queue.pop(); }
    std::vector<uint8_t> out(cands.size(), 0);
    for (size_t i = 0; i < cands.size(); i++) {
        out[i] = left.count(cands[i].read) ? 1 : 0;
        if (!out[i] && pushed.count(cands[i].read)) g.evicted_everywhere++;
    }
    return out;
}

// ---- the serial copy of select_kernel's loop for one query -------------------------------------------------------------------------------
static std::vector<uint8_t> by_lanes(const std::vector<Cand> &cands, uint32_t coverage, uint32_t extent) {
    const size_t n = cands.size();
    std::vector<uint64_t> keys(n);
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; i++) { keys[i] = select_rank_key(0u, cands[i].score); order[i] = (uint32_t)i; }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });     // sort_u64_pairs: stable
    std::vector<uint8_t> count(extent, 0), mark(n, 0);
    for (size_t k = 0; k < n; k++) {
        const uint32_t c = order[k];
        const uint32_t len = (uint32_t)cands[c].list.size();
        const uint32_t *list = cands[c].list.data();
        bool any = false;
        if (len > 64u) g.trips_above_one++;
        if (len % 64u) g.partial_trips++;
        for (uint32_t base = 0; base < len; base += 64u)
            for (uint32_t lane = 0; lane < 64u; lane++) {
                const uint32_t t = base + lane;
                if (t < len) {
                    const uint32_t pos = list[t];
                    if (pos < extent) {
                        const uint32_t cnt = count[pos];
                        if (select_takes(cnt, coverage)) { count[pos] = (uint8_t)(cnt + 1u); any = true; }
                        else if (cnt == 255u) g.saturated++;
                    }
                }
            }
        mark[c] = any ? 1 : 0;
    }
    for (uint32_t p = 0; p < extent; p++) CHECK(count[p] <= coverage);
    return mark;
}

static void compare(const std::vector<Cand> &cands, uint32_t coverage) {
    uint32_t extent = 0;
    for (const Cand &c : cands) {
        CHECK(!c.list.empty());
        for (size_t i = 1; i < c.list.size(); i++) CHECK(c.list[i] > c.list[i - 1]);
        extent = std::max(extent, c.list.back() + 1u);
    }
    const std::vector<uint8_t> want = by_heaps(cands, coverage, extent), got = by_lanes(cands, coverage, extent);
    CHECK(want == got);
    g.cases++;
    g.candidates += cands.size();
    for (uint8_t m : got) g.selected += m;
}

// Every assignment of a score from {-1, 0, 1, 2} and a non-empty subset of 4 positions to each of n candidates, at coverage 1, 2 and 3.
// BOUNDED: all 60^n assignments for n = 1, 2, 3 (219 660 of them); for n = 4, 5 and 6 -- 60^4 ... 60^6, up to 4.7 * 10^10 -- a seeded
// sample of 50 000 assignments each, so that the program runs in seconds under the sanitizers.
static std::vector<Cand> enumerated(uint64_t code, uint32_t n) {
    std::vector<Cand> cands(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t digit = (uint32_t)(code % 60u);
        code /= 60u;
        cands[i].read = 10u + 3u * i;
        cands[i].score = (int32_t)(digit % 4u) - 1;
        const uint32_t subset = digit / 4u + 1u;        // 1 ... 15
        for (uint32_t p = 0; p < 4u; p++) if (subset >> p & 1u) cands[i].list.push_back(p);
    }
    return cands;
}

static void check_enumerated(std::mt19937_64 &rng) {
    for (uint32_t coverage = 1; coverage <= 3; coverage++) {
        uint64_t total = 1;
        for (uint32_t n = 1; n <= 6; n++) {
            total *= 60u;
            if (n <= 3) for (uint64_t code = 0; code < total; code++) compare(enumerated(code, n), coverage);
            else for (int it = 0; it < 50000; it++) compare(enumerated(rng() % total, n), coverage);
        }
    }
}

static Cand seeded(std::mt19937_64 &rng, uint32_t read, uint32_t extent, uint32_t len) {
    Cand c;
    c.read = read;
    std::vector<uint32_t> all(extent);
    for (uint32_t i = 0; i < extent; i++) all[i] = i;
    if (len >= extent) c.list = all;
    else {                                               // a run with holes: what a chain's list looks like
        const uint32_t span = std::min(extent, len + (uint32_t)(rng() % (len / 4u + 2u)));
        const uint32_t first = (uint32_t)(rng() % (extent - span + 1u));
        std::vector<uint32_t> run(all.begin() + first, all.begin() + first + span);
        std::shuffle(run.begin(), run.end(), rng);
        run.resize(len);
        std::sort(run.begin(), run.end());
        c.list = run;
    }
    c.score = select_list_score((uint32_t)c.list.size(), c.list.front(), c.list.back());
    return c;
}

static void check_seeded(std::mt19937_64 &rng) {
    const uint32_t coverages[3] = {1u, 20u, 255u};
    for (uint32_t coverage : coverages)
        for (uint32_t n = 1; n <= 300; n += (n < 40 ? 1 : 13)) {
            const uint32_t extent = 20u + (uint32_t)(rng() % 400u);
            std::vector<Cand> cands;
            for (uint32_t i = 0; i < n; i++) cands.push_back(seeded(rng, 5u + 2u * i, extent, 1u + (uint32_t)(rng() % std::min(extent, 60u))));
            compare(cands, coverage);
        }
    // list lengths at the wave: 1, 63, 64, 65, 128, 129 -- thirty candidates of each, over one stretch of 140 positions
    const uint32_t lens[6] = {1u, 63u, 64u, 65u, 128u, 129u};
    for (uint32_t coverage : coverages) {
        std::vector<Cand> cands;
        for (uint32_t i = 0; i < 180u; i++) cands.push_back(seeded(rng, i, 140u, lens[i % 6u]));
        compare(cands, coverage);
    }
    // counter saturation: 300 candidates on the same two positions at coverage 255 -- the byte stops at 255, and 255 candidates are selected
    {
        std::vector<Cand> cands(300);
        for (uint32_t i = 0; i < 300u; i++) { cands[i].read = i; cands[i].list = {0u, 7u}; cands[i].score = (int32_t)(rng() % 5u) - 2; }
        const uint64_t before = g.saturated;
        compare(cands, 255u);
        CHECK(g.saturated > before);
        const std::vector<uint8_t> m = by_lanes(cands, 255u, 8u);
        CHECK(std::count(m.begin(), m.end(), 1) == 255);
    }
}

static void check_rules() {
    // the rank key: descending in the score, whatever the sign; the query above it
    const int32_t s[5] = {INT32_MIN, -1, 0, 1, INT32_MAX};
    for (int i = 0; i + 1 < 5; i++) CHECK(select_rank_word(s[i]) > select_rank_word(s[i + 1]));
    CHECK(select_rank_word(INT32_MAX) == 0u && select_rank_word(INT32_MIN) == 0xFFFFFFFFu);
    for (int i = 0; i < 5; i++) for (int j = 0; j < 5; j++) {
        CHECK(select_rank_key(7u, s[i]) < select_rank_key(8u, s[j]));
        CHECK((select_rank_key(7u, s[i]) < select_rank_key(7u, s[j])) == (s[i] > s[j]));
    }
    CHECK(select_rank_key(0xFFFFFFFFu, 0) >> 32 == 0xFFFFFFFFull);
    // the counter step
    CHECK(select_takes(0u, 1u) && !select_takes(1u, 1u) && select_takes(254u, 255u) && !select_takes(255u, 255u) && select_takes(19u, 20u) && !select_takes(20u, 20u));
    // the score of a list: mergeAlignmentScore's loop (:376-382) on the same list
    std::mt19937_64 rng(5);
    for (int it = 0; it < 2000; it++) {
        std::vector<uint32_t> list{(uint32_t)(rng() % 1000u)};
        const uint32_t n = 1u + (uint32_t)(rng() % 300u);
        for (uint32_t i = 1; i < n; i++) list.push_back(list.back() + 1u + (uint32_t)(rng() % 4u == 0 ? rng() % 9u : 0u));
        int32_t score = 0;
        for (size_t i = 0; i + 1 < list.size(); i++) { score += 1; score -= (int32_t)(list[i + 1] - list[i] - 1u); }
        score += 1;
        CHECK(select_list_score((uint32_t)list.size(), list.front(), list.back()) == score);
    }
    CHECK(select_list_score(1u, 0xFFFFFFFFu, 0xFFFFFFFFu) == 1 && select_list_score(2u, 0u, 0x7FFFFFFFu) == 4 - (int64_t)0x80000000ll);
    // where a record starts, past 2^32: 64-bit arithmetic
    CHECK(select_record_start(0u, 0u) == 0u && select_record_start(3u, 10u) == 64u);
    CHECK(select_record_start(1ull << 30, 1ull << 31) == (8ull << 30) + (4ull << 31));
    CHECK(select_record_start(0xFFFFFFFFull, 0xFFFFFFFFull) == 12ull * 0xFFFFFFFFull);
    CHECK(select_record_start(600000000ull, 0u) > (1ull << 32) && select_record_start(0u, 1100000000ull) > (1ull << 32));
}

int main() {
    std::mt19937_64 rng(20240607);
    check_rules();
    check_enumerated(rng);
    check_seeded(rng);
    std::printf("ok: %llu cases, %llu candidates, %llu selected, %llu pushed and evicted everywhere, %llu ties at the cut, %llu saturated steps, %llu partial trips, "
                "%llu lists above one trip\n", (unsigned long long)g.cases, (unsigned long long)g.candidates, (unsigned long long)g.selected,
                (unsigned long long)g.evicted_everywhere, (unsigned long long)g.ties_at_the_cut, (unsigned long long)g.saturated, (unsigned long long)g.partial_trips,
                (unsigned long long)g.trips_above_one);
    return 0;
}
