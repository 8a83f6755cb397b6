// The two pieces of arithmetic mdbg_tool's readSelection leans on, driven without a library or a GPU:
//   metamdbg_amd/host/ordered_place.hpp  OrderedPlace: items finished out of order learn their file offset as soon as every earlier one is in
//   metamdbg_amd/host/bgzf_slabs.hpp     which blocks of a BGZF file make the next slab of text, and where the slab behind it begins
// A model text of records of known lengths stands in for mdbg_fastx_whole_records: the cut is the last record boundary at or before
// the end of what was inflated.  Prints "case <name> ok" per case; any failed check prints what failed and the exit status is 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../metamdbg_amd/host/bgzf_slabs.hpp"
#include "../../metamdbg_amd/host/ordered_place.hpp"

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("  FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); g_failed++; return; } } while (0)

// ---- placement ------------------------------------------------------------------------------------------------------
// items 0 .. n-1 of sizes[] are added in `order`: every offset is the prefix sum of the earlier sizes, nothing is placed before all its
// predecessors (and itself) were added, every item is placed exactly once
static void placement_case(const char *name, const std::vector<uint64_t> &sizes, const std::vector<uint64_t> &order) {
    const size_t n = sizes.size();
    std::vector<uint64_t> prefix(n + 1, 0);
    for (size_t i = 0; i < n; i++) prefix[i + 1] = prefix[i] + sizes[i];
    std::vector<char> added(n, 0);
    std::vector<int> placed(n, 0);
    size_t addedBelow = 0;                     // items [0, addedBelow) have all been added
    uint64_t lastPlaced = 0;
    bool bad = false;
    mdbg_host::OrderedPlace place;
    CHECK(order.size() == n, "%s: the order names %zu of %zu items", name, order.size(), n);
    for (uint64_t seq : order) {
        added[seq] = 1;
        while (addedBelow < n && added[addedBelow]) addedBelow++;
        place.add(seq, sizes[seq], [&](uint64_t s, uint64_t at) {
            if (s >= n || s >= addedBelow || at != prefix[s] || placed[s] || (s && s != lastPlaced + 1)) bad = true;
            if (s < n) placed[s]++;
            lastPlaced = s;
        });
        CHECK(!bad, "%s: after item %llu was added", name, (unsigned long long)seq);
        // whatever can be placed is placed at once: nothing is held back either
        CHECK(place.next_seq() == addedBelow, "%s: %llu placed, %zu could be", name, (unsigned long long)place.next_seq(), addedBelow);
        CHECK(place.end_offset() == prefix[addedBelow], "%s: end offset", name);
    }
    for (size_t i = 0; i < n; i++) CHECK(placed[i] == 1, "%s: item %zu was placed %d times", name, i, placed[i]);
    CHECK(place.waiting() == 0 && place.next_seq() == n && place.end_offset() == prefix[n], "%s: the end state", name);
    printf("case placement %s ok\n", name);
}

static void placement_cases() {
    std::mt19937_64 rng(7);
    {
        std::vector<uint64_t> sizes(100), order(100);
        for (auto &s : sizes) s = rng() % 1000;
        for (size_t i = 0; i < 100; i++) order[i] = 99 - i;
        placement_case("reverse", sizes, order);
    }
    {
        // three consumers take the numbers in turn (c, c + 3, ...) and finish at different speeds: one, two and five a round
        const size_t n = 301;
        std::vector<uint64_t> sizes(n), order;
        for (auto &s : sizes) s = rng() % 5000;
        size_t next[3] = {0, 1, 2};
        const int speed[3] = {1, 2, 5};
        while (order.size() < n)
            for (int c = 2; c >= 0; c--)
                for (int k = 0; k < speed[c] && next[c] < n; k++, next[c] += 3) order.push_back(next[c]);
        placement_case("three-consumers", sizes, order);
    }
    {
        std::vector<uint64_t> sizes = {0, 0, 7, 0, 0, 0, 3, 0}, order = {3, 7, 0, 2, 1, 6, 5, 4};
        placement_case("zero-byte-items", sizes, order);
        placement_case("all-zero-bytes", std::vector<uint64_t>(8, 0), order);
    }
    placement_case("single-item", {42}, {0});
    {
        const size_t n = 10000;
        std::vector<uint64_t> sizes(n), order(n);
        for (auto &s : sizes) s = rng() % ((uint64_t)1 << 33);      // offsets pass 2^32 early
        std::iota(order.begin(), order.end(), 0);
        std::shuffle(order.begin(), order.end(), rng);
        placement_case("10000-random", sizes, order);
    }
}

// ---- BGZF slabs ----------------------------------------------------------------------------------------------------------
struct SlabRun { std::vector<std::pair<uint64_t, uint64_t>> slabs; mdbg_host::BgzfNext last; int inflations = 0; };

// the whole file through bgzf_next_slab: the slabs' [begin, end) in the file's text, and how the run ended
static SlabRun cut_into_slabs(const std::vector<uint64_t> &cum, const std::vector<uint64_t> &recordEnds, uint64_t batchText) {
    SlabRun run;
    mdbg_host::BgzfCursor c;
    size_t b0 = 0, b1 = 0;
    const size_t nb = cum.size() - 1;
    for (int guard = 0; guard < 1000000; guard++) {
        uint64_t begin = 0, end = 0;
        run.last = mdbg_host::bgzf_next_slab(
            cum, c, batchText,
            [&](size_t x0, size_t x1) -> uint64_t {
                if (!(x0 < x1 && x1 <= nb)) { printf("  FAILED: blocks [%zu, %zu) of %zu\n", x0, x1, nb); g_failed++; exit(1); }
                b0 = x0; b1 = x1; run.inflations++;
                return cum[x1] - cum[x0];
            },
            [&](uint64_t from, uint64_t n) -> uint64_t {       // the last record boundary in (from, n] of the inflated text, else from
                const uint64_t top = cum[b0] + n;
                auto it = std::upper_bound(recordEnds.begin(), recordEnds.end(), top);
                if (it == recordEnds.begin()) return from;
                const uint64_t at = *(it - 1);
                return at > cum[b0] + from ? at - cum[b0] : from;
            },
            &begin, &end);
        if (run.last != mdbg_host::BgzfNext::SLAB) return run;
        run.slabs.emplace_back(cum[b0] + begin, cum[b0] + end);
        (void)b1;
    }
    printf("  FAILED: the file never ended\n");
    g_failed++;
    exit(1);
}

// isize per block and length per record (the two add up to the same text); tooLong: the run must stop with READ_TOO_LONG (a record no
// slab can hold) instead of tiling -- what it handed out until then still has to be in order
static void bgzf_case(const char *name, const std::vector<uint64_t> &isize, const std::vector<uint64_t> &records, uint64_t batchText, bool tooLong = false) {
    std::vector<uint64_t> cum(isize.size() + 1, 0), ends;
    for (size_t i = 0; i < isize.size(); i++) cum[i + 1] = cum[i] + isize[i];
    uint64_t total = 0;
    for (uint64_t r : records) ends.push_back(total += r);
    CHECK(total == cum.back(), "%s: the model's blocks hold %llu bytes and its records %llu", name, (unsigned long long)cum.back(), (unsigned long long)total);
    const SlabRun run = cut_into_slabs(cum, ends, batchText);
    uint64_t at = 0;
    for (size_t i = 0; i < run.slabs.size(); i++) {
        CHECK(run.slabs[i].first == at, "%s: slab %zu begins at %llu, its predecessor ended at %llu", name, i, (unsigned long long)run.slabs[i].first, (unsigned long long)at);
        CHECK(run.slabs[i].second > run.slabs[i].first, "%s: slab %zu is empty", name, i);
        at = run.slabs[i].second;
        const bool fileLast = !tooLong && i + 1 == run.slabs.size();
        if (!fileLast) CHECK(std::binary_search(ends.begin(), ends.end(), at), "%s: slab %zu ends at %llu, inside a record", name, i, (unsigned long long)at);
    }
    if (tooLong) CHECK(run.last == mdbg_host::BgzfNext::READ_TOO_LONG && at < total, "%s: expected the raise --batch-bases condition", name);
    else CHECK(run.last == mdbg_host::BgzfNext::NONE && at == total, "%s: the slabs cover %llu of %llu bytes", name, (unsigned long long)at, (unsigned long long)total);
    printf("case bgzf %s ok (%zu slabs, %d inflations)\n", name, run.slabs.size(), run.inflations);
}

static void bgzf_cases() {
    using V = std::vector<uint64_t>;
    bgzf_case("one-block", V{30}, V{10, 10, 10}, 8);
    bgzf_case("one-block-large-batch", V{30}, V{10, 10, 10}, 1000);
    bgzf_case("empty-blocks", V{0, 0, 10, 0, 10, 10, 0, 0, 10, 0}, V{5, 5, 5, 5, 5, 5, 5, 5}, 12);
    bgzf_case("only-empty-blocks", V{0, 0, 0}, V{}, 12);
    bgzf_case("block-larger-than-batch", V{100, 100, 50}, V{25, 25, 25, 25, 25, 25, 25, 25, 25, 25}, 10);
    // 28 = the end of the first run's third block would be 30: the first cut is inside block 2; the second lands on cum[5] = 50
    bgzf_case("record-spans-three-blocks-and-one-ends-on-an-edge", V{10, 10, 10, 10, 10, 10, 10, 10}, V{28, 22, 30}, 25);
    bgzf_case("records-end-on-every-edge", V{10, 10, 10, 10}, V{10, 10, 10, 10}, 10);
    bgzf_case("record-longer-than-batch", V{10, 10, 10, 10, 10, 10, 10, 10, 10, 10}, V{5, 60, 35}, 25, true);
    bgzf_case("first-record-longer-than-batch", V{100, 100}, V{150, 50}, 10, true);
    bgzf_case("batch-of-one", V{3, 2, 0, 4}, V{1, 1, 1, 1, 1, 1, 1, 1, 1}, 1);
    bgzf_case("batch-of-one-record-of-two-blocks", V{1, 1, 1, 1}, V{1, 2, 1}, 1);                  // (a run grows by one block past the batch)
    bgzf_case("batch-of-one-record-of-three-blocks", V{1, 1, 1, 1, 1}, V{1, 3, 1}, 1, true);
    // blocks and records of at most a quarter of the batch always tile
    std::mt19937_64 rng(11);
    for (int round = 0; round < 200; round++) {
        const uint64_t batchText = 4 + rng() % 400;
        V records, isize;
        uint64_t total = 0;
        for (size_t i = 0, n = 1 + rng() % 200; i < n; i++) { records.push_back(1 + rng() % (batchText / 4)); total += records.back(); }
        for (uint64_t left = total; left;) {
            const uint64_t s = rng() % 5 == 0 ? 0 : std::min<uint64_t>(left, 1 + rng() % (batchText / 4));
            isize.push_back(s);
            left -= s;
        }
        if (rng() % 2) isize.push_back(0);
        const int before = g_failed;
        bgzf_case(("random-" + std::to_string(round)).c_str(), isize, records, batchText);
        if (g_failed != before) return;
    }
}

int main() {
    placement_cases();
    bgzf_cases();
    printf(g_failed ? "FAILED %d\n" : "all ok\n", g_failed);
    return g_failed ? 1 : 0;
}
