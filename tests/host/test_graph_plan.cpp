// host/graph_plan.hpp -- the arithmetic of a `graph` job -- against the expressions as they stood inside graph_main, graph_pieces, graph_rank's
// caller and upload_read_range of mdbg_tool.cpp before they moved to the header (the commit before this file), copied below as parent_*:
// over chosen offsets (no read, one read, reads without minimizers, a read exactly at the limit, a limit of 1, 64 and 65 pieces) and over a
// few thousand random read sets.  And the properties a set of cuts must have whatever the parent did: the pieces cover the reads in order,
// none holds more than the limit, and none could have taken the next read as well.
#include "../../metamdbg_amd/host/graph_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <random>

using namespace graph_plan;

static unsigned long n_checks = 0;
#define CHECK(cond, ...) do { n_checks++; if (!(cond)) { printf("%s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

// ---- the parent's expressions -------------------------------------------------------------------------------------------------------------
// graph_main's loop and graph_pieces' first line; 1: "one read has more minimizers than a piece may hold", 2: "more than 64 pieces"
static int parent_cuts(const std::vector<uint64_t> &offs, uint64_t maxMins, std::vector<size_t> &cuts) {
    const size_t nReads = offs.size() - 1;
    cuts = {0};
    for (size_t r = 0, first = 0; r < nReads; r++) {
        if (offs[r + 1] - offs[r] > maxMins) return 1;
        if (offs[r + 1] - offs[first] > maxMins) { cuts.push_back(r); first = r; }
    }
    cuts.push_back(nReads);
    if (cuts.size() > 2) {                                  // (graph_pieces is only called for more than one piece)
        const uint32_t n = (uint32_t)(cuts.size() - 1);
        if (n > 64) return 2;
    }
    return 0;
}
static std::vector<std::string> parent_files(const std::string &dir, bool firstPass, uint32_t k, size_t firstK) {
    std::vector<std::string> recFiles{dir + "/kminmerData_abundance.txt"};
    if (firstPass) recFiles.push_back(dir + "/kminmerData_abundance_init.txt");
    if (k == firstK + 1) recFiles.push_back(dir + "/kminmerData_abundance_init_k" + std::to_string(firstK + 1) + ".txt");
    return recFiles;
}

static std::vector<uint64_t> offsets_of(const std::vector<uint64_t> &counts) {
    std::vector<uint64_t> offs{0};
    for (uint64_t c : counts) offs.push_back(offs.back() + c);
    return offs;
}

static void check_cuts(const std::vector<uint64_t> &offs, uint64_t maxMins) {
    std::vector<size_t> cuts, want;
    const Refusal got = piece_cuts(offs, maxMins, cuts);
    const int parent = parent_cuts(offs, maxMins, want);
    CHECK((int)got == parent, "refusal %d, the parent's %d (%zu reads, limit %llu)", (int)got, parent, offs.size() - 1, (unsigned long long)maxMins);
    if (got == Refusal::read_above_limit) return;
    CHECK(cuts == want, "cuts differ from the parent's (%zu reads, limit %llu)", offs.size() - 1, (unsigned long long)maxMins);
    const size_t nReads = offs.size() - 1;
    CHECK(cuts.size() >= 2 && cuts.front() == 0 && cuts.back() == nReads, "the cuts do not span the reads");
    for (size_t p = 0; p + 1 < cuts.size(); p++) {
        CHECK(cuts[p] < cuts[p + 1] || nReads == 0, "piece %zu is empty", p);
        CHECK(offs[cuts[p + 1]] - offs[cuts[p]] <= maxMins, "piece %zu holds more than the limit", p);
        if (p + 2 < cuts.size()) CHECK(offs[cuts[p + 1] + 1] - offs[cuts[p]] > maxMins, "piece %zu had room for the next read", p);
    }
    CHECK((got == Refusal::too_many_pieces) == (cuts.size() - 1 > 64), "%zu pieces, refusal %d", cuts.size() - 1, (int)got);
}

static void check_ranges(const std::vector<uint64_t> &offs) {
    const size_t nReads = offs.size() - 1;
    for (int G : {1, 2, 3, 4, 7, 8, 64}) {
        size_t at = 0;
        for (int r = 0; r < G; r++) {
            const std::pair<size_t, size_t> got = rank_range(nReads, r, G);
            CHECK(got.first == nReads * (size_t)r / (size_t)G && got.second == nReads * (size_t)(r + 1) / (size_t)G, "rank %d of %d over %zu reads", r, G, nReads);
            CHECK(got.first == at && got.second >= at, "rank %d of %d does not follow the rank before it", r, G);
            at = got.second;
            const size_t r0 = got.first, r1 = got.second;
            const std::pair<size_t, size_t> b = byte_range(offs, r0, r1);
            const size_t b0 = 5 * r0 + 4 * (size_t)offs[r0], b1 = 5 * r1 + 4 * (size_t)offs[r1];
            CHECK(b.first == b0 && b.second == b1, "bytes of reads [%zu, %zu)", r0, r1);
            CHECK(b.second - b.first == 5 * (r1 - r0) + 4 * (size_t)(offs[r1] - offs[r0]), "a range is not the bytes of its records");
        }
        CHECK(at == nReads, "the ranks of %d do not cover %zu reads", G, nReads);
    }
    const std::pair<size_t, size_t> all = byte_range(offs, 0, nReads);
    CHECK(all.first == 0 && all.second == 5 * nReads + 4 * (size_t)offs[nReads], "the whole file");
}

int main() {
    // chosen offsets
    const std::vector<std::vector<uint64_t>> chosen = {
        {}, {0}, {7}, {0, 0, 0}, {0, 5, 0, 0, 5, 0}, {3, 4, 3}, {10}, {10, 10, 10}, {1, 1, 1, 1}, {9, 1, 10, 1, 9, 10},
        std::vector<uint64_t>(64, 10), std::vector<uint64_t>(65, 10), std::vector<uint64_t>(128, 5), std::vector<uint64_t>(130, 5),
        {4000000000ull, 4000000000ull, 5}};
    for (const std::vector<uint64_t> &counts : chosen) {
        const std::vector<uint64_t> offs = offsets_of(counts);
        for (uint64_t limit : {1ull, 2ull, 3ull, 4ull, 5ull, 6ull, 7ull, 9ull, 10ull, 11ull, 19ull, 20ull, 21ull, 640ull, 3500000000ull, 4000000000ull, ~0ull}) check_cuts(offs, limit);
        check_ranges(offs);
    }
    {   // the seams, spelled out
        std::vector<size_t> cuts;
        CHECK(piece_cuts(offsets_of({}), 1, cuts) == Refusal::none && cuts == std::vector<size_t>({0, 0}), "no read: one empty piece");
        CHECK(piece_cuts(offsets_of({10}), 10, cuts) == Refusal::none && cuts == std::vector<size_t>({0, 1}), "a read exactly at the limit");
        CHECK(piece_cuts(offsets_of({10}), 9, cuts) == Refusal::read_above_limit, "a read above the limit");
        CHECK(piece_cuts(offsets_of({1, 0, 1, 1}), 1, cuts) == Refusal::none && cuts == std::vector<size_t>({0, 2, 3, 4}), "a limit of 1");
        CHECK(piece_cuts(offsets_of(std::vector<uint64_t>(64, 10)), 10, cuts) == Refusal::none && cuts.size() == 65, "64 pieces");
        CHECK(piece_cuts(offsets_of(std::vector<uint64_t>(65, 10)), 10, cuts) == Refusal::too_many_pieces && cuts.size() == 66, "65 pieces");
    }
    // random read sets: sizes and limits that give one piece, a few, about 64, and far too many
    std::mt19937_64 rng(12345);
    for (int trial = 0; trial < 4000; trial++) {
        const size_t nReads = rng() % (trial % 4 == 0 ? 8 : 600);
        const uint64_t top = 1 + rng() % (trial % 3 == 0 ? 3 : 200);
        std::vector<uint64_t> counts(nReads);
        for (uint64_t &c : counts) c = rng() % 5 == 0 ? 0 : rng() % (top + 1);
        const std::vector<uint64_t> offs = offsets_of(counts);
        const uint64_t total = offs.back();
        for (uint64_t limit : {(uint64_t)1, top - 1, top, top + 1, total / 65 + 1, total / 64 + 1, total / 63 + top, total / 7 + top, total / 2 + top, total, total + 1})
            if (limit) check_cuts(offs, limit);
        if (trial % 16 == 0) check_ranges(offs);
    }
    // the record files of a pass
    for (int firstPass = 0; firstPass < 2; firstPass++)
        for (size_t firstK = 3; firstK < 6; firstK++)
            for (uint32_t k = 3; k < 9; k++) {
                const std::vector<std::string> got = record_files("/d/tmp", firstPass != 0, k, firstK);
                CHECK(got == parent_files("/d/tmp", firstPass != 0, k, firstK), "record files of firstPass %d k %u firstK %zu", firstPass, k, firstK);
                CHECK(got.size() == 1u + (firstPass ? 1 : 0) + (k == firstK + 1 ? 1 : 0) && got[0] == "/d/tmp/kminmerData_abundance.txt", "which files");
            }
    printf("ok: %lu checks\n", n_checks);
    return 0;
}
