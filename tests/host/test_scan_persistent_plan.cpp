// csrc/scan_plan.hpp -- the persistent launch of the pre-filtered scan -- compiled for the host: the grid, the clipping of the last
// run, that runs drawn from one counter in any order cover [0, n) exactly once, and that the deal of runs to regions is even.  The
// expectations are stated here from the rule (min(n_cu, ceil(n / (waves R))), runs of R from a fetch-and-add), not taken from the header.
#include "../../metamdbg_amd/csrc/scan_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <random>

using namespace mdbg;

static unsigned long n_checks = 0;
#define CHECK(cond, ...) do { n_checks++; if (!(cond)) { printf("%s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static void grid() {
    const int n_cu = 256;
    for (unsigned waves : {8u, 16u})
        for (unsigned R : {1u, 2u, 3u, 4u, 8u, 16u}) {
            const uint32_t g = waves * R;
            CHECK(persistent_grid(0, waves, R, n_cu, 0) == 1, "no items: one workgroup, which finds the counter used up");
            CHECK(persistent_grid(1, waves, R, n_cu, 0) == 1, "one item");
            CHECK(persistent_grid(g - 1, waves, R, n_cu, 0) == 1, "waves R - 1");
            CHECK(persistent_grid(g, waves, R, n_cu, 0) == 1, "waves R");
            CHECK(persistent_grid(g + 1, waves, R, n_cu, 0) == 2, "waves R + 1");
            CHECK(persistent_grid(g * 255u + 1u, waves, R, n_cu, 0) == 256, "the last CU gets one item");
            CHECK(persistent_grid(g * 256u + 1u, waves, R, n_cu, 0) == 256, "never more workgroups than CUs");
            CHECK(persistent_grid(10000000u, waves, R, n_cu, 0) == 256, "the benchmark's batch");
            CHECK(persistent_grid(0xFFFFFFFFu, waves, R, n_cu, 0) == 256, "the largest batch");
            CHECK(persistent_grid(10000000u, waves, R, 0, 0) == 1, "an unknown CU count: one workgroup still scans everything");
            for (uint32_t cap : {1u, 2u, 3u, 300u}) {
                CHECK(persistent_grid(10000000u, waves, R, n_cu, cap) == (cap < 256u ? cap : 256u), "the tests' cap");
                CHECK(persistent_grid(1, waves, R, n_cu, cap) == 1, "the cap never raises a grid");
            }
        }
    CHECK(persistent_grab(0) == 4 && persistent_grab(1) == 1 && persistent_grab(3) == 3 && persistent_grab(0xFFFFFFFFu) == PERSISTENT_GRAB_MAX, "R: the option, 0 = 4");
    CHECK(persistent_taken(1, 0) && !persistent_taken(0, 0) && !persistent_taken(1, 32) && !persistent_taken(0, 2), "an explicit reads-per-wave names the chunked form");
}

static void clipping() {
    for (unsigned R = 1; R <= 17; R++)
        for (uint32_t n = 0; n <= 4 * R + 3; n++) {           // every n mod R, several runs
            uint64_t covered = 0;
            for (uint64_t start = 0; start < (uint64_t)n + 3ull * R; start += R) {
                const uint32_t end = persistent_run_end(start, R, n);
                if (start >= n) { CHECK(end == n, "a run drawn behind the end is empty"); continue; }
                CHECK(end > start && end - start <= R && end <= n, "R %u n %u start %llu end %u", R, n, (unsigned long long)start, end);
                CHECK(end == n || end - start == R, "only the last run is short");
                CHECK(start == covered, "runs follow each other");
                covered = end;
            }
            CHECK(covered == n, "R %u n %u: covered %llu", R, n, (unsigned long long)covered);
        }
    // near the top of the 32-bit range the sum start + R does not wrap
    CHECK(persistent_run_end(0xFFFFFFF0ull, 64, 0xFFFFFFFFu) == 0xFFFFFFFFu, "clipped at the largest n");
    CHECK(persistent_run_end(0x100000000ull, 64, 0xFFFFFFFFu) == 0xFFFFFFFFu, "a start past 2^32 is behind the end");
}

// waves in any order: each draws (fetch-and-add of R) whenever its run is used up and leaves when it draws a start >= n, as the kernel does
static void interleavings() {
    std::mt19937_64 rng(20250607);
    std::vector<uint8_t> seen;
    for (int round = 0; round < 4000; round++) {
        const unsigned waves = 1 + (unsigned)(rng() % 64), R = 1 + (unsigned)(rng() % 9);
        const uint32_t n = (uint32_t)(rng() % 3000);
        struct Wave { uint32_t next = 0, end = 0; bool gone = false; };
        std::vector<Wave> w(waves);
        seen.assign(n, 0);
        uint64_t counter = 0, alive = waves, steps = 0;
        while (alive) {
            Wave &v = w[rng() % waves];
            if (v.gone) continue;
            CHECK(++steps < 1000000, "terminates");
            if (v.next == v.end) {
                const uint64_t start = counter; counter += R;
                if (start >= n) { v.gone = true; alive--; continue; }
                v.next = (uint32_t)start; v.end = persistent_run_end(start, R, n);
            }
            const uint32_t r = v.next++;
            CHECK(r < n && !seen[r], "item %u of %u taken twice or out of range", r, n);
            seen[r] = 1;
        }
        for (uint32_t i = 0; i < n; i++) CHECK(seen[i], "item %u of %u never taken (waves %u R %u)", i, n, waves, R);
        CHECK(counter <= (uint64_t)n + (uint64_t)(waves + 1) * R, "every wave overshoots once at the most");
    }
}

static void regions() {
    for (unsigned R : {1u, 2u, 3u, 4u, 8u, 16u})
        for (uint32_t n_regions : {1u, 2u, 8u, 64u})
            for (uint32_t n : {0u, 1u, 17u, 8191u, 8192u, 100003u}) {
                std::vector<uint32_t> items(n_regions, 0);
                for (uint32_t r = 0; r < n; r++) {
                    const uint32_t g = persistent_region(r, R, n_regions);
                    CHECK(g < n_regions, "region in range");
                    if (r % R) CHECK(g == persistent_region(r - 1, R, n_regions), "a run stays in one region");
                    items[g]++;
                }
                const uint32_t lo = *std::min_element(items.begin(), items.end()), hi = *std::max_element(items.begin(), items.end());
                CHECK(hi - lo <= R, "R %u regions %u n %u: %u .. %u items a region", R, n_regions, n, lo, hi);
            }
}

int main() {
    grid();
    clipping();
    interleavings();
    regions();
    printf("ok: %lu checks\n", n_checks);
    return 0;
}
