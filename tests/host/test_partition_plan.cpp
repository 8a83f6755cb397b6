// csrc/partition_plan.hpp -- the plan of the first pass's radix split -- compiled for the host.  PINNED values, printed by a scratch
// program that held the expressions of PartRun::split_group as they stood before the plan was moved out of it (the commit before this
// file), and PROPERTIES of a level's shares: they cover every record of every segment exactly once, in order, every share but a
// segment's last is a multiple of the tile, and block -> (segment, share) is one to one over the level's grid.
#include "../../metamdbg_amd/csrc/partition_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>

using namespace mdbg;

static unsigned long n_checks = 0;
#define CHECK(cond, ...) do { n_checks++; if (!(cond)) { printf("%s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

// level (1: level 1, 2: deeper), records, segments, tile -> blocks_per_seg, grid
static void pinned() {
    struct Row { int level; uint64_t n, n_seg; uint32_t tile, blocks_per_seg; uint64_t grid; };
    const Row rows[] = {
        {1, 0ull, 1ull, 1024u, 0u, 0ull},             // (min(tiles, 2048) of no records; the first pass never asks)
        {1, 1ull, 1ull, 1024u, 1u, 1ull},
        {1, 1ull, 1ull, 2048u, 1u, 1ull},
        {1, 1ull, 1ull, 4096u, 1u, 1ull},
        {1, 4ull, 1ull, 1024u, 1u, 1ull},
        {1, 4ull, 1ull, 2048u, 1u, 1ull},
        {1, 4ull, 1ull, 4096u, 1u, 1ull},
        {1, 1023ull, 1ull, 1024u, 1u, 1ull},
        {1, 1023ull, 1ull, 2048u, 1u, 1ull},
        {1, 1023ull, 1ull, 4096u, 1u, 1ull},
        {1, 1024ull, 1ull, 1024u, 1u, 1ull},
        {1, 1024ull, 1ull, 2048u, 1u, 1ull},
        {1, 1024ull, 1ull, 4096u, 1u, 1ull},
        {1, 1025ull, 1ull, 1024u, 2u, 2ull},
        {1, 1025ull, 1ull, 2048u, 1u, 1ull},
        {1, 1025ull, 1ull, 4096u, 1u, 1ull},
        {1, 2049ull, 1ull, 1024u, 3u, 3ull},
        {1, 2049ull, 1ull, 2048u, 2u, 2ull},
        {1, 2049ull, 1ull, 4096u, 1u, 1ull},
        {1, 96003ull, 1ull, 1024u, 94u, 94ull},
        {1, 96003ull, 1ull, 2048u, 47u, 47ull},
        {1, 96003ull, 1ull, 4096u, 24u, 24ull},
        {1, 4194304ull, 1ull, 1024u, 2048u, 2048ull},
        {1, 4194304ull, 1ull, 2048u, 2048u, 2048ull},
        {1, 4194304ull, 1ull, 4096u, 1024u, 1024ull},
        {1, 4194305ull, 1ull, 1024u, 2048u, 2048ull},
        {1, 4194305ull, 1ull, 2048u, 2048u, 2048ull},
        {1, 4194305ull, 1ull, 4096u, 1025u, 1025ull},
        {1, 344000000ull, 1ull, 1024u, 2048u, 2048ull},
        {1, 344000000ull, 1ull, 2048u, 2048u, 2048ull},
        {1, 344000000ull, 1ull, 4096u, 2048u, 2048ull},
        {1, 4294967295ull, 1ull, 1024u, 2048u, 2048ull},
        {1, 4294967295ull, 1ull, 2048u, 2048u, 2048ull},
        {1, 4294967295ull, 1ull, 4096u, 2048u, 2048ull},
        {2, 0ull, 2ull, 1024u, 1u, 2ull},
        {2, 0ull, 2ull, 2048u, 1u, 2ull},
        {2, 0ull, 2ull, 4096u, 1u, 2ull},
        {2, 0ull, 8ull, 1024u, 1u, 8ull},
        {2, 0ull, 8ull, 2048u, 1u, 8ull},
        {2, 0ull, 8ull, 4096u, 1u, 8ull},
        {2, 0ull, 256ull, 1024u, 1u, 256ull},
        {2, 0ull, 256ull, 2048u, 1u, 256ull},
        {2, 0ull, 256ull, 4096u, 1u, 256ull},
        {2, 0ull, 512ull, 1024u, 1u, 512ull},
        {2, 0ull, 512ull, 2048u, 1u, 512ull},
        {2, 0ull, 512ull, 4096u, 1u, 512ull},
        {2, 0ull, 4096ull, 1024u, 1u, 4096ull},
        {2, 0ull, 4096ull, 2048u, 1u, 4096ull},
        {2, 0ull, 4096ull, 4096u, 1u, 4096ull},
        {2, 0ull, 65536ull, 1024u, 1u, 65536ull},
        {2, 0ull, 65536ull, 2048u, 1u, 65536ull},
        {2, 0ull, 65536ull, 4096u, 1u, 65536ull},
        {2, 1ull, 2ull, 1024u, 1u, 2ull},
        {2, 1ull, 2ull, 2048u, 1u, 2ull},
        {2, 1ull, 2ull, 4096u, 1u, 2ull},
        {2, 1ull, 8ull, 1024u, 1u, 8ull},
        {2, 1ull, 8ull, 2048u, 1u, 8ull},
        {2, 1ull, 8ull, 4096u, 1u, 8ull},
        {2, 1ull, 256ull, 1024u, 1u, 256ull},
        {2, 1ull, 256ull, 2048u, 1u, 256ull},
        {2, 1ull, 256ull, 4096u, 1u, 256ull},
        {2, 1ull, 512ull, 1024u, 1u, 512ull},
        {2, 1ull, 512ull, 2048u, 1u, 512ull},
        {2, 1ull, 512ull, 4096u, 1u, 512ull},
        {2, 1ull, 4096ull, 1024u, 1u, 4096ull},
        {2, 1ull, 4096ull, 2048u, 1u, 4096ull},
        {2, 1ull, 4096ull, 4096u, 1u, 4096ull},
        {2, 1ull, 65536ull, 1024u, 1u, 65536ull},
        {2, 1ull, 65536ull, 2048u, 1u, 65536ull},
        {2, 1ull, 65536ull, 4096u, 1u, 65536ull},
        {2, 1025ull, 2ull, 1024u, 1u, 2ull},
        {2, 1025ull, 2ull, 2048u, 1u, 2ull},
        {2, 1025ull, 2ull, 4096u, 1u, 2ull},
        {2, 1025ull, 8ull, 1024u, 1u, 8ull},
        {2, 1025ull, 8ull, 2048u, 1u, 8ull},
        {2, 1025ull, 8ull, 4096u, 1u, 8ull},
        {2, 1025ull, 256ull, 1024u, 1u, 256ull},
        {2, 1025ull, 256ull, 2048u, 1u, 256ull},
        {2, 1025ull, 256ull, 4096u, 1u, 256ull},
        {2, 1025ull, 512ull, 1024u, 1u, 512ull},
        {2, 1025ull, 512ull, 2048u, 1u, 512ull},
        {2, 1025ull, 512ull, 4096u, 1u, 512ull},
        {2, 1025ull, 4096ull, 1024u, 1u, 4096ull},
        {2, 1025ull, 4096ull, 2048u, 1u, 4096ull},
        {2, 1025ull, 4096ull, 4096u, 1u, 4096ull},
        {2, 1025ull, 65536ull, 1024u, 1u, 65536ull},
        {2, 1025ull, 65536ull, 2048u, 1u, 65536ull},
        {2, 1025ull, 65536ull, 4096u, 1u, 65536ull},
        {2, 96000ull, 2ull, 1024u, 47u, 94ull},
        {2, 96000ull, 2ull, 2048u, 24u, 48ull},
        {2, 96000ull, 2ull, 4096u, 12u, 24ull},
        {2, 96000ull, 8ull, 1024u, 12u, 96ull},
        {2, 96000ull, 8ull, 2048u, 6u, 48ull},
        {2, 96000ull, 8ull, 4096u, 3u, 24ull},
        {2, 96000ull, 256ull, 1024u, 1u, 256ull},
        {2, 96000ull, 256ull, 2048u, 1u, 256ull},
        {2, 96000ull, 256ull, 4096u, 1u, 256ull},
        {2, 96000ull, 512ull, 1024u, 1u, 512ull},
        {2, 96000ull, 512ull, 2048u, 1u, 512ull},
        {2, 96000ull, 512ull, 4096u, 1u, 512ull},
        {2, 96000ull, 4096ull, 1024u, 1u, 4096ull},
        {2, 96000ull, 4096ull, 2048u, 1u, 4096ull},
        {2, 96000ull, 4096ull, 4096u, 1u, 4096ull},
        {2, 96000ull, 65536ull, 1024u, 1u, 65536ull},
        {2, 96000ull, 65536ull, 2048u, 1u, 65536ull},
        {2, 96000ull, 65536ull, 4096u, 1u, 65536ull},
        {2, 5000000ull, 2ull, 1024u, 2048u, 4096ull},
        {2, 5000000ull, 2ull, 2048u, 1221u, 2442ull},
        {2, 5000000ull, 2ull, 4096u, 611u, 1222ull},
        {2, 5000000ull, 8ull, 1024u, 512u, 4096ull},
        {2, 5000000ull, 8ull, 2048u, 306u, 2448ull},
        {2, 5000000ull, 8ull, 4096u, 153u, 1224ull},
        {2, 5000000ull, 256ull, 1024u, 16u, 4096ull},
        {2, 5000000ull, 256ull, 2048u, 10u, 2560ull},
        {2, 5000000ull, 256ull, 4096u, 5u, 1280ull},
        {2, 5000000ull, 512ull, 1024u, 8u, 4096ull},
        {2, 5000000ull, 512ull, 2048u, 5u, 2560ull},
        {2, 5000000ull, 512ull, 4096u, 3u, 1536ull},
        {2, 5000000ull, 4096ull, 1024u, 1u, 4096ull},
        {2, 5000000ull, 4096ull, 2048u, 1u, 4096ull},
        {2, 5000000ull, 4096ull, 4096u, 1u, 4096ull},
        {2, 5000000ull, 65536ull, 1024u, 1u, 65536ull},
        {2, 5000000ull, 65536ull, 2048u, 1u, 65536ull},
        {2, 5000000ull, 65536ull, 4096u, 1u, 65536ull},
        {2, 344000000ull, 2ull, 1024u, 2048u, 4096ull},
        {2, 344000000ull, 2ull, 2048u, 2048u, 4096ull},
        {2, 344000000ull, 2ull, 4096u, 2048u, 4096ull},
        {2, 344000000ull, 8ull, 1024u, 512u, 4096ull},
        {2, 344000000ull, 8ull, 2048u, 512u, 4096ull},
        {2, 344000000ull, 8ull, 4096u, 512u, 4096ull},
        {2, 344000000ull, 256ull, 1024u, 16u, 4096ull},
        {2, 344000000ull, 256ull, 2048u, 16u, 4096ull},
        {2, 344000000ull, 256ull, 4096u, 16u, 4096ull},
        {2, 344000000ull, 512ull, 1024u, 8u, 4096ull},
        {2, 344000000ull, 512ull, 2048u, 8u, 4096ull},
        {2, 344000000ull, 512ull, 4096u, 8u, 4096ull},
        {2, 344000000ull, 4096ull, 1024u, 1u, 4096ull},
        {2, 344000000ull, 4096ull, 2048u, 1u, 4096ull},
        {2, 344000000ull, 4096ull, 4096u, 1u, 4096ull},
        {2, 344000000ull, 65536ull, 1024u, 1u, 65536ull},
        {2, 344000000ull, 65536ull, 2048u, 1u, 65536ull},
        {2, 344000000ull, 65536ull, 4096u, 1u, 65536ull},
    };
    for (const Row &w : rows) {
        const uint32_t bps = w.level == 1 ? level1_blocks_per_seg(w.n, w.tile) : deeper_blocks_per_seg(w.n, w.n_seg, w.tile);
        CHECK(bps == w.blocks_per_seg, "level %d n %llu segs %llu tile %u: %u", w.level, (unsigned long long)w.n, (unsigned long long)w.n_seg, w.tile, bps);
        CHECK(level_grid(w.n_seg, bps) == w.grid, "grid %u", level_grid(w.n_seg, bps));
    }
}

// segment boundaries: n records in n_seg segments -- `shape` 0: equal, 1: all in the last, 2: uneven with empty ones and one of a single record
static std::vector<uint64_t> segments(uint64_t n, uint32_t n_seg, int shape) {
    std::vector<uint64_t> pos(n_seg + 1, 0);
    uint64_t x = 88172645463325252ull;
    for (uint32_t s = 1; s <= n_seg; s++) {
        uint64_t len = 0;
        const uint64_t left = n - pos[s - 1];
        if (s == n_seg) len = left;
        else if (shape == 0) len = n / n_seg;
        else if (shape == 2) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            const uint32_t kind = (uint32_t)(x % 5);
            len = kind == 0 ? 0 : kind == 1 ? 1 : (x >> 8) % (2 * (n / n_seg) + 1);
        }
        pos[s] = pos[s - 1] + (len < left ? len : left);
    }
    return pos;
}

// one level over the segments `pos` (stride 1): the shares of the blocks of its grid
static void level_properties(const std::vector<uint64_t> &pos, uint32_t n_seg, uint32_t bps, uint32_t tile) {
    const uint64_t items = level_grid(n_seg, bps);
    uint64_t at = 0;                                         // shares in item order tile the records in order
    for (uint64_t item = 0; item < items; item++) {
        uint32_t seg, j; uint64_t b, e;
        split_item((uint32_t)item, bps, seg, j);
        CHECK(seg < n_seg && j < bps && (uint64_t)seg * bps + j == item, "item %llu", (unsigned long long)item);
        split_share(pos[seg], pos[seg + 1], j, bps, tile, b, e);
        if (j == 0) CHECK(at == pos[seg] && b == pos[seg], "segment %u starts at %llu, share at %llu", seg, (unsigned long long)pos[seg], (unsigned long long)b);
        CHECK(b == at && e >= b && e <= pos[seg + 1], "item %llu: [%llu, %llu) after %llu", (unsigned long long)item, (unsigned long long)b, (unsigned long long)e, (unsigned long long)at);
        if (e != pos[seg + 1]) CHECK((e - b) % tile == 0 && e > b, "a share that is not its segment's last: %llu records", (unsigned long long)(e - b));
        if (j + 1 == bps) CHECK(e == pos[seg + 1], "segment %u ends at %llu, its last share at %llu", seg, (unsigned long long)pos[seg + 1], (unsigned long long)e);
        at = e;
    }
    CHECK(at == pos[n_seg], "covered %llu of %llu", (unsigned long long)at, (unsigned long long)pos[n_seg]);
}

static void properties() {
    const uint64_t records[] = {1, 1023, 1024, 1025, 2049, 12289, 96000, 300001, 9000000};
    const uint32_t tiles[] = {1024, 2048, 4096}, shares[] = {1, 2, 3, 256};
    const uint32_t bits[] = {3, 5};                          // ways per level: 8 and 32 -- up to 3 levels, 1024 segments at the last
    for (uint64_t n : records) for (uint32_t tile : tiles) {
        // level 1: one segment, a share per tile up to the cap, none empty
        const uint32_t bps1 = level1_blocks_per_seg(n, tile);
        CHECK(bps1 >= 1 && bps1 <= PART_LEVEL1_BLOCKS && (uint64_t)(bps1 - 1) * tile < n, "level 1: %u shares of %llu records", bps1, (unsigned long long)n);
        level_properties({0, n}, 1, bps1, tile);
        for (uint32_t b : bits) for (int shape = 0; shape < 3; shape++) {
            uint32_t n_seg = 1;
            for (uint32_t level = 2; level <= 3; level++) {
                n_seg <<= b;
                const uint32_t bps = deeper_blocks_per_seg(n, n_seg, tile);
                CHECK(bps >= 1 && (uint64_t)bps * n_seg <= std::max<uint64_t>(PART_DEEPER_BLOCKS, n_seg), "deeper: %u shares, %u segments", bps, n_seg);
                level_properties(segments(n, n_seg, shape), n_seg, bps, tile);
                // whatever the shares per segment (zero-length, one-record and uneven segments among them), they cover
                for (uint32_t c : shares) level_properties(segments(n, n_seg, shape), n_seg, c, tile);
            }
        }
    }
}

int main() {
    pinned();
    properties();
    printf("ok: %lu checks\n", n_checks);
    return 0;
}
