// csrc/scan_plan.hpp -- the host's plan of a scan -- compiled for the host.  Two kinds of expectation, neither taken from the header:
// PINNED values, printed by a scratch program that held the expressions of mdbg_scan / launch_scan as they stood before the plan was
// moved out of them (the commit before this file), and PROPERTIES derived from the rules the comments state.
#include "../../metamdbg_amd/csrc/scan_plan.hpp"
#include <cstdio>
#include <cstdlib>

using namespace mdbg;

constexpr int STAGE_CAP = 384, PF_STAGE_CAP = 176;              // the kernels' (scan.hip)
constexpr uint32_t SEG_TILE_BASES = 2048, SEG_G = 16384;        // segments_dev.hpp

static unsigned long n_checks = 0;
#define CHECK(cond, ...) do { n_checks++; if (!(cond)) { printf("%s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

// density_threshold (common.hpp) of the densities used here: inputs, pinned like the rest
constexpr uint64_t T_0005 = 0x0147ae13fffffff8ull, T_02 = 0x3333333fffffff00ull, T_1 = 0xfffffffffffffc00ull, T_002 = 0x051eb84fffffffe0ull;

static void region_plan() {
    struct Row { uint32_t n; uint64_t n_bases; uint32_t max_len; float density; bool hpc;
                 uint32_t n_regions; uint64_t region_cap, capacity, reserve; bool avg_fits_stage; uint32_t pf_len_limit; bool pf_split; };
    const Row rows[] = {
        // the benchmark's batch, with and without hpc
        {1000000u, 10000000000ull, 10000u, 0.005f, true,  64u, 2019720ull, 129262080ull, 8144416ull, true, 27142u, false},
        {1000000u, 10000000000ull, 10000u, 0.005f, false,  64u, 2019720ull, 129262080ull, 8144416ull, true, 0u, false},
        // the steps of the region count
        {1u, 10000ull, 10000u, 0.005f, true,  1u, 4224ull, 4224ull, 65800ull, true, 27142u, false},
        {8191u, 81910000ull, 10000u, 0.005f, true,  1u, 1060734ull, 1060734ull, 131831ull, true, 27142u, false},
        {8192u, 81920000ull, 10000u, 0.005f, true,  2u, 532479ull, 1064958ull, 132095ull, true, 27142u, false},
        {524288u, 5242880000ull, 10000u, 0.005f, true,  64u, 1060863ull, 67895232ull, 4308988ull, true, 27142u, false},
        // the average read just below and just above what the four-wave stage expects: 64 285.7 bases with hpc, 51 428.6 without
        {1000u, 64285000ull, 70000u, 0.005f, true,  1u, 485948ull, 485948ull, 95907ull, true, 0u, false},
        {1000u, 64286000ull, 70000u, 0.005f, true,  1u, 485954ull, 485954ull, 95908ull, false, 0u, false},
        {1000u, 51428000ull, 70000u, 0.005f, false,  1u, 402377ull, 402377ull, 90684ull, true, 0u, false},
        {1000u, 51429000ull, 70000u, 0.005f, false,  1u, 402384ull, 402384ull, 90685ull, false, 0u, false},
        // ... and the pre-filtered variant's: 27 142.9 bases; a longest read at the limit splits the batch, one below does not
        {1000u, 27142000ull, 30000u, 0.005f, true,  1u, 244518ull, 244518ull, 80818ull, true, 27142u, true},
        {1000u, 27143000ull, 30000u, 0.005f, true,  1u, 244525ull, 244525ull, 80818ull, true, 0u, false},
        {1000u, 27142000ull, 27142u, 0.005f, true,  1u, 244518ull, 244518ull, 80818ull, true, 27142u, true},
        {1000u, 27142000ull, 27141u, 0.005f, true,  1u, 244518ull, 244518ull, 80818ull, true, 27142u, false},
        // tests/test_gpu_parity.py::test_scan_too_many_long_reads_abandon_the_block_path (70 long reads)
        {200u, 2865000ull, 40000u, 0.02f, true,  1u, 91385ull, 91385ull, 71247ull, true, 0u, false},
        {200u, 2165000ull, 30000u, 0.02f, false,  1u, 73185ull, 73185ull, 70110ull, true, 0u, false},
        // no reads
        {0u, 0ull, 0u, 0.005f, true,  1u, 4096ull, 4096ull, 65792ull, false, 0u, false},
    };
    for (const Row &w : rows) {
        const BlockRoute br = plan_block_route(w.n, w.n_bases, w.max_len, w.density, w.hpc, false, false, 0, true, STAGE_CAP);
        const RegionPlan rp = plan_regions(w.n, w.n_bases, w.max_len, w.density, w.hpc, SegTotals{}, SEG_G, SEG_TILE_BASES, PF_STAGE_CAP);
        CHECK(rp.n_regions == w.n_regions && rp.region_cap == w.region_cap && rp.capacity == w.capacity && rp.reserve == w.reserve,
              "n %u bases %llu: %u regions of %llu = %llu, reserve %llu", w.n, (unsigned long long)w.n_bases, rp.n_regions, (unsigned long long)rp.region_cap,
              (unsigned long long)rp.capacity, (unsigned long long)rp.reserve);
        CHECK(br.avg_fits_stage == w.avg_fits_stage && br.block_path_but_length == (w.n != 0), "n %u bases %llu hpc %d: avg_fits_stage %d", w.n, (unsigned long long)w.n_bases, (int)w.hpc,
              (int)br.avg_fits_stage);
        CHECK(rp.pf_len_limit == w.pf_len_limit && rp.pf_split == w.pf_split, "n %u bases %llu max %u: pf_len_limit %u split %d", w.n, (unsigned long long)w.n_bases, w.max_len,
              rp.pf_len_limit, (int)rp.pf_split);
        CHECK(rp.seg_rows == 0 && rp.seg_regions == 1 && rp.seg_region_cap == 4096, "no views, yet seg_rows %llu", (unsigned long long)rp.seg_rows);
    }
    // the views' side, in the benchmark's batch: {reads cut, views, tiles} -> seg_rows, seg_regions, seg_region_cap (and the reserve with them)
    struct Seg { uint64_t n_cut, n_views, n_tiles, seg_rows; uint32_t seg_regions; uint64_t seg_region_cap, reserve; };
    const Seg segs[] = {
        {0ull, 0ull, 0ull,  0ull, 1u, 4096ull, 8144416ull},
        {1ull, 1ull, 8ull,  4266ull, 1u, 8362ull, 8148682ull},
        {1000ull, 8191ull, 65528ull,  1400628ull, 1u, 1404724ull, 9545044ull},
        {1000ull, 8192ull, 65536ull,  1400799ull, 2u, 704495ull, 9545215ull},
        {100000ull, 1000000ull, 4500000ull,  123908094ull, 64u, 1940159ull, 132052510ull},
        {100000ull, 1000000ull, 5000000ull,  129004094ull, 64u, 2019784ull, 137148510ull},        // (more tiles than the batch has bases: capped)
    };
    for (const Seg &g : segs) {
        SegTotals t; t.n_cut = g.n_cut; t.n_views = g.n_views; t.n_tiles = g.n_tiles;
        const RegionPlan rp = plan_regions(1000000u, 10000000000ull, 10000u, 0.005f, true, t, SEG_G, SEG_TILE_BASES, PF_STAGE_CAP);
        CHECK(rp.seg_rows == g.seg_rows && rp.seg_regions == g.seg_regions && rp.seg_region_cap == g.seg_region_cap && rp.reserve == g.reserve,
              "%llu views: seg_rows %llu in %u regions of %llu, reserve %llu", (unsigned long long)g.n_views, (unsigned long long)rp.seg_rows, rp.seg_regions,
              (unsigned long long)rp.seg_region_cap, (unsigned long long)rp.reserve);
        CHECK(rp.n_regions == 64u && rp.capacity == 129262080ull, "the batch's own regions moved with its views");
    }
    // a view of the default segment length fits the pre-filtered stage at density 0.005f (27 142 bases), one of 32 768 bases does not
    CHECK(plan_regions(1000u, 100000000ull, 100000u, 0.005f, true, SegTotals{}, 16384u, SEG_TILE_BASES, PF_STAGE_CAP).seg_pf_limit == 27142u, "seg_pf_limit");
    CHECK(plan_regions(1000u, 100000000ull, 100000u, 0.005f, true, SegTotals{}, 32768u, SEG_TILE_BASES, PF_STAGE_CAP).seg_pf_limit == 0u, "seg_pf_limit");
    CHECK(plan_regions(1000u, 100000000ull, 100000u, 0.005f, false, SegTotals{}, 16384u, SEG_TILE_BASES, PF_STAGE_CAP).seg_pf_limit == 0u, "seg_pf_limit without hpc");
}

// the rules of the route, from their statement: masked reads are routed one by one while 8 of them are at most n + 128; the block path
// wants reads, a density below 0.2f, lengths below 2^31, and no side masks but routed ones
static void route_rules() {
    auto route = [](uint32_t n, uint32_t max_len, float density, bool has_n, bool listed, uint32_t n_masked, bool bump) {
        return plan_block_route(n, (uint64_t)n * 1000u, max_len, density, true, has_n, listed, n_masked, bump, STAGE_CAP);
    };
    CHECK(route(1000, 1000, 0.005f, true, true, 141, true).route_masked && route(1000, 1000, 0.005f, true, true, 141, true).block_path_but_length, "8 * 141 = 1128 <= 1128");
    CHECK(!route(1000, 1000, 0.005f, true, true, 142, true).route_masked && !route(1000, 1000, 0.005f, true, true, 142, true).block_path_but_length, "8 * 142 > 1128");
    CHECK(!route(1000, 1000, 0.005f, true, false, 1, true).route_masked, "no list of the masked reads");
    CHECK(!route(1000, 1000, 0.005f, false, true, 1, true).route_masked, "no side masks");
    CHECK(route(1000, 1000, 0.19f, false, false, 0, true).block_path_but_length && !route(1000, 1000, 0.2f, false, false, 0, true).block_path_but_length, "density 0.2f");
    CHECK(route(1000, 0x7FFFFFFFu, 0.005f, false, false, 0, true).block_path_but_length && !route(1000, 0x80000000u, 0.005f, false, false, 0, true).block_path_but_length, "2^31");
    CHECK(!route(1000, 1000, 0.005f, false, false, 0, false).block_path_but_length, "MDBG_SCAN_NO_BUMP");
    // segmentation: the GPU test's batch at the default setting does not want it (its average fits); "2" wants it for any read over a segment
    const BlockRoute fits = plan_block_route(200u, 2865000ull, 40000u, 0.02f, true, false, false, 0, true, STAGE_CAP);
    CHECK(!segments_wanted(fits, 1, 40000u, SEG_G, STAGE_CAP, true, T_002, 0), "automatic, average fits");
    CHECK(!segments_wanted(fits, 2, 40000u, SEG_G, STAGE_CAP, true, T_002, 0), "a segment itself would outgrow the stage: 16384 x 0.0224 + 24 = 391");
    const BlockRoute sparse = plan_block_route(200u, 2865000ull, 40000u, 0.005f, true, false, false, 0, true, STAGE_CAP);
    CHECK(segments_wanted(sparse, 2, 40000u, SEG_G, STAGE_CAP, true, T_0005, 0) && !segments_wanted(sparse, 2, SEG_G, SEG_G, STAGE_CAP, true, T_0005, 0), "every eligible read");
    CHECK(!segments_wanted(sparse, 1, 40000u, SEG_G, STAGE_CAP, true, T_0005, 0) && !segments_wanted(sparse, 0, 40000u, SEG_G, STAGE_CAP, true, T_0005, 0) &&
          !segments_wanted(sparse, 2, 40000u, SEG_G, STAGE_CAP, false, T_0005, 0) && !segments_wanted(sparse, 2, 40000u, SEG_G, STAGE_CAP, true, T_1, 0) &&
          !segments_wanted(sparse, 2, 40000u, SEG_G, STAGE_CAP, true, T_0005, 4273492457u), "automatic; never; MDBG_SCAN_NO_APPROX; density 1.0f; too wide a slack");
    const BlockRoute outgrows = plan_block_route(10u, 1000000ull, 100000u, 0.005f, true, false, false, 0, true, STAGE_CAP);
    CHECK(!outgrows.avg_fits_stage && segments_wanted(outgrows, 1, 100000u, SEG_G, STAGE_CAP, true, T_0005, 0), "automatic, average outgrows the stage");
}

static void candidate_test() {
    struct Row { uint64_t threshold; uint32_t slack; bool usable; };
    const Row rows[] = {
        {T_0005, 0u, true}, {T_0005, 1u << 15, true}, {T_02, 0u, true}, {T_02, 1u << 15, true}, {T_1, 0u, false}, {T_1, 1u << 15, false},
        {T_0005, 4273492456u, true}, {T_0005, 4273492457u, false},     // the largest slack that holds at 0.005f, the smallest that does not
    };
    for (const Row &w : rows) CHECK(candidate_test_usable(w.threshold, w.slack) == w.usable, "threshold %llx slack %u", (unsigned long long)w.threshold, w.slack);
}

static void grids() {
    struct Row { uint32_t n_items, option; unsigned blocks; };          // four waves a workgroup, 2 reads a wave unless the option says otherwise
    const Row rows[] = {{0u, 0u, 1u}, {1u, 0u, 1u}, {8u, 0u, 1u}, {9u, 0u, 2u}, {1000000u, 0u, 125000u}, {4294967295u, 0u, 536870912u},
                        {0u, 3u, 1u}, {9u, 3u, 1u}, {1000000u, 3u, 83334u}, {4294967295u, 3u, 357913942u}};
    for (const Row &w : rows) CHECK(scan_blocks(w.n_items, 4, w.option) == w.blocks, "%u items, option %u: %u blocks", w.n_items, w.option, scan_blocks(w.n_items, 4, w.option));
    struct Pf { uint32_t n_items; unsigned pf_waves; uint32_t option; int n_cu; unsigned per_wave; uint32_t chunk; unsigned blocks; };
    const Pf pfs[] = {
        {0u, 16u, 0u, 256, 2u, 32u, 1u}, {1000u, 16u, 0u, 256, 2u, 32u, 32u}, {16383u, 16u, 0u, 256, 2u, 32u, 512u}, {16384u, 16u, 0u, 256, 2u, 32u, 512u},
        {500000u, 16u, 0u, 256, 32u, 512u, 977u}, {10000000u, 16u, 0u, 256, 32u, 512u, 19532u}, {4294967295u, 16u, 0u, 256, 32u, 512u, 8388608u},
        {0u, 8u, 0u, 256, 2u, 16u, 1u}, {1000u, 8u, 0u, 256, 2u, 16u, 63u}, {16383u, 8u, 0u, 256, 2u, 16u, 1024u}, {16384u, 8u, 0u, 256, 4u, 32u, 512u},
        {500000u, 8u, 0u, 256, 32u, 256u, 1954u}, {10000000u, 8u, 0u, 256, 32u, 256u, 39063u}, {4294967295u, 8u, 0u, 256, 32u, 256u, 16777216u},
        {1000u, 16u, 64u, 256, 2u, 1024u, 1u}, {10000000u, 16u, 64u, 256, 32u, 1024u, 9766u}, {10000000u, 8u, 64u, 256, 32u, 512u, 19532u},
        {10000000u, 16u, 4294967295u, 256, 32u, 16777216u, 1u}, {4294967295u, 8u, 4294967295u, 256, 32u, 16777216u, 256u},      // (the chunk's cap, 2^24)
        {500000u, 16u, 0u, 0, 32u, 512u, 977u}, {500000u, 8u, 0u, 0, 32u, 256u, 1954u},                                         // (no CU count: as one)
    };
    for (const Pf &w : pfs) {
        const PrefilterGrid g = prefilter_grid(w.n_items, w.pf_waves, w.option, w.n_cu);
        CHECK(prefilter_reads_per_wave(w.n_cu, w.n_items, w.pf_waves) == w.per_wave && g.chunk == w.chunk && g.blocks == w.blocks,
              "%u items, %u waves, option %u: %u a wave, chunk %u, %u blocks", w.n_items, w.pf_waves, w.option, prefilter_reads_per_wave(w.n_cu, w.n_items, w.pf_waves), g.chunk, g.blocks);
    }
}

static void lds() {
    constexpr size_t TOTAL = 163840;
    unsigned long unbound = 0;
    for (size_t lds = 8192; lds <= 65536; lds += 512) {
        CHECK(scan_lds_padding(0, 0, 0, lds) == 0, "no reserve and no pad asked for, static %zu", lds);
        CHECK(scan_lds_padding(4096, 0, 0, lds) == 4096 && scan_lds_padding(4096, 65536, 0, lds) == 4096, "\"scan_lds_pad\" is taken as it is");
        for (size_t reserve = 0; reserve <= TOTAL; reserve += 256) {
            const size_t pad = scan_lds_padding(0, reserve, 0, lds);
            CHECK(pad % 256 == 0, "reserve %zu static %zu: pad %zu", reserve, lds, pad);
            CHECK(lds + pad <= 65536, "reserve %zu static %zu: pad %zu", reserve, lds, pad);
            CHECK(pad == scan_lds_padding(0, reserve, TOTAL, lds) || reserve == 0, "a CU's LDS given or left at its default");
            if (reserve == 0) continue;
            if (pad + 256 > 65536 - lds && pad != 0) continue;           // the 64 KB ceiling may have bound
            unbound++;
            const size_t fit = std::max<size_t>(2, (TOTAL - reserve) / lds), block = lds + pad;
            CHECK((fit + 1) * block > TOTAL && fit * block <= TOTAL, "reserve %zu static %zu: %zu blocks of %zu", reserve, lds, fit, block);
        }
    }
    CHECK(unbound > 640ul * 100ul, "property 3 was checked %lu times only", unbound);
    // a CU with more LDS than three 64 KB blocks: two blocks cannot be padded to keep a third out, the ceiling binds
    for (size_t lds = 8192; lds < 65536; lds += 512) {
        const size_t pad = scan_lds_padding(0, 250000, 262144, lds);
        CHECK(pad % 256 == 0 && lds + pad <= 65536 && lds + pad > 65536 - 256, "static %zu: pad %zu under the ceiling", lds, pad);
    }
    CHECK(scan_lds_padding(0, 4096, 0, 0) == 0, "static LDS unknown");
    // waves of the pre-filtered variant, at the three boundaries of the room beside the reserve (static LDS 100 000 and 60 000 bytes)
    const size_t lds16 = 100000, lds8 = 60000;
    CHECK(prefilter_wave_count(0, TOTAL - lds16, lds16, lds8) == 16 && prefilter_wave_count(0, 0, lds16, lds8) == 16, "16 waves fit");
    CHECK(prefilter_wave_count(0, TOTAL - lds16 + 1, lds16, lds8) == 8 && prefilter_wave_count(0, TOTAL - lds8, lds16, lds8) == 8, "8 waves fit");
    CHECK(prefilter_wave_count(0, TOTAL - lds8 + 1, lds16, lds8) == 0 && prefilter_wave_count(0, TOTAL, lds16, lds8) == 0 && prefilter_wave_count(0, TOTAL + 1, lds16, lds8) == 0, "none fits");
    CHECK(prefilter_wave_count(65536, 0, lds16, lds8) == 8 && prefilter_wave_count(lds16, 0, lds16, lds8) == 16, "a CU's LDS as given");
}

// the placement restated: both lists in one, sorted by read, a running sum from the first row
static void check_placement(const std::vector<uint32_t> &ol, const std::vector<uint32_t> &oc, const std::vector<uint32_t> &ml, const std::vector<uint32_t> &mc,
                            uint64_t capacity, uint64_t first_row, uint64_t reserve, bool fits) {
    const Placement pl = place_unfinished_reads(ol, oc, ml, mc, capacity, first_row, reserve);
    struct It { uint32_t read, cnt, kind; };
    std::vector<It> all;
    for (size_t i = 0; i < ol.size(); i++) all.push_back({ol[i], oc[i], 0});
    for (size_t i = 0; i < ml.size(); i++) all.push_back({ml[i], mc[i], 1});
    std::stable_sort(all.begin(), all.end(), [](const It &x, const It &y) { return x.read < y.read; });
    uint64_t at = first_row;
    size_t seen[2] = {0, 0};
    for (const It &it : all) {
        const size_t i = seen[it.kind]++;
        CHECK(i < pl.list[it.kind].size() && pl.list[it.kind][i] == it.read && pl.cnt[it.kind][i] == it.cnt && pl.start[it.kind][i] == at, "read %u of kind %u at row %llu", it.read,
              it.kind, (unsigned long long)at);
        at += it.cnt;
    }
    for (int k = 0; k < 2; k++) CHECK(pl.list[k].size() == seen[k] && pl.cnt[k].size() == seen[k] && pl.start[k].size() == seen[k], "kind %d: %zu placed", k, pl.list[k].size());
    CHECK(pl.rows == at - first_row && pl.fits == fits && fits == (at <= capacity + reserve), "%llu rows, fits %d", (unsigned long long)pl.rows, (int)pl.fits);
}

static void placement() {
    const std::vector<uint32_t> ol = {90, 4, 17, 55}, oc = {700, 400, 0, 1200}, ml = {5, 3, 60, 91}, mc = {10, 0, 33, 7};      // interleaved; counts of 0
    const uint64_t total = 700 + 400 + 1200 + 10 + 33 + 7;
    check_placement(ol, oc, ml, mc, 100000, 100000, total, true);             // exactly at the reserve
    check_placement(ol, oc, ml, mc, 100000, 100000, total - 1, false);        // one row over
    check_placement(ol, oc, ml, mc, 100000, 100500, total + 500, true);       // behind 500 joined rows, which take of the reserve too
    check_placement(ol, oc, ml, mc, 100000, 100500, total + 499, false);
    check_placement(ol, oc, {}, {}, 5000, 5000, 1ull << 40, true);            // an empty kind
    check_placement({}, {}, ml, mc, 5000, 5000, 50, true);
    check_placement({}, {}, ml, mc, 5000, 5000, 49, false);
    check_placement({}, {}, {}, {}, 5000, 5000, 0, true);
    check_placement({7}, {0xFFFFFFFFu}, {8}, {0xFFFFFFFFu}, 1ull << 33, 1ull << 33, 0x1FFFFFFFEull, true);       // rows are 64-bit
}

int main() {
    region_plan();
    route_rules();
    candidate_test();
    grids();
    lds();
    placement();
    for (uint32_t n : {0u, 3u, 200u}) {         // at most n / 4 + 16 overflowing reads are placed and re-run
        const uint32_t most = n / 4 + 16;
        CHECK(overflowing_reads_are_few(most, n) && !overflowing_reads_are_few(most + 1, n) && overflowing_reads_are_few(0, n), "n %u", n);
    }
    CHECK(overflowing_reads_are_few(66, 200) && !overflowing_reads_are_few(70, 200) && overflowing_reads_are_few(60, 200), "the GPU test's two cases");
    // long reads keep the split while they hold at most 1/32 of the bases
    CHECK(!long_reads_outweigh_split(0, 0) && !long_reads_outweigh_split(1, 32) && long_reads_outweigh_split(1, 31) && !long_reads_outweigh_split(312500000ull, 10000000000ull) &&
          long_reads_outweigh_split(312500001ull, 10000000000ull), "1/32 of the bases");
    printf("ok: %lu checks\n", n_checks);
    return 0;
}
