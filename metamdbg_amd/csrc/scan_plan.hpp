// The host's plan of a scan (scan.hip: mdbg_scan, launch_scan) as plain arithmetic: which path a batch takes, how its output is cut into
// regions, how many workgroups, how much LDS padding.  Numbers in, numbers out and no HIP, so that a stand-alone host program can check
// it (tests/host/test_scan_plan.cpp).  The kernels' capacities (STAGE_CAP, PF_STAGE_CAP, ...) stay with the kernels and come in as arguments.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mdbg {

// The candidate test (the upper half of the hash against a 32-bit limit) can be used for this threshold and slack
// (not when the candidate limit would saturate -- a threshold within a few 2^32 of 2^64, density 1.0f: the full verdict then)
inline bool candidate_test_usable(uint64_t threshold, uint32_t cand_slack) { return (threshold >> 32) + 3ull + (uint64_t)cand_slack < 0xFFFFFFFFull; }

// ---- which path.  The block-structured kernels write every read's rows once, where a wave found room; batches they cannot take go
// through the general path.
// A read may stage `stage_cap` minimizers; the few that select more are re-run by the general kernel into a reserve behind
// the regions.  Batches whose AVERAGE read is expected to outgrow the stage go straight to the general path.
// A batch in which a few reads carry side-mask bits (an N here and there, soft-masked stretches) stays on this path: the block
// kernel skips those reads (ScanArgs::skip) and they alone are counted, placed and scanned by the general kernel.
struct BlockRoute {
    bool route_masked, block_path_but_length, avg_fits_stage;
    double rows_per_base;
};
inline BlockRoute plan_block_route(uint32_t n, uint64_t n_bases, uint32_t max_len, float density, bool hpc, bool has_n, bool masked_listed, uint32_t n_masked,
                                   bool bump_allowed, int stage_cap) {
    BlockRoute r;
    r.route_masked = has_n && masked_listed && (uint64_t)n_masked * 8ull <= (uint64_t)n + 128ull;
    r.block_path_but_length = n && (!has_n || r.route_masked) && bump_allowed && density < 0.2f && max_len < (1u << 31);
    r.rows_per_base = (double)density * (hpc ? 0.8 : 1.0) * 1.4;
    r.avg_fits_stage = n && (double)n_bases / (double)n * r.rows_per_base + 24.0 < (double)stage_cap;
    return r;
}

// "scan_segments": the plain reads of more than one segment are cut into views (segments_dev.hpp) -- 1: in a batch that would leave
// this path for its reads' length alone, and which stays if any read can be cut; 2: there and in every batch that takes this path.  Views are
// scanned by the candidate-hash kernels (as reads in bump mode are, but for MDBG_SCAN_NO_APPROX and thresholds near 2^64)
inline bool segments_wanted(const BlockRoute &r, uint32_t scan_segments, uint32_t max_len, uint32_t seg_G, int stage_cap, bool approx_allowed, uint64_t threshold,
                            uint32_t cand_slack) {
    const bool wanted = scan_segments == 2u || (scan_segments == 1u && !r.avg_fits_stage);        // (2 includes what 1 does)
    return r.block_path_but_length && wanted && max_len > seg_G && (double)seg_G * r.rows_per_base + 24.0 < (double)stage_cap && approx_allowed &&
           candidate_test_usable(threshold, cand_slack);
}

// ---- the block path's output: regions, the views' regions, the reserve behind them, and what the pre-filtered variant may take
struct SegTotals { uint64_t n_cut = 0, n_views = 0, n_tiles = 0; };       // reads cut; views and tiles of the reads long enough to be (those of unsegmentable reads are dead)
struct RegionPlan {
    uint32_t n_regions, seg_regions, pf_len_limit, seg_pf_limit;
    uint64_t region_cap, capacity, seg_rows, seg_region_cap, reserve;
    double pf_limit_bases;
    bool pf_split;
};
inline uint32_t region_count(uint64_t items) {
    uint32_t regions = 1;
    while (regions < 64u && (uint64_t)regions * 8192ull <= items) regions <<= 1;
    return regions;
}
inline RegionPlan plan_regions(uint32_t n, uint64_t n_bases, uint32_t max_len, float density, bool hpc, const SegTotals &seg, uint32_t seg_G, uint32_t seg_tile_bases,
                               int pf_stage_cap) {
    RegionPlan r;
    // the output arrays are cut into regions, each with its own cursor (reads are dealt to the waves round-robin, so the regions
    // fill evenly); small batches use one
    r.n_regions = region_count(n);
    r.region_cap = ((uint64_t)((double)n_bases * (double)density * 1.3) + 64ull * n) / r.n_regions + 4096ull;
    r.capacity = r.region_cap * r.n_regions;
    // views write their rows to arrays of their own, cut into regions like the batch's; the join copies them behind the batch's regions,
    // in front of the reads that outgrow a stage.  (The batch's regions above are still sized from all its bases, the cut reads' included,
    // which no longer write there: a batch of contigs holds about three times the rows it needs -- 10 bytes a row, 0.0065 rows a base.)
    const uint64_t seg_bases = std::min<uint64_t>(seg.n_tiles * seg_tile_bases, n_bases);
    r.seg_rows = seg.n_cut ? (uint64_t)((double)seg_bases * (double)density * 1.3) + 64ull * seg.n_views + 4096ull : 0ull;
    r.seg_regions = region_count(seg.n_views);
    r.seg_region_cap = r.seg_rows / r.seg_regions + 4096ull;
    r.reserve = r.capacity / 16 + 65536 + r.seg_rows;       // rows behind the regions for reads that outgrow the stage (and the joined reads)
    // The pre-filtered variant stages pf_stage_cap rows a read, under half of the four-wave kernels'.  A read is expected to fit it below pf_len_limit
    // bases (the expectation above against that stage: 27 kb at density 0.005f).  The variant is taken when the AVERAGE read is below that;
    // a few longer reads in such a batch are scanned by the four-wave kernel in a launch of its own (launch_scan), so that a tail of
    // long reads neither keeps the batch from the variant nor is left to the general kernel
    r.pf_limit_bases = ((double)pf_stage_cap - 24.0) / ((double)density * 0.8 * 1.4);
    r.pf_len_limit = hpc && (double)n_bases / (double)n < r.pf_limit_bases ? (uint32_t)std::min(r.pf_limit_bases, 4294967295.0) : 0u;
    r.pf_split = r.pf_len_limit && max_len >= r.pf_len_limit;
    r.seg_pf_limit = hpc && (double)seg_G < r.pf_limit_bases ? (uint32_t)std::min(r.pf_limit_bases, 4294967295.0) : 0u;
    return r;
}

// Reads too long for the variant's stage: when they hold at most 1/32 of the batch's bases the four-wave kernel scans them in a launch
// of its own (every other read flagged in its `skip`), the variant the rest.  That launch is sparse -- most waves of a block idle -- so
// a batch with many long reads loses more there than the variant gains (measured: profiles/prefilter_varied_lengths.txt) and keeps
// the four-wave kernel for all its reads.
inline bool long_reads_outweigh_split(uint64_t long_bases, uint64_t batch_bases) { return long_bases * 32ull > batch_bases; }

// the host places and re-runs the reads that outgrew the stage only while they are few; a batch with more takes the general path
inline bool overflowing_reads_are_few(uint32_t n_over, uint32_t n) { return n_over <= n / 4 + 16; }

// ---- grids
// "scan_reads_per_wave" left at 0: what a wave takes before its workgroup retires.  The four-wave and the general kernels keep 2 (see
// scan_blocks).  A workgroup of the pre-filtered variant copies the 64 KB bitmap, clears its rings and passes two barriers before its
// first read, with nothing else of the scan on its CU meanwhile: at 2 reads a wave that is paid 312 500 times for 10 M reads.  Measured
// (profiles/split_residency_reads_per_wave.txt), 10 M x 10 kb alone: 71.1 / 67.7 / 65.3 / 64.6 / 63.7 / 64.0 / 65.4 ms at 2 / 4 / 8 / 16 /
// 32 / 64 / 128; 500 000 reads of 1 .. 25 kb: 3.94 / 3.27 / 3.00 / 2.85 / 2.79 / 2.74 / 2.71 ms.  With two batches in flight the step
// gains more than the scan alone and keeps gaining up to 128 -- but from 64 on because the other batch's first pass is held back (its
// kernels' time follows the life of a scan workgroup, DESIGN.md 4.4: 27 / 41 / 57 / 66 ms of first pass a step at 16 / 32 / 64 / 128 under a
// scan launch of 82 / 80 / 78 / 77 ms), and a first pass as long as a scan launch is what the pipeline would wait for next.  32 is the
// largest value at which it stays at half a launch.  The batch must also leave every CU PREFILTER_MIN_GROUPS_PER_CU workgroups (the 500 000
// reads above are 1.9 a CU at 64): a small batch would otherwise leave CUs idle for the length of a workgroup.
constexpr unsigned SCAN_READS_PER_WAVE = 2, PREFILTER_READS_PER_WAVE = 32, PREFILTER_MIN_GROUPS_PER_CU = 2;

inline unsigned prefilter_reads_per_wave(int n_cu, uint32_t n_items, unsigned waves) {
    unsigned per_wave = PREFILTER_READS_PER_WAVE;
    const uint64_t want = (uint64_t)PREFILTER_MIN_GROUPS_PER_CU * (uint64_t)std::max(n_cu, 1);
    while (per_wave > SCAN_READS_PER_WAVE && (uint64_t)n_items / ((uint64_t)waves * per_wave) < want) per_wave /= 2;
    return per_wave;
}

// Workgroups of the four-wave and of the general kernel, of `waves` waves.  A few reads per wave, then the wave retires.  One resident
// generation of persistent waves (the first design)
// took 17.9 ms for 1 M x 10 kb reads although every wave had the same work: CUs do not all run at the same
// speed, and the kernel ended with the slowest.  Dealt out by the dispatcher as slots free up, the same reads take
// 15.4 ms; short-lived workgroups also let the kernels of another stream (a second batch in flight, RCCL) in
// instead of queueing them behind the resident generation.  The per-block set-up (1024-entry LUT) is noise next
// to a 10 kb read.  2 reads per wave measured best with two batches in flight: a waiting kernel of the other batch gets
// a slot within ~0.2 ms (MDBG_SCAN_READS_PER_WAVE to tune).
inline unsigned scan_blocks(uint32_t n_items, int waves, uint32_t reads_per_wave_option) {
    const uint64_t per_wave = reads_per_wave_option ? reads_per_wave_option : SCAN_READS_PER_WAVE;
    uint64_t blocks = ((uint64_t)n_items + waves * per_wave - 1) / (waves * per_wave);
    if (blocks < 1) blocks = 1;
    if (blocks > 0x7FFFFFFFull) blocks = 0x7FFFFFFFull;
    return (unsigned)blocks;
}
// the pre-filtered variant: a workgroup of pf_waves waves deals its chunk of reads out to its waves
struct PrefilterGrid { uint32_t chunk; unsigned blocks; };
inline PrefilterGrid prefilter_grid(uint32_t n_items, unsigned pf_waves, uint32_t reads_per_wave_option, int n_cu) {
    const uint64_t chunk = std::min<uint64_t>((uint64_t)pf_waves * (reads_per_wave_option ? reads_per_wave_option : prefilter_reads_per_wave(n_cu, n_items, pf_waves)), 1u << 24);
    const uint64_t blocks = std::min<uint64_t>(std::max<uint64_t>(1, ((uint64_t)n_items + chunk - 1) / chunk), 0x7FFFFFFFull);
    return PrefilterGrid{(uint32_t)chunk, (unsigned)blocks};
}

// ---- the pre-filtered variant's PERSISTENT launch ("scan_persistent"): as many workgroups as fit the device at once -- one per CU --
// and none pending behind them.  Every wave draws runs of R consecutive items from one 64-bit counter in device memory (a returning
// add of R; the kernel repeats this arithmetic) until it draws a start at or behind n_items.  No workgroup waits for another: whatever
// subset of the grid is resident, the counter hands every item out exactly once and a workgroup that starts late finds it used up.
// R ("scan_grab_reads"; 0 = this default): one address takes about 88 returning adds a microsecond (the cursors' price, ScanArgs::cursor);
// 10 M reads in 62 ms would be 161 / 80 / 40 / 20 adds a microsecond at R = 1 / 2 / 4 / 8.  Measured alone (profiles/scan_persistent_lone_scan.txt),
// 10 M x 10 kb: 121.2 / 61.6 / 61.05 / 60.95 / 61.0 ms at R = 1 / 2 / 4 / 8 / 16 against 62.9 ms chunked -- at R = 1 the launch runs at the
// counter's rate, 83 adds a microsecond; 500 000 reads of 1 .. 25 kb: 6.09 / 3.11 / 2.57 / 2.62 / 2.72 ms against 2.74 chunked -- a long run
// leaves the end of a launch to the wave that drew it.  4 is the smallest R within a run's spread (0.1 ms) of the best on the first and the best on the second.
constexpr unsigned PERSISTENT_GRAB_READS = 4, PERSISTENT_GRAB_MAX = 1u << 16;
inline unsigned persistent_grab(uint32_t grab_option) { return grab_option ? std::min<uint32_t>(grab_option, PERSISTENT_GRAB_MAX) : PERSISTENT_GRAB_READS; }
// an explicit "scan_reads_per_wave" asks for the chunked form by name and gets it, whatever "scan_persistent" says
inline bool persistent_taken(uint32_t persistent_option, uint32_t reads_per_wave_option) { return persistent_option && !reads_per_wave_option; }
// workgroups: min(n_cu, ceil(n_items / (waves * R))), at least 1; blocks_cap > 0 ("scan_persistent_blocks", tests) caps them further
inline unsigned persistent_grid(uint32_t n_items, unsigned waves, unsigned grab, int n_cu, uint32_t blocks_cap) {
    const uint64_t per_group = (uint64_t)waves * grab;
    uint64_t blocks = std::min<uint64_t>(((uint64_t)n_items + per_group - 1) / per_group, (uint64_t)std::max(n_cu, 1));
    if (blocks_cap) blocks = std::min<uint64_t>(blocks, blocks_cap);
    return (unsigned)std::max<uint64_t>(blocks, 1);
}
// the run a wave holds after drawing `start` (the counter's value before its add): [start, end), empty when the counter is used up
inline uint32_t persistent_run_end(uint64_t start, unsigned grab, uint32_t n_items) {
    return start >= n_items ? (uint32_t)n_items : (uint32_t)std::min<uint64_t>(start + grab, n_items);
}
// Rows to regions: by the item's run, not by the wave that drew it -- consecutive runs go to consecutive regions, so the fill is even
// within one run a region whichever workgroups got onto a CU and when
inline uint32_t persistent_region(uint32_t item, unsigned grab, uint32_t n_regions) { return (item / grab) & (n_regions - 1u); }

// ---- LDS (lds_per_cu 0: not known, a CU of gfx950 has 160 KB)
inline size_t lds_of_a_cu(size_t lds_per_cu) { return lds_per_cu ? lds_per_cu : 163840u; }
// the pre-filtered variant takes as many waves a workgroup as leave "scan_lds_reserve" free: 16, else 8, else none
inline unsigned prefilter_wave_count(size_t lds_per_cu, size_t reserve, size_t lds16, size_t lds8) {
    const size_t total = lds_of_a_cu(lds_per_cu);
    const size_t room = total > reserve ? total - reserve : 0;
    return lds16 <= room ? 16u : lds8 <= room ? 8u : 0u;
}
// Unused dynamic LDS caps the four-wave kernel's blocks per CU (mdbg_set_option): "scan_lds_pad" gives the bytes as they are;
// "scan_lds_reserve" says how much of a CU's LDS the kernel is to LEAVE to other contexts' kernels, whatever the variant
// (30 KB a block for FASTA with homopolymer compression, 36.5 KB for FASTQ): as many blocks as fit beside the reserve, and
// enough padding that one more does not.  (lds: the kernel's static LDS; 0 where it was not or could not be asked: no padding of ours.)
inline unsigned scan_lds_padding(unsigned pad_option, size_t reserve, size_t lds_per_cu, size_t lds) {
    unsigned lds_pad = pad_option;
    if (lds_pad || !reserve || !lds) return lds_pad;
    const size_t total = lds_of_a_cu(lds_per_cu);
    size_t fit = total > reserve ? (total - reserve) / lds : 1;
    // never fewer than two blocks per CU: one block would have to be padded to more than half a CU's LDS -- beyond the 64 KB
    // a block may ask for, the launch would fail with hipErrorInvalidValue instead of capping anything (round-4 ADVICE);
    // a reserve that large is answered with the two-block form (and whatever LDS that leaves)
    if (fit < 2) fit = 2;
    const size_t need = total / (fit + 1) + 1;          // a block of this size: fit + 1 of them are more than a CU has
    if (need > lds) lds_pad = (unsigned)(((need - lds) + 255u) / 256u * 256u);
    const size_t most = (size_t)65536 > lds ? (size_t)65536 - lds : 0;        // static + dynamic LDS of a block stay within 64 KB
    if (lds_pad > most) lds_pad = (unsigned)(most / 256u * 256u);
    return lds_pad;
}

// ---- reads the block kernel did not finish: those that outgrew its stage (kind 0; long reads, listed with their exact counts) and
// those it skipped for their side masks (kind 1).  Both kinds are placed in read order behind the regions, from first_row on, each
// kind in lists of its own for the variant of the general kernel that scans it.
struct Placement {
    std::vector<uint32_t> list[2], cnt[2];
    std::vector<uint64_t> start[2];
    uint64_t rows;       // of the placed reads
    bool fits;           // first_row + rows is within the reserve behind `capacity`
};
inline Placement place_unfinished_reads(const std::vector<uint32_t> &over_list, const std::vector<uint32_t> &over_cnt, const std::vector<uint32_t> &masked_list,
                                        const std::vector<uint32_t> &masked_cnt, uint64_t capacity, uint64_t first_row, uint64_t reserve) {
    // one order over both kinds: (read, count, kind)
    struct Item { uint32_t read, cnt, kind; };
    std::vector<Item> items;
    items.reserve(over_list.size() + masked_list.size());
    for (size_t i = 0; i < over_list.size(); i++) items.push_back(Item{over_list[i], over_cnt[i], 0u});
    for (size_t i = 0; i < masked_list.size(); i++) items.push_back(Item{masked_list[i], masked_cnt[i], 1u});
    std::sort(items.begin(), items.end(), [](const Item &x, const Item &y) { return x.read < y.read; });
    Placement pl;
    uint64_t at = first_row;
    for (const Item &it : items) { pl.list[it.kind].push_back(it.read); pl.cnt[it.kind].push_back(it.cnt); pl.start[it.kind].push_back(at); at += it.cnt; }
    pl.rows = at - first_row;
    pl.fits = at - capacity <= reserve;
    return pl;
}

}  // namespace mdbg
