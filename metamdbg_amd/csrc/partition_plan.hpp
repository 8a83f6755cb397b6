// The plan of the first pass's radix split (partition.hip) as plain arithmetic: how a level's records are cut into the shares its blocks
// take, and how many blocks a level launches.  Numbers in, numbers out and no HIP, so that a stand-alone host program can check it
// (tests/host/test_partition_plan.cpp); the kernels call split_item and split_share on the device.
//
// A level splits n_seg segments independently.  A segment is cut into blocks_per_seg shares, each a multiple of the scatter's tile but
// for the segment's last; block seg * blocks_per_seg + j of the launch takes share j of segment seg, writes its own histogram column and
// takes its own `place` column.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MDBG_PLAN_FN __host__ __device__ inline
#else
#define MDBG_PLAN_FN inline
#endif

namespace mdbg {

constexpr uint32_t PART_LEVEL1_BLOCKS = 2048;          // level 1: at most this many shares of the one segment
constexpr uint32_t PART_DEEPER_BLOCKS = 4096;          // deeper levels: about this many blocks over all segments

// block -> (segment, share of it)
MDBG_PLAN_FN void split_item(uint32_t block, uint32_t blocks_per_seg, uint32_t &seg, uint32_t &j) {
    seg = block / blocks_per_seg; j = block % blocks_per_seg;
}

// share j of the segment [s0, s1): [b, e)
MDBG_PLAN_FN void split_share(uint64_t s0, uint64_t s1, uint32_t j, uint32_t blocks_per_seg, uint32_t tile, uint64_t &b, uint64_t &e) {
    const uint64_t len = s1 - s0;
    uint64_t per = (len + blocks_per_seg - 1) / blocks_per_seg;
    per = (per + tile - 1) / tile * tile;
    b = s0 + (uint64_t)j * per; if (b > s1) b = s1;
    e = b + per; if (e > s1) e = s1;
}

// level 1: one segment of n records (the flat minimizer positions), a share per tile up to PART_LEVEL1_BLOCKS.  n = 0 gives 0 (no
// block): the first pass never asks (part_applicable wants n >= k >= 1)
MDBG_PLAN_FN uint32_t level1_blocks_per_seg(uint64_t n, uint32_t tile) {
    const uint64_t tiles = (n + tile - 1) / tile;
    return (uint32_t)(tiles < PART_LEVEL1_BLOCKS ? tiles : PART_LEVEL1_BLOCKS);
}

// deeper levels: n records in n_seg segments of about equal length
MDBG_PLAN_FN uint32_t deeper_blocks_per_seg(uint64_t n, uint64_t n_seg, uint32_t tile) {
    const uint64_t avg_tiles = (n / n_seg + tile - 1) / tile;
    uint64_t room = PART_DEEPER_BLOCKS / n_seg; if (room < 1) room = 1;
    uint64_t v = room < avg_tiles ? room : avg_tiles; if (v < 1) v = 1;
    return (uint32_t)v;
}

// blocks of a level's launches
MDBG_PLAN_FN uint32_t level_grid(uint64_t n_seg, uint32_t blocks_per_seg) { return (uint32_t)(n_seg * blocks_per_seg); }

// ---- buckets and levels (host only) ---------------------------------------------------------------------------------------------
// more distinct keys than the buckets of one launch hold (one 512-thread workgroup per bucket, and a launch of 2^32 threads wraps): not
// for this path -- 2^22 buckets of 2048 slots are 6.7 G keys per key group, more than the 2^32 minimizers a call takes
constexpr uint32_t PART_MAX_BITS = 22;

// the least n <= cap with 2^n >= b
inline uint32_t bits_to_hold(double b, uint32_t cap) {
    uint32_t n = 0;
    while ((double)(1ull << n) < b && n < cap) n++;
    return n;
}

// Bucket bits so that a bucket's distinct keys fit its LDS table of `slots`.  The first pass sizes for the estimated distinct keys of one
// key group; the owner of a sharded pass for its ROWS (a key arrives once from every rank that saw it, so this is generous), and stops one
// past PART_MAX_BITS, which is its "too many".
// (a mean load of up to 0.78: the fullest of 65 536 buckets is then near 0.9, where an LDS probe sequence is still a dozen slots -- and
// one radix level less is worth more than short probes: at 6 x coverage, 46 M keys in 172 M instances, 0.70 asked for a third level)
inline uint32_t first_pass_bits(double keys_est, uint64_t n_groups, uint32_t slots) { return bits_to_hold(keys_est / (double)n_groups / (0.78 * slots), 40); }
inline uint32_t owner_bits(uint64_t n_recv, uint32_t slots) { return bits_to_hold((double)n_recv / (0.78 * slots), PART_MAX_BITS + 1); }

inline uint32_t levels_for(uint32_t bits) { return bits <= 8 ? 1u : (bits + 7u) / 8u; }

// the key groups of a first pass: the fewest (a power of two, at most 2^16) whose instances fit the record budget
inline uint32_t group_bits_for(uint64_t inst_est, uint64_t max_records) {
    uint32_t group_bits = 0;
    while (((inst_est + ((1ull << group_bits) - 1)) >> group_bits) > max_records && group_bits < 16) group_bits++;
    return group_bits;
}

// How the bucket bits are shared between the levels -- two policies, and which is the faster for the owner nobody has measured:
//   LEVEL1_BY_MIX  the first pass: level 1 splits the flat positions by window_mix and takes 8 bits whenever there are that many (so
//                  the sketch rarely changes it and the histogram is not run twice); the deeper levels share the rest evenly, by the
//                  bits of hash_lo below the key group's
//   ALL_BY_HASH    the owner of a sharded pass: its rows carry hash_lo already, every level shares the bits evenly, from the top
enum class LevelShare { LEVEL1_BY_MIX, ALL_BY_HASH };

struct LevelPlan { uint32_t bits, shift, ways; uint64_t n_seg; };

struct BucketPlan {
    uint32_t lds_slots = 0, bucket_bits = 0, n_levels = 1;
    LevelPlan lv[3] = {};
    bool too_many_buckets() const { return bucket_bits > PART_MAX_BITS; }
};

// lv[l] of every level (the first three of a plan that has too many buckets to run)
inline void plan_levels(BucketPlan &p, uint32_t group_bits, LevelShare share) {
    p.n_levels = levels_for(p.bucket_bits);
    uint32_t left = p.bucket_bits, used = share == LevelShare::LEVEL1_BY_MIX ? group_bits : 0u;
    uint64_t segs = 1;
    for (uint32_t l = 0; l < p.n_levels && l < 3; l++) {
        const bool by_mix = l == 0 && share == LevelShare::LEVEL1_BY_MIX;
        const uint32_t b = by_mix ? (left < 8u ? left : 8u) : (left + (p.n_levels - l) - 1) / (p.n_levels - l);
        p.lv[l].bits = b; p.lv[l].ways = 1u << b; p.lv[l].n_seg = segs;
        p.lv[l].shift = (by_mix || used + b == 0) ? 0u : 64u - used - b;      // (one way: the digit is masked to 0 whatever the shift)
        if (!by_mix) used += b;
        left -= b; segs <<= b;
    }
}

// The first pass.  keys_est: distinct keys of all groups; extra_bits: what earlier attempts added after a bucket outgrew its table;
// forced_slots, forced_bits: "partition_lds_slots", "partition_bits" (0: planned here).
inline BucketPlan first_pass_plan(double keys_est, uint64_t n_groups, uint32_t group_bits, uint32_t extra_bits, uint32_t forced_slots, uint32_t forced_bits) {
    BucketPlan p;
    const uint32_t b1024 = first_pass_bits(keys_est, n_groups, 1024) + extra_bits, b2048 = first_pass_bits(keys_est, n_groups, 2048) + extra_bits;
    // (1024 slots where they need no level more than 2048 would: four buckets instead of two per CU count a fifth faster)
    p.lds_slots = forced_slots ? forced_slots : (levels_for(b1024) <= levels_for(b2048) && b1024 <= PART_MAX_BITS ? 1024u : 2048u);
    p.bucket_bits = (forced_bits ? forced_bits : first_pass_bits(keys_est, n_groups, p.lds_slots)) + extra_bits;
    // level 1 takes 8 bits whenever there are that many, the deeper levels share the rest
    plan_levels(p, group_bits, LevelShare::LEVEL1_BY_MIX);
    return p;
}

// The owner's side of a sharded pass over n_recv rows; forced_slots: "partition_lds_slots" (256 and 2048 are taken, anything else is 1024).
// too_many_buckets(): no levels are planned, the one-table form takes the rows.
inline BucketPlan owner_plan(uint64_t n_recv, uint32_t forced_slots) {
    BucketPlan p;
    p.lds_slots = forced_slots == 256 || forced_slots == 2048 ? forced_slots : 1024u;
    p.bucket_bits = owner_bits(n_recv, p.lds_slots);
    if (!p.too_many_buckets()) plan_levels(p, 0, LevelShare::ALL_BY_HASH);
    return p;
}

}  // namespace mdbg
