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

}  // namespace mdbg
