// The device header csrc/prefilter.hpp compiled for the host: the selected-key bitmap of the pre-filtered scan kernel, over EVERY
// 15-digit key.
//
//   * the keys a homopolymer-compressed read can produce as a canonical window (repeat-free, their own canonical form) are counted:
//     9 565 938 of the 19 131 876 repeat-free ones; 47 791 of them are selected at density 0.005f;
//   * the bitmap is built with the header's builder (prefilter_build_range, the function the device kernel calls) and every selected
//     key's bit must be set, at the kernel's geometry and at the shrunk test geometry -- no false negative is what the kernel's
//     exactness rests on;
//   * the false-positive rate over the possible keys that are NOT selected is printed (the pytest wrapper bounds it loosely).
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/prefilter.hpp"
#include <algorithm>
#include <cstdio>
#include <thread>
#include <vector>

// common.hpp's density_threshold (that header needs the HIP runtime): hash < T  <=>  (double)hash < (double)density * 2^64
static uint64_t density_threshold(float density) {
    const double bound = (double)density * 18446744073709551616.0;
    uint64_t lo = 0, hi = UINT64_MAX;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((double)mid >= bound) hi = mid; else lo = mid + 1;
    }
    return lo;
}

static bool repeat_free_plain(uint32_t v) {
    for (unsigned i = 0; i + 1 < 15; i++)
        if (((v >> (2 * i)) & 3u) == ((v >> (2 * i + 2)) & 3u)) return false;
    return true;
}

static uint32_t revcomp_plain(uint32_t v) {
    uint32_t r = 0;
    for (unsigned i = 0; i < 15; i++) r |= (((v >> (2 * i)) & 3u) ^ 2u) << (2 * (14 - i));
    return r;
}

struct Part {
    unsigned long long repeat_free = 0, possible = 0, selected = 0, helper_mismatches = 0;
    unsigned long long missing[2] = {0, 0}, false_pos[2] = {0, 0};
    std::vector<uint8_t> map[2];
};

static const unsigned LOG2[2] = {mdbg::PREFILTER_LOG2_BITS, mdbg::PREFILTER_MIN_LOG2_BITS};

static void build(unsigned t, unsigned nt, uint64_t threshold, Part *p) {
    for (int g = 0; g < 2; g++) {
        p->map[g].assign((1u << LOG2[g]) / 8u, 0);
        std::vector<uint8_t> &m = p->map[g];
        mdbg::prefilter_build_range(t, nt, threshold, LOG2[g], [&](uint32_t idx) { m[idx >> 3] |= (uint8_t)(1u << (idx & 7u)); });
    }
}

static void check(unsigned t, unsigned nt, uint64_t threshold, const std::vector<uint8_t> *maps, Part *p) {
    for (uint64_t v64 = t; v64 < mdbg::PREFILTER_KEYS; v64 += nt) {
        const uint32_t v = (uint32_t)v64;
        const bool rf = mdbg::prefilter_repeat_free(v);
        if ((v & 0xFFFu) == (t & 0xFFFu) || rf) {          // the bit tricks against the digit loops: every repeat-free key and a sample of the rest
            if (rf != repeat_free_plain(v) || mdbg::prefilter_revcomp(v) != revcomp_plain(v)) p->helper_mismatches++;
        }
        if (!rf) continue;
        p->repeat_free++;
        if (!mdbg::prefilter_key_possible(v)) continue;
        p->possible++;
        const bool sel = mdbg::kmer_hash32(v) < threshold;
        if (sel != mdbg::prefilter_key_selected(v, threshold)) p->helper_mismatches++;
        p->selected += sel;
        for (int g = 0; g < 2; g++) {
            const uint32_t idx = mdbg::prefilter_index(v, LOG2[g]);
            const bool bit = (maps[g][idx >> 3] >> (idx & 7u)) & 1u;
            if (sel && !bit) p->missing[g]++;
            if (!sel && bit) p->false_pos[g]++;
        }
    }
}

int main() {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 4u : std::min(nt, 16u);
    const uint64_t threshold = density_threshold(0.005f);
    std::vector<Part> parts(nt);
    {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++) th.emplace_back(build, t, nt, threshold, &parts[t]);
        for (auto &t : th) t.join();
    }
    std::vector<uint8_t> maps[2];
    unsigned long long set_bits[2] = {0, 0};
    for (int g = 0; g < 2; g++) {
        maps[g].assign((1u << LOG2[g]) / 8u, 0);
        for (auto &p : parts)
            for (size_t i = 0; i < maps[g].size(); i++) maps[g][i] |= p.map[g][i];
        for (uint8_t b : maps[g]) set_bits[g] += (unsigned)__builtin_popcount(b);
    }
    {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++) th.emplace_back(check, t, nt, threshold, maps, &parts[t]);
        for (auto &t : th) t.join();
    }
    Part s;
    for (auto &p : parts) {
        s.repeat_free += p.repeat_free; s.possible += p.possible; s.selected += p.selected; s.helper_mismatches += p.helper_mismatches;
        for (int g = 0; g < 2; g++) { s.missing[g] += p.missing[g]; s.false_pos[g] += p.false_pos[g]; }
    }
    printf("threshold %llu\n", (unsigned long long)threshold);
    printf("repeat-free %llu\ncanonical %llu\nselected %llu\nhelper mismatches %llu\n", s.repeat_free, s.possible, s.selected, s.helper_mismatches);
    for (int g = 0; g < 2; g++)
        printf("log2_bits %u set %llu missing %llu false-positive %llu of %llu rate %.6f\n", LOG2[g], set_bits[g], s.missing[g], s.false_pos[g],
               s.possible - s.selected, (double)s.false_pos[g] / (double)(s.possible - s.selected));
    return (s.helper_mismatches == 0 && s.missing[0] == 0 && s.missing[1] == 0) ? 0 : 1;
}
