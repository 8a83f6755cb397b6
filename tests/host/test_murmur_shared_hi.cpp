// The device header csrc/murmur.hpp compiled for the host: the candidate hash with the finalisers' upper half shared
// (kmer_hash32_hi_shared, kmer_hash32_hi_shared_x2) against kmer_hash32_hi_merged, for EVERY key v < 2^32.
//
//   * where the guard word passes (>= 68) the shared form must equal the merged form bit for bit;
//   * the keys whose guard word fails are listed, and for l = 13 .. 16 those below 4^l that have no two equal adjacent digits
//     among their l base-4 digits -- the only keys a homopolymer-compressed read can produce.  The scan kernel drops the guard
//     under compression at l = 15 on the strength of that list being empty (scan.hip, the GUARD tag).
//   * on a sample (every 64th key, and every failing key) both lanes of the x2 form, with and without the running minimum.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/murmur.hpp"
#include <algorithm>
#include <cstdio>
#include <thread>
#include <vector>

static bool repeat_free(uint32_t v, unsigned l) {
    for (unsigned i = 0; i + 1 < l; i++)
        if (((v >> (2 * i)) & 3u) == ((v >> (2 * i + 2)) & 3u)) return false;
    return true;
}

struct Part {
    unsigned long long mismatches = 0, x2_mismatches = 0, x2_checked = 0;
    std::vector<uint32_t> failing;
};

static void check_x2(uint32_t va, uint32_t vb, Part &p) {
    uint32_t ga, gb;
    (void)mdbg::kmer_hash32_hi_shared(va, ga);
    (void)mdbg::kmer_hash32_hi_shared(vb, gb);
    uint32_t ra, rb, g = 0xFFFFFFFFu, rn_a, rn_b, gn = 12345u;
    mdbg::kmer_hash32_hi_shared_x2<true>(va, vb, ra, rb, g);
    mdbg::kmer_hash32_hi_shared_x2<false>(va, vb, rn_a, rn_b, gn);
    p.x2_checked++;
    bool ok = g == std::min(ga, gb) && gn == 12345u && ra == rn_a && rb == rn_b;
    if (ga >= 68u && ra != mdbg::kmer_hash32_hi_merged(va)) ok = false;
    if (gb >= 68u && rb != mdbg::kmer_hash32_hi_merged(vb)) ok = false;
    // the running minimum only ever falls
    uint32_t g2 = 100u;
    mdbg::kmer_hash32_hi_shared_x2<true>(va, vb, ra, rb, g2);
    if (g2 != std::min(100u, std::min(ga, gb))) ok = false;
    if (!ok) p.x2_mismatches++;
}

static void run(uint64_t lo, uint64_t hi, Part *out) {
    Part p;
    for (uint64_t v64 = lo; v64 < hi; v64++) {
        const uint32_t v = (uint32_t)v64;
        uint32_t g;
        const uint32_t r = mdbg::kmer_hash32_hi_shared(v, g);
        if (g >= 68u) {
            if (r != mdbg::kmer_hash32_hi_merged(v)) p.mismatches++;
        } else {
            p.failing.push_back(v);
            check_x2(v, v * 2654435761u + 1u, p);
            check_x2(v ^ 0x5bd1e995u, v, p);
        }
        if ((v & 63u) == 0u) check_x2(v, (v * 2654435761u) ^ 0x9e3779b9u, p);
    }
    *out = p;
}

int main() {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 4u : std::min(nt, 16u);
    std::vector<Part> parts(nt);
    std::vector<std::thread> th;
    const uint64_t N = 1ull << 32;
    for (unsigned t = 0; t < nt; t++) th.emplace_back(run, N * t / nt, N * (t + 1) / nt, &parts[t]);
    for (auto &t : th) t.join();
    unsigned long long mism = 0, x2m = 0, x2n = 0;
    std::vector<uint32_t> failing;
    for (auto &p : parts) {
        mism += p.mismatches; x2m += p.x2_mismatches; x2n += p.x2_checked;
        failing.insert(failing.end(), p.failing.begin(), p.failing.end());
    }
    std::sort(failing.begin(), failing.end());
    printf("mismatches %llu\n", mism);
    printf("x2 checked %llu mismatches %llu\n", x2n, x2m);
    printf("failing %zu:", failing.size());
    for (uint32_t v : failing) printf(" %u", v);
    printf("\n");
    for (unsigned l = 13; l <= 16; l++) {
        std::vector<uint32_t> below, free_;
        for (uint32_t v : failing)
            if (l == 16 || v < (1u << (2 * l))) { below.push_back(v); if (repeat_free(v, l)) free_.push_back(v); }
        printf("l %u below %zu:", l, below.size());
        for (uint32_t v : below) printf(" %u", v);
        printf("\nl %u repeat-free %zu:", l, free_.size());
        for (uint32_t v : free_) printf(" %u", v);
        printf("\n");
    }
    return (mism == 0 && x2m == 0) ? 0 : 1;
}
