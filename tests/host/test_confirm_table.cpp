// The device header csrc/prefilter.hpp compiled for the host: the selected-key TABLE the pre-filtered scan kernel takes its candidates'
// verdicts from, built with the header's builder (the functions the device kernels call) and checked over EVERY 15-digit key.
//
// Per (density, log2 buckets) case:
//   * every possible key's look-up is prefilter_key_selected or ASK, and ASK comes from buckets whose state says so only;
//   * builder and probe agree on hash, bucket and tag for every key (the bucket and tag of a key rebuild its hash when the geometry
//     has 2^16 buckets);
//   * a bucket without keys answers NO for every possible key, whatever its (zero) tag slots hold, and the repeated tags of a partly
//     filled bucket are tags of its own keys: an empty slot never matches a key that is not selected;
//   * the occupancy histogram and the number of overflowed buckets are printed (the pytest wrapper asserts them).
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/prefilter.hpp"
#include <algorithm>
#include <atomic>
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

// 0x9E3779B1^-1 mod 2^32 (Newton's iteration doubles the correct low bits: 3 -> 6 -> 12 -> 24 -> 48)
static uint32_t inverse32(uint32_t a) { uint32_t x = a; for (int i = 0; i < 4; i++) x *= 2u - a * x; return x; }
static const uint32_t MULT_INVERSE = inverse32(0x9E3779B1u);

// the builder's read-modify-write, as the device's atomics (the program's threads share the table)
struct AtomicOps {
    uint32_t add(uint32_t *p, uint32_t v) const { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
    uint32_t orr(uint32_t *p, uint32_t v) const { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
};

struct Sums {
    unsigned long long possible = 0, selected = 0, yes = 0, ask = 0, wrong = 0, ask_unmarked = 0, index_mismatch = 0, empty_hit = 0, filler_bad = 0;
};

template <class F>
static void parallel(unsigned nt, F f) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back(f, t);
    for (auto &t : th) t.join();
}

static bool run_case(float density, unsigned log2_buckets, unsigned nt, bool expect_no_overflow) {
    const uint64_t threshold = density_threshold(density);
    const size_t nb = (size_t)1 << log2_buckets;
    std::vector<uint32_t> table(nb * mdbg::CONFIRM_BUCKET_WORDS, 0u), counts(nb, 0u);
    parallel(nt, [&](unsigned t) { mdbg::confirm_table_insert_range(t, nt, threshold, log2_buckets, table.data(), counts.data(), AtomicOps()); });
    unsigned long long overflowed = 0, hist[17] = {0};
    unsigned max_count = 0;
    for (size_t b = 0; b < nb; b++) {
        overflowed += mdbg::confirm_table_finish_bucket(&table[b * mdbg::CONFIRM_BUCKET_WORDS], counts[b]);
        hist[std::min(counts[b], 16u)]++;
        max_count = std::max(max_count, counts[b]);
    }
    const unsigned long long overflowed_by_count = overflowed;
    if (mdbg::confirm_table_needs_verify(log2_buckets)) {
        std::atomic<unsigned long long> marked{0};
        parallel(nt, [&](unsigned t) { mdbg::confirm_table_verify_range(t, nt, threshold, log2_buckets, table.data(), AtomicOps(), [&]() { marked++; }); });
        overflowed += marked.load();
    }
    // the tags a bucket stores, listed from the keys themselves: what the repeated tags of a partly filled bucket must come from
    std::vector<Sums> parts(nt);
    parallel(nt, [&](unsigned t) {
        Sums &s = parts[t];
        for (uint64_t v64 = t; v64 < mdbg::PREFILTER_KEYS; v64 += nt) {
            const uint32_t v = (uint32_t)v64;
            const uint32_t h = mdbg::confirm_hash(v), b = mdbg::confirm_bucket(h, log2_buckets), tag = mdbg::confirm_tag(h);
            // builder and probe index: one multiply, top bits, low bits; with 2^16 buckets they rebuild h, and h rebuilds v
            if (h != v * 0x9E3779B1u || b != (uint32_t)(((uint64_t)h) >> (32u - log2_buckets)) || tag != (h & 0xFFFFu) || b >= nb) s.index_mismatch++;
            if (log2_buckets == 16u && (((b << 16) | tag) != h || (uint32_t)(h * MULT_INVERSE) != v)) s.index_mismatch++;
            if (!mdbg::prefilter_key_possible(v)) continue;
            s.possible++;
            const bool sel = mdbg::prefilter_key_selected(v, threshold);
            s.selected += sel;
            const uint32_t *w = &table[(size_t)b * mdbg::CONFIRM_BUCKET_WORDS];
            const uint32_t state = w[3] >> 16;
            const uint32_t a = mdbg::confirm_lookup(table.data(), log2_buckets, v);
            if (a == mdbg::CONFIRM_ASK) {
                s.ask++;
                if (!(state & mdbg::CONFIRM_OVERFLOW)) s.ask_unmarked++;
            } else {
                if (state & mdbg::CONFIRM_OVERFLOW) s.ask_unmarked++;      // a marked bucket must answer ASK
                if ((a == mdbg::CONFIRM_YES) != sel) s.wrong++;
                s.yes += a == mdbg::CONFIRM_YES;
            }
            if (counts[b] == 0u) {          // a bucket without keys: zero words, NO whatever the tag
                if (w[0] | w[1] | w[2] | w[3]) s.filler_bad++;
                if (a != mdbg::CONFIRM_NO) s.empty_hit++;
            }
        }
    });
    // every stored slot of a valid bucket is the tag of a selected key of that bucket (the repeats included)
    unsigned long long filler_bad = 0;
    {
        std::vector<std::vector<uint16_t>> tags(nb);
        for (uint64_t v = 0; v < mdbg::PREFILTER_KEYS; v++) {
            if (!mdbg::prefilter_repeat_free((uint32_t)v)) continue;
            if (!mdbg::prefilter_key_selected((uint32_t)v, threshold)) continue;
            const uint32_t h = mdbg::confirm_hash((uint32_t)v);
            tags[mdbg::confirm_bucket(h, log2_buckets)].push_back((uint16_t)mdbg::confirm_tag(h));
        }
        for (size_t b = 0; b < nb; b++) {
            const uint32_t *w = &table[b * mdbg::CONFIRM_BUCKET_WORDS];
            if (tags[b].size() != counts[b]) filler_bad++;
            if (!((w[3] >> 16) & mdbg::CONFIRM_VALID)) continue;
            for (unsigned s = 0; s < mdbg::CONFIRM_SLOTS; s++) {
                const uint16_t t = (uint16_t)(w[s >> 1] >> (16u * (s & 1u)));
                if (std::find(tags[b].begin(), tags[b].end(), t) == tags[b].end()) filler_bad++;
            }
            for (uint16_t t : tags[b])          // and every key's tag is there
                if (mdbg::confirm_verdict(w[0], w[1], w[2], (w[3] & 0xFFFFu) | (mdbg::CONFIRM_VALID << 16), t) != mdbg::CONFIRM_YES) filler_bad++;
        }
    }
    Sums s;
    for (auto &p : parts) {
        s.possible += p.possible; s.selected += p.selected; s.yes += p.yes; s.ask += p.ask; s.wrong += p.wrong; s.ask_unmarked += p.ask_unmarked;
        s.index_mismatch += p.index_mismatch; s.empty_hit += p.empty_hit; s.filler_bad += p.filler_bad;
    }
    s.filler_bad += filler_bad;
    printf("case density %g log2_buckets %u threshold %llu\n", (double)density, log2_buckets, (unsigned long long)threshold);
    printf("  possible %llu selected %llu\n", s.possible, s.selected);
    printf("  occupancy");
    for (unsigned c = 0; c <= 16; c++) if (hist[c]) printf(" %u%s:%llu", c, c == 16 ? "+" : "", hist[c]);
    printf(" max %u\n", max_count);
    printf("  overflowed %llu (by count %llu)\n", overflowed, overflowed_by_count);
    printf("  answers yes %llu ask %llu wrong %llu ask-mismatch %llu index-mismatch %llu empty-hit %llu filler-bad %llu\n", s.yes, s.ask, s.wrong,
           s.ask_unmarked, s.index_mismatch, s.empty_hit, s.filler_bad);
    bool ok = s.wrong == 0 && s.ask_unmarked == 0 && s.index_mismatch == 0 && s.empty_hit == 0 && s.filler_bad == 0;
    if (expect_no_overflow && (overflowed != 0 || s.ask != 0 || s.yes != s.selected)) ok = false;
    printf("  %s\n", ok ? "ok" : "FAILED");
    return ok;
}

int main() {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 4u : std::min(nt, 16u);
    bool ok = true;
    ok &= run_case(0.005f, mdbg::CONFIRM_LOG2_BUCKETS, nt, true);
    ok &= run_case(0.01f, mdbg::CONFIRM_LOG2_BUCKETS, nt, false);
    ok &= run_case(0.005f, 13u, nt, false);          // a test geometry in which verdicts and ASK mix
    ok &= run_case(0.005f, mdbg::CONFIRM_MIN_LOG2_BUCKETS, nt, false);
    return ok ? 0 : 1;
}
