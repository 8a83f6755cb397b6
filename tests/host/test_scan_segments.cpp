// The device header csrc/segments_dev.hpp compiled for the host: per-tile run-start counts, the compressed offsets c_s of the
// segments, the windows a view owns and the verdict "unsegmentable", against a direct, character-by-character homopolymer
// compression of seeded reads -- random bases, run-free reads, homopolymers placed at, before and across every cut (every length
// 1 .. 40, then 100, 1000, the lengths around a tile less l run starts 2020 / 2032 - 2035, around one tile 2047 - 2049, 2100, around
// two tiles 4095 - 4097, and 5000), lengths 2048 m + {-1, 0, 1}.  The owned ranges of a read's views must partition [0, C).
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/segments_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace mdbg;

static unsigned long n_reads = 0, n_views = 0, n_unsegmentable = 0, n_cut_in_run = 0;

static std::vector<uint64_t> pack(const std::vector<uint8_t> &b) {
    std::vector<uint64_t> w((b.size() + 31) / 32 + 2, 0);       // (reads are padded; a word behind the last is never read)
    for (size_t i = 0; i < b.size(); i++) w[i / 32] |= (uint64_t)(b[i] & 3u) << (2 * (i % 32));
    return w;
}

// one read, one segment length, one l: everything the header says against the direct compression
static bool check(const std::vector<uint8_t> &b, uint32_t G, uint32_t K, bool hpc, const char *what) {
    const uint32_t L = (uint32_t)b.size();
    const std::vector<uint64_t> w = pack(b);
    // direct: start[i] = base i starts a run; before[i] = run starts among [0, i)
    std::vector<uint32_t> before(L + 1, 0);
    for (uint32_t i = 0; i < L; i++) before[i + 1] = before[i] + ((!hpc || i == 0 || b[i] != b[i - 1]) ? 1u : 0u);
    const uint32_t C = before[L];
    auto fail = [&](const char *why, long a0, long a1, long a2) {
        printf("%s (L %u, G %u, l %u, hpc %d): %s: %ld %ld %ld\n", what, L, G, K, (int)hpc, why, a0, a1, a2);
        return false;
    };
    const uint32_t nT = seg_tiles(L), nS = seg_count(L, G);
    std::vector<uint32_t> runs(nT), excl(nT + 1, 0);
    for (uint32_t t = 0; t < nT; t++) {
        const uint32_t lo = t * SEG_TILE_BASES, hi = lo + SEG_TILE_BASES < L ? lo + SEG_TILE_BASES : L;
        runs[t] = hpc ? seg_tile_run_starts(w.data(), L, t) : hi - lo;
        if (runs[t] != before[hi] - before[lo]) return fail("run starts of a tile", t, runs[t], before[hi] - before[lo]);
        excl[t + 1] = excl[t] + runs[t];
    }
    if (excl[nT] != C) return fail("compressed length", excl[nT], C, 0);
    if (nS < 2) return true;
    n_reads++;
    bool ok_header = true, ok_direct = true;
    for (uint32_t s = 1; s < nS; s++) {
        const uint32_t cut = s * G, hi = cut + SEG_TILE_BASES < L ? cut + SEG_TILE_BASES : L;
        ok_header = ok_header && seg_cut_ok(L, cut, runs[cut / SEG_TILE_BASES], K);
        ok_direct = ok_direct && (hi == L || before[hi] - before[cut] >= K);
        if (hpc && b[cut] == b[cut - 1]) n_cut_in_run++;
    }
    if (ok_header != ok_direct) return fail("the verdict on the cuts", ok_header, ok_direct, 0);
    if (!ok_header) n_unsegmentable++;
    uint32_t next_owned = 0;
    for (uint32_t s = 0; s < nS; s++) {
        const uint32_t c_s = seg_offset(hpc ? excl.data() : nullptr, s, nS, L, G, C), c_n = seg_offset(hpc ? excl.data() : nullptr, s + 1, nS, L, G, C);
        if (c_s != before[s * G]) return fail("c_s", s, c_s, before[s * G]);
        if (c_n != (s + 1 < nS ? before[(s + 1) * G] : C)) return fail("c_{s+1}", s, c_n, 0);
        const SegView v = seg_view_make(7, s, nS, L, G, c_s, c_n, ok_header);
        n_views++;
        if (v.read != 7 || v.tile0 * SEG_TILE_BASES != s * G || v.c_s != c_s) return fail("view start", s, v.tile0, v.c_s);
        if (v.c_s != next_owned) return fail("owned ranges leave a gap or overlap", s, v.c_s, next_owned);
        next_owned = v.c_s + v.n_own;
        const uint32_t raw0 = s * G, raw1 = raw0 + v.raw_len;
        if (raw1 > L || v.raw_len == 0) return fail("view end", s, raw1, L);
        if (((v.flags & SEG_FIRST) != 0) != (s == 0) || ((v.flags & SEG_LAST) != 0) != (s + 1 == nS) ||
            ((v.flags & SEG_DEAD) != 0) != !ok_header)
            return fail("view flags", s, v.flags, 0);
        if ((v.flags & SEG_LAST) && raw1 != L) return fail("the last view ends the read", s, raw1, L);
        if (!(v.flags & SEG_LAST) && raw1 != ((s + 1) * G + SEG_TILE_BASES < L ? (s + 1) * G + SEG_TILE_BASES : L)) return fail("halo of one tile", s, raw1, 0);
        // what the cut rule is for: a live view that does not reach the read's end sees, behind its last owned window, the l bases of
        // the window AND the run start behind it -- n_own + l run starts in all
        if (ok_header && raw1 != L && before[raw1] - before[raw0] < v.n_own + K) return fail("halo too short for the last owned window", s, before[raw1] - before[raw0], v.n_own + K);
    }
    if (next_owned != C) return fail("owned ranges do not end at C", next_owned, C, 0);
    return true;
}

static bool check_all(const std::vector<uint8_t> &b, const char *what) {
    for (uint32_t G : {2048u, 4096u, 16384u})
        for (uint32_t K : {15u, 13u})
            for (bool hpc : {true, false})
                if (!check(b, G, K, hpc, what)) return false;
    return true;
}

int main() {
    std::mt19937_64 rng(20261019);
    auto random_read = [&](uint32_t L) { std::vector<uint8_t> b(L); for (auto &c : b) c = (uint8_t)(rng() & 3u); return b; };
    auto run_free = [&](uint32_t L) { std::vector<uint8_t> b(L); uint8_t p = (uint8_t)(rng() & 3u); for (auto &c : b) { p = (uint8_t)((p + 1u + rng() % 3u) & 3u); c = p; } return b; };
    // the word-level primitive at every prefix length
    for (int i = 0; i < 2000; i++) {
        const uint64_t x = rng() & rng();      // (runs are common)
        const uint32_t prev = (uint32_t)(rng() & 3u);
        for (uint32_t nv = 0; nv <= 32; nv++) {
            uint32_t direct = 0, p = prev;
            for (uint32_t k = 0; k < nv; k++) { const uint32_t c = (uint32_t)(x >> (2 * k)) & 3u; direct += c != p; p = c; }
            if (seg_word_run_starts(x, prev, nv) != direct) { printf("word %016llx prev %u nvalid %u: %u, direct %u\n", (unsigned long long)x, prev, nv, seg_word_run_starts(x, prev, nv), direct); return 1; }
        }
    }
    // lengths 2048 m + {-1, 0, 1}, random and run-free
    for (uint32_t m = 1; m <= 9; m++)
        for (int d = -1; d <= 1; d++) {
            if (!check_all(random_read(2048 * m + d), "random")) return 1;
            if (!check_all(run_free(2048 * m + d), "run-free")) return 1;
        }
    for (uint32_t L : {40000u, 70001u}) if (!check_all(random_read(L), "random, long")) return 1;
    // homopolymers of 1 .. 40 bases and of chosen lengths up to 5000 at, before and across every cut of a read of 5 tiles and a bit
    std::vector<uint32_t> hp_len;
    for (uint32_t h = 1; h <= 40; h++) hp_len.push_back(h);
    for (uint32_t h : {100u, 1000u, 2020u, 2032u, 2033u, 2034u, 2035u, 2047u, 2048u, 2049u, 2100u, 4095u, 4096u, 4097u, 5000u}) hp_len.push_back(h);
    const uint32_t L0 = 5 * 2048 + 777;
    for (uint32_t h : hp_len)
        for (uint32_t cut = 2048; cut < L0; cut += 2048)
            for (int place = 0; place < 5; place++) {
                // the run starts at the cut, ends on it, ends one base in front of it, straddles it by 3 bases, straddles it in the middle
                long at = place == 0 ? (long)cut : place == 1 ? (long)cut - (long)h : place == 2 ? (long)cut - (long)h - 1 : place == 3 ? (long)cut - 3 : (long)cut - (long)h / 2;
                if (at < 1 || at + (long)h > (long)L0) continue;
                std::vector<uint8_t> b = run_free(L0);
                const uint8_t c = (uint8_t)((b[at - 1] + 1u) & 3u);          // another base than the one in front of the run
                for (uint32_t k = 0; k < h; k++) b[at + k] = c;
                if (!check_all(b, "homopolymer")) return 1;
            }
    if (n_unsegmentable == 0 || n_unsegmentable == n_reads || n_cut_in_run == 0) { printf("both verdicts and cuts inside runs must occur: %lu of %lu, %lu\n", n_unsegmentable, n_reads, n_cut_in_run); return 1; }
    printf("ok: %lu reads, %lu views, %lu unsegmentable, %lu cuts inside a run\n", n_reads, n_views, n_unsegmentable, n_cut_in_run);
    return 0;
}
