// The device header csrc/spans_dev.hpp compiled for the host.
//   1. spans_select_flag over every shape of flag word: empty, one flag at each of the 32 bases, all 32, flags only in the bottom or
//      only in the top half, the partial last word of a read, seeded random words -- against a bit-by-bit walk.
//   2. The flag words and the coordinate map rle[j] of seeded reads, built by a serial copy of the kernels' lanes (spans_tile_runs_kernel,
//      spans_read_sums_kernel) and queried through spans_rle at EVERY j in 0 .. L', against EncoderRLE::execute's rule restated over the
//      characters (Commons.hpp:4163-4203): runs across word, 64-word and tile borders, a run of 5000, a read that is one run, lengths
//      1 .. 70 and around the tile, N runs, "aA", IUPAC letters that share a code, an N next to a G.  The side masks are derived from the
//      characters the way pack_ascii_kernel derives them.
//   3. spans_compose against MDBG::getKminmers' arithmetic (Commons.hpp:5401-5526) for forward, reversed and tie windows, k = 2 .. 6
//      (k = 2: the second minimizer is the last), over seeded strictly increasing spans.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/spans_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

using namespace mdbg;

static unsigned long n_words_checked = 0, n_shapes = 0, n_reads = 0, n_queries = 0, n_windows = 0, n_ties = 0, n_empty_words = 0, n_empty_tiles = 0;

static bool fail(const char *what, long a0 = 0, long a1 = 0, long a2 = 0) {
    printf("FAILED: %s: %ld %ld %ld\n", what, a0, a1, a2);
    return false;
}

// ---- 1. select ---------------------------------------------------------------------------------------------------------------------
static bool check_word(uint64_t d, const char *shape) {
    if (d & ~SPANS_EVEN) return fail("a flag word with an odd bit", (long)d);
    uint32_t j = 0;
    for (uint32_t base = 0; base < 32; base++) {
        if (!((d >> (2 * base)) & 1ull)) continue;
        const uint32_t got = spans_select_flag(d, j);
        if (got != base) { printf("%s: ", shape); return fail("select", (long)j, (long)got, (long)base); }
        j++;
    }
    if (j != spans_count_flags(d)) return fail("count", (long)j, (long)spans_count_flags(d));
    n_words_checked++;
    return true;
}

static bool check_select() {
    bool ok = check_word(0ull, "empty");
    for (uint32_t b = 0; b < 32 && ok; b++) ok = check_word(1ull << (2 * b), "one flag");
    ok = ok && check_word(SPANS_EVEN, "all 32");
    ok = ok && check_word(SPANS_EVEN & 0xFFFFFFFFull, "bottom half");
    ok = ok && check_word(SPANS_EVEN & ~0xFFFFFFFFull, "top half");
    for (uint32_t nv = 1; nv < 32 && ok; nv++) ok = check_word(SPANS_EVEN & ((1ull << (2 * nv)) - 1ull), "partial last word");
    n_shapes = 6;
    std::mt19937_64 rng(7);
    for (int i = 0; i < 200000 && ok; i++) {
        uint64_t d = rng() & SPANS_EVEN;
        if (i % 3 == 1) d &= rng();                // sparse
        if (i % 3 == 2) d |= rng() & SPANS_EVEN;   // dense
        if (i % 7 == 0) d &= 0xFFFFFFFFull;
        if (i % 11 == 0) d &= ~0xFFFFFFFFull;
        ok = check_word(d, "random");
    }
    n_shapes++;
    // spread: bit i -> bit 2i
    for (int i = 0; i < 1000 && ok; i++) {
        const uint32_t v = (uint32_t)rng();
        uint64_t want = 0;
        for (int b = 0; b < 32; b++) want |= (uint64_t)((v >> b) & 1u) << (2 * b);
        if (spans_spread(v) != want) ok = fail("spread", (long)v);
    }
    return ok;
}

// ---- 2. the map --------------------------------------------------------------------------------------------------------------------
struct Packed {
    std::vector<uint64_t> words;
    std::vector<uint32_t> inv, brk;
    bool any_inv = false, any_brk = false;
};

static Packed pack(const std::string &s) {
    const size_t L = s.size(), nw = (L + 31) / 32;
    Packed p;
    p.words.assign(nw, 0); p.inv.assign(nw, 0); p.brk.assign(nw, 0);
    for (size_t i = 0; i < L; i++) {
        const uint8_t c = (uint8_t)s[i];
        p.words[i / 32] |= (uint64_t)((c >> 1) & 3u) << (2 * (i % 32));
        if ((c >> 3) & 1u) { p.inv[i / 32] |= 1u << (i % 32); p.any_inv = true; }
        if (i && c != (uint8_t)s[i - 1] && ((c ^ (uint8_t)s[i - 1]) & 0x0Eu) == 0) { p.brk[i / 32] |= 1u << (i % 32); p.any_brk = true; }
    }
    return p;
}

// with_masks: hand the side masks over although the read has no bit in them (a plain read inside a batch that carries masks)
static bool check_read(const std::string &s, bool with_masks, const char *what) {
    const uint32_t L = (uint32_t)s.size();
    // the reference's rule over the characters: rle[] of EncoderRLE::execute
    std::vector<uint32_t> rle;
    for (uint32_t i = 0; i < L; i++) if (i == 0 || s[i] != s[i - 1]) rle.push_back(i);
    const uint32_t C = (uint32_t)rle.size();
    rle.push_back(L);
    const Packed p = pack(s);
    const bool masks = with_masks || p.any_inv || p.any_brk;
    const uint32_t *inv = masks ? p.inv.data() : nullptr, *brk = (with_masks || p.any_brk) ? p.brk.data() : nullptr;
    const uint32_t nwords = (L + 31) / 32, nT = (L + SPANS_TILE_BASES - 1) / SPANS_TILE_BASES;
    // a serial copy of the kernels' lanes
    std::vector<uint32_t> tile_excl(nT ? nT : 1, 0);
    std::vector<uint16_t> word_excl((size_t)(nT ? nT : 1) * SPANS_TILE_WORDS, 0);
    uint32_t carry = 0;
    for (uint32_t t = 0; t < nT; t++) {
        uint32_t inc = 0;
        for (uint32_t lane = 0; lane < SPANS_TILE_WORDS; lane++) {
            const uint32_t wi = t * SPANS_TILE_WORDS + lane;
            uint32_t c = 0;
            if (wi < nwords) {
                const uint64_t d = spans_read_word_flags(p.words.data(), inv, brk, L, wi);
                c = spans_count_flags(d);
                // the flags themselves against the characters
                for (uint32_t b = 0; b < 32; b++) {
                    const uint32_t i = wi * 32 + b;
                    const bool want = i < L && (i == 0 || s[i] != s[i - 1]);
                    if ((((d >> (2 * b)) & 1ull) != 0) != want) { printf("%s (L %u): ", what, L); return fail("flag", (long)i, (long)want); }
                }
                if (d & ~SPANS_EVEN) return fail("odd bit in a read's flag word", (long)wi);
                if (c == 0) n_empty_words++;
            }
            word_excl[(size_t)t * SPANS_TILE_WORDS + lane] = (uint16_t)inc;
            inc += c;
        }
        tile_excl[t] = carry;
        if (inc == 0) n_empty_tiles++;
        carry += inc;
    }
    if (carry != C) { printf("%s (L %u): ", what, L); return fail("compressed length", (long)carry, (long)C); }
    const SpansReadMap m{p.words.data(), inv, brk, L, carry, nT, tile_excl.data(), word_excl.data()};
    for (uint32_t j = 0; j <= C; j++) {
        const uint32_t got = spans_rle(m, j);
        if (got != rle[j]) { printf("%s (L %u, L' %u): ", what, L, C); return fail("rle", (long)j, (long)got, (long)rle[j]); }
        n_queries++;
    }
    n_reads++;
    return true;
}

static std::string random_read(std::mt19937_64 &rng, uint32_t L, int flavour) {
    static const char plain[] = "ACGT", iupac[] = "ACGTNacgtnRYKMSWBDHVrykm";
    std::string s;
    while (s.size() < L) {
        const char c = flavour == 0 ? plain[rng() % 4] : iupac[rng() % (sizeof(iupac) - 1)];
        uint32_t run = 1;
        const uint32_t dice = (uint32_t)(rng() % 100);
        if (dice < 30) run = 2 + (uint32_t)(rng() % 4);
        else if (dice < 33) run = 20 + (uint32_t)(rng() % 80);
        else if (dice < 34 && flavour != 2) run = 1000 + (uint32_t)(rng() % 1500);
        s.append(run, c);
    }
    s.resize(L);
    return s;
}

static bool check_map() {
    std::mt19937_64 rng(11);
    bool ok = true;
    for (uint32_t L = 1; L <= 70 && ok; L++)
        for (int f = 0; f < 3 && ok; f++) ok = check_read(random_read(rng, L, f), f == 1, "short");
    for (uint32_t L : {127u, 128u, 129u, 2047u, 2048u, 2049u, 2080u, 4095u, 4096u, 4097u, 6000u, 10000u})
        for (int f = 0; f < 3 && ok; f++) ok = check_read(random_read(rng, L, f), f == 2, "around the tile");
    for (int i = 0; i < 1000 && ok; i++) ok = check_read(random_read(rng, 1 + (uint32_t)(rng() % 9000), i % 3), i % 5 == 0, "random");
    // one run: L' = 1
    for (uint32_t L : {1u, 31u, 32u, 33u, 2048u, 5000u}) ok = ok && check_read(std::string(L, 'A'), false, "one run") && check_read(std::string(L, 'N'), false, "one run of N");
    // runs across a word border, a 64-word border (= the tile border, base 2048) and ending exactly on a word border
    for (uint32_t at : {30u, 31u, 32u, 62u, 2040u, 2046u, 2047u, 2048u, 4090u})
        for (uint32_t run : {2u, 3u, 5u, 40u, 70u, 5000u}) {
            if (!ok) break;
            std::string s = random_read(rng, at, 2);
            if (!s.empty() && s.back() == 'G') s.back() = 'T';
            s += std::string(run, 'G') + random_read(rng, 100, 2);
            if (s[at + run] == 'G') s[at + run] = 'C';
            ok = check_read(s, false, "a run across a border");
            std::string e = s.substr(0, at + run);                     // the read ends with the run
            ok = ok && check_read(e, false, "a run at the end");
        }
    for (uint32_t end : {32u, 64u, 2048u, 4096u}) {                    // the last run ends exactly on a word border
        std::string s = random_read(rng, end - 7, 2);
        if (s.back() == 'A') s.back() = 'C';
        ok = ok && check_read(s + std::string(7, 'A'), false, "last run ends on a word border");
    }
    // characters: N next to G (same code), N runs, "aA", letters that share a code (C and S and c: code 1 ...), across a word border too
    for (const char *unit : {"GN", "NG", "GNNNG", "aA", "AaAa", "CSc", "RrR", "TtNnGg", "ACGTNNNNNNNNNNacgtRYKM"}) {
        for (uint32_t shift = 0; shift < 40 && ok; shift += 3) {
            std::string s = random_read(rng, shift, 0);
            for (int rep = 0; rep < 12; rep++) s += unit;
            ok = check_read(s, false, unit);
        }
    }
    return ok;
}

// ---- 3. the composition --------------------------------------------------------------------------------------------------------------
static bool check_compose() {
    std::mt19937_64 rng(13);
    for (int round = 0; round < 20000; round++) {
        const uint32_t k = 2 + (uint32_t)(rng() % 5), n = k + (uint32_t)(rng() % 6);
        // spans of n minimizers: S strictly increasing, E strictly increasing, S < E
        std::vector<uint32_t> S(n), E(n), m(n);
        uint32_t at = (uint32_t)(rng() % 50);
        for (uint32_t i = 0; i < n; i++) { S[i] = at; at += 1 + (uint32_t)(rng() % 30); }
        for (uint32_t i = 0; i < n; i++) E[i] = S[i] + 13 + (i ? E[i - 1] - S[i - 1] - 13 : 0) / 2 + (uint32_t)(rng() % 9);
        for (uint32_t i = 1; i < n; i++) if (E[i] <= E[i - 1]) E[i] = E[i - 1] + 1;
        for (uint32_t i = 0; i < n; i++) m[i] = (uint32_t)(rng() % 5);          // few values: ties and palindromes occur
        for (uint32_t i = 0; i + k <= n; i++) {
            // KmerVec::normalize's flag: the vector against its reverse, a tie reverses
            bool reversed = true, tie = true;
            for (uint32_t a = 0; a < k; a++) {
                if (m[i + a] == m[i + k - 1 - a]) continue;
                reversed = m[i + a] > m[i + k - 1 - a];
                tie = false;
                break;
            }
            if (tie) n_ties++;
            // getKminmers: first, second, last but one, last
            const uint32_t i1 = i, i2 = i + 1, ib = i + k - 2, il = i + k - 1;
            const uint32_t read_pos_start = S[i1], read_pos_end = S[il] + (E[il] - S[il]);
            const uint32_t want_start = reversed ? read_pos_end - E[ib] : S[i2] - read_pos_start;
            const uint32_t want_end = reversed ? S[i2] - read_pos_start : read_pos_end - E[ib];
            const SpanFields f = spans_compose(S[i1], S[i2], E[ib], E[il], reversed);
            if (f.pos_start != read_pos_start || f.pos_end != read_pos_end || f.seq_length_start != want_start || f.seq_length_end != want_end)
                return fail("compose", (long)k, (long)i, (long)reversed);
            if (k == 2 && (i2 != il || i1 != ib)) return fail("k = 2 indices");
            n_windows++;
        }
    }
    return true;
}

int main() {
    if (!check_select() || !check_map() || !check_compose()) return 1;
    printf("ok: %lu flag words in %lu shapes, %lu reads, %lu queries, %lu empty words, %lu empty tiles, %lu windows, %lu ties\n", n_words_checked, n_shapes,
           n_reads, n_queries, n_empty_words, n_empty_tiles, n_windows, n_ties);
    return 0;
}
