// The device header csrc/complexity_dev.hpp compiled for the host: the +-1 (Walsh-Hadamard) form of a word's 2-mer square sum
// against a direct count, and the per-read SUSPECT decision in the new form (sum weight Q > 816 nW) against the form it replaces
// (sum weight sq > 332 nW), on whole synthetic reads -- among them reads steered onto the threshold itself.
//
//     sq(w) = sum over the 16 2-mers v of count(v)^2 over the 32 positions of word w (the last completed by the next word's
//             first base)  =  64 + word_pair_q(w) / 4
//
// sq is a sum of 16 squares whose bases sum to 32, so it is even, and so is every weighted sum of them: the nearest a read can
// come to the threshold 332 nW (even) is the threshold itself and 2 to either side, which is what the steered reads land on.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/complexity_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static unsigned base_of(uint64_t x, unsigned i) { return (unsigned)(x >> (2 * i)) & 3u; }

// direct count: the 16 2-mers over the 32 slots of x, the last one completed by base 0 of the next word
static uint32_t sq_direct(uint64_t x, uint64_t next) {
    uint32_t c[16] = {0};
    for (unsigned i = 0; i < 32; i++) {
        const unsigned b0 = base_of(x, i), b1 = i < 31 ? base_of(x, i + 1) : base_of(next, 0);
        c[b0 * 4 + b1]++;
    }
    uint32_t s = 0;
    for (unsigned v = 0; v < 16; v++) s += c[v] * c[v];
    return s;
}

static unsigned long n_words = 0;
static bool check_word(uint64_t x, uint64_t next, const char *what) {
    const uint32_t sq = sq_direct(x, next), q = mdbg::word_pair_q(x, (uint32_t)next);
    n_words++;
    if (q % 4u != 0u || 64u + q / 4u != sq || q > mdbg::CX_Q_MAX) {
        printf("%s: word %016llx next %016llx: direct %u, header 64 + %u / 4\n", what, (unsigned long long)x, (unsigned long long)next, sq, q);
        return false;
    }
    return true;
}

// codes: A 0, C 1, T 2, G 3 (bits 1-2 of the ASCII character)
static unsigned gc_base(std::mt19937_64 &g, double gc) {
    const double u = (double)(g() >> 11) / 9007199254740992.0;
    if (u < gc) return (g() & 1u) ? 1u : 3u;
    return (g() & 1u) ? 0u : 2u;
}

struct Read {
    std::vector<uint64_t> w;
    uint32_t len;
    unsigned get(uint32_t i) const { return base_of(w[i / 32], i % 32); }
    void set(uint32_t i, unsigned b) { w[i / 32] = (w[i / 32] & ~(3ull << (2 * (i % 32)))) | ((uint64_t)b << (2 * (i % 32))); }
};
static Read make_read(uint32_t len) { Read r; r.len = len; r.w.assign((len + 31) / 32 + 1, 0ull); return r; }

// both forms of the read's sum, over the words the kernels weigh (0 .. nW, each complete and followed by a base)
static void read_sums(const Read &r, uint64_t &sum_sq, uint64_t &sum_q) {
    const uint32_t nW = mdbg::complexity_windows(r.len);
    sum_sq = 0; sum_q = 0;
    uint64_t weights = 0;
    for (uint32_t w = 0; (uint64_t)(w + 1) * 32u + 1u <= r.len; w++) {
        const uint32_t wt = mdbg::complexity_word_weight(w, nW);
        weights += wt;
        sum_sq += (uint64_t)wt * sq_direct(r.w[w], r.w[w + 1]);
        sum_q += (uint64_t)wt * mdbg::word_pair_q(r.w[w], (uint32_t)r.w[w + 1]);
    }
    if (weights != 2ull * nW) { printf("weights of a read of %u bases sum to %llu, not 2 x %u\n", r.len, (unsigned long long)weights, nW); exit(1); }
}

static unsigned long n_reads = 0, n_suspect = 0;
static bool check_read(const Read &r, const char *what) {
    const uint32_t nW = mdbg::complexity_windows(r.len);
    uint64_t ssq, sq_;
    read_sums(r, ssq, sq_);
    const bool old_form = ssq > (uint64_t)mdbg::CX_SQ_LIMIT_PER_WINDOW * nW, new_form = nW ? mdbg::complexity_suspect(sq_, nW) : false;
    n_reads++; n_suspect += new_form;
    if ((nW ? old_form : false) != new_form || (ssq & 1u)) {
        printf("%s: read of %u bases (%u windows): sum sq %llu against %llu, sum Q %llu against %llu\n", what, r.len, nW, (unsigned long long)ssq,
               332ull * nW, (unsigned long long)sq_, 816ull * nW);
        return false;
    }
    return true;
}

int main(int argc, char **argv) {
    const unsigned long n_random = argc > 1 ? strtoul(argv[1], nullptr, 10) : 450000ul;
    std::mt19937_64 g(20240917);
    // ---- words ----
    for (unsigned long i = 0; i < n_random; i++) if (!check_word(g(), g(), "uniform")) return 1;
    for (unsigned long i = 0; i < n_random; i++) {
        uint64_t x = 0, nx = 0;
        for (unsigned b = 0; b < 32; b++) { x |= (uint64_t)gc_base(g, 0.30) << (2 * b); nx |= (uint64_t)gc_base(g, 0.30) << (2 * b); }
        if (!check_word(x, nx, "30 % GC")) return 1;
    }
    for (unsigned c = 0; c < 4; c++)                                   // homopolymers, every successor
        for (unsigned nb = 0; nb < 4; nb++) if (!check_word(0x5555555555555555ull * c, nb, "homopolymer")) return 1;
    for (unsigned p = 2; p <= 6; p++)                                   // every unit of period 2 .. 6, every phase, the period kept or broken at the seam
        for (unsigned unit = 0; unit < (1u << (2 * p)); unit++)
            for (unsigned phase = 0; phase < p; phase++) {
                uint64_t x = 0;
                for (unsigned b = 0; b < 32; b++) x |= (uint64_t)((unit >> (2 * ((b + phase) % p))) & 3u) << (2 * b);
                const uint64_t cont = (unit >> (2 * ((32 + phase) % p))) & 3u;
                for (unsigned nb = 0; nb < 4; nb++) if (!check_word(x, nb, "period")) return 1;
                if (!check_word(x, cont | (g() << 2), "period, continued")) return 1;
            }
    for (unsigned i = 0; i < 32; i++)                                   // every single-base change of an all-A word
        for (unsigned b = 1; b < 4; b++)
            for (unsigned nb = 0; nb < 4; nb++) if (!check_word((uint64_t)b << (2 * i), nb | (g() << 2), "one base off poly-A")) return 1;
    for (unsigned long i = 0; i < 60000; i++) {                         // two letters only, and words of very few runs
        const unsigned a = (unsigned)g() & 3u, b = (unsigned)g() & 3u;
        uint64_t x = 0, m = g() & g() & 0x5555555555555555ull;
        if (i & 1) m = g() & 0x5555555555555555ull;
        for (unsigned k = 0; k < 32; k++) x |= (uint64_t)(((m >> (2 * k)) & 1u) ? a : b) << (2 * k);
        if (!check_word(x, g(), "two letters")) return 1;
    }
    if (n_words < 1000000ul && argc <= 1) { printf("only %lu words\n", n_words); return 1; }

    // ---- whole reads: old form against new form ----
    const uint32_t lens[] = {1, 33, 65, 66, 67, 97, 98, 129, 130, 500, 2048, 2049, 4097, 10000};
    for (uint32_t len : lens)
        for (unsigned kind = 0; kind < 8; kind++)
            for (unsigned rep = 0; rep < 6; rep++) {
                Read r = make_read(len);
                const unsigned period = kind >= 3 && kind <= 6 ? kind - 1 : 0;      // 2 .. 5
                for (uint32_t i = 0; i < len; i++) {
                    unsigned b;
                    if (kind == 0) b = (unsigned)g() & 3u;
                    else if (kind == 1) b = gc_base(g, 0.30);
                    else if (kind == 2) b = rep & 3u;
                    else if (period) b = (i % period + rep) & 3u;
                    else b = (i * 3u < len) ? ((i & 1u) ? 0u : 1u) : ((unsigned)g() & 3u);      // a low-complexity third, then random
                    if (kind >= 2 && (g() % 97u) == 0u && rep >= 3) b = (unsigned)g() & 3u;     // with a few errors
                    r.set(i, b);
                }
                if (!check_read(r, "read")) return 1;
            }
    // reads steered onto the threshold: from a random read, single-base changes that bring sum sq nearer to 332 nW + delta
    unsigned long landed[3] = {0, 0, 0};
    const uint32_t steer_lens[] = {66, 98, 131, 200, 333, 700};
    for (uint32_t len : steer_lens)
        for (int di = 0; di < 3; di++)
            for (unsigned rep = 0; rep < 8; rep++) {
                const uint32_t nW = mdbg::complexity_windows(len);
                const int64_t target = (int64_t)332 * nW + 2 * (di - 1);
                Read r = make_read(len);
                for (uint32_t i = 0; i < len; i++) r.set(i, (unsigned)g() & 3u);
                uint64_t ssq, sq_;
                read_sums(r, ssq, sq_);
                for (unsigned it = 0; it < 30000 && (int64_t)ssq != target; it++) {
                    const uint32_t i = (uint32_t)(g() % len);
                    const unsigned old_b = r.get(i), nb = (i && (g() & 1u)) ? r.get(i - 1) : ((unsigned)g() & 3u);
                    r.set(i, nb);
                    uint64_t s2, q2;
                    read_sums(r, s2, q2);
                    const int64_t d_old = llabs((int64_t)ssq - target), d_new = llabs((int64_t)s2 - target);
                    if (d_new <= d_old) ssq = s2; else r.set(i, old_b);
                }
                if ((int64_t)ssq == target) landed[di]++;
                if (!check_read(r, "steered read")) return 1;
            }
    if (landed[0] < 10 || landed[1] < 10 || landed[2] < 10) { printf("too few reads on the threshold: %lu below, %lu on, %lu above\n", landed[0], landed[1], landed[2]); return 1; }
    if (n_suspect == 0 || n_suspect == n_reads) { printf("one-sided: %lu of %lu reads suspect\n", n_suspect, n_reads); return 1; }
    printf("ok: %lu words, %lu reads (%lu suspect), on the threshold -2/0/+2: %lu/%lu/%lu\n", n_words, n_reads, n_suspect, landed[0], landed[1], landed[2]);
    return 0;
}
