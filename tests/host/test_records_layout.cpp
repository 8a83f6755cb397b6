// The device header csrc/records_dev.hpp compiled for the host: the composition of a record file's bytes (rec_emit) run in a serial
// copy of records_write_kernel's loop -- groups of 16 lanes, a grid-stride loop over the records -- into a buffer of exactly n_bytes
// preset to a sentinel, with a count per byte of how often it was stored and a map of which section of which record every byte
// belongs to.  Checked: every byte stored exactly once; a word store is aligned and lies inside one section of one record; nothing
// outside [0, n_bytes); the bytes equal a field-by-field serialisation.  Inputs, both forms: every count 0 .. 70 at every residue of
// the record's start mod 4; zero records; one record; a record of 70 001 values among short ones; seeded random sets; other lane counts.
// The offset arithmetic is also checked with more than 2^32 minimizers in front of a record, with no buffer behind it.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/records_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace mdbg;

static unsigned long long n_sets = 0, n_records = 0, n_bytes_checked = 0, n_word_stores = 0, n_byte_stores = 0, n_far = 0;
static bool seen[2][71][4];

struct Set {
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> m, pos, meanq, len;
    std::vector<uint8_t> dir, qual;
    bool per_read_quality = true;
    uint32_t meanq_all = 0x7FC00000u;            // a NaN
};

static Set make_set(const std::vector<uint32_t> &counts, std::mt19937_64 &rng) {
    Set s;
    static const uint32_t special[] = {0u, 0xFFFFFFFFu, 0x80000000u, 0x000000FFu, 0xFF000000u, 0x01020304u};
    static const uint32_t qbits[] = {0x7FC00000u, 0xFFC00001u, 0x7F800000u, 0x00000000u, 0x80000000u, 0x41A4CCCDu};
    for (uint32_t c : counts) {
        for (uint32_t i = 0; i < c; i++) {
            const uint64_t x = rng();
            s.m.push_back((x & 15u) < 6u ? special[x & 7u ? (x >> 8) % 6u : 0u] : (uint32_t)(x >> 32));
            s.pos.push_back((uint32_t)(rng() >> 20));
            s.dir.push_back((uint8_t)(rng() & 1u));
            s.qual.push_back((uint8_t)(rng() >> 40));
        }
        s.off.push_back(s.off.back() + c);
        s.meanq.push_back((rng() & 3u) == 0u ? qbits[rng() % 6u] : (uint32_t)rng());
        s.len.push_back((uint32_t)rng());
    }
    return s;
}

// field by field; sec[i] = which section of which record byte i belongs to
static std::vector<uint8_t> serialise(int form, const Set &s, std::vector<uint64_t> &sec) {
    std::vector<uint8_t> out;
    sec.clear();
    auto put = [&](const void *p, size_t n, uint64_t id) { const uint8_t *b = (const uint8_t *)p; out.insert(out.end(), b, b + n); sec.insert(sec.end(), n, id); };
    for (size_t r = 0; r + 1 < s.off.size(); r++) {
        const uint64_t o = s.off[r];
        const uint32_t n = (uint32_t)(s.off[r + 1] - o);
        const uint8_t circ = 0;
        put(&n, 4, 8 * r + 0);
        put(&circ, 1, 8 * r + 1);
        put(s.m.data() + o, 4 * (size_t)n, 8 * r + 2);
        if (form != REC_INIT) continue;
        put(s.pos.data() + o, 4 * (size_t)n, 8 * r + 3);
        put(s.dir.data() + o, n, 8 * r + 4);
        put(s.qual.data() + o, n, 8 * r + 5);
        const uint32_t q = s.per_read_quality ? s.meanq[r] : s.meanq_all;
        put(&q, 4, 8 * r + 6);
        put(&s.len[r], 4, 8 * r + 7);
    }
    return out;
}

struct BufferSink {
    std::vector<uint8_t> &buf;
    std::vector<uint8_t> &hits;
    const std::vector<uint64_t> &sec;
    const char *err = nullptr;
    uint64_t err_at = 0;
    void fail(const char *why, uint64_t at) { if (!err) { err = why; err_at = at; } }
    void byte(uint64_t at, uint8_t v) {
        n_byte_stores++;
        if (at >= buf.size()) { fail("a byte store outside [0, n_bytes)", at); return; }
        buf[at] = v;
        if (hits[at] < 255) hits[at]++;
    }
    void word(uint64_t at, uint32_t v) {
        n_word_stores++;
        if (at & 3u) { fail("a word store that is not aligned", at); return; }
        if (at + 4 > buf.size()) { fail("a word store outside [0, n_bytes)", at); return; }
        if (sec[at] != sec[at + 1] || sec[at] != sec[at + 2] || sec[at] != sec[at + 3]) fail("a word store across a section or record border", at);
        memcpy(buf.data() + at, &v, 4);
        for (int b = 0; b < 4; b++) if (hits[at + b] < 255) hits[at + b]++;
    }
};

static bool check(int form, const Set &s, uint32_t lanes, uint32_t groups, const char *what) {
    std::vector<uint64_t> sec;
    const std::vector<uint8_t> want = serialise(form, s, sec);
    const uint64_t n_reads = s.off.size() - 1;
    const uint64_t n_bytes = rec_start(form, n_reads, s.off.back());
    if (n_bytes != want.size()) { printf("%s (form %d): rec_start of the end says %llu bytes, the serialisation has %zu\n", what, form, (unsigned long long)n_bytes, want.size()); return false; }
    std::vector<uint8_t> buf(n_bytes, 0xA5), hits(n_bytes, 0);          // exactly n_bytes: the sanitizer sees a store behind them
    BufferSink sink{buf, hits, sec};
    RecSource src{s.m.data(), s.pos.data(), s.dir.data(), s.qual.data(), s.per_read_quality ? s.meanq.data() : nullptr, s.meanq_all, s.len.data()};
    // the kernel's loop: group g of `groups` takes records g, g + groups, ...; its lanes run one after the other here
    for (uint32_t g = 0; g < groups; g++)
        for (uint64_t r = g; r < n_reads; r += groups) {
            const uint64_t o = s.off[r], n = s.off[r + 1] - o;
            if (rec_start(form, r, o) + rec_bytes(form, n) != rec_start(form, r + 1, s.off[r + 1])) { printf("%s: record %llu does not end where the next begins\n", what, (unsigned long long)r); return false; }
            for (uint32_t lane = 0; lane < lanes; lane++) rec_emit(form, src, r, o, n, lane, lanes, sink);
            if (n <= 70) seen[form][n][rec_start(form, r, o) & 3u] = true;
        }
    if (sink.err) { printf("%s (form %d, %u lanes): %s at byte %llu of %llu\n", what, form, lanes, sink.err, (unsigned long long)sink.err_at, (unsigned long long)n_bytes); return false; }
    for (uint64_t i = 0; i < n_bytes; i++) {
        if (hits[i] != 1) { printf("%s (form %d, %u lanes): byte %llu of %llu (record %llu, section %llu) was stored %u times\n", what, form, lanes, (unsigned long long)i,
                                   (unsigned long long)n_bytes, (unsigned long long)(sec[i] / 8), (unsigned long long)(sec[i] % 8), (unsigned)hits[i]); return false; }
        if (buf[i] != want[i]) { printf("%s (form %d, %u lanes): byte %llu of %llu (record %llu, section %llu) is %02x, the serialisation has %02x\n", what, form, lanes,
                                        (unsigned long long)i, (unsigned long long)n_bytes, (unsigned long long)(sec[i] / 8), (unsigned long long)(sec[i] % 8), buf[i], want[i]); return false; }
    }
    n_sets++; n_records += n_reads; n_bytes_checked += n_bytes;
    return true;
}

// no buffer: where the stores of one record fall when `o` minimizers -- more than 2^32 -- stand in front of it
struct RangeSink {
    uint64_t lo, hi, stored = 0;
    bool bad = false;
    void byte(uint64_t at, uint8_t) { if (at < lo || at >= hi) bad = true; stored++; }
    void word(uint64_t at, uint32_t) { if (at < lo || at + 4 > hi || (at & 3u)) bad = true; stored += 4; }
};

static bool check_far(int form, uint64_t r, uint64_t o, uint32_t n) {
    const unsigned __int128 want = form == REC_INIT ? (unsigned __int128)13 * r + (unsigned __int128)10 * o : (unsigned __int128)5 * r + (unsigned __int128)4 * o;
    const uint64_t at = rec_start(form, r, o);
    if ((unsigned __int128)at != want || at <= 0xFFFFFFFFull) { printf("rec_start(form %d, r %llu, o %llu) = %llu\n", form, (unsigned long long)r, (unsigned long long)o, (unsigned long long)at); return false; }
    if (rec_start(form, r + 1, o + n) - at != rec_bytes(form, n)) { printf("rec_bytes(form %d, %u) does not agree with rec_start\n", form, n); return false; }
    // the arrays are indexed from `o` on: hand the composition pointers moved back by o so that only [o, o + n) is ever touched
    std::vector<uint32_t> v(n + 1, 0x11223344u), per_read(1, 7u);
    std::vector<uint8_t> b(n + 1, 0x5Au);
    RecSource src{v.data() - o, v.data() - o, b.data() - o, b.data() - o, nullptr, 0x7FC00000u, per_read.data() - r};
    RangeSink sink{at, at + rec_bytes(form, n)};
    for (uint32_t lane = 0; lane < 16; lane++) rec_emit(form, src, r, o, n, lane, 16, sink);
    if (sink.bad || sink.stored != rec_bytes(form, n)) { printf("far record (form %d, r %llu, o %llu, n %u): %llu bytes stored of %llu%s\n", form, (unsigned long long)r, (unsigned long long)o, n,
                                                                (unsigned long long)sink.stored, (unsigned long long)rec_bytes(form, n), sink.bad ? ", some outside the record" : ""); return false; }
    n_far++;
    return true;
}

int main() {
    std::mt19937_64 rng(20240607);
    bool ok = true;
    for (int form = 0; form < 2 && ok; form++) {
        // every count 0 .. 70, four records in a row: a record's start moves on by 5 + 4 c (PLAIN) or 13 + 10 c (INIT), an odd number, so the
        // four meet the four residues (asserted below, not assumed)
        std::vector<uint32_t> counts;
        for (uint32_t c = 0; c <= 70; c++) for (int k = 0; k < 4; k++) counts.push_back(c);
        Set every = make_set(counts, rng);
        ok = ok && check(form, every, 16, 5, "every count at every residue");
        every.per_read_quality = false;
        ok = ok && check(form, every, 16, 1, "every count, one mean quality for all");
        ok = ok && check(form, make_set({}, rng), 16, 3, "zero records");
        for (uint32_t c : {0u, 1u, 2u, 3u, 4u, 5u, 17u, 64u}) ok = ok && check(form, make_set({c}, rng), 16, 2, "one record");
        ok = ok && check(form, make_set({3, 0, 12, 70001, 1, 0, 5}, rng), 16, 4, "a record of 70 001 values among short ones");
        for (int t = 0; t < 40 && ok; t++) {
            std::vector<uint32_t> c((size_t)(rng() % 300));
            for (uint32_t &x : c) x = (rng() & 7u) == 0u ? (uint32_t)(rng() % 400) : (uint32_t)(rng() % 24);
            ok = ok && check(form, make_set(c, rng), 16, 1 + (uint32_t)(rng() % 7), "random set");
        }
        // who stores a byte depends on the lanes, which bytes are stored does not
        for (uint32_t lanes : {1u, 2u, 7u, 64u}) ok = ok && check(form, every, lanes, 3, "other lane counts");
        for (uint32_t c = 0; c <= 70 && ok; c++)
            for (int a = 0; a < 4; a++)
                if (!seen[form][c][a]) { printf("form %d: no record of %u values began at residue %d\n", form, c, a); ok = false; }
        for (uint64_t o : {(1ull << 32) + 7, (1ull << 33) + 1, (1ull << 40) + 2, (1ull << 40) + 3})
            for (uint64_t r : {1ull, 2ull, 1000003ull, 4000000000ull})
                for (uint32_t n : {0u, 1u, 9u, 70u}) ok = ok && check_far(form, r, o, n);
    }
    if (!ok) return 1;
    printf("ok: %llu sets, %llu records, %llu bytes, %llu word stores, %llu byte stores, %d count-residue pairs, %llu records behind 2^32 minimizers\n", n_sets, n_records,
           n_bytes_checked, n_word_stores, n_byte_stores, 2 * 71 * 4, n_far);
    return 0;
}
