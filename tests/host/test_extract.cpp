// The device header csrc/extract_dev.hpp compiled for the host, behind a serial copy of extract_copy_kernel's lane loop: one wave of 64
// lanes over the whole batch, a lane an aligned pair of output words a trip, the owner kept from trip to trip and found anew by
// extract_next_owner when the lane has left it, the word's index in the sequence, extract_word, one store a word.
//   1. Every start 0 .. 63 x every length 0 .. 130 x both orientations x both forms, with and without an invalid mask whose bits sit at
//      the range's first and last base and just outside it, in a read that ends with the range and in one that goes on -- against a
//      character-level model of memcpy + Utils::revcomp + DnaBitset2 (toBasespace/ToBasespaceGfa.hpp:1050-1103, utils/DnaBitset.hpp:
//      118-242).  Each read's words and mask words live in a heap block of exactly ceil(L / 32) entries: a read of a word outside the
//      read's own words is a heap overflow under the address sanitizer.
//   2. Seeded batches of ranges over several reads packed back to back (the next read's words follow a read's last), lengths 0 and
//      70 000 among them, a stretch of 600 ranges of at most 8 bases (a lane's next owner far away), ranges that end at their read's
//      last base: every output word written exactly once, padding zero, and the same bytes whatever the words of the OTHER reads hold.
//   3. extract_part_range against the reference's substr arithmetic on the oriented string.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/extract_dev.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

using namespace mdbg;

static unsigned long n_ranges = 0, n_words_out = 0, n_masked = 0, n_at_end = 0, n_batches = 0, n_parts = 0, n_two_words = 0, n_far_owners = 0;

static bool fail(const char *what, long a0 = 0, long a1 = 0, long a2 = 0, long a3 = 0) {
    printf("FAILED: %s: %ld %ld %ld %ld\n", what, a0, a1, a2, a3);
    return false;
}

// ---- the model, over characters -----------------------------------------------------------------------------------------------------
// what the packed read still knows of a character: N under bit 3, else the upper-case base of its 2-bit code
static char known(char c) { return (c & 8) ? 'N' : "ACTG"[(c >> 1) & 3]; }
static char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

static std::string model_string(const std::string &read, uint32_t start, uint32_t length, bool reversed) {
    std::string s(length, '\0');
    memcpy(&s[0], read.data() + start, length);
    for (char &c : s) c = known(c);
    if (reversed) {
        std::reverse(s.begin(), s.end());
        for (char &c : s) c = complement(c);
    }
    return s;
}

static std::vector<uint8_t> model_bytes(const std::string &s, uint32_t form) {
    if (form == EXTRACT_ASCII) return std::vector<uint8_t>(s.begin(), s.end());
    std::vector<uint8_t> d((s.size() + 3) / 4, 0);
    for (size_t i = 0; i < s.size(); i++) {
        const unsigned shift = 6 - 2 * (i % 4);
        switch (s[i]) {
            case 'A': d[i / 4] |= 0u << shift; break;
            case 'C': d[i / 4] |= 1u << shift; break;
            case 'G': d[i / 4] |= 2u << shift; break;
            case 'T': d[i / 4] |= 3u << shift; break;
        }
    }
    return d;
}

// ---- packing, as pack_ascii_kernel derives words and mask from the characters ----------------------------------------------------------
struct Packed {
    std::unique_ptr<uint64_t[]> words;      // exactly ceil(L / 32)
    std::unique_ptr<uint32_t[]> inv;
    uint32_t n_words;
};
static Packed pack(const std::string &read) {
    Packed p;
    p.n_words = (uint32_t)((read.size() + 31) / 32);
    p.words.reset(new uint64_t[p.n_words]());
    p.inv.reset(new uint32_t[p.n_words]());
    for (size_t i = 0; i < read.size(); i++) {
        p.words[i / 32] |= (uint64_t)((read[i] >> 1) & 3) << (2 * (i % 32));
        if (read[i] & 8) p.inv[i / 32] |= 1u << (i % 32);
    }
    return p;
}

// ---- the lane loop ------------------------------------------------------------------------------------------------------------------------
// ranges over reads whose words start at word_off[read] of `words` (inv: null for a batch without masks); the bytes of the batch
static bool run_batch(const uint64_t *const *read_words, const uint32_t *const *read_inv, const std::vector<ExtractRange> &ranges, uint32_t form,
                      std::vector<uint64_t> &off, std::vector<uint8_t> &bytes) {
    const size_t n = ranges.size();
    off.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + 8ull * extract_words(ranges[i].length, form);
    const uint64_t n_words = off[n] / 8;
    std::vector<uint64_t> out(n_words, 0xDEADBEEFDEADBEEFull);
    std::vector<uint8_t> written(n_words, 0);
    // one wave over the whole batch: lane l takes the pairs l, l + 64, ... and keeps the request it is inside of, as extract_copy_kernel's do
    const uint64_t n_pairs = (n_words + 1) / 2;
    uint32_t first = 0;
    while (n_words && off[first + 1] == 0) first++;                      // csr_owner: the last request whose offset is at most byte 0
    for (uint32_t lane = 0; lane < 64; lane++) {
        uint32_t r = first;
        for (uint64_t p = lane; p < n_pairs; p += 64)
            for (uint64_t g = 2 * p; g < 2 * p + 2 && g < n_words; g++) {
                if (g * 8 >= off[r + 1]) {
                    const uint32_t before = r;
                    r = extract_next_owner(off.data(), (uint32_t)n, r, g * 8);
                    if (r - before > 64) n_far_owners++;
                }
                if (!(off[r] <= g * 8 && g * 8 < off[r + 1])) return fail("owner", (long)g, (long)r);
                const ExtractRange rg = ranges[r];
                out[g] = extract_word(read_words[rg.read], read_inv ? read_inv[rg.read] : nullptr, rg.start, rg.length, rg.reversed != 0, (uint32_t)(g - off[r] / 8), form);
                written[g]++;
            }
    }
    for (uint64_t g = 0; g < n_words; g++)
        if (written[g] != 1) return fail("an output word not written exactly once", (long)g, written[g]);
    n_words_out += n_words;
    bytes.resize(off[n]);
    for (uint64_t g = 0; g < n_words; g++)
        for (int b = 0; b < 8; b++) bytes[g * 8 + b] = (uint8_t)(out[g] >> (8 * b));     // little-endian stores
    return true;
}

static bool check_batch(const std::vector<std::string> &reads, const std::vector<ExtractRange> &ranges, const std::vector<uint64_t> &off,
                        const std::vector<uint8_t> &bytes, uint32_t form) {
    for (size_t i = 0; i < ranges.size(); i++) {
        const ExtractRange rg = ranges[i];
        const std::vector<uint8_t> want = model_bytes(model_string(reads[rg.read], rg.start, rg.length, rg.reversed != 0), form);
        if (want.size() != extract_bytes(rg.length, form)) return fail("extract_bytes", (long)i, (long)want.size());
        if (off[i] % 8 || off[i + 1] - off[i] < want.size() || off[i + 1] - off[i] >= want.size() + 8) return fail("offsets", (long)i, (long)off[i], (long)off[i + 1]);
        for (size_t b = 0; b < want.size(); b++)
            if (bytes[off[i] + b] != want[b])
                return fail("start / length / reversed / form", rg.start, rg.length, rg.reversed, form) ||
                       fail("byte (range, byte, got, want)", (long)i, (long)b, bytes[off[i] + b], want[b]);
        for (uint64_t b = off[i] + want.size(); b < off[i + 1]; b++)
            if (bytes[b] != 0) return fail("padding not zero", (long)i, (long)b, bytes[b]);
        n_ranges++;
    }
    return true;
}

static std::string random_read(std::mt19937_64 &rng, size_t n, const char *letters) {
    const size_t k = strlen(letters);
    std::string s(n, 'A');
    for (char &c : s) c = letters[rng() % k];
    return s;
}

// ---- 1. the sweep ---------------------------------------------------------------------------------------------------------------------
static bool check_sweep() {
    std::mt19937_64 rng(11);
    for (uint32_t start = 0; start < 64; start++)
        for (uint32_t length = 0; length <= 130; length++)
            for (uint32_t tail = 0; tail <= 5; tail += 5)
                for (int masked = 0; masked < 2; masked++) {
                    std::string read = random_read(rng, start + length + tail, masked ? "ACGTacgtRSW" : "ACGT");
                    if (read.empty()) continue;
                    if (masked) {                       // bits at the range's first and last base and just outside it
                        if (start > 0) read[start - 1] = 'N';
                        if (length > 0) read[start] = 'n';
                        if (length > 1) read[start + length - 1] = 'K';
                        if (tail > 0) read[start + length] = 'Y';
                        if (length > 40 && rng() % 2) read[start + length / 2] = 'M';
                        n_masked++;
                    }
                    if (tail == 0) n_at_end++;
                    if ((start & 31u) + (length < 32u ? length : 32u) > 32u) n_two_words++;
                    const Packed p = pack(read);
                    const uint64_t *rw[1] = {p.words.get()};
                    const uint32_t *ri[1] = {p.inv.get()};
                    const std::vector<std::string> reads{read};
                    for (uint32_t reversed = 0; reversed < 2; reversed++)
                        for (uint32_t form = 0; form < 2; form++) {
                            const std::vector<ExtractRange> ranges{ExtractRange{0, start, length, reversed}};
                            std::vector<uint64_t> off;
                            std::vector<uint8_t> bytes;
                            if (!run_batch(rw, masked ? ri : nullptr, ranges, form, off, bytes)) return false;
                            if (!check_batch(reads, ranges, off, bytes, form)) return false;
                        }
                }
    return true;
}

// ---- 2. batches over reads packed back to back ------------------------------------------------------------------------------------------
static bool check_batches() {
    std::mt19937_64 rng(12);
    for (int batch = 0; batch < 6; batch++) {
        const bool masked = batch % 2 == 1;
        std::vector<std::string> reads;
        for (size_t len : {1, 31, 32, 33, 64, 100, 257, 2048, 2049, 5000})
            reads.push_back(random_read(rng, len, masked ? "ACGTNacgtnRYKMSW" : "ACGT"));
        reads.push_back(random_read(rng, 70000 + (batch % 3), masked ? "ACGTTTGGCAN" : "ACGT"));
        // one buffer, every read at an even word (objects.hpp), so that the next read's words follow a read's last
        std::vector<uint64_t> word_off(reads.size() + 1, 0);
        for (size_t r = 0; r < reads.size(); r++) word_off[r + 1] = word_off[r] + ((reads[r].size() + 31) / 32 + 1) / 2 * 2;
        std::vector<uint64_t> words(word_off.back(), 0);
        std::vector<uint32_t> inv(word_off.back(), 0);
        std::vector<const uint64_t *> rw(reads.size());
        std::vector<const uint32_t *> ri(reads.size());
        for (size_t r = 0; r < reads.size(); r++) {
            const Packed p = pack(reads[r]);
            std::copy(p.words.get(), p.words.get() + p.n_words, words.begin() + word_off[r]);
            std::copy(p.inv.get(), p.inv.get() + p.n_words, inv.begin() + word_off[r]);
            rw[r] = words.data() + word_off[r];
            ri[r] = inv.data() + word_off[r];
        }
        std::vector<ExtractRange> ranges;
        for (uint32_t r = 0; r < reads.size(); r++) {
            const uint32_t L = (uint32_t)reads[r].size();
            ranges.push_back(ExtractRange{r, 0, L, 0});                       // the whole read (LoadUnitigsFunctor)
            ranges.push_back(ExtractRange{r, 0, L, 1});
            ranges.push_back(ExtractRange{r, L, 0, (uint32_t)(r & 1)});       // nothing, at the read's end
            for (int i = 0; i < 12; i++) {
                const uint32_t len = (uint32_t)(rng() % (std::min(L, 300u) + 1u));
                const bool at_end = i % 3 == 0;
                ranges.push_back(ExtractRange{r, at_end ? L - len : (uint32_t)(rng() % (L - len + 1u)), len, (uint32_t)(rng() & 1)});
                if (at_end) n_at_end++;
            }
        }
        std::shuffle(ranges.begin(), ranges.end(), rng);
        for (int i = 0; i < 600; i++) {                                      // a stretch of ranges of 0 .. 8 bases: a lane's next pair is far more than 64 requests on
            const uint32_t len = (uint32_t)(rng() % 9u);
            ranges.push_back(ExtractRange{9, (uint32_t)(rng() % (5000u - len)), len, (uint32_t)(rng() & 1)});
        }
        for (uint32_t form = 0; form < 2; form++) {
            std::vector<uint64_t> off, off2;
            std::vector<uint8_t> bytes, bytes2;
            if (!run_batch(rw.data(), masked ? ri.data() : nullptr, ranges, form, off, bytes)) return false;
            if (!check_batch(reads, ranges, off, bytes, form)) return false;
            // the same ranges of read 4 alone while every other read's words and mask words are flipped: nothing of a neighbour is used
            std::vector<ExtractRange> mine;
            for (const ExtractRange &rg : ranges) if (rg.read == 4) mine.push_back(rg);
            std::vector<uint8_t> before;
            if (!run_batch(rw.data(), masked ? ri.data() : nullptr, mine, form, off2, before)) return false;
            for (size_t w = 0; w < words.size(); w++)
                if (w < word_off[4] || w >= word_off[4] + (reads[4].size() + 31) / 32) { words[w] = ~words[w]; inv[w] = ~inv[w]; }
            if (!run_batch(rw.data(), masked ? ri.data() : nullptr, mine, form, off2, bytes2)) return false;
            for (size_t w = 0; w < words.size(); w++)
                if (w < word_off[4] || w >= word_off[4] + (reads[4].size() + 31) / 32) { words[w] = ~words[w]; inv[w] = ~inv[w]; }
            if (before != bytes2) return fail("a range's bytes depend on another read's words", batch, form);
        }
        n_batches++;
    }
    return true;
}

// ---- 3. the three parts -------------------------------------------------------------------------------------------------------------------
static bool check_parts() {
    std::mt19937_64 rng(13);
    for (int i = 0; i < 20000; i++) {
        const std::string read = random_read(rng, 40 + rng() % 200, "ACGT");
        const uint32_t L = (uint32_t)read.size(), ps = (uint32_t)(rng() % L), pe = ps + (uint32_t)(rng() % (L - ps + 1u));
        const uint32_t ls = (uint32_t)(rng() % (pe - ps + 1u)), le = (uint32_t)(rng() % (pe - ps + 1u));
        const bool reversed = rng() & 1;
        const std::string entire = model_string(read, ps, pe - ps, reversed);      // memcpy + revcomp
        for (uint32_t part = 0; part < 3; part++) {
            const std::string want = part == EXTRACT_ENTIRE ? entire : part == EXTRACT_LEFT ? entire.substr(0, ls) : entire.substr(entire.size() - le, le);
            uint32_t start = 0, length = 0;
            if (extract_part_range(ps, pe, ls, le, reversed, part, start, length) != 0u) return fail("a fine request refused", i, part);
            if ((uint64_t)start + length > L || model_string(read, start, length, reversed) != want) return fail("part", i, part, start, length);
            n_parts++;
        }
        uint32_t s, l;
        if (extract_part_range(ps, pe, pe - ps + 1u, le, reversed, EXTRACT_LEFT, s, l) != EXTRACT_BAD_OVERHANG) return fail("ls too large accepted", i);
        if (extract_part_range(ps, pe, ls, pe - ps + 1u, reversed, EXTRACT_ENTIRE, s, l) != EXTRACT_BAD_OVERHANG) return fail("le too large accepted", i);
        if (extract_part_range(ps, pe, ls, le, reversed, 3u, s, l) != EXTRACT_BAD_PART) return fail("part 3 accepted", i);
    }
    return true;
}

int main() {
    if (!check_sweep() || !check_batches() || !check_parts()) return 1;
    printf("ok: %lu ranges, %lu output words, %lu masked reads, %lu ranges at a read's end, %lu with a second source word, %lu batches, %lu parts, "
           "%lu owners more than 64 requests on\n", n_ranges, n_words_out, n_masked, n_at_end, n_two_words, n_batches, n_parts, n_far_owners);
    return 0;
}
