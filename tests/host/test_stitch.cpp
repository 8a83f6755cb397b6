// The device header csrc/stitch_dev.hpp compiled for the host, behind serial copies of the lane loops of stitch_copy_kernel and
// fasta_write_kernel (csrc/stitch.hip): a few waves of 64 lanes over contiguous spans of the output's pairs of words, a lane an aligned pair
// a trip, its contig and its piece kept from trip to trip and found anew by extract_next_owner, stitch_word, one store a word; for the
// text the record kept, fasta_bases8 inside a sequence and fasta_byte elsewhere, nothing stored behind the last byte.
// Against a character-level model of what CreateBaseContigsFunctor does with a piece (toBasespace/ToBasespaceGfa.hpp:1479-1795): the
// read-oriented string, DnaBitset2 (an invalid character is A), Utils::revcomp when the contig's window is reversed (that A is T now), +=.
//   1. Pieces of 0 .. 70 bases joined at every offset mod 32 behind a piece of 0 .. 31 bases, all four (read window reversed) x (flip),
//      both forms, with mask bits at a piece's first and last base and just outside, in reads that end with the piece and reads that go
//      on.  Each read's words and mask words live in a heap block of exactly ceil(L / 32) entries.
//   2. 40 one-base pieces in a row, empty pieces between full ones, contigs of 0, 1, 31, 32, 33, 63, 64, 65 and 4097 bases, one 70 000-base
//      contig of 700 pieces among 2 000 tiny ones; the ranges entry's rule (an invalid base is A in both orientations).
//   3. The text: names of every decimal width, all flags, an empty contig between two full ones, sequences of 0 .. 40 bases.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../metamdbg_amd/csrc/stitch_dev.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

using namespace mdbg;

static unsigned long n_contigs_checked = 0, n_words_out = 0, n_pieces_checked = 0, n_over_two = 0, n_32_pieces = 0, n_at_end = 0, n_masked_pieces = 0, n_far_owners = 0,
                     n_records = 0, n_text_bytes = 0, n_outside = 0;

static bool fail(const char *what, long a0 = 0, long a1 = 0, long a2 = 0, long a3 = 0) {
    printf("FAILED: %s: %ld %ld %ld %ld\n", what, a0, a1, a2, a3);
    return false;
}

// ---- the model, over characters -----------------------------------------------------------------------------------------------------
static char known(char c) { return (c & 8) ? 'N' : "ACTG"[(c >> 1) & 3]; }
static char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }
static void revcomp(std::string &s) {
    std::reverse(s.begin(), s.end());
    for (char &c : s) c = complement(c);
}

struct Piece { uint32_t read, start, length; bool read_reversed, flip; };

// what a piece adds to its contig; spans_entry: the stored piece went through DnaBitset2 before the flip
static std::string model_piece(const std::vector<std::string> &reads, const Piece &p, uint32_t form, bool spans_entry) {
    std::string s = reads[p.read].substr(p.start, p.length);
    for (char &c : s) c = known(c);
    if (p.read_reversed) revcomp(s);
    if (form == EXTRACT_BITSET && spans_entry)
        for (char &c : s) if (c == 'N') c = 'A';                      // DnaBitset2 of the stored piece
    if (p.flip) revcomp(s);
    if (form == EXTRACT_BITSET)
        for (char &c : s) if (c == 'N') c = 'A';                      // DnaBitset2 of the result
    return s;
}

static std::vector<uint8_t> model_bytes(const std::string &s, uint32_t form) {
    if (form == EXTRACT_ASCII) return std::vector<uint8_t>(s.begin(), s.end());
    std::vector<uint8_t> d((s.size() + 3) / 4, 0);
    for (size_t i = 0; i < s.size(); i++) {
        const unsigned code = s[i] == 'C' ? 1u : s[i] == 'G' ? 2u : s[i] == 'T' ? 3u : 0u;
        d[i / 4] |= (uint8_t)(code << (6 - 2 * (i % 4)));
    }
    return d;
}

// ---- packing: every read in heap blocks of exactly its size ------------------------------------------------------------------------------
struct Packed {
    std::vector<std::unique_ptr<uint64_t[]>> words;
    std::vector<std::unique_ptr<uint32_t[]>> inv;
    std::vector<const uint64_t *> w;
    std::vector<const uint32_t *> m;
    bool masked = false;
    const uint64_t *words_of(uint64_t r) const { return w[r]; }
};
struct HostSrc {
    const Packed *p;
    const uint64_t *words(uint64_t w0) const { return p->w[w0]; }
    const uint32_t *mask(uint64_t w0) const { return p->masked ? p->m[w0] : nullptr; }
};
static void pack(Packed &p, const std::vector<std::string> &reads, bool masked) {
    p.masked = masked;
    for (const std::string &read : reads) {
        const size_t nw = (read.size() + 31) / 32;
        p.words.emplace_back(new uint64_t[nw]());
        p.inv.emplace_back(new uint32_t[nw]());
        for (size_t i = 0; i < read.size(); i++) {
            p.words.back()[i / 32] |= (uint64_t)((read[i] >> 1) & 3) << (2 * (i % 32));
            if (read[i] & 8) p.inv.back()[i / 32] |= 1u << (i % 32);
        }
        p.w.push_back(p.words.back().get());
        p.m.push_back(p.inv.back().get());
    }
}

static uint32_t last_at_most(const std::vector<uint64_t> &off, uint64_t at) {      // csr_owner
    uint32_t lo = 0, hi = (uint32_t)off.size() - 1;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= at) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the lane loop of stitch_copy_kernel ------------------------------------------------------------------------------------------------
struct Batch {
    std::vector<Piece> pieces;
    std::vector<uint64_t> poff{0};
    void end_contig() { poff.push_back(pieces.size()); }
};

static bool run_stitch(const std::vector<std::string> &reads, const Packed &packed, const Batch &b, uint32_t form, bool spans_entry, uint32_t n_waves,
                       std::vector<uint64_t> &off, std::vector<uint32_t> &lengths, std::vector<uint8_t> &bytes) {
    const uint32_t n_pieces = (uint32_t)b.pieces.size(), n = (uint32_t)b.poff.size() - 1;
    // the plan (stitch_emit, stitch_contigs_kernel)
    std::vector<StitchRec> recs(n_pieces ? n_pieces : 1);
    std::vector<uint64_t> pbase(n_pieces + 1, 0);
    for (uint32_t i = 0; i < n_pieces; i++) {
        const Piece &p = b.pieces[i];
        if ((uint64_t)p.start + p.length > reads[p.read].size()) return fail("the test's own piece lies outside its read", i);
        const bool flip = spans_entry && p.flip;
        recs[i] = p.length ? StitchRec{(uint64_t)p.read | ((p.read_reversed != p.flip) ? STITCH_REC_REVERSED : 0ull) | (flip ? STITCH_REC_INVALID_T : 0ull), p.start, p.length}
                           : StitchRec{0ull, 0u, 0u};
        pbase[i + 1] = pbase[i] + p.length;
        if (p.length && p.start + p.length == reads[p.read].size()) n_at_end++;
    }
    off.assign(n + 1, 0);
    lengths.assign(n, 0);
    for (uint32_t c = 0; c < n; c++) {
        lengths[c] = (uint32_t)(pbase[b.poff[c + 1]] - pbase[b.poff[c]]);
        off[c + 1] = off[c] + 8ull * extract_words(lengths[c], form);
    }
    const uint64_t n_words = off[n] / 8, n_pairs = (n_words + 1) / 2;
    std::vector<uint64_t> out(n_words, 0xDEADBEEFDEADBEEFull);
    std::vector<uint8_t> written(n_words, 0);
    const HostSrc src{&packed};
    const uint32_t per_word = form == EXTRACT_ASCII ? 8u : 32u;
    const uint64_t per = ((n_pairs + n_waves - 1) / n_waves + 63) / 64 * 64;       // wave_span
    for (uint32_t wave = 0; wave < n_waves; wave++) {
        const uint64_t begin = std::min<uint64_t>(wave * per, n_pairs), end = n_pairs - begin < per ? n_pairs : begin + per;
        if (begin >= end) continue;
        const uint32_t c0 = last_at_most(off, begin * 16);
        const uint32_t p0 = last_at_most(pbase, pbase[b.poff[c0]] + (uint64_t)per_word * (2 * begin - off[c0] / 8));
        for (uint32_t lane = 0; lane < 64; lane++) {
            uint32_t c = c0;
            StitchPiece pc;
            stitch_piece_load(pc, p0, pbase.data(), recs.data());
            for (uint64_t p = begin + lane; p < end; p += 64)
                for (uint64_t g = 2 * p; g < 2 * p + 2 && g < n_words; g++) {
                    if (g * 8 >= off[c + 1]) {
                        const uint32_t before = c;
                        c = extract_next_owner(off.data(), n, c, g * 8);
                        if (c - before > 64) n_far_owners++;
                    }
                    if (!(off[c] <= g * 8 && g * 8 < off[c + 1])) return fail("contig owner", (long)g, (long)c);
                    const uint32_t w = (uint32_t)(g - off[c] / 8), before_piece = pc.p;
                    uint32_t met = 0;
                    out[g] = stitch_word(src, pbase.data(), n_pieces, recs.data(), pc, pbase[b.poff[c]] + (uint64_t)per_word * w, stitch_word_bases(lengths[c], w, form), form, &met);
                    if (pc.p < b.poff[c] || pc.p >= b.poff[c + 1]) return fail("a piece of another contig", (long)g, (long)c, (long)pc.p);
                    if (pc.p - before_piece > 64) n_far_owners++;
                    if (met > 2) n_over_two++;
                    if (met == 32) n_32_pieces++;
                    written[g]++;
                }
        }
    }
    for (uint64_t g = 0; g < n_words; g++)
        if (written[g] != 1) return fail("an output word not written exactly once", (long)g, written[g]);
    n_words_out += n_words;
    bytes.resize(off[n]);
    for (uint64_t g = 0; g < n_words; g++)
        for (int k = 0; k < 8; k++) bytes[g * 8 + k] = (uint8_t)(out[g] >> (8 * k));
    return true;
}

static bool check_stitch(const std::vector<std::string> &reads, const Packed &packed, const Batch &b, bool spans_entry, uint32_t n_waves = 3,
                         std::vector<std::string> *contigs_out = nullptr, std::vector<uint8_t> *bitset_out = nullptr, std::vector<uint64_t> *off_out = nullptr) {
    for (uint32_t form = 0; form < 2; form++) {
        std::vector<uint64_t> off;
        std::vector<uint32_t> lengths;
        std::vector<uint8_t> bytes;
        if (!run_stitch(reads, packed, b, form, spans_entry, n_waves, off, lengths, bytes)) return false;
        for (size_t c = 0; c + 1 < b.poff.size(); c++) {
            std::string s;
            for (uint64_t i = b.poff[c]; i < b.poff[c + 1]; i++) s += model_piece(reads, b.pieces[i], form, spans_entry);
            const std::vector<uint8_t> want = model_bytes(s, form);
            if (lengths[c] != s.size()) return fail("length", (long)c, lengths[c], (long)s.size());
            if (off[c] % 8 || off[c + 1] - off[c] < want.size() || off[c + 1] - off[c] >= want.size() + 8) return fail("offsets", (long)c, (long)off[c], (long)off[c + 1]);
            for (size_t k = 0; k < want.size(); k++)
                if (bytes[off[c] + k] != want[k]) return fail("byte (contig, byte, got, want)", (long)c, (long)k, bytes[off[c] + k], want[k]) || fail("form, spans entry", form, spans_entry);
            for (uint64_t k = off[c] + want.size(); k < off[c + 1]; k++)
                if (bytes[k] != 0) return fail("padding not zero", (long)c, (long)k, bytes[k]);
            n_contigs_checked++;
            if (form == EXTRACT_BITSET && contigs_out) contigs_out->push_back(s);
        }
        if (form == EXTRACT_BITSET && bitset_out) { *bitset_out = bytes; *off_out = off; }
        n_pieces_checked += b.pieces.size();
    }
    return true;
}

static std::string random_read(std::mt19937_64 &rng, size_t n, const char *letters = "ACGT") {
    const size_t k = strlen(letters);
    std::string s(n, 'A');
    for (char &c : s) c = letters[rng() % k];
    return s;
}

// ---- 1. the sweep ---------------------------------------------------------------------------------------------------------------------
static bool check_sweep() {
    std::mt19937_64 rng(21);
    for (uint32_t before = 0; before < 32; before++)
        for (int masked = 0; masked < 2; masked++) {
            std::vector<std::string> reads;
            Batch b;
            for (uint32_t length = 0; length <= 70; length++)
                for (uint32_t combo = 0; combo < 4; combo++) {
                    const uint32_t start = (uint32_t)(rng() % 40), tail = (length + combo) % 2 ? 0u : 5u;
                    std::string read = random_read(rng, start + length + tail);
                    if (read.empty()) read = "A";
                    if (masked) {                       // bits at the piece's first and last base and just outside it
                        if (start > 0) read[start - 1] = 'N';
                        if (length > 0) read[start] = 'n';
                        if (length > 1) read[start + length - 1] = 'K';
                        if (tail > 0) read[start + length] = 'Y';
                        if (length > 0) n_masked_pieces++;
                    }
                    const uint32_t r = (uint32_t)reads.size();
                    reads.push_back(read);
                    reads.push_back(random_read(rng, before + 3, masked ? "ACGTN" : "ACGT"));
                    b.pieces.push_back(Piece{r + 1, 1, before, (combo & 2) != 0, (combo & 1) != 0});      // `before` bases in front: the join's offset mod 32 (mod 8)
                    b.pieces.push_back(Piece{r, start, length, (combo & 1) != 0, (combo & 2) != 0});
                    b.pieces.push_back(Piece{r + 1, 0, 3, (combo & 1) != 0, false});
                    b.end_contig();
                }
            Packed packed;
            pack(packed, reads, masked != 0);
            if (!check_stitch(reads, packed, b, true)) return false;
            if (!check_stitch(reads, packed, b, false, 1)) return false;         // the ranges entry: no flip in the invalid rule
        }
    return true;
}

// ---- 2. the shapes --------------------------------------------------------------------------------------------------------------------
static bool check_shapes() {
    std::mt19937_64 rng(22);
    for (int masked = 0; masked < 2; masked++) {
        const char *letters = masked ? "ACGTACGTACGTN" : "ACGT";
        std::vector<std::string> reads;
        for (size_t len : {1, 31, 32, 33, 64, 100, 257, 2048, 5000}) reads.push_back(random_read(rng, len, letters));
        reads.push_back(random_read(rng, 70000, letters));
        Packed packed;
        pack(packed, reads, masked != 0);
        auto piece = [&](uint32_t r, uint32_t len, bool at_end = false) {
            const uint32_t L = (uint32_t)reads[r].size();
            return Piece{r, at_end ? L - len : (uint32_t)(rng() % (L - len + 1u)), len, (rng() & 1) != 0, (rng() & 1) != 0};
        };
        Batch b;
        for (int i = 0; i < 40; i++) b.pieces.push_back(piece(8, 1, i == 7));      // 40 one-base pieces: a word of 32 pieces
        b.end_contig();
        b.end_contig();                                                             // no piece at all
        for (int i = 0; i < 3; i++) b.pieces.push_back(piece(3, 0));                // nothing but empty pieces
        b.end_contig();
        b.pieces.push_back(piece(5, 0));                                            // empty pieces first, in the middle and last
        b.pieces.push_back(piece(5, 50));
        b.pieces.push_back(piece(5, 0));
        b.pieces.push_back(piece(5, 0));
        b.pieces.push_back(piece(6, 77, true));
        b.pieces.push_back(piece(5, 0));
        b.end_contig();
        for (uint32_t total : {0u, 1u, 31u, 32u, 33u, 63u, 64u, 65u, 4097u}) {     // contigs of these bases, in pieces of at most 700
            for (uint32_t left = total; left;) {
                const uint32_t len = std::min<uint32_t>(left, 1u + (uint32_t)(rng() % 700));
                b.pieces.push_back(piece(8, len, rng() % 4 == 0));
                left -= len;
            }
            b.end_contig();
        }
        for (uint32_t r = 0; r < reads.size(); r++) {                               // every read whole, each orientation and flip
            for (uint32_t combo = 0; combo < 4; combo++) {
                b.pieces.push_back(Piece{r, 0, (uint32_t)reads[r].size(), (combo & 1) != 0, (combo & 2) != 0});
                b.end_contig();
            }
        }
        for (int i = 0; i < 1000; i++) { b.pieces.push_back(piece(7, 1 + (uint32_t)(rng() % 9))); b.end_contig(); }       // tiny contigs ...
        for (int i = 0; i < 700; i++) b.pieces.push_back(piece(9, 100));            // ... one of 70 000 bases in 700 pieces ...
        b.end_contig();
        for (int i = 0; i < 1000; i++) { b.pieces.push_back(piece(7, 1 + (uint32_t)(rng() % 9))); b.end_contig(); }       // ... and tiny ones again
        for (uint32_t waves : {1u, 3u, 16u}) {
            if (!check_stitch(reads, packed, b, true, waves)) return false;
            if (!check_stitch(reads, packed, b, false, waves)) return false;
        }
        // a read cut into pieces and put back together is the read; reversed, the pieces in reverse order, its reverse complement
        for (uint32_t cut : {1u, 7u, 31u, 32u, 33u}) {
            Batch f;
            const uint32_t L = (uint32_t)reads[7].size();
            for (uint32_t at = 0; at < L; at += cut) f.pieces.push_back(Piece{7, at, std::min(cut, L - at), false, false});
            f.end_contig();
            for (uint32_t i = (uint32_t)f.poff[1]; i-- > 0;) { Piece p = f.pieces[i]; p.read_reversed = true; f.pieces.push_back(p); }
            f.end_contig();
            f.pieces.push_back(Piece{7, 0, L, false, false});
            f.end_contig();
            f.pieces.push_back(Piece{7, 0, L, true, false});
            f.end_contig();
            for (uint32_t form = 0; form < 2; form++) {
                std::vector<uint64_t> off;
                std::vector<uint32_t> lengths;
                std::vector<uint8_t> bytes;
                if (!run_stitch(reads, packed, f, form, false, 2, off, lengths, bytes)) return false;
                const uint64_t size = off[1];
                if (off[2] != 2 * size || off[4] != 4 * size || memcmp(&bytes[0], &bytes[off[2]], size) || memcmp(&bytes[off[1]], &bytes[off[3]], size))
                    return fail("a read put back together is not the read", cut, form);
            }
            if (!check_stitch(reads, packed, f, false, 2)) return false;
        }
    }
    return true;
}

// ---- 3. the text ----------------------------------------------------------------------------------------------------------------------
// the lane loop of fasta_write_kernel over a buffer of exactly n_bytes between two guards
static bool run_fasta(const std::vector<uint64_t> &seq_off, const std::vector<uint32_t> &lengths, const std::vector<uint8_t> &seq_bytes, const std::vector<uint32_t> &names,
                      const std::vector<uint8_t> &flags, uint32_t n_waves, std::string &text) {
    const uint32_t n = (uint32_t)lengths.size();
    std::vector<uint64_t> roff(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) roff[i + 1] = roff[i] + fasta_record_bytes(names[i], flags[i], lengths[i]);
    const uint64_t n_bytes = roff[n], n_words = (n_bytes + 7) / 8, n_pairs = (n_words + 1) / 2;
    const size_t guard = 32;
    std::vector<uint8_t> buf(n_bytes + 2 * guard, 0xEE), times(n_bytes, 0);
    uint8_t *out = buf.data() + guard;
    const uint64_t per = ((n_pairs + n_waves - 1) / n_waves + 63) / 64 * 64;
    struct Rec { uint32_t r; uint64_t lo, hi; uint32_t name, flag, length, header; const uint8_t *seq; };
    auto load = [&](Rec &o, uint32_t r) {
        o = Rec{r, roff[r], roff[r + 1], names[r], flags[r], lengths[r], fasta_header_bytes(names[r], flags[r], lengths[r]), seq_bytes.data() + seq_off[r]};
    };
    for (uint32_t wave = 0; wave < n_waves; wave++) {
        const uint64_t begin = std::min<uint64_t>(wave * per, n_pairs), end = n_pairs - begin < per ? n_pairs : begin + per;
        if (begin >= end) continue;
        const uint32_t r0 = last_at_most(roff, begin * 16);
        for (uint32_t lane = 0; lane < 64; lane++) {
            Rec o;
            load(o, r0);
            for (uint64_t p = begin + lane; p < end; p += 64) {
                uint64_t v[2] = {0, 0};
                for (uint32_t h = 0; h < 2; h++) {
                    const uint64_t at = 16 * p + 8 * h;
                    if (at >= n_bytes) break;
                    if (at >= o.hi) load(o, extract_next_owner(roff.data(), n, o.r, at));
                    if (!(o.lo <= at && at < o.hi)) return fail("record owner", (long)at, (long)o.r);
                    const uint64_t k = at - o.lo;
                    if (k >= o.header && k - o.header + 8 <= o.length) { v[h] = fasta_bases8(o.seq, k - o.header); continue; }
                    for (uint32_t bb = 0; bb < 8; bb++) {
                        if (at + bb >= n_bytes) break;
                        if (at + bb >= o.hi) load(o, o.r + 1);
                        v[h] |= (uint64_t)fasta_byte(o.name, o.flag, o.length, o.header, o.seq, at + bb - o.lo) << (8 * bb);
                    }
                }
                const uint64_t at = 16 * p;
                for (uint64_t bb = at; bb < std::min(at + 16, n_bytes); bb++) {        // (the kernel: one 16-byte store, or bytes up to n_bytes)
                    out[bb] = (uint8_t)(v[(bb - at) / 8] >> (8 * ((bb - at) % 8)));
                    times[bb]++;
                }
            }
        }
    }
    for (uint64_t i = 0; i < n_bytes; i++)
        if (times[i] != 1) return fail("a byte of the text not written exactly once", (long)i, times[i]);
    for (size_t i = 0; i < guard; i++)
        if (buf[i] != 0xEE || buf[guard + n_bytes + i] != 0xEE) n_outside++;
    text.assign((const char *)out, n_bytes);
    n_text_bytes += n_bytes;
    return true;
}

static bool check_text() {
    std::mt19937_64 rng(23);
    std::vector<std::string> reads{random_read(rng, 3000, "ACGTACGTN")};
    Packed packed;
    pack(packed, reads, true);
    const uint32_t width_names[] = {0u, 7u, 10u, 99u, 100u, 4321u, 54321u, 654321u, 7654321u, 87654321u, 987654321u, 1000000000u, 4294967295u};
    for (uint32_t flag = 0; flag < 3; flag++) {
        Batch b;
        std::vector<uint32_t> names;
        std::vector<uint8_t> flags;
        uint32_t at = 0;
        auto contig = [&](uint32_t len, uint32_t name, uint32_t fl) {
            if (len) b.pieces.push_back(Piece{0, (uint32_t)(rng() % (3000 - len)), len, (rng() & 1) != 0, (rng() & 1) != 0});
            b.end_contig();
            names.push_back(name);
            flags.push_back((uint8_t)fl);
        };
        for (uint32_t name : width_names) contig(1 + (at++ % 50), name, flag);         // every decimal width
        for (uint32_t len = 0; len <= 40; len++) contig(len, len * 11u, (flag + len) % 3);
        contig(500, 1, flag);                                                        // an empty contig between two full ones
        contig(0, 2, flag);
        contig(700, 3, flag);
        contig(0, 4294967295u, 2);                                                   // ... and one last
        std::vector<std::string> contigs;
        std::vector<uint8_t> bitset;
        std::vector<uint64_t> off;
        if (!check_stitch(reads, packed, b, true, 2, &contigs, &bitset, &off)) return false;
        std::vector<uint32_t> lengths;
        std::string want;
        for (size_t c = 0; c < contigs.size(); c++) {
            lengths.push_back((uint32_t)contigs[c].size());
            if (contigs[c].empty()) want += ">ctg" + std::to_string(names[c]) + "l\nA\n";
            else want += ">ctg" + std::to_string(names[c]) + (flags[c] == 0 ? "l" : "c") + "\n" + contigs[c] + "\n";
            n_records++;
        }
        for (uint32_t waves : {1u, 2u, 7u}) {
            std::string text;
            if (!run_fasta(off, lengths, bitset, names, flags, waves, text)) return false;
            if (text != want) {
                size_t i = 0;
                while (i < text.size() && i < want.size() && text[i] == want[i]) i++;
                return fail("text (flag, waves, first difference, sizes)", flag, waves, (long)i, (long)text.size() * 1000000 + (long)want.size());
            }
        }
    }
    // zero sequences: zero bytes
    std::string text = "x";
    if (!run_fasta({0}, {}, {}, {}, {}, 2, text) || !text.empty()) return fail("zero sequences");
    return true;
}

int main() {
    if (!check_sweep() || !check_shapes() || !check_text()) return 1;
    printf("ok: %lu contigs, %lu pieces, %lu output words, %lu words of more than two pieces, %lu words of 32 pieces, %lu pieces at a read's end, %lu masked pieces, "
           "%lu owners more than 64 on, %lu records, %lu bytes of text, %lu bytes touched outside the text\n",
           n_contigs_checked, n_pieces_checked, n_words_out, n_over_two, n_32_pieces, n_at_end, n_masked_pieces, n_far_owners, n_records, n_text_bytes, n_outside);
    return 0;
}
