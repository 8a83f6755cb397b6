// test_deflate_core.cpp -- metamdbg_amd/csrc/deflate_core.hpp (the serial core of the device's DEFLATE decoder) against zlib, on the
// host and under the address and undefined-behaviour sanitizers: the decoder's every read and write is bounds-checked here before the
// same text runs on a GPU.  The driver below is inflate.hip's wave loop written serially: fill the window, one step, resolve the
// step's tokens with the same bounds checks.  Every buffer is a heap block of its exact size, so a byte read or written outside
// [payload, payload + csize) or [text, text + isize) is a sanitizer report.
//
//   test_deflate_core [seed [mutants]]
#include "../../metamdbg_amd/csrc/deflate_core.hpp"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

using Bytes = std::vector<uint8_t>;

struct Arrays {
    alignas(4) uint8_t win[DFL_WIN];
    uint16_t lit_count[32], lit_sym[DFL_LIT_CAP], lit_fast[1u << DFL_LIT_ROOT];
    uint16_t dist_count[32], dist_sym[DFL_DIST_CAP], dist_fast[1u << DFL_DIST_ROOT];
    uint8_t lens[DFL_LENS];
    uint32_t tok[DFL_TOKENS];
};

// the member [payload, +csize) into exactly isize bytes: 0 or a DFL_E_* code; *text receives what was produced
static uint32_t core_inflate(const uint8_t *payload_in, uint32_t csize, uint32_t isize, uint32_t crc, bool check_crc, Bytes *text) {
    std::unique_ptr<uint8_t[]> payload(new uint8_t[csize ? csize : 1]);      // exact size, own block
    if (csize) memcpy(payload.get(), payload_in, csize);
    std::unique_ptr<uint8_t[]> out(new uint8_t[isize ? isize : 1]);
    std::unique_ptr<Arrays> a(new Arrays);
    dfl_mem m;
    m.win = a->win;
    m.lit_count = a->lit_count; m.lit_sym = a->lit_sym; m.lit_fast = a->lit_fast;
    m.dist_count = a->dist_count; m.dist_sym = a->dist_sym; m.dist_fast = a->dist_fast;
    m.lens = a->lens; m.tok = a->tok;
    dfl_state st;
    dfl_begin(st, csize, isize);
    uint32_t err = DFL_OK;
    bool done = false;
    const uint64_t max_steps = dfl_max_steps(csize);
    for (uint64_t step = 0; step < max_steps; step++) {
        if (dfl_window_stale(st.bitpos, st.wbase, csize, st.filled != 0)) {
            st.wbase = dfl_window_base(payload.get(), st.bitpos, csize);
            st.filled = 1;
            for (uint32_t lane = 0; lane < 64; lane++) dfl_fill_lane(reinterpret_cast<uint32_t *>(a->win), payload.get(), csize, st.wbase, lane);
        }
        dfl_step(st, m);
        if (st.act == DFL_ACT_STORED) {
            for (uint32_t j = 0; j < st.stored_len; j++) {
                const uint64_t o = (uint64_t)st.out0 + j, s = (uint64_t)st.stored_at + j;
                if (o < isize && s < csize) out[o] = payload[s];
            }
        } else if (st.act == DFL_ACT_TOKENS) {
            uint64_t o = st.out0;
            for (uint32_t t = 0; t < st.n_tok && t < DFL_TOKENS; t++) {
                const uint32_t k = a->tok[t];
                if (!(k & DFL_TOK_MATCH)) {
                    if (o < isize) out[o] = (uint8_t)k;
                    o++;
                    continue;
                }
                const uint32_t len = (k >> 16) & 511u, dist = k & 0xFFFFu;
                for (uint32_t j = 0; j < len; j++) {
                    const uint64_t d = o + j;
                    if (dist && dist <= o && d < isize) out[d] = out[o - dist + (j % dist)];
                }
                o += len;
            }
        }
        if (dfl_finished(st)) { done = true; break; }
    }
    err = st.err;
    if (err == DFL_OK && !done) err = DFL_E_INPUT;
    if (err == DFL_OK && st.out != isize) err = DFL_E_SIZE;
    if (err == DFL_OK && check_crc) {
        // as the kernel does it: 64 lanes over contiguous pieces, combined with x^(8 * bytes behind the piece)
        uint32_t table[256];
        for (uint32_t i = 0; i < 256; i++) table[i] = dfl_crc_table_entry(i);
        const uint32_t piece = (isize + 63) / 64;
        uint32_t all = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t b0 = (uint64_t)lane * piece, e0 = b0 + piece;
            const uint32_t b = (uint32_t)(b0 < isize ? b0 : isize), e = (uint32_t)(e0 < isize ? e0 : isize);
            uint32_t reg = lane == 0 ? 0xFFFFFFFFu : 0u;
            for (uint32_t i = b; i < e; i++) reg = dfl_crc_byte(table, reg, out[i]);
            all ^= dfl_crc_mul(reg, dfl_crc_xpow8(isize - e));
        }
        if ((all ^ 0xFFFFFFFFu) != crc) err = DFL_E_CRC;
    }
    if (text) text->assign(out.get(), out.get() + (err == DFL_OK || err == DFL_E_CRC ? isize : 0));
    return err;
}

// zlib's raw inflate of the payload: true when the stream ends having produced exactly isize bytes
static bool zlib_inflate(const Bytes &payload, uint32_t isize, Bytes *text) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) { fprintf(stderr, "inflateInit2 failed\n"); exit(2); }
    Bytes out((size_t)isize + 1024);                              // room to see that it yields more
    z.next_in = const_cast<Bytef *>(payload.data());
    z.avail_in = (uInt)payload.size();
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    const int rc = inflate(&z, Z_FINISH);
    const size_t n = z.total_out;
    inflateEnd(&z);
    if (rc != Z_STREAM_END || n != isize) return false;
    out.resize(n);
    *text = out;
    return true;
}

static Bytes raw_deflate(const Bytes &data, int level, int strategy, size_t flush_every = 0) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, strategy) != Z_OK) { fprintf(stderr, "deflateInit2 failed\n"); exit(2); }
    Bytes out(deflateBound(&z, (uLong)data.size()) + 64 + (flush_every ? data.size() / flush_every * 16 : 0));
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    size_t at = 0;
    if (flush_every) {
        while (data.size() - at > flush_every) {
            z.next_in = const_cast<Bytef *>(data.data() + at);
            z.avail_in = (uInt)flush_every;
            if (deflate(&z, Z_FULL_FLUSH) != Z_OK) { fprintf(stderr, "deflate(flush) failed\n"); exit(2); }
            at += flush_every;
        }
    }
    z.next_in = const_cast<Bytef *>(data.data() + at);
    z.avail_in = (uInt)(data.size() - at);
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) { fprintf(stderr, "deflate failed\n"); exit(2); }
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

struct Member { std::string name; Bytes payload; Bytes text; };
static std::vector<Member> g_members;
static int g_failures = 0;

static void fail(const std::string &what) {
    fprintf(stderr, "FAIL: %s\n", what.c_str());
    g_failures++;
}

static void check_member(const Member &mb) {
    const uint32_t crc = (uint32_t)crc32(0L, mb.text.data(), (uInt)mb.text.size());
    Bytes got;
    const uint32_t err = core_inflate(mb.payload.data(), (uint32_t)mb.payload.size(), (uint32_t)mb.text.size(), crc, true, &got);
    if (err != DFL_OK) { fail(mb.name + ": " + dfl_reason(err)); return; }
    if (got != mb.text) { fail(mb.name + ": text differs from zlib's"); return; }
    // and the CRC is really looked at
    if (core_inflate(mb.payload.data(), (uint32_t)mb.payload.size(), (uint32_t)mb.text.size(), crc ^ 0x00010000u, true, nullptr) != DFL_E_CRC)
        fail(mb.name + ": a wrong CRC-32 passed");
}

// an item is cut into BGZF-sized pieces and each is a member of its own
static void add_item(const std::string &name, const Bytes &data, int level, int strategy, size_t block = 0xff00, size_t flush_every = 0) {
    size_t at = 0;
    int piece = 0;
    do {
        const size_t n = data.size() - at < block ? data.size() - at : block;
        Member mb;
        mb.name = name + "#" + std::to_string(piece++);
        mb.text.assign(data.begin() + at, data.begin() + at + n);
        mb.payload = raw_deflate(mb.text, level, strategy, flush_every);
        Bytes z;
        if (!zlib_inflate(mb.payload, (uint32_t)n, &z) || z != mb.text) { fprintf(stderr, "zlib does not round-trip %s\n", mb.name.c_str()); exit(2); }
        g_members.push_back(mb);
        at += n;
    } while (at < data.size());
}

struct BitWriter {
    Bytes out;
    uint32_t acc = 0, n = 0;
    void bits(uint32_t v, uint32_t k) { for (uint32_t i = 0; i < k; i++) { acc |= ((v >> i) & 1u) << n; if (++n == 8) { out.push_back((uint8_t)acc); acc = 0; n = 0; } } }
    void code(uint32_t c, uint32_t len) { for (uint32_t i = 0; i < len; i++) bits((c >> (len - 1 - i)) & 1u, 1); }    // most significant bit first
    Bytes done() { if (n) { out.push_back((uint8_t)acc); acc = 0; n = 0; } return out; }
};
// A dynamic block by hand: literals 'A', 'C', end-of-block and length 3, two bits each; ONE distance code (distance 1) of length 1 --
// an incomplete code that zlib accepts.  with_dist = false: HDIST's single entry has length 0 (no distance code) and no match is used.
static Member handmade_dynamic(bool with_dist) {
    BitWriter w;
    w.bits(1, 1); w.bits(2, 2);                                  // final, dynamic
    w.bits(258 - 257, 5); w.bits(0, 5); w.bits(18 - 4, 4);       // HLIT 258, HDIST 1, HCLEN 18
    // code-length code: symbols 0, 1, 2, 18 with two bits each -> canonical codes 00, 01, 10, 11
    const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 18; i++) { const int s = order[i]; w.bits(s == 0 || s == 1 || s == 2 || s == 18 ? 2 : 0, 3); }
    auto zeros = [&](uint32_t nrep) { w.code(3, 2); w.bits(nrep - 11, 7); };
    zeros(65); w.code(2, 2); w.code(0, 2); w.code(2, 2);         // lens[65] = 2, lens[66] = 0, lens[67] = 2
    zeros(138); zeros(50);                                       // lens[68 .. 255] = 0
    w.code(2, 2); w.code(2, 2);                                  // lens[256] = lens[257] = 2
    if (with_dist) w.code(1, 2); else w.code(0, 2);              // the distance code's single entry
    // literal/length codes in symbol order: 'A' 00, 'C' 01, 256 10, 257 11
    Member mb;
    w.code(0, 2); w.code(1, 2);
    mb.text = {'A', 'C'};
    if (with_dist) {
        w.code(3, 2); w.code(0, 1);                              // length 3, distance 1
        w.code(0, 2);
        w.code(3, 2); w.code(0, 1);
        mb.text = {'A', 'C', 'C', 'C', 'C', 'A', 'A', 'A', 'A'};
    }
    w.code(2, 2);
    mb.payload = w.done();
    mb.name = with_dist ? "handmade: one distance code" : "handmade: no distance code";
    Bytes z;
    if (!zlib_inflate(mb.payload, (uint32_t)mb.text.size(), &z) || z != mb.text) { fprintf(stderr, "zlib refuses the hand-made block (%s)\n", mb.name.c_str()); exit(2); }
    return mb;
}

static Bytes dna(std::mt19937_64 &rng, size_t n, size_t line) {
    Bytes d;
    size_t col = 0;
    while (d.size() < n) {
        d.push_back("ACGT"[rng() & 3]);
        if (line && ++col == line) { d.push_back('\n'); col = 0; }
    }
    d.resize(n);
    return d;
}
static Bytes fastq(std::mt19937_64 &rng, size_t n) {
    std::string s;
    int r = 0;
    while (s.size() < n) {
        const size_t len = 50 + rng() % 400;
        s += "@read" + std::to_string(r++) + "\n";
        for (size_t i = 0; i < len; i++) s += "ACGT"[rng() & 3];
        s += "\n+\n";
        for (size_t i = 0; i < len; i++) s += (char)(33 + rng() % 48);
        s += "\n";
    }
    s.resize(n);
    return Bytes(s.begin(), s.end());
}
static Bytes periodic(std::mt19937_64 &rng, size_t period, size_t n) {
    Bytes p(period), d(n);
    for (auto &c : p) c = (uint8_t)rng();
    for (size_t i = 0; i < n; i++) d[i] = p[i % period];
    return d;
}
static Bytes random_bytes(std::mt19937_64 &rng, size_t n) {
    Bytes d(n);
    for (auto &c : d) c = (uint8_t)rng();
    return d;
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20240611;
    const int n_mutants = argc > 2 ? atoi(argv[2]) : 2400;
    std::mt19937_64 rng(seed);
    const int levels[4] = {0, 1, 6, 9};
    const int strategies[4] = {Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE};
    const char *sname[4] = {"default", "fixed", "huffman", "rle"};
    {
        Bytes mixed = fastq(rng, 30000);
        const Bytes d = dna(rng, 20000, 80);
        mixed.insert(mixed.end(), d.begin(), d.end());
        for (int l : levels)
            for (int s = 0; s < 4; s++) add_item(std::string("mixed level ") + std::to_string(l) + " " + sname[s], mixed, l, strategies[s]);
    }
    add_item("dna one line", dna(rng, 70000, 0), 6, Z_DEFAULT_STRATEGY);
    add_item("dna 60 columns", dna(rng, 70000, 60), 6, Z_DEFAULT_STRATEGY);
    add_item("dna 60 columns level 1", dna(rng, 70000, 60), 1, Z_DEFAULT_STRATEGY);
    add_item("fastq 33-80", fastq(rng, 140000), 6, Z_DEFAULT_STRATEGY);
    add_item("65280 of one byte", Bytes(65280, 'A'), 6, Z_DEFAULT_STRATEGY, 65536);
    add_item("65536 of one byte", Bytes(65536, 'T'), 9, Z_DEFAULT_STRATEGY, 65536);
    for (size_t p : {1, 2, 3, 4, 63, 64, 65, 257, 258, 259}) add_item("period " + std::to_string(p), periodic(rng, p, 20000 + p), 6, Z_DEFAULT_STRATEGY);
    {
        Bytes d = random_bytes(rng, 40 * 1024);
        d.insert(d.end(), d.begin(), d.begin() + 300);
        add_item("far match", d, 9, Z_DEFAULT_STRATEGY);
    }
    add_item("random (stored)", random_bytes(rng, 65536), 6, Z_DEFAULT_STRATEGY, 65536);
    add_item("empty", Bytes(), 6, Z_DEFAULT_STRATEGY);
    add_item("one byte", Bytes(1, 'x'), 6, Z_DEFAULT_STRATEGY);
    add_item("two bytes", Bytes{'x', 'y'}, 6, Z_DEFAULT_STRATEGY);
    add_item("block size 3000", fastq(rng, 9000), 6, Z_DEFAULT_STRATEGY, 3000);
    add_item("full flush every 1000", fastq(rng, 30000), 6, Z_DEFAULT_STRATEGY, 0xff00, 1000);
    add_item("full flush every 1000, stored", random_bytes(rng, 5000), 0, Z_DEFAULT_STRATEGY, 0xff00, 1000);
    g_members.push_back(handmade_dynamic(true));
    g_members.push_back(handmade_dynamic(false));

    for (const Member &mb : g_members) check_member(mb);

    // the refusals the GPU tests send to the device, here first
    {
        const Member &mb = g_members[0];
        Bytes t;
        const uint32_t cs = (uint32_t)mb.payload.size(), is = (uint32_t)mb.text.size();
        if (core_inflate(mb.payload.data(), cs, is + 1, 0, false, &t) == DFL_OK) fail("isize one too large passed");
        if (core_inflate(mb.payload.data(), cs, is - 1, 0, false, &t) == DFL_OK) fail("isize one too small passed");
        if (core_inflate(mb.payload.data(), cs - 1, is, 0, false, &t) == DFL_OK) fail("csize one short passed");
        Bytes p = mb.payload;
        p[0] |= 6;
        if (core_inflate(p.data(), cs, is, 0, false, &t) != DFL_E_TYPE) fail("block type 3 was not refused as such");
        Bytes s = {0x01, 0x05, 0x00, 0xFA, 0xFE, 'h', 'e', 'l', 'l', 'o'};      // NLEN should be 0xFFFA
        if (core_inflate(s.data(), (uint32_t)s.size(), 5, 0, false, &t) != DFL_E_STORED) fail("a wrong NLEN was not refused as such");
        if (core_inflate(nullptr, 0, 0, 0, false, &t) != DFL_E_INPUT) fail("an empty payload was not refused as exhausted");
    }

    // mutants: whatever zlib makes of the damaged stream, the core makes the same of it
    int agreed_ok = 0, agreed_bad = 0;
    for (int i = 0; i < n_mutants; i++) {
        const Member &mb = g_members[rng() % g_members.size()];
        Bytes p = mb.payload;
        uint32_t isize = (uint32_t)mb.text.size();
        const unsigned kind = (unsigned)(rng() % 8);
        std::string what;
        if (kind < 5 && !p.empty()) {
            // header bytes are hit more often than their share: that is where the tables come from
            const size_t at = (rng() & 1) ? rng() % p.size() : rng() % (p.size() < 96 ? p.size() : 96);
            const unsigned bit = (unsigned)(rng() & 7);
            p[at] ^= (uint8_t)(1u << bit);
            what = "bit " + std::to_string(bit) + " of byte " + std::to_string(at) + " flipped";
        } else if (kind < 7 && !p.empty()) {
            const size_t cut = 1 + rng() % 8;
            p.resize(p.size() > cut ? p.size() - cut : 0);
            what = "truncated by " + std::to_string(cut);
        } else {
            const int delta = (int)(rng() % 7) - 3;
            const long v = (long)isize + (delta ? delta : 1);
            isize = (uint32_t)(v < 0 ? 0 : v > (long)DFL_MAX_ISIZE ? DFL_MAX_ISIZE : v);
            what = "isize " + std::to_string(isize) + " for " + std::to_string(mb.text.size());
        }
        Bytes want, got;
        const bool z_ok = zlib_inflate(p, isize, &want);
        const uint32_t err = core_inflate(p.data(), (uint32_t)p.size(), isize, 0, false, &got);
        if (z_ok) {
            if (err != DFL_OK) fail(mb.name + ", " + what + ": zlib inflates it, the core says " + dfl_reason(err));
            else if (got != want) fail(mb.name + ", " + what + ": text differs from zlib's");
            agreed_ok++;
        } else {
            if (err == DFL_OK) fail(mb.name + ", " + what + ": zlib refuses it, the core does not");
            agreed_bad++;
        }
    }
    if (g_failures) { fprintf(stderr, "%d failures\n", g_failures); return 1; }
    printf("ok %zu members, %d mutants (%d still inflate, %d refused)\n", g_members.size(), n_mutants, agreed_ok, agreed_bad);
    return 0;
}
