// test_gzip_core.cpp -- the gzip chunk decoder of metamdbg_amd/csrc/deflate_core.hpp (gz_step) against zlib, on the host and under the
// address and undefined-behaviour sanitizers, before the same text runs on a GPU.  The driver is gzip.hip written serially: the wave
// loop of gzip_decode_kernel (fill the window, one step, resolve the step's tokens into 16-bit symbols with the same bounds checks, a
// second pass at the format's maximum for a chunk that overflows 8 symbols a byte), the window chain of gzip_windows_kernel, the
// translation of gzip_translate_kernel and the CRC-32 by pieces of gzip_crc_kernel.  Every buffer is a heap block of its exact size.
// Ground truth for block boundaries is zlib's own inflate(Z_BLOCK) (data_type & 128, its unused bits).  Also checked: the header
// search of host/gzip_parallel.hpp as mdbg_host::gzip_find_block.
//
//   test_gzip_core [seed [mutants per item]]
#include "../../metamdbg_amd/csrc/deflate_core.hpp"
#include "../../metamdbg_amd/host/gzip_parallel.hpp"

#include <zlib.h>

#include <algorithm>
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
struct Border { uint32_t at, crc, isize; };
struct Decoded {
    std::unique_ptr<uint16_t[]> sym;
    uint32_t n = 0, status = 0, ended = 0;
    uint64_t end_bit = 0;
    std::vector<Border> borders;
};

// bits [start, stop) of `file` as one chunk with room for `cap` symbols (gzip_decode_kernel, one wave)
static void core_chunk(const Bytes &file, uint64_t start, uint64_t stop, uint32_t reach0, bool at_header, bool at_maximum, Decoded &D) {
    const uint64_t first = start >> 3;
    const uint32_t csize = (uint32_t)((stop == GZ_TO_END ? file.size() : (stop + 7) / 8) - first);
    std::unique_ptr<uint8_t[]> payload(new uint8_t[csize ? csize : 1]);
    if (csize) memcpy(payload.get(), file.data() + first, csize);
    const uint32_t cap = at_maximum ? (uint32_t)gz_max_symbols(csize) : csize * 8u + 64u;
    const uint32_t border_cap = csize / 20u + 2u;
    D.sym.reset(new uint16_t[cap]);
    D.borders.clear();
    uint16_t *out = D.sym.get();
    std::unique_ptr<Border[]> bord(new Border[border_cap]);
    std::unique_ptr<Arrays> a(new Arrays);
    dfl_mem m;
    m.win = a->win;
    m.lit_count = a->lit_count; m.lit_sym = a->lit_sym; m.lit_fast = a->lit_fast;
    m.dist_count = a->dist_count; m.dist_sym = a->dist_sym; m.dist_fast = a->dist_fast;
    m.lens = a->lens; m.tok = a->tok;
    gz_state st;
    gz_begin(st, (uint32_t)(start & 7u), stop == GZ_TO_END ? GZ_TO_END : stop - first * 8, csize, cap, reach0, at_header);
    bool done = false;
    const uint64_t max_steps = gz_max_steps(csize);
    for (uint64_t step = 0; step < max_steps; step++) {
        if (dfl_window_stale(st.bitpos, st.wbase, csize, st.filled != 0)) {
            st.wbase = dfl_window_base(payload.get(), st.bitpos, csize);
            st.filled = 1;
            for (uint32_t lane = 0; lane < 64; lane++) dfl_fill_lane(reinterpret_cast<uint32_t *>(a->win), payload.get(), csize, st.wbase, lane);
        }
        gz_step(st, m);
        if (st.act == GZ_ACT_BORDER) {
            const uint32_t bi = st.n_borders - 1u;
            if (st.n_borders >= 1u && bi < border_cap) { bord[bi].at = st.out0; bord[bi].crc = st.border_crc; bord[bi].isize = st.border_isize; }
            else st.err = GZ_E_BORDERS;
        } else if (st.act == DFL_ACT_STORED) {
            for (uint32_t j = 0; j < st.stored_len; j++) {
                const uint64_t o = (uint64_t)st.out0 + j, s = (uint64_t)st.stored_at + j;
                if (o < cap && s < csize) out[o] = payload[s];
            }
        } else if (st.act == DFL_ACT_TOKENS) {
            uint64_t o = st.out0;
            for (uint32_t t = 0; t < st.n_tok && t < DFL_TOKENS; t++) {
                const uint32_t k = a->tok[t];
                if (!(k & DFL_TOK_MATCH)) {
                    if (o < cap) out[o] = (uint16_t)(k & 255u);
                    o++;
                    continue;
                }
                const uint32_t len = (k >> 16) & 511u, dist = k & 0xFFFFu;
                if (dist && dist <= GZ_REACH) {
                    const int64_t src0 = (int64_t)o - (int64_t)dist;
                    for (uint32_t j = 0; j < len; j++) {
                        const uint64_t d = o + j;
                        const int64_t s = src0 + (int64_t)(j % dist);
                        if (d < cap && s < (int64_t)d) out[d] = s < 0 ? (uint16_t)(GZ_MARK + (uint32_t)((int64_t)GZ_REACH + s)) : out[s];
                    }
                }
                o += len;
            }
        }
        if (gz_finished(st)) { done = true; break; }
    }
    D.status = st.err;
    if (D.status == DFL_OK && !done) D.status = DFL_E_INPUT;
    D.n = st.out; D.ended = st.ended; D.end_bit = first * 8 + st.bitpos;
    if (D.status == DFL_OK) D.borders.assign(bord.get(), bord.get() + st.n_borders);
}

// the file as the chunks that start at byte 0 (a member header) and at `starts` (bits), the last one through the end: 0 or a status;
// *text receives the text (mdbg_bytes_inflate_gzip on a fresh stream, one call)
static uint32_t core_gzip(const Bytes &file, const std::vector<uint64_t> &starts, Bytes *text, uint32_t *n_members = nullptr, uint32_t *n_overflowed = nullptr) {
    const size_t nc = starts.size() + 1;
    std::vector<Decoded> D(nc);
    if (file.empty()) return DFL_E_INPUT;
    for (size_t i = 0; i < nc; i++) {
        const uint64_t start = i ? starts[i - 1] : 0, stop = i + 1 < nc ? starts[i] : GZ_TO_END;
        if ((start >> 3) >= file.size() || (stop != GZ_TO_END && (stop <= start || (stop + 7) / 8 > file.size()))) return GZ_E_STOP;     // (the entry point's range check)
        core_chunk(file, start, stop, i ? GZ_REACH : 0u, i == 0, false, D[i]);
        if (D[i].status == GZ_E_OVERFLOW) {
            core_chunk(file, start, stop, i ? GZ_REACH : 0u, i == 0, true, D[i]);
            if (n_overflowed) ++*n_overflowed;
        }
        if (D[i].status != DFL_OK) return D[i].status;
        if (i + 1 < nc && D[i].ended != GZ_END_STOP) return GZ_E_STOP;
        if (i + 1 < nc && D[i].end_bit != stop) return GZ_E_PAST;
    }
    // places
    std::vector<uint64_t> t0(nc);
    std::vector<int64_t> mstart(nc);
    struct Seg { uint64_t begin, end; uint32_t crc, isize; bool ended; };
    std::vector<Seg> segs;
    uint64_t total = 0, seg_begin = 0;
    int64_t ms = 0;
    for (size_t i = 0; i < nc; i++) {
        t0[i] = total; mstart[i] = ms;
        for (const Border &b : D[i].borders) {
            if (b.at > D[i].n) return GZ_E_BORDERS;
            segs.push_back({seg_begin, total + b.at, b.crc, b.isize, true});
            seg_begin = total + b.at;
            ms = (int64_t)seg_begin;
        }
        total += D[i].n;
    }
    if (D[nc - 1].ended == GZ_END_STOP) return GZ_E_STOP;         // (a whole file ends with a member)
    std::unique_ptr<uint8_t[]> out(new uint8_t[total ? total : 1]);
    // the window chain, then everything else
    uint32_t bad = DFL_OK;
    auto byte_of = [&](size_t i, uint32_t v) -> uint8_t {
        if (!(v & GZ_MARK)) return (uint8_t)v;
        const int64_t src = (int64_t)t0[i] - (int64_t)GZ_REACH + (int64_t)(v & (GZ_MARK - 1u));
        if (src < mstart[i] || src < 0) { bad = GZ_E_BACKREF; return 0; }      // (a fresh stream carries nothing)
        return out[src];
    };
    for (size_t i = 0; i < nc; i++) {
        const uint32_t tail = D[i].n < GZ_REACH ? D[i].n : GZ_REACH;
        for (uint32_t k = D[i].n - tail; k < D[i].n; k++) out[t0[i] + k] = byte_of(i, D[i].sym[k]);
    }
    for (size_t i = nc; i-- > 0;) {                                // (in any order: these symbols read the windows only)
        const uint32_t n = D[i].n > GZ_REACH ? D[i].n - GZ_REACH : 0u;
        for (uint32_t k = 0; k < n; k++) out[t0[i] + k] = byte_of(i, D[i].sym[k]);
    }
    if (bad != DFL_OK) return bad;
    // CRC-32 by pieces that never straddle a border
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; i++) table[i] = dfl_crc_table_entry(i);
    for (const Seg &g : segs) {
        uint32_t acc = 0;
        for (uint64_t at = g.begin; at < g.end; at += 16384) {
            const uint32_t len = (uint32_t)std::min<uint64_t>(16384, g.end - at);
            const uint32_t part = (len + 63u) / 64u;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t b0 = lane * part < len ? lane * part : len, e0 = b0 + part < len ? b0 + part : len;
                uint32_t reg = 0;
                for (uint32_t i = b0; i < e0; i++) reg = dfl_crc_byte(table, reg, out[at + i]);
                acc ^= dfl_crc_mul(reg, dfl_crc_xpow8((uint32_t)((g.end - (at + len) + (len - e0)) % 0xFFFFFFFFull)));
            }
        }
        const uint64_t len = g.end - g.begin;
        const uint32_t reg = acc ^ dfl_crc_mul(0xFFFFFFFFu, dfl_crc_xpow8((uint32_t)(len % 0xFFFFFFFFull)));
        if ((uint32_t)len != g.isize) return GZ_E_ISIZE;
        if ((reg ^ 0xFFFFFFFFu) != g.crc) return DFL_E_CRC;
    }
    if (n_members) *n_members = (uint32_t)segs.size();
    if (text) text->assign(out.get(), out.get() + total);
    return DFL_OK;
}

// ---- zlib ----------------------------------------------------------------------------------------------------------------------------
// the file as gzread takes it: members one after the other, what follows the last and is no member header is ignored.  false: zlib
// refuses.  *starts (optional): the bit of every deflate block header, with inflate(Z_BLOCK);
// *before: the text in front of each
static bool zlib_gzip(const Bytes &file, Bytes *text, std::vector<uint64_t> *starts = nullptr, std::vector<uint64_t> *before = nullptr) {
    text->clear();
    size_t at = 0;
    bool first = true;
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 15 + 16) != Z_OK) { fprintf(stderr, "inflateInit2 failed\n"); exit(2); }
    bool ok = true;
    while (ok) {
        if (!first && !(file.size() - at >= 2 && file[at] == 0x1F && file[at + 1] == 0x8B)) break;
        if (first && file.size() < 2) { ok = false; break; }
        inflateReset(&z);
        z.next_in = const_cast<Bytef *>(file.data() + at);
        z.avail_in = (uInt)(file.size() - at);
        Bytes buf(1 << 16);
        for (;;) {
            z.next_out = buf.data();
            z.avail_out = (uInt)buf.size();
            const int rc = inflate(&z, Z_BLOCK);
            text->insert(text->end(), buf.data(), buf.data() + (buf.size() - z.avail_out));
            if (rc == Z_STREAM_END) break;
            if (rc != Z_OK) { ok = false; break; }
            if ((z.data_type & 128) && !(z.data_type & 64) && starts) {
                const uint64_t bit = (uint64_t)(file.size() - z.avail_in) * 8 - (uint64_t)(z.data_type & 7);
                starts->push_back(bit); before->push_back(text->size());
            }
            if (z.avail_in == 0 && z.avail_out != 0 && !(z.data_type & 128)) { ok = false; break; }     // the input ended inside the member
        }
        if (!ok) break;
        at = file.size() - z.avail_in;
        first = false;
    }
    inflateEnd(&z);
    return ok;
}

static Bytes gzip_member(const Bytes &data, int level, int strategy = Z_DEFAULT_STRATEGY, size_t sync_every = 0, gz_header *head = nullptr) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, level, Z_DEFLATED, 15 + 16, 8, strategy) != Z_OK) { fprintf(stderr, "deflateInit2 failed\n"); exit(2); }
    if (head) deflateSetHeader(&z, head);
    Bytes out(deflateBound(&z, (uLong)data.size()) + 1024 + (sync_every ? data.size() / sync_every * 16 : 0));
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    size_t at = 0;
    if (sync_every)
        while (data.size() - at > sync_every) {
            z.next_in = const_cast<Bytef *>(data.data() + at);
            z.avail_in = (uInt)sync_every;
            if (deflate(&z, Z_SYNC_FLUSH) != Z_OK) { fprintf(stderr, "deflate(flush) failed\n"); exit(2); }
            at += sync_every;
        }
    z.next_in = const_cast<Bytef *>(data.data() + at);
    z.avail_in = (uInt)(data.size() - at);
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) { fprintf(stderr, "deflate failed\n"); exit(2); }
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

// ---- the corpus ----------------------------------------------------------------------------------------------------------------------
static Bytes fasta_text(std::mt19937_64 &rng, size_t n) {
    Bytes t;
    size_t r = 0;
    while (t.size() < n) {
        const std::string h = ">read_" + std::to_string(r++) + " ccs\n";
        t.insert(t.end(), h.begin(), h.end());
        const size_t L = 2000 + rng() % 9000;
        for (size_t i = 0; i < L; i++) { t.push_back("ACGT"[rng() & 3]); if (i % 80 == 79) t.push_back('\n'); }
        t.push_back('\n');
    }
    t.resize(n);
    return t;
}
static Bytes fastq_text(std::mt19937_64 &rng, size_t n) {
    Bytes t;
    size_t r = 0;
    while (t.size() < n) {
        const std::string h = "@read_" + std::to_string(r++) + "\n";
        t.insert(t.end(), h.begin(), h.end());
        const size_t L = 500 + rng() % 5000;
        for (size_t i = 0; i < L; i++) t.push_back("ACGT"[rng() & 3]);
        t.push_back('\n'); t.push_back('+'); t.push_back('\n');
        for (size_t i = 0; i < L; i++) t.push_back((uint8_t)(33 + rng() % 48));
        t.push_back('\n');
    }
    t.resize(n);
    return t;
}
static Bytes cat(std::initializer_list<Bytes> parts) {
    Bytes o;
    for (const Bytes &p : parts) o.insert(o.end(), p.begin(), p.end());
    return o;
}

struct Item { std::string name; Bytes file; bool text_item; };

static int failures = 0;
static void fail(const std::string &what) { fprintf(stderr, "FAIL %s\n", what.c_str()); failures++; }

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1952;
    const int n_mutants = argc > 2 ? atoi(argv[2]) : 24;
    std::mt19937_64 rng(seed);
    std::vector<Item> items;
    const Bytes fa = fasta_text(rng, 340000), fq = fastq_text(rng, 380000);
    for (int level : {1, 6, 9}) {
        items.push_back({"fasta level " + std::to_string(level), gzip_member(fa, level), true});
        items.push_back({"fastq level " + std::to_string(level), gzip_member(fq, level), true});
    }
    items.push_back({"stored only", gzip_member(fq, 0), false});
    items.push_back({"fixed Huffman", gzip_member(fa, 6, Z_FIXED, 50000), false});
    items.push_back({"sync flush points", gzip_member(fq, 6, Z_DEFAULT_STRATEGY, 30000), false});
    const Bytes a(fa.begin(), fa.begin() + 120000), b(fq.begin(), fq.begin() + 110000), c(fa.begin() + 120000, fa.begin() + 250000);
    items.push_back({"three members", cat({gzip_member(a, 6), gzip_member(b, 1), gzip_member(c, 9)}), false});
    items.push_back({"an empty member in the middle", cat({gzip_member(a, 6), gzip_member(Bytes(), 6), gzip_member(b, 6)}), false});
    {
        gz_header head;
        memset(&head, 0, sizeof head);
        static uint8_t extra[700];
        for (size_t i = 0; i < sizeof extra; i++) extra[i] = (uint8_t)(i * 7);
        static char name[] = "reads.fastq";
        head.extra = extra; head.extra_len = sizeof extra; head.name = reinterpret_cast<Bytef *>(name); head.hcrc = 1; head.os = 3;
        items.push_back({"FEXTRA + FNAME + FHCRC", cat({gzip_member(a, 6), gzip_member(b, 6, Z_DEFAULT_STRATEGY, 0, &head)}), false});
    }
    {
        Bytes g = gzip_member(c, 6);
        for (int i = 0; i < 300; i++) g.push_back((uint8_t)(rng() | 1));
        items.push_back({"trailing garbage", g, false});
    }
    {
        Bytes run(600000, (uint8_t)'A');
        items.push_back({"a run (more than 8 symbols a byte)", gzip_member(run, 9), false});
    }

    uint64_t n_decodes = 0, n_chunks = 0, n_still = 0, n_refused = 0, n_found = 0;
    uint32_t n_overflowed = 0;
    for (const Item &it : items) {
        Bytes want;
        std::vector<uint64_t> all, before;
        if (!zlib_gzip(it.file, &want, &all, &before) || all.empty()) { fail(it.name + ": zlib refuses the item"); continue; }
        const std::vector<uint64_t> starts(all.begin() + 1, all.end());       // (chunk 0 starts at the file's first member header)
        std::vector<uint64_t> third;
        for (size_t i = 0; i < starts.size(); i += 3) third.push_back(starts[i]);
        int v = 0;
        const std::vector<uint64_t> none;
        const std::vector<uint64_t> *cuts[3] = {&starts, &third, &none};
        for (const std::vector<uint64_t> *cut : cuts) {
            const std::vector<uint64_t> &s = *cut;
            Bytes got;
            const uint32_t rc = core_gzip(it.file, s, &got, nullptr, &n_overflowed);
            n_decodes++; n_chunks += s.size() + 1;
            if (rc != DFL_OK) fail(it.name + " (cut " + std::to_string(v) + "): " + dfl_reason(rc));
            else if (got != want) fail(it.name + " (cut " + std::to_string(v) + "): the text differs");
            v++;
        }
        // ---- mutants: what zlib yields, or a refusal -------------------------------------------------------------------------------
        for (int k = 0; k < n_mutants; k++) {
            Bytes f = it.file;
            std::vector<uint64_t> s = k & 1 ? third : starts;
            std::string what;
            switch (k % 6) {
                case 0: { const size_t p = rng() % (f.size() * 8); f[p >> 3] ^= (uint8_t)(1u << (p & 7)); what = "bit " + std::to_string(p) + " flipped"; break; }
                case 1: { const size_t p = 4 + rng() % 6; f[p] ^= (uint8_t)(1u << (rng() & 7)); what = "header byte " + std::to_string(p) + " changed"; break; }   // MTIME, XFL, OS
                case 2: { f.resize(rng() % f.size()); while (!s.empty() && (s.back() + 7) / 8 >= f.size()) s.pop_back(); what = "cut to " + std::to_string(f.size()) + " bytes"; break; }
                case 3: { if (s.empty()) continue; const size_t i = rng() % s.size(); s[i] += (rng() & 1) ? 1 : -1; what = "start " + std::to_string(i) + " moved by a bit"; break; }
                case 4: { const size_t p = f.size() - 1 - rng() % 8; f[p] ^= (uint8_t)(1u << (rng() & 7)); what = "trailer byte changed"; break; }
                default: { const size_t p = f.size() - 1 - rng() % std::min<size_t>(f.size(), 4000); f[p] ^= 0x10; what = "a late bit flipped"; break; }
            }
            Bytes zt, got;
            const bool zok = zlib_gzip(f, &zt);
            const uint32_t rc = core_gzip(f, s, &got);
            if (rc == DFL_OK) {
                n_still++;
                if (!zok) fail(it.name + ", " + what + ": accepted, zlib refuses");
                else if (got != zt) fail(it.name + ", " + what + ": accepted with another text than zlib's");
            } else n_refused++;
        }
        // ---- the header search ------------------------------------------------------------------------------------------------------
        if (it.text_item) {
            for (uint64_t from = 0; from + 65536 <= it.file.size(); from += 65536) {
                size_t k = 0;
                while (k < all.size() && (all[k] < from * 8 || !mdbg_host::gzip_is_dynamic_nonfinal(it.file.data(), it.file.size(), all[k]))) k++;
                if (k == all.size() || all[k] / 8 + 65536 > it.file.size() || all[k] >= (from + 65536) * 8) continue;
                const uint64_t found = mdbg_host::gzip_find_block(it.file.data(), it.file.size(), from * 8, (from + 65536) * 8);
                if (found != all[k]) fail(it.name + ": gzip_find_block from byte " + std::to_string(from) + " gives bit " + std::to_string(found) + ", the first header is at " + std::to_string(all[k]));
                else n_found++;
            }
        }
    }
    if (!n_overflowed) fail("no chunk overflowed 8 symbols a byte");
    if (!n_still || !n_refused) fail("the mutants exercise one side only");
    if (!n_found) fail("no header search was checked");
    if (failures) { fprintf(stderr, "%d failure(s)\n", failures); return 1; }
    printf("ok %zu items, %llu decodes of %llu chunks, %llu mutants (%llu still inflate, %llu refused), %llu header searches\n", items.size(), (unsigned long long)n_decodes,
           (unsigned long long)n_chunks, (unsigned long long)(n_still + n_refused), (unsigned long long)n_still, (unsigned long long)n_refused, (unsigned long long)n_found);
    return 0;
}
