// deflate_core.hpp -- the serial core of the device's DEFLATE decoder (RFC 1951): bit reader, code-length decoding, table construction,
// symbol decoder and the CRC-32 arithmetic, as plain inline functions over caller-supplied arrays.  inflate.hip runs them on lane 0 of
// a wave over arrays in LDS; tests/host/test_deflate_core.cpp compiles the same text with g++ under the address and undefined-behaviour
// sanitizers and compares it with zlib, so every read and write of the decoder has been bounds-checked on a CPU.
//
// One gzip member of a BGZF file (at most 64 KB of text, the window is the member) is decoded in STEPS.  A step either reads one deflate
// block header (stored: the copy is handed to the caller; fixed / dynamic: the tables are built) or decodes up to DFL_TOKENS tokens -- a
// literal or a (length, distance) pair -- which the caller resolves into text.  A step reads its input from a WINDOW of DFL_WIN payload
// bytes that the caller keeps filled (dfl_window_stale / dfl_fill_lane); a step needs at most DFL_NEED of them.
//
// Bounds: the bit reader yields zeros beyond the payload and every step ends by checking that no bit beyond it was consumed
// (DFL_E_INPUT); a window index is checked against DFL_WIN, a table index against the table's size; a token is only emitted when its
// output lies inside [0, isize) and its distance inside the text produced so far.  No loop runs longer than a constant or a
// count read from a checked header.
//
// A chunk of an ordinary gzip file (gzip.hip; tests/host/test_gzip_core.cpp) is decoded by the same parts behind another step function:
// gz_step, further down.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define DFL_HD __host__ __device__ __forceinline__
#else
#define DFL_HD inline
#endif

constexpr uint32_t DFL_WIN = 2048;        // payload bytes in the window
constexpr uint32_t DFL_NEED = 640;        // a step consumes fewer: a dynamic header is at most 17 + 19 * 3 + 316 * 14 bits = 563 bytes,
                                          // DFL_TOKENS tokens at most 64 * 48 bits = 384 bytes (+ 8 of look-ahead)
constexpr uint32_t DFL_TOKENS = 64;       // tokens per step: one per lane of the wave that resolves them
constexpr uint32_t DFL_LIT_ROOT = 9, DFL_DIST_ROOT = 6;       // index bits of the direct tables (longer codes: canonical walk)
constexpr uint32_t DFL_LIT_CAP = 288, DFL_DIST_CAP = 32;
constexpr uint32_t DFL_LENS = 352;        // scratch: 288 + 32 code lengths, then the 19 of the code-length code at [320, 339)
constexpr uint32_t DFL_MAX_ISIZE = 65536, DFL_MAX_CSIZE = 65536;      // a BGZF member is at most 64 KB, headers included
constexpr uint32_t DFL_TOK_MATCH = 0x80000000u;               // token: a literal's byte, or this | length << 16 | distance

enum { DFL_OK = 0, DFL_E_TYPE = 1, DFL_E_STORED = 2, DFL_E_CODE = 3, DFL_E_SYMBOL = 4, DFL_E_DIST = 5, DFL_E_INPUT = 6, DFL_E_SIZE = 7, DFL_E_CRC = 8,
       // a chunk of an ordinary gzip file (gz_step)
       GZ_E_PAST = 9, GZ_E_BACKREF = 10, GZ_E_HEADER = 11, GZ_E_ISIZE = 12, GZ_E_OVERFLOW = 13, GZ_E_STOP = 14, GZ_E_BORDERS = 15 };
enum { DFL_ACT_NONE = 0, DFL_ACT_TOKENS = 1, DFL_ACT_STORED = 2 };

inline const char *dfl_reason(uint32_t e) {
    switch (e) {
        case DFL_E_TYPE: return "reserved block type";
        case DFL_E_STORED: return "stored LEN/NLEN mismatch";
        case DFL_E_CODE: return "over-subscribed or unusably incomplete code";
        case DFL_E_SYMBOL: return "invalid symbol";
        case DFL_E_DIST: return "distance beyond the block's own output";
        case DFL_E_INPUT: return "input exhausted";
        case DFL_E_SIZE: return "output not equal to isize";
        case DFL_E_CRC: return "CRC-32 mismatch";
        case GZ_E_PAST: return "ran past the next chunk's start";
        case GZ_E_BACKREF: return "reference before the member's start";
        case GZ_E_HEADER: return "bad member header";
        case GZ_E_ISIZE: return "length does not match ISIZE";
        case GZ_E_OVERFLOW: return "more symbols than the format allows";
        case GZ_E_STOP: return "the stream ended in front of the chunk's stop";
        case GZ_E_BORDERS: return "more members than the chunk's bytes can hold";
        default: return "unknown status";
    }
}

// ---- bit input ---------------------------------------------------------------------------------------------------------------------
struct dfl_bits {
    const uint8_t *win;       // win[i] is payload byte wbase + i, i < DFL_WIN
    uint32_t wbase, end;      // end: the payload's size
    uint64_t pos;             // next payload byte to fetch (runs past `end` by the few zero bytes the look-ahead fetched)
    uint64_t buf;
    uint32_t cnt, fault;      // fault: a fetch outside the window (the caller did not keep it filled)
};
DFL_HD uint32_t dfl_fetch(dfl_bits &b) {
    uint32_t v = 0;
    if (b.pos < b.end) {
        const uint64_t i = b.pos - b.wbase;
        if (i < DFL_WIN) v = b.win[i]; else b.fault = 1;
    }
    b.pos++;
    return v;
}
DFL_HD void dfl_need(dfl_bits &b, uint32_t n /* <= 32 */) {
    for (int i = 0; i < 4 && b.cnt < n; i++) { b.buf |= (uint64_t)dfl_fetch(b) << b.cnt; b.cnt += 8; }
}
DFL_HD void dfl_drop(dfl_bits &b, uint32_t n) { b.buf >>= n; b.cnt -= n; }            // n <= cnt
DFL_HD uint32_t dfl_peek(dfl_bits &b, uint32_t n /* < 32 */) { dfl_need(b, n); return (uint32_t)b.buf & ((1u << n) - 1u); }
DFL_HD uint32_t dfl_take(dfl_bits &b, uint32_t n /* < 32 */) { const uint32_t v = dfl_peek(b, n); dfl_drop(b, n); return v; }
DFL_HD uint64_t dfl_bitpos(const dfl_bits &b) { return b.pos * 8 - b.cnt; }
DFL_HD void dfl_seed(dfl_bits &b, const uint8_t *win, uint32_t wbase, uint32_t end, uint64_t bitpos) {
    b.win = win; b.wbase = wbase; b.end = end; b.pos = bitpos >> 3; b.buf = 0; b.cnt = 0; b.fault = 0;
    const uint32_t r = (uint32_t)(bitpos & 7u);
    if (r) { b.buf = dfl_fetch(b) >> r; b.cnt = 8 - r; }
}

// ---- the window --------------------------------------------------------------------------------------------------------------------
// true: the window must be filled again at dfl_window_base() before the next step
DFL_HD bool dfl_window_stale(uint64_t bitpos, uint32_t wbase, uint32_t csize, bool filled) {
    const uint64_t p = bitpos >> 3;
    if (!filled || p < wbase) return true;
    return p + DFL_NEED > (uint64_t)wbase + DFL_WIN && (uint64_t)wbase + DFL_WIN < csize;
}
// the window starts at the byte the reader stands in, moved back so that payload + base is 4-byte aligned where that is possible
DFL_HD uint32_t dfl_window_base(const uint8_t *payload, uint64_t bitpos, uint32_t csize) {
    uint64_t p = bitpos >> 3;
    if (p > csize) p = csize;
    const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(payload) + p) & 3u);
    return (uint32_t)(p >= mis ? p - mis : p);
}
// lane `lane` of 64 fills its 8 words of the window; no byte outside [payload, payload + csize) is read (zeros stand in)
DFL_HD void dfl_fill_lane(uint32_t *win32, const uint8_t *payload, uint32_t csize, uint32_t wbase, uint32_t lane) {
    for (uint32_t j = 0; j < DFL_WIN / 256; j++) {
        const uint32_t w = j * 64u + (lane & 63u);                   // < DFL_WIN / 4
        const uint64_t at = (uint64_t)wbase + 4ull * w;
        uint32_t v = 0;
        if (at + 4 <= csize && ((reinterpret_cast<uintptr_t>(payload) + at) & 3u) == 0) {
            v = *reinterpret_cast<const uint32_t *>(payload + at);
        } else {
            for (uint32_t k = 0; k < 4; k++)
                if (at + k < csize) v |= (uint32_t)payload[at + k] << (8 * k);
        }
        win32[w] = v;
    }
}

// ---- codes -------------------------------------------------------------------------------------------------------------------------
// A canonical Huffman code as counts per length and the symbols in code order (the walk of zlib's contrib/puff), with a direct table
// over the first `root` stream bits for the codes that fit them: entry = length << 9 | symbol, 0 = none.
struct dfl_code {
    uint16_t *count;          // [32]: codes per length, then (while the code is built) where each length's symbols start
    uint16_t *sym;            // [cap]
    uint16_t *fast;           // [1 << root]
    uint32_t root, cap;
};
// 0 = usable.  Accepted are complete codes and, with allow_single, no code at all or a single code of length 1 (host/inflate.hpp
// build_table; zlib's inflate_table draws the same line).  Everything else -- over-subscribed, otherwise incomplete -- is refused.
DFL_HD int dfl_build(const dfl_code &c, const uint8_t *lens, uint32_t n, bool allow_single) {
    if (n > c.cap) return -1;
    for (uint32_t l = 0; l < 16; l++) c.count[l] = 0;
    for (uint32_t i = 0; i < (1u << c.root); i++) c.fast[i] = 0;
    for (uint32_t s = 0; s < n; s++) c.count[lens[s] & 15u]++;
    c.count[0] = 0;
    uint32_t maxlen = 15;
    while (maxlen > 0 && !c.count[maxlen]) maxlen--;
    if (maxlen == 0) return allow_single ? 0 : -1;               // no codes: every look-up fails
    int left = 1;
    for (uint32_t l = 1; l <= 15; l++) {
        left = (left << 1) - (int)c.count[l];
        if (left < 0) return -1;
    }
    if (left > 0 && !(allow_single && maxlen == 1)) return -1;
    uint16_t *offs = c.count + 16;
    offs[0] = 0; offs[1] = 0;
    for (uint32_t l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + c.count[l]);
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t l = lens[s] & 15u;
        if (!l) continue;
        const uint32_t i = offs[l]++;
        if (i < c.cap) c.sym[i] = (uint16_t)s;
    }
    uint32_t code = 0, idx = 0;
    for (uint32_t l = 1; l <= c.root; l++) {
        for (uint32_t k = 0; k < c.count[l]; k++, idx++, code++) {
            if (idx >= c.cap) return -1;
            uint32_t rev = 0;                                     // codes are packed from their most significant bit
            for (uint32_t i = 0; i < l; i++) rev |= ((code >> i) & 1u) << (l - 1 - i);
            const uint16_t e = (uint16_t)((l << 9) | c.sym[idx]);
            for (uint32_t i = rev; i < (1u << c.root); i += 1u << l) c.fast[i] = e;
        }
        code <<= 1;
    }
    return 0;
}
// the next symbol, or -1 when the bits are no code
DFL_HD int dfl_sym(dfl_bits &b, const dfl_code &c) {
    uint32_t v = dfl_peek(b, 15);
    const uint32_t e = c.fast[v & ((1u << c.root) - 1u)];
    if (e) { dfl_drop(b, e >> 9); return (int)(e & 511u); }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= 15; l++) {
        code |= v & 1u;
        v >>= 1;
        const uint32_t cnt = c.count[l];
        if (code >= first && code - first < cnt) {
            const uint32_t i = index + (code - first);
            dfl_drop(b, l);
            return i < c.cap ? (int)c.sym[i] : -1;
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

// ---- one member --------------------------------------------------------------------------------------------------------------------
struct dfl_mem {              // the caller's arrays (LDS on the device)
    uint8_t *win;             // [DFL_WIN], 4-byte aligned
    uint16_t *lit_count, *lit_sym, *lit_fast;        // [32], [DFL_LIT_CAP], [1 << DFL_LIT_ROOT]
    uint16_t *dist_count, *dist_sym, *dist_fast;     // [32], [DFL_DIST_CAP], [1 << DFL_DIST_ROOT]
    uint8_t *lens;            // [DFL_LENS]
    uint32_t *tok;            // [DFL_TOKENS]
};
struct dfl_state {
    uint64_t bitpos;          // of the payload, in front of the next step
    uint32_t csize, isize;
    uint32_t out;             // text bytes accounted for
    uint32_t wbase, filled;   // the window
    uint32_t in_block, final, err;
    // what the last step asks of the caller
    uint32_t act;
    uint32_t out0;            // DFL_ACT_TOKENS / DFL_ACT_STORED: the text offset the step's output starts at
    uint32_t n_tok;           // DFL_ACT_TOKENS: tokens in mem.tok
    uint32_t stored_at, stored_len;   // DFL_ACT_STORED: payload bytes [stored_at, +stored_len) are the text at out0
};
DFL_HD void dfl_begin(dfl_state &st, uint32_t csize, uint32_t isize) {
    st.bitpos = 0; st.csize = csize; st.isize = isize; st.out = 0; st.wbase = 0; st.filled = 0;
    st.in_block = 0; st.final = 0; st.err = DFL_OK; st.act = DFL_ACT_NONE; st.out0 = 0; st.n_tok = 0; st.stored_at = 0; st.stored_len = 0;
}
DFL_HD bool dfl_finished(const dfl_state &st) { return st.err != DFL_OK || (st.final && !st.in_block); }
// steps that decode a member at most: every step consumes a bit
DFL_HD uint64_t dfl_max_steps(uint32_t csize) { return (uint64_t)csize * 8 + 1; }

DFL_HD dfl_code dfl_lit_code(const dfl_mem &m) { dfl_code c; c.count = m.lit_count; c.sym = m.lit_sym; c.fast = m.lit_fast; c.root = DFL_LIT_ROOT; c.cap = DFL_LIT_CAP; return c; }
DFL_HD dfl_code dfl_dist_code(const dfl_mem &m) { dfl_code c; c.count = m.dist_count; c.sym = m.dist_sym; c.fast = m.dist_fast; c.root = DFL_DIST_ROOT; c.cap = DFL_DIST_CAP; return c; }

DFL_HD uint32_t dfl_fixed_tables(const dfl_mem &m) {
    for (uint32_t i = 0; i < 288; i++) m.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (uint32_t i = 0; i < 32; i++) m.lens[288 + i] = 5;
    if (dfl_build(dfl_lit_code(m), m.lens, 288, false)) return DFL_E_CODE;
    if (dfl_build(dfl_dist_code(m), m.lens + 288, 32, false)) return DFL_E_CODE;
    return DFL_OK;
}
// the header of a dynamic block behind its three type bits
DFL_HD uint32_t dfl_dynamic_tables(dfl_bits &b, const dfl_mem &m) {
    const uint32_t hlit = dfl_take(b, 5) + 257, hdist = dfl_take(b, 5) + 1, hclen = dfl_take(b, 4) + 4;
    if (hlit > 286 || hdist > 30) return DFL_E_CODE;
    // 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15, five bits each
    const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                              11ull << 50 | 4ull << 55;
    const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    uint8_t *cl = m.lens + 320;
    for (uint32_t i = 0; i < 19; i++) cl[i] = 0;
    for (uint32_t i = 0; i < hclen; i++) {                        // hclen <= 19
        const uint32_t s = (uint32_t)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31u);
        cl[s < 19 ? s : 0] = (uint8_t)dfl_take(b, 3);
    }
    // the code-length code lives in the distance code's arrays until the lengths are read
    const dfl_code cc = dfl_dist_code(m);
    if (dfl_build(cc, cl, 19, false)) return DFL_E_CODE;
    const uint32_t total = hlit + hdist;                          // <= 316
    uint32_t n = 0;
    for (uint32_t guard = 0; n < total && guard < total; guard++) {       // every pass adds at least one entry
        const int s = dfl_sym(b, cc);
        if (s < 0 || s > 18) return DFL_E_CODE;
        if (s < 16) { m.lens[n++] = (uint8_t)s; continue; }
        uint32_t rep, val = 0;
        if (s == 16) {
            if (n == 0) return DFL_E_CODE;
            val = m.lens[n - 1];
            rep = 3 + dfl_take(b, 2);
        } else if (s == 17) rep = 3 + dfl_take(b, 3);
        else rep = 11 + dfl_take(b, 7);
        if (n + rep > total) return DFL_E_CODE;
        for (uint32_t k = 0; k < rep; k++) m.lens[n++] = (uint8_t)val;
    }
    if (n < total) return DFL_E_CODE;
    if (m.lens[256] == 0) return DFL_E_CODE;                      // no end-of-block code
    if (dfl_build(dfl_lit_code(m), m.lens, hlit, true)) return DFL_E_CODE;
    if (dfl_build(dfl_dist_code(m), m.lens + hlit, hdist, true)) return DFL_E_CODE;
    return DFL_OK;
}

// Up to DFL_TOKENS tokens of the open block into m.tok.  `pos` is the output position (advanced), `limit` the output's bound
// (beyond it: DFL_E_SIZE); a distance may be at most `maxd` (DFL_E_DIST) and may reach back to position `lo` at the lowest (`e_lo`).
// The end-of-block code clears in_block.
DFL_HD uint32_t dfl_tokens(dfl_bits &b, const dfl_mem &m, uint32_t &pos, uint32_t limit, uint32_t maxd, int64_t lo, uint32_t e_lo, uint32_t &n,
                           uint32_t &in_block) {
    const dfl_code lit = dfl_lit_code(m), dist = dfl_dist_code(m);
    while (n < DFL_TOKENS) {
        const int s = dfl_sym(b, lit);
        if (s < 0 || s > 285) return DFL_E_SYMBOL;
        if (s < 256) {
            if (pos >= limit) return DFL_E_SIZE;
            m.tok[n++] = (uint32_t)s;
            pos++;
            continue;
        }
        if (s == 256) { in_block = 0; break; }
        const uint32_t i = (uint32_t)s - 257u;                 // 0 .. 28
        uint32_t len;
        if (i < 8) len = 3 + i;
        else if (i == 28) len = 258;
        else { const uint32_t x = (i >> 2) - 1; len = 3 + ((4 + (i & 3u)) << x) + dfl_take(b, x); }
        const int d = dfl_sym(b, dist);
        if (d < 0 || d > 29) return DFL_E_SYMBOL;
        uint32_t off;
        if (d < 4) off = 1 + (uint32_t)d;
        else { const uint32_t x = ((uint32_t)d >> 1) - 1; off = 1 + ((2 + ((uint32_t)d & 1u)) << x) + dfl_take(b, x); }
        if (off > maxd) return DFL_E_DIST;
        if ((int64_t)pos - (int64_t)off < lo) return e_lo;
        if ((uint64_t)pos + len > limit) return DFL_E_SIZE;
        m.tok[n++] = DFL_TOK_MATCH | (len << 16) | off;
        pos += len;
    }
    return DFL_OK;
}

// One step.  The window must hold the payload from (bitpos >> 3) on for DFL_NEED bytes or up to its end.
DFL_HD void dfl_step(dfl_state &st, const dfl_mem &m) {
    dfl_bits b;
    dfl_seed(b, m.win, st.wbase, st.csize, st.bitpos);
    st.act = DFL_ACT_NONE;
    st.n_tok = 0;
    st.out0 = st.out;
    uint32_t err = DFL_OK;
    bool stored = false;
    if (!st.in_block) {
        st.final = dfl_take(b, 1);
        const uint32_t type = dfl_take(b, 2);
        if (type == 0) {
            dfl_drop(b, b.cnt & 7u);
            const uint32_t len = dfl_take(b, 16), nlen = dfl_take(b, 16);
            const uint64_t at = dfl_bitpos(b) >> 3;               // whole bytes here
            if (dfl_bitpos(b) > (uint64_t)st.csize * 8 || b.fault) err = DFL_E_INPUT;
            else if ((len ^ 0xFFFFu) != nlen) err = DFL_E_STORED;
            else if (at + len > st.csize) err = DFL_E_INPUT;
            else if ((uint64_t)st.out + len > st.isize) err = DFL_E_SIZE;
            else {
                stored = true;
                st.act = DFL_ACT_STORED;
                st.stored_at = (uint32_t)at;
                st.stored_len = len;
                st.out += len;
                st.bitpos = (at + len) * 8;
            }
        } else if (type == 1) {
            err = dfl_fixed_tables(m);
            st.in_block = 1;
        } else if (type == 2) {
            err = dfl_dynamic_tables(b, m);
            st.in_block = 1;
        } else err = DFL_E_TYPE;
    } else {
        uint32_t pos = st.out, n = 0;
        err = dfl_tokens(b, m, pos, st.isize, 0xFFFFFFFFu, 0, DFL_E_DIST, n, st.in_block);
        st.n_tok = n;
        st.out = pos;
        st.act = DFL_ACT_TOKENS;
    }
    // bits that do not exist were read as zeros: whatever they decoded to, the input ended first
    if (!stored && (dfl_bitpos(b) > (uint64_t)st.csize * 8 || b.fault)) err = DFL_E_INPUT;
    if (err != DFL_OK) { st.err = err; st.act = DFL_ACT_NONE; st.n_tok = 0; return; }
    if (!stored) st.bitpos = dfl_bitpos(b);
}

// ---- a chunk of an ordinary gzip file ------------------------------------------------------------------------------------------------
// The two-pass scheme of host/gzip_parallel.hpp: a chunk is bits [start, stop) of the file, it starts at a deflate block header (or at a
// gzip member header) and is decoded WITHOUT the 32 KB in front of it into 16-bit symbols -- a byte, or GZ_MARK + p for "byte p of the
// unknown 32 KB in front of the chunk".  The steps are those of a BGZF member plus three: a member header (RFC 1952: magic, CM = 8,
// FEXTRA / FNAME / FCOMMENT / FHCRC by its flags), the rest of a long header, and a member trailer, after which the caller notes a
// BORDER (symbol position, CRC-32, ISIZE) and the next member's header follows or the stream ends (what is no header is ignored, as
// gzread does).  Behind a border no distance reaches in front of it.  After every block: the reader stands on `stop` (the chunk is
// done), or beyond it (GZ_E_PAST: `stop`, the next chunk's start, was no block header).
//
// Bounds, as above: the payload is [0, csize) bytes and bits beyond it read as zeros and fail the step; an output position is checked
// against `cap`; every step consumes at least one bit (a header step 80, a trailer step 64, a step of a long header at least 8), so
// gz_max_steps bounds the loop.
constexpr uint32_t GZ_MARK = 0x8000u, GZ_REACH = 32768u;
constexpr uint64_t GZ_TO_END = ~0ull;
constexpr uint32_t GZ_MAX_SPAN = 1u << 21;                     // bytes of a chunk: 1032 symbols a byte stay below 2^32
enum { GZ_PH_HEADER = 0, GZ_PH_HEADER_REST = 1, GZ_PH_BLOCK = 2, GZ_PH_TRAILER = 3, GZ_PH_DONE = 4 };
enum { GZ_ACT_BORDER = 3 };
enum { GZ_END_STOP = 0, GZ_END_BORDER = 1, GZ_END_STREAM = 2 };     // how a chunk ended: on its stop inside a member, on its stop behind a trailer, with the file's last member
struct gz_state {
    uint64_t bitpos, stop;    // bits of the payload; stop: GZ_TO_END = through the end of the last member
    int64_t lo;               // the lowest symbol position a distance may reach: -reach0 at first, the last border's position behind one
    uint32_t csize, cap, out, wbase, filled, in_block, final, err;
    uint32_t phase, hflags, skip, hcrc, ended, n_borders;
    uint32_t act, out0, n_tok, stored_at, stored_len;
    uint32_t border_crc, border_isize;    // GZ_ACT_BORDER: a member ended at symbol position out0 with this trailer
};
DFL_HD void gz_begin(gz_state &st, uint32_t start_bit /* < 8 */, uint64_t stop, uint32_t csize, uint32_t cap, uint32_t reach0, bool at_header) {
    st.bitpos = start_bit; st.stop = stop; st.lo = -(int64_t)(reach0 < GZ_REACH ? reach0 : GZ_REACH); st.csize = csize; st.cap = cap; st.out = 0;
    st.wbase = 0; st.filled = 0; st.in_block = 0; st.final = 0; st.err = DFL_OK; st.phase = at_header ? GZ_PH_HEADER : GZ_PH_BLOCK; st.hflags = 0; st.skip = 0; st.hcrc = 0;
    st.ended = GZ_END_STOP; st.n_borders = 0; st.act = DFL_ACT_NONE; st.out0 = 0; st.n_tok = 0; st.stored_at = 0; st.stored_len = 0; st.border_crc = 0; st.border_isize = 0;
}
DFL_HD bool gz_finished(const gz_state &st) { return st.err != DFL_OK || st.phase == GZ_PH_DONE; }
DFL_HD uint64_t gz_max_steps(uint32_t csize) { return (uint64_t)csize * 8 + 2; }
// symbols a chunk of `csize` bytes holds at the most: a match of 258 costs two bits at the least (1032 a byte), and a last one may begin in the last bit
DFL_HD uint64_t gz_max_symbols(uint32_t csize) { return (uint64_t)csize * 1032 + 258; }

// the CRC-32 register over a header byte (no table: a header is a few bytes)
DFL_HD uint32_t gz_hcrc(uint32_t reg, uint32_t byte) {
    uint32_t c = (reg ^ byte) & 255u;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    return c ^ (reg >> 8);
}
// a block ended at st.bitpos
DFL_HD void gz_block_end(gz_state &st) {
    if (st.final) { st.phase = GZ_PH_TRAILER; return; }
    if (st.stop == GZ_TO_END || st.bitpos < st.stop) return;
    if (st.bitpos == st.stop) st.phase = GZ_PH_DONE; else st.err = GZ_E_PAST;
}

DFL_HD void gz_step(gz_state &st, const dfl_mem &m) {
    dfl_bits b;
    dfl_seed(b, m.win, st.wbase, st.csize, st.bitpos);
    st.act = DFL_ACT_NONE;
    st.n_tok = 0;
    st.out0 = st.out;
    uint32_t err = DFL_OK;
    bool jumped = false;      // the step set st.bitpos itself
    bool boundary = false;    // the step ends where a block header is due
    if (st.phase == GZ_PH_HEADER) {
        uint32_t h[10];
        st.hcrc = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < 10; i++) { h[i] = dfl_take(b, 8); st.hcrc = gz_hcrc(st.hcrc, h[i]); }
        if ((st.bitpos & 7u) || h[0] != 0x1Fu || h[1] != 0x8Bu || h[2] != 8u || (h[3] & 0xE0u)) err = GZ_E_HEADER;
        else {
            st.hflags = h[3] & (4u | 8u | 16u | 2u);
            st.skip = 0;
            if (st.hflags & 4u) {
                const uint32_t x0 = dfl_take(b, 8), x1 = dfl_take(b, 8);
                st.hcrc = gz_hcrc(gz_hcrc(st.hcrc, x0), x1);
                st.skip = x0 | x1 << 8;
                if (!st.skip) st.hflags &= ~4u;
            }
            st.phase = st.hflags ? GZ_PH_HEADER_REST : GZ_PH_BLOCK;
            st.final = 0; st.in_block = 0;
            boundary = !st.hflags;
        }
    } else if (st.phase == GZ_PH_HEADER_REST) {                    // at most 256 bytes a step, at least one
        if (st.hflags & 4u) {                                      // FEXTRA: st.skip bytes
            for (uint32_t i = 0; i < 256 && st.skip; i++, st.skip--) st.hcrc = gz_hcrc(st.hcrc, dfl_take(b, 8));
            if (!st.skip) st.hflags &= ~4u;
        } else if (st.hflags & (8u | 16u)) {                       // FNAME, then FCOMMENT: up to their zero byte
            const uint32_t flag = (st.hflags & 8u) ? 8u : 16u;
            for (uint32_t i = 0; i < 256; i++) {
                if ((dfl_bitpos(b) >> 3) >= st.csize) { err = DFL_E_INPUT; break; }
                const uint32_t c = dfl_take(b, 8);
                st.hcrc = gz_hcrc(st.hcrc, c);
                if (c == 0) { st.hflags &= ~flag; break; }
            }
        } else if (st.hflags & 2u) {                               // FHCRC: the low half of the header's CRC-32
            if (dfl_take(b, 16) != ((st.hcrc ^ 0xFFFFFFFFu) & 0xFFFFu)) err = GZ_E_HEADER;
            st.hflags &= ~2u;
        }
        if (!st.hflags) { st.phase = GZ_PH_BLOCK; boundary = true; }
    } else if (st.phase == GZ_PH_TRAILER) {
        dfl_drop(b, b.cnt & 7u);
        const uint32_t c0 = dfl_take(b, 16), c1 = dfl_take(b, 16), i0 = dfl_take(b, 16), i1 = dfl_take(b, 16);
        const uint64_t at = dfl_bitpos(b) >> 3;
        if (at > st.csize || b.fault) err = st.stop == GZ_TO_END ? DFL_E_INPUT : GZ_E_PAST;
        else {
            st.act = GZ_ACT_BORDER;
            st.border_crc = c0 | c1 << 16; st.border_isize = i0 | i1 << 16;
            st.n_borders++;
            st.lo = st.out;
            st.final = 0;
            if (st.stop != GZ_TO_END && at * 8 >= st.stop) {
                if (at * 8 == st.stop) { st.phase = GZ_PH_DONE; st.ended = GZ_END_BORDER; } else err = GZ_E_PAST;
            } else if (at + 2 <= st.csize && dfl_peek(b, 16) == 0x8B1Fu) st.phase = GZ_PH_HEADER;
            else if (st.stop != GZ_TO_END) err = GZ_E_STOP;
            else { st.phase = GZ_PH_DONE; st.ended = GZ_END_STREAM; }
            st.bitpos = at * 8; jumped = true;
        }
    } else if (st.phase == GZ_PH_BLOCK && !st.in_block) {
        st.final = dfl_take(b, 1);
        const uint32_t type = dfl_take(b, 2);
        if (type == 0) {
            dfl_drop(b, b.cnt & 7u);
            const uint32_t len = dfl_take(b, 16), nlen = dfl_take(b, 16);
            const uint64_t at = dfl_bitpos(b) >> 3;
            if (at > st.csize || b.fault) err = st.stop == GZ_TO_END ? DFL_E_INPUT : GZ_E_PAST;
            else if ((len ^ 0xFFFFu) != nlen) err = DFL_E_STORED;
            else if (at + len > st.csize) err = st.stop == GZ_TO_END ? DFL_E_INPUT : GZ_E_PAST;
            else if ((uint64_t)st.out + len > st.cap) err = GZ_E_OVERFLOW;
            else {
                jumped = true;
                st.act = DFL_ACT_STORED;
                st.stored_at = (uint32_t)at;
                st.stored_len = len;
                st.out += len;
                st.bitpos = (at + len) * 8;
                boundary = true;
            }
        } else if (type == 1) {
            err = dfl_fixed_tables(m);
            st.in_block = 1;
        } else if (type == 2) {
            err = dfl_dynamic_tables(b, m);
            st.in_block = 1;
        } else err = DFL_E_TYPE;
    } else if (st.phase == GZ_PH_BLOCK) {
        uint32_t pos = st.out, n = 0;
        err = dfl_tokens(b, m, pos, st.cap, GZ_REACH, st.lo, GZ_E_BACKREF, n, st.in_block);
        if (err == DFL_E_SIZE) err = GZ_E_OVERFLOW;
        st.n_tok = n;
        st.out = pos;
        st.act = DFL_ACT_TOKENS;
    } else err = DFL_E_INPUT;                                      // (no step is asked of a finished chunk)
    // bits that do not exist were read as zeros: whatever they decoded to, the input ended first (a chunk's input ends with its stop)
    if (!jumped && (dfl_bitpos(b) > (uint64_t)st.csize * 8 || b.fault)) err = st.stop == GZ_TO_END ? DFL_E_INPUT : GZ_E_PAST;
    if (err != DFL_OK) { st.err = err; st.act = DFL_ACT_NONE; st.n_tok = 0; return; }
    if (!jumped) st.bitpos = dfl_bitpos(b);
    if (st.act == DFL_ACT_TOKENS && !st.in_block) boundary = true;
    if (boundary) {
        gz_block_end(st);
        if (st.err != DFL_OK) { st.act = DFL_ACT_NONE; st.n_tok = 0; }
    }
}

// ---- CRC-32 (gzip: polynomial 0xEDB88320 reflected) --------------------------------------------------------------------------------
// The register after a piece is linear in the register before it: after n bytes, reg = reg0 * x^(8n) + raw(piece) (mod P).  So lanes
// take contiguous pieces -- lane 0 starts from 0xFFFFFFFF, the others from 0 -- and lane i's register, multiplied by x^(8 * bytes
// behind its piece), is its share of the whole; the shares are XORed and the result inverted.
constexpr uint32_t DFL_CRC_POLY = 0xEDB88320u;
DFL_HD uint32_t dfl_crc_table_entry(uint32_t i) {
    uint32_t c = i & 255u;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ DFL_CRC_POLY : c >> 1;
    return c;
}
// a * b mod P; bit 31 is x^0
DFL_HD uint32_t dfl_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        if ((a >> i) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ DFL_CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 n) mod P
DFL_HD uint32_t dfl_crc_xpow8(uint32_t n) {
    uint32_t r = 0x80000000u, sq = 0x00800000u;                   // x^0, x^8
    for (int i = 0; i < 32 && n; i++, n >>= 1) {
        if (n & 1u) r = dfl_crc_mul(r, sq);
        sq = dfl_crc_mul(sq, sq);
    }
    return r;
}
DFL_HD uint32_t dfl_crc_byte(const uint32_t *table /* 256 */, uint32_t reg, uint32_t byte) { return table[(reg ^ byte) & 255u] ^ (reg >> 8); }
