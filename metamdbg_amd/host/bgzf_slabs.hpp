// bgzf_slabs.hpp -- which blocks of a BGZF file make the next slab of text for the device parse, and where the slab after it begins.
// Arithmetic on the blocks' text offsets alone (cum[b]: the bytes of text in front of block b, cum[nb]: all of it -- a block's isize is
// cum[b + 1] - cum[b]): no library call, no GPU.  The device calls come in as two functions (DeviceTextFeed::next_bgzf_slab).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mdbg_host {

// the next slab begins `begin` bytes into the text of block `block`
struct BgzfCursor { size_t block = 0; uint64_t begin = 0; };

// the cursor moves over empty blocks; false: the file has no block left
inline bool bgzf_skip_empty(const std::vector<uint64_t> &cum, BgzfCursor &c) {
    const size_t nb = cum.size() - 1;
    while (c.block < nb && cum[c.block + 1] == cum[c.block] && c.begin == 0) c.block++;
    return c.block < nb;
}

// The blocks [c.block, b1) of a slab's first attempt: a run of at most batchText bytes of text, one block at the least -- and one block
// more when a cut is pending (the first block is mostly the last slab's).  Returns b1.
inline size_t bgzf_first_run(const std::vector<uint64_t> &cum, const BgzfCursor &c, uint64_t batchText) {
    const size_t nb = cum.size() - 1, b0 = c.block;
    size_t b1 = b0;
    while (b1 < nb && (b1 == b0 || cum[b1 + 1] - cum[b0] <= batchText)) b1++;
    if (c.begin && b1 < nb) b1++;
    return b1;
}

// Not one whole record in [b0, b1), b1 < nb: the run grows to twice its text (64 KB at the least) within batchText, by one block at the
// least.  false: it is larger than batchText already -- a single read is ("raise --batch-bases")
inline bool bgzf_grow_run(const std::vector<uint64_t> &cum, size_t b0, size_t &b1, uint64_t batchText) {
    const size_t nb = cum.size() - 1;
    const uint64_t sum = cum[b1] - cum[b0];
    if (sum > batchText) return false;
    const uint64_t upto = std::max<uint64_t>(2 * sum, 65536);
    do b1++; while (b1 < nb && cum[b1] - cum[b0] < upto && cum[b1 + 1] - cum[b0] <= batchText);
    return true;
}

// the slab of blocks [b0, b1) ends `cut` bytes into its text: the next one begins there -- at a block's edge, or inside the block that
// holds the place (inflated a second time)
inline BgzfCursor bgzf_after_cut(const std::vector<uint64_t> &cum, size_t b0, size_t b1, uint64_t cut) {
    const uint64_t at = cum[b0] + cut;                     // in the file's text
    if (at == cum[b1]) return BgzfCursor{b1, 0};
    const size_t b = (size_t)(std::upper_bound(cum.begin(), cum.end(), at) - cum.begin()) - 1;
    return BgzfCursor{b, at - cum[b]};
}

enum class BgzfNext { NONE, SLAB, READ_TOO_LONG };

// The next slab of the file.  inflate(b0, b1) brings the text of blocks [b0, b1) to offset 0 of the caller's buffer (dropping what an
// earlier attempt left there) and returns its length; whole_records(begin, n) says where the last whole record of [begin, n) of that text ends (begin: none).
// SLAB: [*begin, *end) of the text is to be parsed and the cursor stands where the next slab begins -- all but the file's last slab end
// behind their last whole record, the last one is parsed whole.  NONE: the file has no text left (a buffer may be left to drop).
// READ_TOO_LONG: batchText bytes of text hold no whole record.
template <typename Inflate, typename WholeRecords>
BgzfNext bgzf_next_slab(const std::vector<uint64_t> &cum, BgzfCursor &c, uint64_t batchText, Inflate &&inflate, WholeRecords &&whole_records, uint64_t *begin, uint64_t *end) {
    const size_t nb = cum.size() - 1;
    if (!bgzf_skip_empty(cum, c)) return BgzfNext::NONE;
    const size_t b0 = c.block;
    size_t b1 = bgzf_first_run(cum, c, batchText);
    for (;;) {
        const uint64_t n_text = inflate(b0, b1);           // cum[b1] - cum[b0], as the inflating side counted it
        *begin = c.begin;
        *end = n_text;
        if (b1 == nb) {                                    // the file's last slab is parsed whole
            c = BgzfCursor{nb, 0};
            return *begin < n_text ? BgzfNext::SLAB : BgzfNext::NONE;
        }
        const uint64_t cut = *begin < n_text ? whole_records(*begin, n_text) : *begin;
        if (cut > *begin) {
            *end = cut;
            c = bgzf_after_cut(cum, b0, b1, cut);
            return BgzfNext::SLAB;
        }
        // not one whole record yet: more blocks, up to a batch of them
        if (!bgzf_grow_run(cum, b0, b1, batchText)) return BgzfNext::READ_TOO_LONG;
    }
}

}  // namespace mdbg_host
