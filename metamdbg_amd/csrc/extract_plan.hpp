// extract_plan.hpp -- what the plans of extract.hip and stitch.hip share: the result handle, the range and the checks of one request
// (a lane's body), the sum of the bases, the step from word offsets to byte offsets and the words of a refusal.
#pragma once
#include "common.hpp"
#include "extract_dev.hpp"
#include "objects.hpp"

struct mdbg_sequences {
    uint64_t n = 0, n_bases = 0, n_bytes = 0;
    int form = 0;
    mdbg::DevBuf<uint64_t> d_off;       // n + 1: byte offsets, multiples of 8
    mdbg::DevBuf<uint32_t> d_len;       // n: bases
    mdbg::DevBuf<uint8_t> d_bytes;      // n_bytes
};

namespace mdbg {

// the fields of the spans a plan reads
struct SpansView {
    const uint64_t *woff; uint64_t n_windows; const uint32_t *len; const uint8_t *rev; const uint32_t *ps, *pe, *ls, *le;
};
inline SpansView spans_view(const mdbg_spans *s) { return SpansView{s->d_woff.p, s->n_windows, s->d_len.p, s->d_rev.p, s->d_ps.p, s->d_pe.p, s->d_ls.p, s->d_le.p}; }

#ifdef __HIPCC__
// A (window, part) request: the window's read by a search over the window offsets, the range by extract_part_range.  0 = fine.
__device__ __forceinline__ uint32_t extract_request_range(uint64_t window, uint32_t part, const SpansView &sp, const uint32_t *read_len, uint32_t n_reads,
                                                          ExtractRange &rg) {
    if (part > EXTRACT_RIGHT) return EXTRACT_BAD_PART;
    if (window >= sp.n_windows) return EXTRACT_BAD_WINDOW;
    rg.read = csr_owner(sp.woff, n_reads, window);
    rg.reversed = sp.rev[window] ? 1u : 0u;
    const uint32_t L = read_len[rg.read];
    if (sp.len[rg.read] != L) return EXTRACT_BAD_READ_LENGTH;
    const uint32_t why = extract_part_range(sp.ps[window], sp.pe[window], sp.ls[window], sp.le[window], rg.reversed != 0u, part, rg.start, rg.length);
    if (!why && (uint64_t)rg.start + rg.length > L) return EXTRACT_BAD_RANGE;
    return why;
}

// a range given by the caller
__device__ __forceinline__ uint32_t extract_given_range(uint32_t read, uint32_t start, uint32_t length, const uint32_t *read_len, uint32_t n_reads) {
    if (read >= n_reads) return EXTRACT_BAD_READ;
    if ((uint64_t)start + length > read_len[read]) return EXTRACT_BAD_RANGE;
    return 0u;
}

// the bases of all requests: a lane's sum over its trips, summed over the wave, one atomic a wave
__device__ __forceinline__ void plan_add_bases(unsigned long long mine, unsigned long long *total) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(total, mine);
}
#endif

// word offsets -> byte offsets, in place (n1 entries), queued on the context's stream
void extract_offsets_to_bytes(mdbg_ctx *ctx, uint64_t *d_off, uint64_t n1);
const char *extract_why_text(uint32_t why);

}  // namespace mdbg
