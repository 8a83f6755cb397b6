// complexity_dev.hpp -- the 2-mer bound behind the low-complexity filter, for the device and for a host program.
//
// The reference scores a read by the mean, over windows of 64 positions, of sum_v c_v (c_v - 1) / 2 over the 3-mers v of the
// window, and drops it when the mean of score / 61 exceeds 5 (computeSequenceComplexity, ReadSelection.hpp:1171-1228).  The scan
// bounds that from above with the 2-mer counts of single words (scan.hip, "complexity"): with
//     sq(w) = sum over the 16 2-mers v of (count of v among the 32 positions of word w, the last one completed by the first
//             base of word w + 1)^2
// a read is a SUSPECT, to be decided exactly by complexity_exact_kernel, when
//     sum_w weight(w) * sq(w)  >  (300 + 32) * nW,            nW = number of windows, weight(w) = number of windows word w is in.
//
// sq(w) in +-1 (Walsh-Hadamard) form.  Write the 32 positions as four bit planes in "slot" order: L / H = low / high bit of the
// 2-bit code of the base, NL / NH = the same of the base after it.  A position's pair (base, next base) is a point of
// {0,1}^4; c = its 16 counts, and for a mask u in {0,1}^4 the transform  C(u) = sum_v (-1)^(u.v) c_v  is
//     32 - 2 popc(S_a ^ T_b),   u = (a, b),   S = {0, L, H, L ^ H},   T = {0, NL, NH, NL ^ NH}
// (a position adds -1 exactly when the planes selected by u have odd parity there).  Parseval over the 16 masks:
//     sum_v c_v^2 = (1/16) sum_u C(u)^2 = (1/16) (32^2 + 4 sum_{(a,b) != (0,0)} (popc(S_a ^ T_b) - 16)^2) = 64 + Q / 4,
//     Q(w) = sum over the 15 pairs (a,b) != (0,0) of (popc(S_a ^ T_b) - 16)^2.
// No indicator planes, the six pairs with a == 0 or b == 0 need no XOR, and v_bcnt_u32_b32 adds the -16 through its second source:
// 15 x (popcount-add, multiply-add) + 9 XORs + the two XORs S_3, T_3 where the indicator form took 8 planes + 16 x (and,
// popcount, multiply-add).
//
// The decision in Q.  Word w lies in window w (if w < nW) and in window w - 1 (if 1 <= w <= nW): weight 1 for w = 0 and w = nW,
// 2 between, 0 beyond, so the weights of a read sum to exactly 2 nW (nW >= 1).  Then
//     sum_w weight sq = 64 * 2 nW + (1/4) sum_w weight Q  >  332 nW     <=>     sum_w weight Q  >  4 (332 - 128) nW = 816 nW
// in integers, with no rounding anywhere (Q is a multiple of 4, but nothing here relies on it).
#pragma once
#include <cstdint>

namespace mdbg {

constexpr uint32_t CX_SQ_LIMIT_PER_WINDOW = 300u + 32u;     // suspect: sum weight sq > this * nW
constexpr uint32_t CX_Q_LIMIT_PER_WINDOW = 4u * (CX_SQ_LIMIT_PER_WINDOW - 2u * 64u);      // 816: the same in Q
static_assert(CX_Q_LIMIT_PER_WINDOW == 816u, "sum weight Q > 816 nW  <=>  sum weight sq > 332 nW");
constexpr uint32_t CX_Q_MAX = 15u * 256u;                    // largest Q of a word

// number of complexity windows of a read of `len` bases (ReadSelection.hpp:1171-1228)
__host__ __device__ __forceinline__ uint32_t complexity_windows(uint32_t len) { return len >= 66u ? (len - 66u) / 32u + 1u : 0u; }

// number of windows word w of a read with nW windows lies in (w = 0xFFFFFFFF, "the word before the first", gives 0)
__host__ __device__ __forceinline__ uint32_t complexity_word_weight(uint32_t w, uint32_t nW) {
    return (w < nW ? 1u : 0u) + ((uint32_t)(w - 1u) < nW ? 1u : 0u);
}

__host__ __device__ __forceinline__ bool complexity_suspect(uint64_t weighted_q, uint32_t nW) {
    return weighted_q > (uint64_t)CX_Q_LIMIT_PER_WINDOW * nW;
}

__host__ __device__ __forceinline__ uint32_t cx_rotr32(uint32_t v, unsigned r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(v, v, r);
#else
    return (v >> r) | (v << (32u - r));
#endif
}

// (popc(m) - 16)^2 + acc: v_bcnt_u32_b32 with -16 as its addend, then v_mad_i32_i24 (asked for by name: left to itself the
// compiler multiplies first and adds the 15 squares three at a time, 22 instructions where these are 15)
__host__ __device__ __forceinline__ uint32_t cx_sq_acc(uint32_t m, uint32_t acc) {
    const int d = (int)__builtin_popcount(m) - 16;
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t out;
    asm("v_mad_i32_i24 %0, %1, %1, %2" : "=v"(out) : "v"(d), "v"(acc));
    return out;
#else
    return (uint32_t)(d * d) + acc;
#endif
}

// Q of the word x (32 bases, 2 bits each, base 0 in the low bits); next_lo32 = the low half of the word after it (only its
// base 0, the successor of base 31, is used).  The two halves of the word are interleaved so that every plane is one register:
// base i < 16 sits at bit 2i, base 16 + i at bit 2i + 1 ("slot" order).  The successor of a slot is the slot two bits up, except
// slot 30 (base 15 -> base 16 = slot 1) and slot 31 (base 31 -> the first base of the next word).  Built from the instructions
// that issue at the fast rate on gfx950 (and / or / xor / add / right shift / v_bitop3, tools/ubench/op_rates.hip) plus rotates.
__host__ __device__ __forceinline__ uint32_t word_pair_q(uint64_t x, uint32_t next_lo32) {
    const uint32_t M = 0x55555555u;
    const uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32);
    const uint32_t th = xh & M;
    const uint32_t L = (xl & M) | (th + th);                       // low code bits in slot order
    const uint32_t H = ((xl >> 1) & M) | (xh & ~M);                // high code bits in slot order
    // successor planes: slot s <- slot s + 2; slot 30 <- slot 1; slot 31 <- base 0 of the next word
    const uint32_t nl = cx_rotr32(next_lo32, 1);                   // bit 31 = low code bit of the next word's base 0
    const uint32_t nh = cx_rotr32(next_lo32, 2);                   // bit 31 = its high code bit
    const uint32_t NL = (L >> 2) | (cx_rotr32(L, 3) & 0x40000000u) | (nl & 0x80000000u);
    const uint32_t NH = (H >> 2) | (cx_rotr32(H, 3) & 0x40000000u) | (nh & 0x80000000u);
    const uint32_t S[4] = {0u, L, H, L ^ H}, T[4] = {0u, NL, NH, NL ^ NH};
    // two chains of multiply-adds, so that one does not wait for the other's result
    uint32_t q0 = 0, q1 = 0;
#pragma unroll
    for (int i = 1; i < 16; i++) {
        const int a = i >> 2, b = i & 3;
        const uint32_t m = a == 0 ? T[b] : (b == 0 ? S[a] : (S[a] ^ T[b]));
        if (i & 1) q0 = cx_sq_acc(m, q0); else q1 = cx_sq_acc(m, q1);
    }
    const uint32_t q = q0 + q1;
    return q;
}

}  // namespace mdbg
