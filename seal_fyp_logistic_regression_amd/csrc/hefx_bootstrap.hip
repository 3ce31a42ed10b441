// hefx_bootstrap.hip -- the kernel of hefx_product_combine (include/hefx_bootstrap.h): a node of a polynomial plan with its
// products still inside,
//   out = sum_p u_p * (a_p (x) b_p) + sum_k w_k * l_k + c        (size 3: the tensor products are not relinearised),
// for n items in lockstep, in one pass over the operands.  Step by step the node is P hefx_multiply, P key switches and one
// hefx_scalar_combine; relinearisation is linear, so the caller relinearises this sum once.  The 3 L N words of every tensor
// product are neither written nor read back: a lane reads the 4 operand records of a product and the 2 of a linear term once.
#include "hefx_internal.h"

namespace hefx {

// TABLE (device words, one descriptor-ring slot per call):
//   [0, P)                 words between the two polynomials of operand a_p (its own row count * N): an operand of a higher
//                          level is read through its own stride -- its row prefix IS the mod-dropped ciphertext, no copy
//   [P, 2P)                the same for b_p
//   [2P, 2P + m)           the same for linear term k
//   then [L][P]            the weights u, row-major per RNS row: the P weights of a workgroup are adjacent scalar loads
//   then [L][m]            the weights w
//   then [L]               the constant (has_const)
//   then n records of 2P + m + 1 pointers:  a_0 .. a_(P-1) | b_0 .. b_(P-1) | l_0 .. l_(m-1) | out
// One workgroup works on 256 adjacent 16-byte records of ONE row j of ONE item i (blockIdx.y = j, blockIdx.z = i), so the
// modulus, the weights, the constant and every pointer are uniform per workgroup; all items and rows run in the one launch.
//
// ORDER OF REDUCTION.  u * a * b does not fit 128 bits (three factors below 2^61).  The weight goes into operand a first:
// ua0 = u a0 mod q, ua1 = u a1 mod q (canonical, below q) -- two Barrett reductions per word and product where reducing the
// three tensor words would take three -- and the four products ua0 b0, ua0 b1, ua1 b0, ua1 b1 are accumulated unreduced.
//
// FOLD BOUND.  hefx_context_create refuses primes of 2^61 and above and the entry refuses weights and constants >= q_j, so
// every factor of an accumulated product (ua, b, w, l) is below 2^61 and a product below 2^122 -- the situation
// mul_sum_kernel's comment derives.  An accumulator starts from the constant (< q < 2^61) or zero, or from a folded residue
// (< 2^61).  `pend` counts the products that went into c1, the accumulator that takes most, since the last fold: two per
// product of the node (c0 and c2 take one), one per linear term (c0 takes one, c2 none).  All six accumulator words are folded
// when pend has reached 32 and another term follows; pend advances by 4 (a pair of products), 2 or 1 and 32 is a multiple of
// all three, so it is hit exactly.  Never more than 32 products on top of a residue: 32 * 2^122 + 2^61 < 2^128.  The fold
// interval is therefore 16 products, or 32 linear terms, or any mix 2 P' + m' = 32.  barrett128's quotient estimate is short by
// at most one for ANY 128-bit value, so the final Barrett gives the canonical residue of the integer sum: the bits of mod_drop,
// multiply, multiply_plain by a constant polynomial, add_many, add_plain.
//
// REGISTERS (-Rpass-analysis=kernel-resource-usage, gfx950, the flags of _build.py): VGPRs 68, SGPRs 67, scratch 0, LDS 0,
// occupancy 7 waves/SIMD.  Measured ("Bootstrapping"): 13 - 18 us per call at N = 16384, L = 5 .. 9, n = 2 for the
// node shapes of a degree-31 plan, 2.1 - 2.7x the multiply_batch + size-3 scalar_combine it replaces; at 2300 waves the call is
// bound by its wave count and the floor of a launch, not by bytes.
struct Acc6 {
    u64 c0xl, c0xh, c0yl, c0yh, c1xl, c1xh, c1yl, c1yh, c2xl, c2xh, c2yl, c2yh;
};

__device__ __forceinline__ void pc_fold(Acc6 &s, const ModConst &mc)
{
    s.c0xl = barrett128(s.c0xl, s.c0xh, mc);
    s.c0yl = barrett128(s.c0yl, s.c0yh, mc);
    s.c1xl = barrett128(s.c1xl, s.c1xh, mc);
    s.c1yl = barrett128(s.c1yl, s.c1yh, mc);
    s.c2xl = barrett128(s.c2xl, s.c2xh, mc);
    s.c2yl = barrett128(s.c2yl, s.c2yh, mc);
    s.c0xh = s.c0yh = s.c1xh = s.c1yh = s.c2xh = s.c2yh = 0;
}

__device__ __forceinline__ void pc_product(Acc6 &s, u64 u, const ulonglong2 &a0, const ulonglong2 &a1, const ulonglong2 &b0,
                                           const ulonglong2 &b1, const ModConst &mc)
{
    const u64 ua0x = mulmod(u, a0.x, mc), ua0y = mulmod(u, a0.y, mc), ua1x = mulmod(u, a1.x, mc), ua1y = mulmod(u, a1.y, mc);
    mac128(s.c0xl, s.c0xh, ua0x, b0.x);
    mac128(s.c0yl, s.c0yh, ua0y, b0.y);
    mac128(s.c1xl, s.c1xh, ua0x, b1.x);
    mac128(s.c1xl, s.c1xh, ua1x, b0.x);
    mac128(s.c1yl, s.c1yh, ua0y, b1.y);
    mac128(s.c1yl, s.c1yh, ua1y, b0.y);
    mac128(s.c2xl, s.c2xh, ua1x, b1.x);
    mac128(s.c2yl, s.c2yh, ua1y, b1.y);
}

__global__ __launch_bounds__(256) void product_combine_kernel(DevTables T, int L, int P, int m, const u64 *__restrict__ tab,
                                                              int has_const)
{
    const int logn = T.logn;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int j = (int)blockIdx.y, item = (int)blockIdx.z;
    const ModConst mc = T.mods[j];
    const size_t head = 2 * (size_t)P + m;
    const u64 *__restrict__ ut = tab + head + (size_t)j * P;
    const u64 *__restrict__ wt = tab + head + (size_t)L * P + (size_t)j * m;
    const size_t weights = (size_t)L * ((size_t)P + m + (has_const ? 1 : 0));
    const u64 *__restrict__ rec = tab + head + weights + (size_t)item * (2 * (size_t)P + m + 1);
    const size_t off = ((size_t)j << logn) + 2 * w;  // word offset of this lane's pair inside a polynomial
    Acc6 s;
    s.c0xl = s.c0yl = has_const ? tab[head + (size_t)L * ((size_t)P + m) + j] : 0;
    s.c0xh = s.c0yh = 0;
    s.c1xl = s.c1xh = s.c1yl = s.c1yh = s.c2xl = s.c2xh = s.c2yl = s.c2yh = 0;
    int pend = 0;  // products in c1 since the last fold (FOLD BOUND); uniform
    int p = 0;
    for (; p + 2 <= P; p += 2) {  // eight independent 16-byte loads in flight per lane
        if (pend == 32) {
            pc_fold(s, mc);
            pend = 0;
        }
        ulonglong2 a0[2], a1[2], b0[2], b1[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const u64 *pa = reinterpret_cast<const u64 *>(rec[p + t]) + off, *pb = reinterpret_cast<const u64 *>(rec[P + p + t]) + off;
            a0[t] = gld16(pa);
            a1[t] = gld16(pa + tab[p + t]);
            b0[t] = gld16(pb);
            b1[t] = gld16(pb + tab[P + p + t]);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) pc_product(s, ut[p + t], a0[t], a1[t], b0[t], b1[t], mc);
        pend += 4;
    }
    if (p < P) {
        if (pend == 32) {
            pc_fold(s, mc);
            pend = 0;
        }
        const u64 *pa = reinterpret_cast<const u64 *>(rec[p]) + off, *pb = reinterpret_cast<const u64 *>(rec[P + p]) + off;
        const ulonglong2 a0 = gld16(pa), a1 = gld16(pa + tab[p]), b0 = gld16(pb), b1 = gld16(pb + tab[P + p]);
        pc_product(s, ut[p], a0, a1, b0, b1, mc);
        pend += 2;
    }
    for (int k = 0; k < m; ++k) {
        if (pend == 32) {
            pc_fold(s, mc);
            pend = 0;
        }
        const u64 *pl = reinterpret_cast<const u64 *>(rec[2 * (size_t)P + k]) + off;
        const ulonglong2 l0 = gld16(pl), l1 = gld16(pl + tab[2 * (size_t)P + k]);
        const u64 wk = wt[k];
        mac128(s.c0xl, s.c0xh, l0.x, wk);
        mac128(s.c0yl, s.c0yh, l0.y, wk);
        mac128(s.c1xl, s.c1xh, l1.x, wk);
        mac128(s.c1yl, s.c1yh, l1.y, wk);
        pend += 1;
    }
    pc_fold(s, mc);
    u64 *out = reinterpret_cast<u64 *>(rec[2 * (size_t)P + m]) + off;  // [3][L][N]
    const size_t poly = (size_t)L << logn;
    gst16(out, make_ulonglong2(s.c0xl, s.c0yl));
    gst16(out + poly, make_ulonglong2(s.c1xl, s.c1yl));
    gst16(out + 2 * poly, make_ulonglong2(s.c2xl, s.c2yl));
}

size_t product_combine_table_words(int L, int n, int P, int m, bool has_const)
{
    return 2 * (size_t)P + m + (size_t)L * ((size_t)P + m + (has_const ? 1 : 0)) + (size_t)n * (2 * (size_t)P + m + 1);
}

hipError_t launch_product_combine(const DevTables &T, int L, int n, int P, int m, const u64 *d_tab, bool has_const, hipStream_t s)
{
    const size_t row_pairs = (size_t)1 << (T.logn - 1);
    const dim3 grid((unsigned)((row_pairs + 255) / 256), (unsigned)L, (unsigned)n), block(256);
    hipLaunchKernelGGL(product_combine_kernel, grid, block, 0, s, T, L, P, m, d_tab, has_const ? 1 : 0);
    return hipGetLastError();
}

}  // namespace hefx
