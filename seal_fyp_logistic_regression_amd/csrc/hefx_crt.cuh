// hefx_crt.cuh -- exact CRT composition per lane, in mixed radix: the device functions behind CKKS decode, the centred base
// extension (mod-raise) and the BFV divide-and-round (hefx_encode.hip, hefx_bfv.hip).  No floating point, no division:
// every step is a canonical residue through the Barrett forms of hefx_modarith.cuh.
#pragma once
#include "hefx_internal.h"

namespace hefx {

// Garner mixed-radix digits of one coefficient: d_j = ((r_j - d_0) q_0^-1 - d_1) q_1^-1 ... mod q_j, from the residues
// r_j = load(j) of rows j < L; x = d_0 + d_1 q_0 + d_2 q_0 q_1 + ... in [0, Q).  Exact modular arithmetic.
template <class Load>
__device__ __forceinline__ void garner_digits_from(const DevTables &T, int L, Load load, u64 *d)
{
    for (int j = 0; j < L; ++j) {
        const ModConst mc = T.mods[j];
        u64 t = load(j, mc);
        for (int i = 0; i < j; ++i) {
            const u64 di = barrett64(d[i], mc.q, mc.r1);
            t = mulmod(submod(t, di, mc.q), T.invmod[(size_t)i * T.k + j].x, mc);
        }
        d[j] = t;
    }
}
// ... of the residues c[j * n]
__device__ __forceinline__ void garner_digits(const DevTables &T, int L, const u64 *__restrict__ c, size_t n, u64 *d)
{
    garner_digits_from(T, L, [=](int j, const ModConst &) { return c[(size_t)j * n]; }, d);
}
// x > floor(Q/2)?  compare the mixed-radix digits from the top (Q is odd: no tie)
__device__ __forceinline__ bool above_half(const u64 *d, const u64 *half, int L)
{
    for (int j = L - 1; j >= 0; --j)
        if (d[j] != half[j]) return d[j] > half[j];
    return false;
}
// x mod m = ((d_(L-1) q_(L-2) + d_(L-2)) q_(L-3) + ... + d_0) mod m, Horner over the digits; rad[i * stride] = q_i mod m
__device__ __forceinline__ u64 horner_digits(const u64 *d, int L, const u64 *__restrict__ rad, size_t stride, const ModConst &mc)
{
    u64 acc = barrett64(d[L - 1], mc.q, mc.r1);
    for (int i = L - 2; i >= 0; --i) acc = addmod(mulmod(acc, rad[(size_t)i * stride], mc), barrett64(d[i], mc.q, mc.r1), mc.q);
    return acc;
}
// floor(x / (q_0 ... q_(lo-1))) mod m: the same Horner over the digits lo .. A-1 only -- in mixed radix the quotient by a
// prefix of the basis IS the upper digits.  A is a compile-time count and the loop is predicated, not bounded, by lo, so
// that d[] stays in registers.
template <int A>
__device__ __forceinline__ u64 horner_upper_digits(const u64 *d, int lo, const u64 *__restrict__ rad, size_t stride,
                                                   const ModConst &mc)
{
    u64 acc = barrett64(d[A - 1], mc.q, mc.r1);
#pragma unroll
    for (int i = A - 2; i >= 0; --i)
        if (i >= lo) acc = addmod(mulmod(acc, rad[(size_t)i * stride], mc), barrett64(d[i], mc.q, mc.r1), mc.q);
    return acc;
}

}  // namespace hefx
