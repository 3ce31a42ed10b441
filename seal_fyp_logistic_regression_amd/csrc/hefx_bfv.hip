// hefx_bfv.hip -- the exact divide-and-round of BFV (include/hefx_bfv.h): R(z) = round(t z / Q) per coefficient, for the
// tensor product of a multiplication (result mod every q_j) and for decryption (result mod t).
//
// Method.  The working basis is the data primes q_0 .. q_(L-1) FOLLOWED by auxiliary primes p_0 .., A rows in all, product
// M = Q P.  In mixed radix over that order, v = d_0 + d_1 q_0 + ... + d_L Q + d_(L+1) Q p_0 + ..., so
//     floor(v / Q) = d_L + d_(L+1) p_0 + d_(L+2) p_0 p_1 + ...
// -- the quotient by Q is the upper digits, nothing is divided.  Q is odd, t z / Q never ends in one half, and so
//     R(z) = floor((t z + (Q-1)/2) / Q)                                  for z of either sign, and for any integer K
//     R(z) = floor((t (z + K Q) + (Q-1)/2) / Q) - t K.
// With K Q >= |z| the numerator v is not negative and the rows of v are those of z times t plus a constant per row
// (`mul`, `add`): one multiply-add per residue, the Garner digits of hefx_crt.cuh, and a Horner of the upper digits mod
// the output modulus.  The multiplication takes K = N Q (|z| < 3 N (Q/2)^2 <= N Q^2), decryption K = 1 (|z| <= Q/2); in
// both t K vanishes modulo every output modulus, so nothing is subtracted.  v < M is the caller's sizing rule
// (hefx_bfv_create).  No centring, no multiword integer, no floating point, no `/` or `%`.
//
// One thread per (coefficient, polynomial), consecutive lanes on consecutive coefficients: every row is read and written
// in whole cache lines.  The row count A is a template parameter so that the digit array is indexed at compile time.
#include "hefx_internal.h"
#include "hefx_crt.cuh"

namespace hefx {

template <int A, bool PLAIN>
__global__ __launch_bounds__(256) void bfv_round_kernel(DevTables T, BfvRoundTables R, int L, const u64 *__restrict__ in,
                                                        size_t in_stride, u64 *__restrict__ out)
{
    const size_t n = (size_t)1 << T.logn;
    const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t poly = blockIdx.y;
    if (a >= n) return;
    const u64 *__restrict__ c = in + poly * in_stride + a;
    const u64 *__restrict__ mul = R.mul, *__restrict__ add = R.add;
    u64 d[A];
    garner_digits_from(
        T, A, [=](int j, const ModConst &mc) { return addmod(mulmod(c[(size_t)j * n], mul[j], mc), add[j], mc.q); }, d);
    if (PLAIN) {
        out[poly * n + a] = horner_upper_digits<A>(d, L, R.rad, 1, R.out);
    } else {
        u64 *__restrict__ o = out + poly * L * n + a;
        for (int j = 0; j < L; ++j) o[(size_t)j * n] = horner_upper_digits<A>(d, L, R.rad + j, (size_t)T.k, T.mods[j]);
    }
}

template <int A>
static hipError_t launch_round_a(const DevTables &T, const BfvRoundTables &R, int L, bool plain, int npoly, const u64 *in,
                                 size_t in_stride, u64 *out, hipStream_t s)
{
    const size_t n = (size_t)1 << T.logn;
    const dim3 grid((unsigned)((n + 255) >> 8), (unsigned)npoly), block(256);
    if (plain)
        hipLaunchKernelGGL((bfv_round_kernel<A, true>), grid, block, 0, s, T, R, L, in, in_stride, out);
    else
        hipLaunchKernelGGL((bfv_round_kernel<A, false>), grid, block, 0, s, T, R, L, in, in_stride, out);
    return hipGetLastError();
}

hipError_t launch_bfv_round(const DevTables &T, const BfvRoundTables &R, int A, int L, bool plain, int npoly, const u64 *in,
                            size_t in_stride, u64 *out, hipStream_t s)
{
    if (L < 1 || L >= A || A > T.k) return hipErrorInvalidValue;
    switch (A) {
#define HEFX_BFV_CASE(N_) \
    case N_: return launch_round_a<N_>(T, R, L, plain, npoly, in, in_stride, out, s);
        HEFX_BFV_CASE(2) HEFX_BFV_CASE(3) HEFX_BFV_CASE(4) HEFX_BFV_CASE(5) HEFX_BFV_CASE(6) HEFX_BFV_CASE(7)
        HEFX_BFV_CASE(8) HEFX_BFV_CASE(9) HEFX_BFV_CASE(10) HEFX_BFV_CASE(11) HEFX_BFV_CASE(12) HEFX_BFV_CASE(13)
        HEFX_BFV_CASE(14) HEFX_BFV_CASE(15) HEFX_BFV_CASE(16)
#undef HEFX_BFV_CASE
    default: return hipErrorInvalidValue;
    }
}

}  // namespace hefx
