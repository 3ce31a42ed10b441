// hefx_bfv.hip -- the exact divide-and-round of BFV (include/hefx_bfv.h): R(z) = round(t z / Q) per coefficient, for the
// tensor product of a multiplication (result mod every q_j) and for decryption (result mod t); and, in the second half of
// the file, the rest of the scheme's arithmetic (Delta m into c_0, the lifted message, the noise budget, the slot order).
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

// ---------------------------------------------------------------------------------------------------------------------
// The rest of the scheme's arithmetic: Delta m added to c_0, the centred lift of a message, the noise budget, the slot
// permutation of BatchEncoder.  Same rules as above: exact, canonical residues through hefx_modarith.cuh, no division.
// ---------------------------------------------------------------------------------------------------------------------
// W coefficients per thread (W = 2: one 16-byte record of every streamed row, when every pointer is 16-byte aligned;
// W = 1: word by word).  m is read once per thread and serves all L rows; a record that straddles ncoeff reads only the
// words d_m holds.
template <int W>
__device__ __forceinline__ void load_words(const u64 *__restrict__ p, u64 *v)
{
    if (W == 2) {
        const ulonglong2 r = gld16(p);
        v[0] = r.x, v[1] = r.y;
    } else {
        v[0] = gld8(p);
    }
}
template <int W>
__device__ __forceinline__ void store_words(u64 *__restrict__ p, const u64 *v)
{
    if (W == 2)
        gst16(p, make_ulonglong2(v[0], v[1]));
    else
        gst8(p, v[0]);
}
// the ncoeff words of m behind position a, zero-filled: `have` of the W are real
template <int W>
__device__ __forceinline__ int load_message(const u64 *__restrict__ m, size_t a, size_t ncoeff, u64 *v)
{
    for (int i = 0; i < W; ++i) v[i] = 0;
    if (a + W <= ncoeff) {
        load_words<W>(m + a, v);
        return W;
    }
    if (a < ncoeff) {  // W == 2 and the last word of an odd count
        v[0] = gld8(m + a);
        return 1;
    }
    return 0;
}

template <int W>
__global__ __launch_bounds__(256) void bfv_scale_add_kernel(DevTables T, BfvFrontTables F, int L, const u64 *__restrict__ m,
                                                            size_t ncoeff, const u64 *c0, u64 *out)
{
    const size_t n = (size_t)1 << T.logn;
    const size_t a = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * W;
    if (a >= n) return;
    u64 mv[W];
    const int have = load_message<W>(m, a, ncoeff, mv);
    for (int j = 0; j < L; ++j) {
        const ModConst mc = T.mods[j];
        const u64 dj = F.delta[j];
        u64 c[W];
        if (c0)
            load_words<W>(c0 + (size_t)j * n + a, c);
        else
            for (int i = 0; i < W; ++i) c[i] = 0;
        for (int i = 0; i < W; ++i)
            if (i < have) c[i] = addmod(c[i], mulmod(mv[i], dj, mc), mc.q);  // any 64-bit m: the product is reduced whole
        store_words<W>(out + (size_t)j * n + a, c);
    }
}

template <int W>
__global__ __launch_bounds__(256) void bfv_lift_plain_kernel(DevTables T, BfvFrontTables F, int L, const u64 *__restrict__ m,
                                                             size_t ncoeff, u64 *__restrict__ out)
{
    const size_t n = (size_t)1 << T.logn;
    const size_t a = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * W;
    if (a >= n) return;
    u64 mv[W];
    const int have = load_message<W>(m, a, ncoeff, mv);
    const u64 t = F.t, half = t >> 1;
    for (int j = 0; j < L; ++j) {
        const ModConst mc = T.mods[j];
        u64 c[W];
        for (int i = 0; i < W; ++i) {
            c[i] = 0;
            if (i < have) c[i] = mv[i] <= half ? barrett64(mv[i], mc.q, mc.r1) : mc.q - barrett64(t - mv[i], mc.q, mc.r1);
        }
        store_words<W>(out + (size_t)j * n + a, c);
    }
}

hipError_t launch_bfv_scale_add(const DevTables &T, const BfvFrontTables &F, int L, const u64 *m, int ncoeff, const u64 *c0,
                                u64 *out, bool vec, hipStream_t s)
{
    const size_t n = (size_t)1 << T.logn;
    if (vec)
        hipLaunchKernelGGL((bfv_scale_add_kernel<2>), dim3((unsigned)((n + 511) >> 9)), dim3(256), 0, s, T, F, L, m,
                           (size_t)ncoeff, c0, out);
    else
        hipLaunchKernelGGL((bfv_scale_add_kernel<1>), dim3((unsigned)((n + 255) >> 8)), dim3(256), 0, s, T, F, L, m,
                           (size_t)ncoeff, c0, out);
    return hipGetLastError();
}

hipError_t launch_bfv_lift_plain(const DevTables &T, const BfvFrontTables &F, int L, const u64 *m, int ncoeff, u64 *out,
                                 bool vec, hipStream_t s)
{
    const size_t n = (size_t)1 << T.logn;
    if (vec)
        hipLaunchKernelGGL((bfv_lift_plain_kernel<2>), dim3((unsigned)((n + 511) >> 9)), dim3(256), 0, s, T, F, L, m,
                           (size_t)ncoeff, out);
    else
        hipLaunchKernelGGL((bfv_lift_plain_kernel<1>), dim3((unsigned)((n + 255) >> 8)), dim3(256), 0, s, T, F, L, m,
                           (size_t)ncoeff, out);
    return hipGetLastError();
}

// Noise budget.  Per coefficient v = t x mod Q as mixed-radix digits (the residues x_j (t mod q_j), Garner); above (Q-1)/2
// the magnitude is Q - v = (Q - 1 - v) + 1, and Q - 1 - v has the digits q_j - 1 - d_j.  The magnitude goes to binary by a
// Horner over L words, and only its bit length leaves the thread: the maximum of the bit lengths is the bit length of the
// maximum.  Waves reduce by shuffles, the workgroup through LDS, and one atomic per workgroup reaches the word the caller
// zeroed on the same stream.  L is a template parameter: digits and words are indexed at compile time.
template <int L>
__global__ __launch_bounds__(256) void bfv_noise_bits_kernel(DevTables T, BfvFrontTables F, LiftTables D, const u64 *__restrict__ x,
                                                             uint32_t *wmax)
{
    __shared__ uint32_t part[4];
    const size_t n = (size_t)1 << T.logn;
    const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bits = 0;
    if (a < n) {
        const u64 *__restrict__ c = x + a;
        const u64 *__restrict__ tm = F.tmod;
        u64 d[L];
        garner_digits_from(T, L, [=](int j, const ModConst &mc) { return mulmod(c[(size_t)j * n], tm[j], mc); }, d);
        const bool neg = above_half(d, D.half, L);
        u64 w[L];
#pragma unroll
        for (int i = 0; i < L; ++i) w[i] = 0;
#pragma unroll
        for (int j = L - 1; j >= 0; --j) {
            const u64 q = T.mods[j].q;
            u64 carry = neg ? q - 1 - d[j] : d[j];
#pragma unroll
            for (int i = 0; i < L; ++i) {  // w = w q + digit
                const u64 lo = w[i] * q, hi = mulhi64(w[i], q);
                w[i] = lo + carry;
                carry = hi + (w[i] < lo);
            }
        }
        u64 carry = neg ? 1 : 0;
#pragma unroll
        for (int i = 0; i < L; ++i) {
            w[i] += carry;
            carry = carry & (w[i] == 0);
        }
#pragma unroll
        for (int i = 0; i < L; ++i)
            if (w[i]) bits = 64u * (uint32_t)i + 64u - (uint32_t)__clzll((long long)w[i]);
    }
    for (int off = 32; off >= 1; off >>= 1) bits = max(bits, (uint32_t)__shfl_xor((int)bits, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(wmax, max(max(part[0], part[1]), max(part[2], part[3])));
}

__global__ void bfv_budget_finish_kernel(const uint32_t *__restrict__ wmax, uint32_t qbits, uint32_t *__restrict__ budget)
{
    const uint32_t w = *wmax + 1;
    *budget = qbits > w ? qbits - w : 0;
}

hipError_t launch_bfv_noise_bits(const DevTables &T, const BfvFrontTables &F, const LiftTables &D, int L, const u64 *x,
                                 uint32_t *wmax, hipStream_t s)
{
    const size_t n = (size_t)1 << T.logn;
    const dim3 grid((unsigned)((n + 255) >> 8)), block(256);
    switch (L) {
#define HEFX_BFV_CASE(N_) \
    case N_: hipLaunchKernelGGL((bfv_noise_bits_kernel<N_>), grid, block, 0, s, T, F, D, x, wmax); break;
        HEFX_BFV_CASE(1) HEFX_BFV_CASE(2) HEFX_BFV_CASE(3) HEFX_BFV_CASE(4) HEFX_BFV_CASE(5) HEFX_BFV_CASE(6)
        HEFX_BFV_CASE(7) HEFX_BFV_CASE(8) HEFX_BFV_CASE(9) HEFX_BFV_CASE(10) HEFX_BFV_CASE(11) HEFX_BFV_CASE(12)
        HEFX_BFV_CASE(13) HEFX_BFV_CASE(14) HEFX_BFV_CASE(15)
#undef HEFX_BFV_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_bfv_budget_finish(const uint32_t *wmax, uint32_t qbits, uint32_t *budget, hipStream_t s)
{
    hipLaunchKernelGGL(bfv_budget_finish_kernel, dim3(1), dim3(1), 0, s, wmax, qbits, budget);
    return hipGetLastError();
}

// BatchEncoder's slot order over the one-prime context {t}: index[i] is the position, in the transform's bit-reversed
// output, of the evaluation point of slot i -- a permutation of 0 .. N-1, so the scatter writes every word of out.
__global__ __launch_bounds__(256) void bfv_slot_scatter_kernel(DevTables Tt, const uint32_t *__restrict__ index,
                                                               const u64 *__restrict__ values, size_t nvalues, u64 *__restrict__ out)
{
    const size_t n = (size_t)1 << Tt.logn;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ModConst mc = Tt.mods[0];
    out[index[i]] = i < nvalues ? barrett64(values[i], mc.q, mc.r1) : 0;
}
__global__ __launch_bounds__(256) void bfv_slot_reduce_kernel(DevTables Tt, const u64 *__restrict__ in, u64 *__restrict__ out)
{
    const size_t n = (size_t)1 << Tt.logn;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ModConst mc = Tt.mods[0];
    out[i] = barrett64(in[i], mc.q, mc.r1);
}
__global__ __launch_bounds__(256) void bfv_slot_gather_kernel(DevTables Tt, const uint32_t *__restrict__ index,
                                                              const u64 *__restrict__ in, u64 *__restrict__ out)
{
    const size_t n = (size_t)1 << Tt.logn;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = in[index[i]];
}

hipError_t launch_bfv_slot_scatter(const DevTables &Tt, const uint32_t *index, const u64 *values, int nvalues, u64 *out,
                                   hipStream_t s)
{
    const size_t n = (size_t)1 << Tt.logn;
    hipLaunchKernelGGL(bfv_slot_scatter_kernel, dim3((unsigned)((n + 255) >> 8)), dim3(256), 0, s, Tt, index, values,
                       (size_t)nvalues, out);
    return hipGetLastError();
}
hipError_t launch_bfv_slot_reduce(const DevTables &Tt, const u64 *in, u64 *out, hipStream_t s)
{
    const size_t n = (size_t)1 << Tt.logn;
    hipLaunchKernelGGL(bfv_slot_reduce_kernel, dim3((unsigned)((n + 255) >> 8)), dim3(256), 0, s, Tt, in, out);
    return hipGetLastError();
}
hipError_t launch_bfv_slot_gather(const DevTables &Tt, const uint32_t *index, const u64 *in, u64 *out, hipStream_t s)
{
    const size_t n = (size_t)1 << Tt.logn;
    hipLaunchKernelGGL(bfv_slot_gather_kernel, dim3((unsigned)((n + 255) >> 8)), dim3(256), 0, s, Tt, index, in, out);
    return hipGetLastError();
}

}  // namespace hefx
