// hefx_encode.hip -- CKKSEncoder::encode on the GPU (App. A.12): canonical embedding with
// slot i <-> root zeta^(3^i), zeta = exp(2 pi i / 2N).  Reference call sites: matrix_mult_benchmark.cpp:291-323,
// logistic_regression_ckks.cpp:222-225,302-305 (one-hot masks inside the LR hot loop), helper.h:333-343.
//
// Math.  The plaintext polynomial p (real, degree < N) has p(zeta^(2r+1)) = A_r for all r < N, where A_r = v_i at
// r = (3^i - 1)/2 and A_(N-1-r) = conj(A_r).  Pairing r with N-1-r:
//     p_k = (2/N) * Re( zeta^(-k) * sum_{r < N/2} A_r * exp(-2 pi i r k / N) ),
// and splitting k = 2k' + kappa turns the inner sum into TWO complex FFTs of N/2 points (kappa = 0, 1) of
// A_r * exp(-2 pi i r kappa / N).  One workgroup per (vector, kappa): N/16 threads, 8 complex points per thread,
// radix-8 decimation-in-frequency passes through LDS (128 KiB of double2 at N = 16384), output scattered from
// bit-reversed order.  Then p_k * scale is rounded half away from zero (std::round, as SEAL does), reduced into
// every RNS row and the rows go through the regular forward NTT.
//
// Parity: floating point -- not bit-exact with any other FFT; |coefficient difference| <= 1 against the CPU
// oracle on a small fraction of coefficients (tested), decode(encode(v)) == v to ~1e-9 at scale 2^40.
#include "hefx_internal.h"
#include "hefx_crt.cuh"

namespace hefx {

__device__ __forceinline__ double2 cmul(double2 a, double2 b)
{
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// Wide coefficients (hefx_ckks_encode_wide, hefx_ckks_encode_scalar).  A rounded coefficient of 2^63 or more is already
// an integer of the form m * 2^e with m < 2^53 (a float64 that large has no fraction bits), so its residue is
// (m mod q) * (2^e mod q) mod q -- the integer encoded is exactly the double the FFT produced, nothing is rounded twice.
// 2^e mod q (11 <= e <= 971) as (2^64 mod q)^(e / 64) * (2^(e % 64) mod q): below e = 64 -- every scale up to 2^116 -- one
// word reduction, beyond it square-and-multiply over the four bits of e / 64.  No table to build or keep resident.
// Below 2^63 the conversion of the narrow kernel.
__device__ __forceinline__ u64 pow2mod(int e, const ModConst &mc)
{
    u64 r = barrett64(1ull << (e & 63), mc.q, mc.r1);
    u64 b = barrett64(mc.nq, mc.q, mc.r1);  // nq = 2^64 - q
    for (e >>= 6; e; e >>= 1) {
        if (e & 1) r = mulmod(r, b, mc);
        b = mulmod(b, b, mc);
    }
    return r;
}
// |co| mod q for an integer-valued double co of any magnitude; canonical in [0, q)
__device__ __forceinline__ u64 wide_residue(double a /* = |co| */, const ModConst &mc)
{
    if (a < 0x1p63) return barrett64((u64)a, mc.q, mc.r1);
    const u64 bits = (u64)__double_as_longlong(a);
    const int e = (int)(bits >> 52) - 1075;  // a = m * 2^e, e >= 11
    const u64 m = (bits & ((1ull << 52) - 1)) | (1ull << 52);
    return mulmod(barrett64(m, mc.q, mc.r1), pow2mod(e, mc), mc);
}

template <int LM>  // M = 2^LM = N/2 complex points
struct FftCfg {
    static constexpr int M = 1 << LM;
    static constexpr int T = M / 8;
    static constexpr int FP = LM / 3;
    static constexpr int R = LM % 3;
};

// one radix-2 DIF butterfly of block length 2*gap on positions (idx, idx+gap)
__device__ __forceinline__ void dif(double2 &u, double2 &v, const double2 *__restrict__ w, int idx, int gap, int M)
{
    const double2 s = make_double2(u.x + v.x, u.y + v.y);
    const double2 d = make_double2(u.x - v.x, u.y - v.y);
    const int j = idx & (gap - 1);
    u = s;
    v = cmul(d, w[j * (M / (2 * gap))]);
}

// SPLIT (N = 32768: 16384 complex points do not fit LDS): the first DIF stage is applied while loading -- half h of
// an FFT of FM = 2*M points keeps a0 + a1 (h = 0: even frequencies) or (a0 - a1) * w_FM^r (h = 1: odd frequencies) --
// and the workgroup runs the remaining M-point transform; blockIdx.x = 2*kappa + h.
// WIDE: the output stage alone differs (wide_residue above); the narrow instantiation is the kernel it always was.
template <int LM, bool SPLIT, bool WIDE>
__global__ __launch_bounds__(FftCfg<LM>::T) void ckks_encode_kernel(DevTables T, EncodeTables E, const double *re,
                                                                   const double *im, int nvalues, double scale, int L,
                                                                   u64 *out /* [count][L][N] coefficient form */)
{
    using C = FftCfg<LM>;
    extern __shared__ __align__(16) double2 fl[];
    const int t = threadIdx.x, vec = blockIdx.y;
    const int kappa = SPLIT ? blockIdx.x >> 1 : blockIdx.x, hh = SPLIT ? blockIdx.x & 1 : 0;
    constexpr int FM = SPLIT ? 2 * C::M : C::M;  // points of the whole FFT = N/2 = size the twiddle table is built for
    const int N = 2 * FM;
    const double *vre = re + (size_t)vec * nvalues;
    const double *vim = im ? im + (size_t)vec * nvalues : nullptr;
    auto load = [&](int r) {  // A_r, pre-twisted for kappa = 1
        const int s = E.slot[r];
        double2 a = make_double2(0.0, 0.0);
        if (s >= 0 && (s >> 1) < nvalues) {
            a.x = vre[s >> 1];
            a.y = vim ? vim[s >> 1] : 0.0;
            if (s & 1) a.y = -a.y;
        }
        return kappa ? cmul(a, E.pre[r]) : a;
    };
    double2 v[8];
    // natural order, r = t + T*e
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int r = t + C::T * e;
        if (SPLIT) {
            const double2 a0 = load(r), a1 = load(r + C::M);
            v[e] = hh ? cmul(make_double2(a0.x - a1.x, a0.y - a1.y), E.wfft[r])
                      : make_double2(a0.x + a1.x, a0.y + a1.y);
        } else {
            v[e] = load(r);
        }
    }
    // radix-8 DIF passes: pass p works on stride S = M / 8^(p+1); gaps 4S, 2S, S
#pragma unroll
    for (int p = 0; p < C::FP; ++p) {
        const int LOGS = LM - 3 * (p + 1);
        const int S = 1 << LOGS;
        const int b = t >> LOGS;
        const int base = b * (8 * S) + (t & (S - 1));
        if (p > 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fl[base + S * e];
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int half = 4 >> u;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e & half) continue;
                dif(v[e], v[e | half], E.wfft, base + S * e, half * S, FM);
            }
        }
        if (p + 1 < C::FP || C::R > 0) {
            __syncthreads();  // everyone has read its inputs of this pass
#pragma unroll
            for (int e = 0; e < 8; ++e) fl[base + S * e] = v[e];
            __syncthreads();
        }
    }
    if (C::R > 0) {  // remaining R stages on groups of G = 2^R contiguous points
        constexpr int G = 1 << C::R, NG = 8 / G;
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int e = 0; e < G; ++e) v[c * G + e] = fl[(t + C::T * c) * G + e];
#pragma unroll
        for (int u = 0; u < C::R; ++u) {
            const int half = G >> (u + 1);
#pragma unroll
            for (int c = 0; c < NG; ++c)
#pragma unroll
                for (int e = 0; e < G; ++e) {
                    if (e & half) continue;
                    dif(v[c * G + e], v[c * G + (e | half)], E.wfft, (t + C::T * c) * G + e, half, FM);
                }
        }
    }
    // position pos holds X[bitrev(pos)]: k' = bitrev(pos), k = 2k' + kappa
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        int pos;
        if (C::R == 0) {
            pos = t * 8 + e;
        } else {
            constexpr int G = 1 << C::R;
            pos = (t + C::T * (e / G)) * G + (e % G);
        }
        int kp = (int)(__brev((unsigned)pos) >> (32 - LM));
        if (SPLIT) kp = 2 * kp + hh;
        const int k = 2 * kp + kappa;
        const double2 z = cmul(v[e], E.post[k]);
        const double co = __builtin_round(z.x * (2.0 / (double)N) * scale);
        const bool neg = co < 0.0;
        if (WIDE) {
            const double a = __builtin_fabs(co);
            for (int j = 0; j < L; ++j) {
                const ModConst mc = T.mods[j];
                const u64 r = wide_residue(a, mc);
                out[((size_t)vec * L + j) * N + k] = neg ? (r ? mc.q - r : 0) : r;
            }
        } else {
            const u64 mag = (u64)__builtin_fabs(co);
            for (int j = 0; j < L; ++j) {
                const ModConst mc = T.mods[j];
                const u64 r = barrett64(mag, mc.q, mc.r1);
                out[((size_t)vec * L + j) * N + k] = neg ? (r ? mc.q - r : 0) : r;
            }
        }
    }
}

// CKKSEncoder::encode(double, scale, plain): the NTT of a constant is that constant in every slot, so plaintext i is
// round_half_away(value_i * scale) mod q_j in every word of row j -- no transform.  One workgroup row per (j, i).
__global__ __launch_bounds__(256) void ckks_encode_scalar_kernel(DevTables T, const double *__restrict__ vals, double scale,
                                                                 int L, u64 *__restrict__ out /* [count][L][N] */)
{
    const size_t n = (size_t)1 << T.logn;
    const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y, i = blockIdx.z;
    if (a >= n) return;
    const double co = __builtin_round(vals[i] * scale);
    const ModConst mc = T.mods[j];
    const u64 r = wide_residue(__builtin_fabs(co), mc);
    out[((size_t)i * L + j) * n + a] = co < 0.0 ? (r ? mc.q - r : 0) : r;
}

// ------------------------------------------------------------------------------------------------
// CKKSEncoder::decode on the GPU: (1) CRT-compose every coefficient from its RNS residues (Garner mixed radix, exact
// modular arithmetic), centre it against floor(Q/2) digit by digit, evaluate it in double (Horner over the mixed-radix
// digits, ~L ulp) and divide by the scale; (2) evaluate p at the slot roots: with p real,
//     A_r = sum_{k<N/2} (p_k + i (-1)^r p_{k+N/2}) zeta^{(2r+1) k},
// i.e. for r = 2r' + par an N/2-point DFT (positive exponent) of c_k * zeta^{(2 par + 1) k}, c_k = p_k +- i p_{k+N/2};
// slot i reads A_r at r = (3^i - 1)/2 or the conjugate of its mirror.  The positive-exponent DFT runs through the
// same DIF passes as encode on conjugated data.
// ------------------------------------------------------------------------------------------------
// (garner_digits, above_half, horner_digits: hefx_crt.cuh -- shared with the BFV rounding of hefx_bfv.hip)
__global__ __launch_bounds__(256) void decode_crt_kernel(DevTables T, DecodeTables D, int L, const u64 *__restrict__ coef,
                                                         double inv_scale, double *__restrict__ p)
{
    const size_t n = (size_t)1 << T.logn;
    const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t vec = blockIdx.y;
    if (a >= n) return;
    u64 d[16];
    garner_digits(T, L, coef + vec * L * n + a, n, d);
    const bool neg = above_half(d, D.half, L);
    if (neg) {  // y = Q - x, digit-wise with borrow (Q = (0, ..., 0 | 1))
        u64 borrow = 0;
        for (int j = 0; j < L; ++j) {
            const u64 q = T.mods[j].q, sub = d[j] + borrow;  // < q + 1
            if (sub == 0) {
                d[j] = 0;
                borrow = 0;
            } else {
                d[j] = q - sub;
                borrow = 1;
            }
        }
    }
    double m = (double)d[L - 1];
    for (int j = L - 2; j >= 0; --j) m = m * (double)T.mods[j].q + (double)d[j];
    p[vec * n + a] = (neg ? -m : m) * inv_scale;
}

// ------------------------------------------------------------------------------------------------
// Exact centred base extension (mod-raise; include/hefx_refresh.h): the integer back end of the digits above.  A
// coefficient x in [0, Q_in) stands for x when x <= floor(Q_in / 2) and for x - Q_in otherwise -- decode's rule -- and
// row j >= L_in of the output holds that integer mod q_j:
//     x mod q_j = ((d_(L-1) q_(L-2) + d_(L-2)) q_(L-3) + ... + d_0) mod q_j   (Horner over the mixed-radix digits),
// minus Q_in mod q_j for a negative one.  No floating point: every step is a canonical residue.  One thread per
// (coefficient, item), consecutive lanes on consecutive coefficients; the new rows may be 40-bit or 60-bit primes, so
// the arithmetic is the ModConst path that serves both.  qmod[i * k + j] = q_i mod q_j.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lift_crt_kernel(DevTables T, LiftTables D, const u64 *__restrict__ qmod, int L_in,
                                                       int L_out, const u64 *__restrict__ coef, u64 *__restrict__ out,
                                                       size_t out_stride)
{
    const size_t n = (size_t)1 << T.logn;
    const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t item = blockIdx.y;
    if (a >= n) return;
    u64 d[16];
    garner_digits(T, L_in, coef + item * L_in * n + a, n, d);
    const bool neg = above_half(d, D.half, L_in);
    u64 *__restrict__ o = out + item * out_stride + a;
    for (int j = L_in; j < L_out; ++j) {
        const ModConst mc = T.mods[j];
        u64 acc = horner_digits(d, L_in, qmod + j, (size_t)T.k, mc);
        if (neg) acc = submod(acc, D.qin[j], mc.q);
        o[(size_t)(j - L_in) * n] = acc;
    }
}

template <int LM, bool SPLIT>
__global__ __launch_bounds__(FftCfg<LM>::T) void decode_fft_kernel(DevTables T, EncodeTables E,
                                                                  const double *__restrict__ p, double *__restrict__ re,
                                                                  double *__restrict__ im)
{
    using C = FftCfg<LM>;
    extern __shared__ __align__(16) double2 fl[];
    const int t = threadIdx.x, vec = blockIdx.y;
    const int par = SPLIT ? blockIdx.x >> 1 : blockIdx.x, hh = SPLIT ? blockIdx.x & 1 : 0;
    constexpr int FM = SPLIT ? 2 * C::M : C::M;  // N/2
    const int N = 2 * FM;
    const double *__restrict__ pv = p + (size_t)vec * N;
    auto load = [&](int k) {  // conj(c_k * zeta^((2 par + 1) k)), zeta^j = conj(post[j]), zeta^N = -1
        double2 c = make_double2(pv[k], par ? -pv[k + FM] : pv[k + FM]);
        const int idx = par ? 3 * k : k;
        double2 z = idx < N ? E.post[idx] : E.post[idx - N];  // conj(zeta^idx) up to sign
        if (idx >= N) z = make_double2(-z.x, -z.y);
        // c * conj(z) conjugated = conj(c) * z
        return cmul(make_double2(c.x, -c.y), z);
    };
    double2 v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = t + C::T * e;
        if (SPLIT) {
            const double2 a0 = load(k), a1 = load(k + C::M);
            v[e] = hh ? cmul(make_double2(a0.x - a1.x, a0.y - a1.y), E.wfft[k])
                      : make_double2(a0.x + a1.x, a0.y + a1.y);
        } else {
            v[e] = load(k);
        }
    }
#pragma unroll
    for (int ps = 0; ps < C::FP; ++ps) {
        const int LOGS = LM - 3 * (ps + 1);
        const int S = 1 << LOGS;
        const int b = t >> LOGS;
        const int base = b * (8 * S) + (t & (S - 1));
        if (ps > 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fl[base + S * e];
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int half = 4 >> u;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e & half) continue;
                dif(v[e], v[e | half], E.wfft, base + S * e, half * S, FM);
            }
        }
        if (ps + 1 < C::FP || C::R > 0) {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 8; ++e) fl[base + S * e] = v[e];
            __syncthreads();
        }
    }
    if (C::R > 0) {
        constexpr int G = 1 << C::R, NG = 8 / G;
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int e = 0; e < G; ++e) v[c * G + e] = fl[(t + C::T * c) * G + e];
#pragma unroll
        for (int u = 0; u < C::R; ++u) {
            const int half = G >> (u + 1);
#pragma unroll
            for (int c = 0; c < NG; ++c)
#pragma unroll
                for (int e = 0; e < G; ++e) {
                    if (e & half) continue;
                    dif(v[c * G + e], v[c * G + (e | half)], E.wfft, (t + C::T * c) * G + e, half, FM);
                }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        int pos;
        if (C::R == 0) {
            pos = t * 8 + e;
        } else {
            constexpr int G = 1 << C::R;
            pos = (t + C::T * (e / G)) * G + (e % G);
        }
        int rp = (int)(__brev((unsigned)pos) >> (32 - LM));
        if (SPLIT) rp = 2 * rp + hh;
        const int r = 2 * rp + par;
        if (r >= FM) continue;  // A_(N-1-r) = conj(A_r): the upper half is redundant
        const int sl = E.slot[r];
        // A_r = conj(v) (the DFT ran on conjugated data); slot value = A_r, or conj(A_r) when r is the mirror root
        const double2 A = make_double2(v[e].x, -v[e].y);
        re[(size_t)vec * FM + (sl >> 1)] = A.x;
        if (im) im[(size_t)vec * FM + (sl >> 1)] = (sl & 1) ? -A.y : A.y;
    }
}

hipError_t launch_decode(const DevTables &T, const EncodeTables &E, const DecodeTables &D, int L, const u64 *coef,
                         int count, double scale, double *p, double *re, double *im, hipStream_t s)
{
    const int n = 1 << T.logn;
    hipLaunchKernelGGL(decode_crt_kernel, dim3((n + 255) / 256, count), dim3(256), 0, s, T, D, L, coef, 1.0 / scale, p);
    const int lm = T.logn - 1;
#define LAUNCHD(LMV, SPL)                                                                                        \
    {                                                                                                            \
        const size_t lds = sizeof(double2) * (size_t)FftCfg<LMV>::M;                                             \
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(decode_fft_kernel<LMV, SPL>),                   \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                         \
        hipLaunchKernelGGL((decode_fft_kernel<LMV, SPL>), dim3(SPL ? 4 : 2, count), dim3(FftCfg<LMV>::T), lds, s, T, \
                           E, p, re, im);                                                                        \
    }
    switch (lm) {
        case 9: LAUNCHD(9, false) break;
        case 10: LAUNCHD(10, false) break;
        case 11: LAUNCHD(11, false) break;
        case 12: LAUNCHD(12, false) break;
        case 13: LAUNCHD(13, false) break;
        case 14: LAUNCHD(13, true) break;
        default: return hipErrorInvalidValue;
    }
#undef LAUNCHD
    return hipGetLastError();
}

hipError_t launch_lift(const DevTables &T, const LiftTables &D, const u64 *qmod, int L_in, int L_out, int count,
                       const u64 *coef, u64 *out, size_t out_stride, hipStream_t s)
{
    const int n = 1 << T.logn;
    hipLaunchKernelGGL(lift_crt_kernel, dim3((n + 255) / 256, count), dim3(256), 0, s, T, D, qmod, L_in, L_out, coef, out,
                       out_stride);
    return hipGetLastError();
}

hipError_t launch_encode(const DevTables &T, const EncodeTables &E, const double *re, const double *im, int nvalues,
                         int count, double scale, int L, u64 *out, bool wide, hipStream_t s)
{
    const int lm = T.logn - 1;
#define LAUNCH1(LMV, SPL, W)                                                                                     \
    {                                                                                                            \
        const size_t lds = sizeof(double2) * (size_t)FftCfg<LMV>::M;                                             \
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ckks_encode_kernel<LMV, SPL, W>),               \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                         \
        hipLaunchKernelGGL((ckks_encode_kernel<LMV, SPL, W>), dim3(SPL ? 4 : 2, count), dim3(FftCfg<LMV>::T), lds, s, \
                           T, E, re, im, nvalues, scale, L, out);                                                \
    }
#define LAUNCH(LMV, SPL)                                                                                         \
    if (wide)                                                                                                    \
        LAUNCH1(LMV, SPL, true)                                                                                  \
    else                                                                                                         \
        LAUNCH1(LMV, SPL, false)
    switch (lm) {
        case 9: LAUNCH(9, false) break;
        case 10: LAUNCH(10, false) break;
        case 11: LAUNCH(11, false) break;
        case 12: LAUNCH(12, false) break;
        case 13: LAUNCH(13, false) break;
        case 14: LAUNCH(13, true) break;  // N = 32768: two half-size workgroups per (vector, kappa)
        default: return hipErrorInvalidValue;
    }
#undef LAUNCH
#undef LAUNCH1
    return hipGetLastError();
}

hipError_t launch_encode_scalar(const DevTables &T, const double *vals, int count, double scale, int L, u64 *out,
                                hipStream_t s)
{
    const int n = 1 << T.logn;
    for (int i0 = 0; i0 < count; i0 += 32768) {  // (the grid's z extent ends at 65535)
        const int cnt = count - i0 < 32768 ? count - i0 : 32768;
        hipLaunchKernelGGL(ckks_encode_scalar_kernel, dim3((n + 255) / 256, L, cnt), dim3(256), 0, s, T, vals + i0, scale, L,
                           out + (size_t)i0 * L * n);
    }
    return hipGetLastError();
}

// HIP loads a translation unit's code object at its first kernel launch (milliseconds); hefx_context_create pays
// that once, up front, instead of the first encode / rotation / encryption of a program.
__global__ void warm_encode_kernel() {}
hipError_t warm_encode(hipStream_t s)
{
    hipLaunchKernelGGL(warm_encode_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace hefx
