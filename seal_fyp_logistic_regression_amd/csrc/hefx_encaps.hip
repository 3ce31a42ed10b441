// hefx_encaps.hip -- the element-wise kernels of sparse-secret encapsulation (include/hefx_encaps.h): the collapsed key and
// the four passes between the transforms of hefx_raise_switch.  The transforms themselves are the engine's, through
// hefx_capi.cpp's transform() at every ring size; the host sequence is hefx_capi.cpp's.
//
// hefx_raise_switch, pass by pass (L = L_out, P = q_(k-1); every arrow that crosses a line is a transform):
//   in [2][1][N]            --INTT_q0-->   coef [2][N]                        (c0, c1 in coefficient form)
//   rs_expand               coef -> xb [2][L-1][N], xp [N]     the centred lift of c1 mod q_1 .. q_(L-1) and mod P, and of c0
//                                                              mod q_1 .. q_(L-1), in ONE pass over the two coefficient rows
//                           --NTT-->       xb, xp
//   rs_product_p            xp, ckey[.][L] -> accp [2][N]      the special prime's row of x Kc: the only row of the product
//                                                              that meets a transform before it is used
//                           --INTT_P-->    accp
//   rs_spread               accp -> tt [2][L][N]               t_j = ((u + floor(P/2)) mod P) mod q_j - floor(P/2) mod q_j
//                           --NTT-->       tt
//   rs_finish               in, xb, ckey, tt -> out [2][L][N]  (x_j Kc_j - t_j) P^-1 (+ the lift of c0): the product of the
//                                                              data rows is formed HERE, in registers -- it is never stored
// No row is written and read back without a transform in between.  All four are bandwidth-bound element-wise passes: one
// 16-byte record per lane, 256 lanes per workgroup, blockIdx.y = the RNS row (its modulus is uniform per workgroup: scalar
// loads of the constants), blockIdx.z = the polynomial where there are two.
//
// ARITHMETIC.  Every word read is canonical (the transforms' outputs, the caller's operands by the ABI) and every word
// written is canonical: the forward transforms take canonical rows under every policy, so no lazy range crosses a kernel
// boundary.  Inside a lane the only lazy values are the [0, 2q) results of barrett128_lt2q / shoup_lazy, folded by csub
// before their next use; they are named at their lines.  Primes are below 2^61 (hefx_context_create), so sums of two
// canonical words stay below 2^62.  The FP64 policy of small primes concerns the transforms and the key MAC only: these
// passes do integer work mod every prime, like the element-wise kernels of hefx_kernels.hip.
#include "hefx_internal.h"

namespace hefx {

// hefx_collapse_key: out[c][r] = sum_{j<L} key[j][c][m(r)], m(r) = r for r < L, k - 1 for r == L.  key [k-1][2][k][N].
// The running sum is canonical after every step (csub of a value below 2q).
__global__ __launch_bounds__(256) void collapse_key_kernel(DevTables T, int L, const u64 *__restrict__ key, u64 *__restrict__ out)
{
    const int logn = T.logn, k = T.k;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int r = (int)blockIdx.y, c = (int)blockIdx.z;
    const int m = r < L ? r : k - 1;
    const u64 q = T.mods[m].q;
    const size_t digit = (size_t)2 * k << logn;  // words of one digit of the key
    const u64 *p = key + (((size_t)c * k + m) << logn) + 2 * w;
    ulonglong2 s = gld16(p);
    for (int j = 1; j < L; ++j) {
        const ulonglong2 v = gld16(p + (size_t)j * digit);
        s.x = csub(s.x + v.x, q);
        s.y = csub(s.y + v.y, q);
    }
    gst16(out + (((size_t)c * (L + 1) + r) << logn) + 2 * w, s);
}

// the centred lift of one coefficient v in [0, q0) into modulus mc.q: v <= half0 stands for v, otherwise for v - q0
// (hefx_mod_raise's rule).  |x| <= half0 < 2^60 is reduced as a magnitude and negated: canonical either way.  `wide`
// (uniform): q0 > q, the magnitude needs the reduction at all.
__device__ __forceinline__ u64 lift_word(u64 v, u64 q0, u64 half0, const ModConst &mc, bool wide)
{
    const bool neg = v > half0;
    u64 a = neg ? q0 - v : v;                    // [0, half0]
    if (wide) a = barrett64(a, mc.q, mc.r1);     // [0, q)
    return neg ? negmod(a, mc.q) : a;            // a <= half0 < q when !wide: canonical
}

// coef [2][N] = (c0, c1) at q_0 in coefficient form.  blockIdx.y = r: r == 0 -> the special prime's row of x (xp),
// r in 1 .. L-1 -> row r of x (xb[0][r-1]) and row r of c0's lift (xb[1][r-1]).
__global__ __launch_bounds__(256) void rs_expand_kernel(DevTables T, int L, const u64 *__restrict__ coef, u64 *__restrict__ xb,
                                                        u64 *__restrict__ xp)
{
    const int logn = T.logn;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int r = (int)blockIdx.y;
    const int m = r ? r : T.k - 1;
    const ModConst mc = T.mods[m];
    const u64 q0 = T.mods[0].q, half0 = q0 >> 1;
    const bool wide = q0 > mc.q;
    const size_t n = (size_t)1 << logn;
    const ulonglong2 c1 = gld16(coef + n + 2 * w);
    const ulonglong2 x = make_ulonglong2(lift_word(c1.x, q0, half0, mc, wide), lift_word(c1.y, q0, half0, mc, wide));
    if (r == 0) {
        gst16(xp + 2 * w, x);
        return;
    }
    const ulonglong2 c0 = gld16(coef + 2 * w);
    const ulonglong2 y = make_ulonglong2(lift_word(c0.x, q0, half0, mc, wide), lift_word(c0.y, q0, half0, mc, wide));
    gst16(xb + ((size_t)(r - 1) << logn) + 2 * w, x);
    gst16(xb + ((size_t)(L - 1 + r - 1) << logn) + 2 * w, y);
}

// accp[c] = xp * ckey[c][L] mod P, both c from one read of xp.  ckey [2][L+1][N].
__global__ __launch_bounds__(256) void rs_product_p_kernel(DevTables T, int L, const u64 *__restrict__ xp, const u64 *__restrict__ ckey,
                                                           u64 *__restrict__ accp)
{
    const int logn = T.logn;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const ModConst mc = T.mods[T.k - 1];
    const ulonglong2 x = gld16(xp + 2 * w);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const ulonglong2 kk = gld16(ckey + (((size_t)c * (L + 1) + L) << logn) + 2 * w);
        gst16(accp + ((size_t)c << logn) + 2 * w, make_ulonglong2(mulmod(x.x, kk.x, mc), mulmod(x.y, kk.y, mc)));  // canonical
    }
}

// u [2][N] = INTT_P(accp), canonical.  tt[c][j] = ((u + floor(P/2)) mod P) mod q_j - (floor(P/2) mod q_j)  mod q_j.
// blockIdx.y = j, blockIdx.z = c.
__global__ __launch_bounds__(256) void rs_spread_kernel(DevTables T, int L, const u64 *__restrict__ u, u64 *__restrict__ tt)
{
    const int logn = T.logn, k = T.k;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int j = (int)blockIdx.y, c = (int)blockIdx.z;
    const ModConst mc = T.mods[j];
    const u64 P = T.mods[k - 1].q, halfP = P >> 1;
    const u64 half_j = T.halfmod[(size_t)(k - 1) * k + j];  // floor(P/2) mod q_j
    const bool wide = P > mc.q;                             // uniform
    ulonglong2 v = gld16(u + ((size_t)c << logn) + 2 * w);
    v.x = csub(v.x + halfP, P);  // u + half < 2P -> [0, P)
    v.y = csub(v.y + halfP, P);
    if (wide) {
        v.x = barrett64(v.x, mc.q, mc.r1);  // [0, q_j)
        v.y = barrett64(v.y, mc.q, mc.r1);
    }
    gst16(tt + (((size_t)c * L + j) << logn) + 2 * w, make_ulonglong2(submod(v.x, half_j, mc.q), submod(v.y, half_j, mc.q)));
}

// out[c][j] = (x_j * ckey[c][j] - tt[c][j]) * P^-1 mod q_j, plus row j of c0's lift when c == 0.  x_0 and the lift's row 0 are
// the input's own rows (in [2][1][N]); rows 1 .. L-1 come from xb [2][L-1][N].  blockIdx.y = j, blockIdx.z = c.
__global__ __launch_bounds__(256) void rs_finish_kernel(DevTables T, int L, const u64 *__restrict__ in, const u64 *__restrict__ xb,
                                                        const u64 *__restrict__ ckey, const u64 *__restrict__ tt, u64 *__restrict__ out)
{
    const int logn = T.logn, k = T.k;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int j = (int)blockIdx.y, c = (int)blockIdx.z;
    const ModConst mc = T.mods[j];
    const ulonglong2 pinv = T.invmod[(size_t)(k - 1) * k + j];  // {P^-1 mod q_j, its Shoup companion}
    const size_t n = (size_t)1 << logn;
    const u64 *xs = j ? xb + ((size_t)(j - 1) << logn) : in + n;  // row j of x
    const ulonglong2 x = gld16(xs + 2 * w);
    const ulonglong2 kk = gld16(ckey + (((size_t)c * (L + 1) + j) << logn) + 2 * w);
    const ulonglong2 t = gld16(tt + (((size_t)c * L + j) << logn) + 2 * w);
    ulonglong2 v;
    v.x = submod(mulmod(x.x, kk.x, mc), t.x, mc.q);  // canonical - canonical -> canonical
    v.y = submod(mulmod(x.y, kk.y, mc), t.y, mc.q);
    v.x = csub(shoup_lazy(v.x, pinv.x, pinv.y, mc.nq), mc.q);  // shoup_lazy: [0, 2q) -> [0, q)
    v.y = csub(shoup_lazy(v.y, pinv.x, pinv.y, mc.nq), mc.q);
    if (c == 0) {  // uniform
        const u64 *ls = j ? xb + ((size_t)(L - 1 + j - 1) << logn) : in;
        const ulonglong2 l = gld16(ls + 2 * w);
        v.x = addmod(v.x, l.x, mc.q);
        v.y = addmod(v.y, l.y, mc.q);
    }
    gst16(out + (((size_t)c * L + j) << logn) + 2 * w, v);
}

static dim3 ew_grid(const DevTables &T, int rows, int polys)
{
    const size_t row_pairs = (size_t)1 << (T.logn - 1);
    return dim3((unsigned)((row_pairs + 255) / 256), (unsigned)rows, (unsigned)polys);
}

hipError_t launch_collapse_key(const DevTables &T, int L, const u64 *key, u64 *out, hipStream_t s)
{
    hipLaunchKernelGGL(collapse_key_kernel, ew_grid(T, L + 1, 2), dim3(256), 0, s, T, L, key, out);
    return hipGetLastError();
}

hipError_t launch_rs_expand(const DevTables &T, int L, const u64 *coef, u64 *xb, u64 *xp, hipStream_t s)
{
    hipLaunchKernelGGL(rs_expand_kernel, ew_grid(T, L, 1), dim3(256), 0, s, T, L, coef, xb, xp);
    return hipGetLastError();
}

hipError_t launch_rs_product_p(const DevTables &T, int L, const u64 *xp, const u64 *ckey, u64 *accp, hipStream_t s)
{
    hipLaunchKernelGGL(rs_product_p_kernel, ew_grid(T, 1, 1), dim3(256), 0, s, T, L, xp, ckey, accp);
    return hipGetLastError();
}

hipError_t launch_rs_spread(const DevTables &T, int L, const u64 *u, u64 *tt, hipStream_t s)
{
    hipLaunchKernelGGL(rs_spread_kernel, ew_grid(T, L, 2), dim3(256), 0, s, T, L, u, tt);
    return hipGetLastError();
}

hipError_t launch_rs_finish(const DevTables &T, int L, const u64 *in, const u64 *xb, const u64 *ckey, const u64 *tt, u64 *out,
                            hipStream_t s)
{
    hipLaunchKernelGGL(rs_finish_kernel, ew_grid(T, L, 2), dim3(256), 0, s, T, L, in, xb, ckey, tt, out);
    return hipGetLastError();
}

}  // namespace hefx
