// hefx_hybrid_encaps.hip -- the element-wise kernels of sparse-secret encapsulation on hybrid keys
// (include/ext/hefx_hybrid_encaps.h): the collapsed hybrid key and the passes between the transforms of
// hefx_hybrid_raise_switch.  The transforms are the engine's, through hefx_capi.cpp's transform() at every ring size; the host
// sequence is hefx_capi.cpp's; the (alpha, L) constants are the table of the hybrid switch (HyTab, hybrid_consts).  The rows
// and the shape of a launch are hefx_hybrid.cuh's, the passes have the shape of hefx_encaps.hip's.
//
// hefx_hybrid_raise_switch, pass by pass (L = L_out, A = alpha; every arrow that crosses a line is a transform):
//   in [2][1][N]            --INTT_q0-->   coef [2][N]                         (c0, c1 in coefficient form)
//   hye_expand              coef -> xb [2][L-1][N], xs [A][N]    x, the centred lift of c1, mod q_1 .. q_(L-1) and mod the A
//                                                                special primes, and y, that of c0, mod q_1 .. q_(L-1), in ONE
//                                                                pass over the two coefficient rows
//                           --NTT-->       xb, xs
//   hye_product             xs, ckey[.][L ..] -> accs [2][A][N]  the special rows of x Kc for both c from one read of x: the only
//                                                                rows of the product that meet a transform before they are used
//                           --INTT-->      accs
//   hy_spread (n = 1)       accs -> tt [2][L][N]                 hefx_hybrid.hip's own pass: u [2][A][N] -> t_j, its layout
//                           --NTT-->       tt
//   hye_finish              in, xb, ckey, tt -> out [2][L][N]    (x_j Kc_j - t_j) P^-1 (+ y_j): the product of the data rows is
//                                                                formed HERE, in registers -- it is never stored
// No row is written and read back without a transform in between.  All are bandwidth-bound element-wise passes: one 16-byte
// record per lane, 256 lanes per workgroup, blockIdx.y = the RNS row (its modulus and constants are uniform per workgroup:
// scalar loads), blockIdx.z = the polynomial where there are two.
//
// ARITHMETIC.  hefx_hybrid.cuh's: every word read and written is canonical.  Inside a lane the only lazy values are the
// [0, 2q) results of shoup_lazy, folded by csub at their line.  The collapse's running sum is canonical after every step.
#include "hefx_hybrid.cuh"

namespace hefx {

// the prime of row r of R = L + A rows (hy_row_mod without a table)
__device__ __forceinline__ int hye_row_mod(int k, int A, int L, int r) { return r < L ? r : k - A + (r - L); }

// hefx_hybrid_collapse_key: out[c][r] = sum_{j<dn} key[j][c][m(r)] mod q_m(r).  key [dnum][2][k][N], out [2][L+A][N].
// blockIdx.y = r, blockIdx.z = c.
__global__ __launch_bounds__(256) void hye_collapse_kernel(DevTables T, int A, int L, int dn, const u64 *__restrict__ key, u64 *__restrict__ out)
{
    const int logn = T.logn, k = T.k;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int r = (int)blockIdx.y, c = (int)blockIdx.z;
    const int m = hye_row_mod(k, A, L, r);
    const u64 q = T.mods[m].q;
    const size_t digit = (size_t)2 * k << logn;  // words of one digit of the key
    const u64 *p = key + (((size_t)c * k + m) << logn) + 2 * w;
    ulonglong2 s = gld16(p);
    for (int j = 1; j < dn; ++j) {
        const ulonglong2 v = gld16(p + (size_t)j * digit);
        s.x = csub(s.x + v.x, q);  // canonical + canonical < 2q -> [0, q)
        s.y = csub(s.y + v.y, q);
    }
    gst16(out + (((size_t)c * (L + A) + r) << logn) + 2 * w, s);
}

// the centred lift of one coefficient v in [0, q0) into modulus mc.q: v <= half0 stands for v, otherwise for v - q0
// (hefx_mod_raise's rule; hefx_encaps.hip's lift_word, which is local to that file).  |x| <= half0 < 2^60 is reduced as a
// magnitude and negated: canonical either way.  `wide` (uniform): q0 > q, the magnitude needs the reduction at all.
__device__ __forceinline__ u64 hye_lift(u64 v, u64 q0, u64 half0, const ModConst &mc, bool wide)
{
    const bool neg = v > half0;
    u64 a = neg ? q0 - v : v;                    // [0, half0]
    if (wide) a = barrett64(a, mc.q, mc.r1);     // [0, q)
    return neg ? negmod(a, mc.q) : a;            // a <= half0 < q when !wide: canonical
}

// coef [2][N] = (c0, c1) at q_0 in coefficient form.  blockIdx.y = r: r < A -> special row r of x (xs[r]); r >= A -> data
// row j = r - A + 1 of x (xb[0][j-1]) and of y (xb[1][j-1]).
__global__ __launch_bounds__(256) void hye_expand_kernel(DevTables T, int A, int L, const u64 *__restrict__ coef, u64 *__restrict__ xb,
                                                         u64 *__restrict__ xs)
{
    const int logn = T.logn;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int r = (int)blockIdx.y;
    const bool special = r < A;  // uniform
    const int j = r - A + 1;
    const ModConst mc = T.mods[special ? T.k - A + r : j];
    const u64 q0 = T.mods[0].q, half0 = q0 >> 1;
    const bool wide = q0 > mc.q;
    const size_t n = (size_t)1 << logn;
    const ulonglong2 c1 = gld16(coef + n + 2 * w);
    const ulonglong2 x = make_ulonglong2(hye_lift(c1.x, q0, half0, mc, wide), hye_lift(c1.y, q0, half0, mc, wide));
    if (special) {
        gst16(xs + ((size_t)r << logn) + 2 * w, x);
        return;
    }
    const ulonglong2 c0 = gld16(coef + 2 * w);
    const ulonglong2 y = make_ulonglong2(hye_lift(c0.x, q0, half0, mc, wide), hye_lift(c0.y, q0, half0, mc, wide));
    gst16(xb + ((size_t)(j - 1) << logn) + 2 * w, x);
    gst16(xb + ((size_t)(L - 1 + j - 1) << logn) + 2 * w, y);
}

// accs[c][t] = xs[t] * ckey[c][L + t] mod q_(k-A+t), both c from one read of xs.  ckey [2][L+A][N].  blockIdx.y = t.
__global__ __launch_bounds__(256) void hye_product_kernel(DevTables T, int A, int L, const u64 *__restrict__ xs, const u64 *__restrict__ ckey,
                                                          u64 *__restrict__ accs)
{
    const int logn = T.logn;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int t = (int)blockIdx.y;
    const ModConst mc = T.mods[T.k - A + t];
    const ulonglong2 x = gld16(xs + ((size_t)t << logn) + 2 * w);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const ulonglong2 kk = gld16(ckey + (((size_t)c * (L + A) + L + t) << logn) + 2 * w);
        gst16(accs + (((size_t)c * A + t) << logn) + 2 * w, make_ulonglong2(mulmod(x.x, kk.x, mc), mulmod(x.y, kk.y, mc)));  // canonical
    }
}

// out[c][j] = (x_j * ckey[c][j] - tt[c][j]) * P^-1 mod q_j, plus y_j when c == 0.  x_0 and y_0 are the input's own rows
// (in [2][1][N]); rows 1 .. L-1 come from xb [2][L-1][N].  blockIdx.y = j, blockIdx.z = c.
__global__ __launch_bounds__(256) void hye_finish_kernel(DevTables T, HyTab H, const u64 *__restrict__ in, const u64 *__restrict__ xb,
                                                         const u64 *__restrict__ ckey, const u64 *__restrict__ tt, u64 *__restrict__ out)
{
    const int logn = T.logn, L = H.L;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int j = (int)blockIdx.y, c = (int)blockIdx.z;
    const ModConst mc = T.mods[j];
    const u64 pinv = H.tab[H.pinv + 2 * j], pinvs = H.tab[H.pinv + 2 * j + 1];  // {P^-1 mod q_j, its Shoup companion}
    const size_t n = (size_t)1 << logn;
    const u64 *xr = j ? xb + ((size_t)(j - 1) << logn) : in + n;  // row j of x
    const ulonglong2 x = gld16(xr + 2 * w);
    const ulonglong2 kk = gld16(ckey + (((size_t)c * (L + H.alpha) + j) << logn) + 2 * w);
    const ulonglong2 t = gld16(tt + (((size_t)c * L + j) << logn) + 2 * w);
    ulonglong2 v;
    v.x = submod(mulmod(x.x, kk.x, mc), t.x, mc.q);  // canonical - canonical -> canonical
    v.y = submod(mulmod(x.y, kk.y, mc), t.y, mc.q);
    v.x = csub(shoup_lazy(v.x, pinv, pinvs, mc.nq), mc.q);  // shoup_lazy: [0, 2q) -> [0, q)
    v.y = csub(shoup_lazy(v.y, pinv, pinvs, mc.nq), mc.q);
    if (c == 0) {  // uniform
        const u64 *yr = j ? xb + ((size_t)(L - 1 + j - 1) << logn) : in;
        const ulonglong2 y = gld16(yr + 2 * w);
        v.x = addmod(v.x, y.x, mc.q);
        v.y = addmod(v.y, y.y, mc.q);
    }
    gst16(out + (((size_t)c * L + j) << logn) + 2 * w, v);
}

hipError_t launch_hye_collapse(const DevTables &T, int alpha, int L, int dn, const u64 *key, u64 *out, hipStream_t s)
{
    hipLaunchKernelGGL(hye_collapse_kernel, hy_grid(T, L + alpha, 2), dim3(256), 0, s, T, alpha, L, dn, key, out);
    return hipGetLastError();
}

hipError_t launch_hye_expand(const DevTables &T, int alpha, int L, const u64 *coef, u64 *xb, u64 *xs, hipStream_t s)
{
    hipLaunchKernelGGL(hye_expand_kernel, hy_grid(T, L - 1 + alpha, 1), dim3(256), 0, s, T, alpha, L, coef, xb, xs);
    return hipGetLastError();
}

hipError_t launch_hye_product(const DevTables &T, int alpha, int L, const u64 *xs, const u64 *ckey, u64 *accs, hipStream_t s)
{
    hipLaunchKernelGGL(hye_product_kernel, hy_grid(T, alpha, 1), dim3(256), 0, s, T, alpha, L, xs, ckey, accs);
    return hipGetLastError();
}

hipError_t launch_hye_finish(const DevTables &T, const HyTab &H, const u64 *in, const u64 *xb, const u64 *ckey, const u64 *tt, u64 *out,
                             hipStream_t s)
{
    hipLaunchKernelGGL(hye_finish_kernel, hy_grid(T, H.L, 2), dim3(256), 0, s, T, H, in, xb, ckey, tt, out);
    return hipGetLastError();
}

}  // namespace hefx
