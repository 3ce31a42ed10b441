// hefx_hybrid.hip -- the element-wise kernels of hybrid key switching (include/hefx_hybrid.h): alpha data primes per RNS
// digit, alpha special primes.  The transforms are the engine's, through hefx_capi.cpp's transform() at every ring size; the
// host sequence and the (alpha, L) constants are hefx_capi.cpp's (hybrid_run, hybrid_consts).  The rows, the shape of a
// launch, the arithmetic ranges and the pieces shared with the hoisted form are hefx_hybrid.cuh's.
//
// One chunk of c items, pass by pass (every arrow that crosses a line is a transform):
//   hy_gather     items -> xn [c][L][N], c0p [c][L][N]     x = pi_g(c1) (or c2 of a relinearisation) and pi_g(c0), NTT form
//                          --INTT-->  xc [c][L][N]
//   hy_convert    xc -> extd [c][dn][L][N], exts [c][dn][alpha][N]   fast base conversion of digit j to every row outside it
//                          --NTT-->   extd (rows 0 .. L-1), exts (the special rows)
//   hy_mac        xn, extd, exts, keys -> accd [c][2][L][N], accs [c][2][alpha][N]
//                          --INTT-->  accs
//   hy_spread     accs -> tt [c][2][L][N]                  the mod-down's remainder, converted from the special rows to the data rows
//                          --NTT-->   tt
//   hy_finish     accd, tt, c0p / the input -> the items' outputs
// hy_gather stages BOTH polynomials of a Galois item: the input is read by that pass alone, so the exact in-place item
// (d_ct_out[i] == d_ct_in[i]) needs no special case.  The own rows of a digit in extd (m in G_j) are never written and
// never read: the MAC takes them from xn.
//
// SHAPE of the lane-loop passes.  hy_gather, hy_mac and hy_finish write one row per workgroup row.  hy_convert and hy_spread
// are the two passes with FEWER source rows than target rows (alpha sources -> up to L + alpha - 1 targets): there the LANE
// loops over the targets.  Write traffic dominates both -- one record written per target either way -- and with the targets
// in the grid every one of them would read the alpha source rows and redo the alpha products y_i (z_t) again:
// alpha (L + alpha) reads and products where alpha suffice.  The loop index is uniform, so the constants of the target are
// scalar loads all the same.  Small batches split the target range over blockIdx.y (at most 4 ways) so that one item still
// fills the chip; every split part redoes the alpha source products, which is why it stays at 4.
#include "hefx_hybrid.cuh"

namespace hefx {

// blockIdx.y = row m, blockIdx.z = item * np + p (np = 1: a relinearisation, x = polynomial 2 as it is; np = 2: a Galois
// item, p == 0 -> x = pi_g(c1), p == 1 -> pi_g(c0)).  out[i] = in[galois_index(i)]; the records 2w, 2w+1 come from ONE
// source record, in either order (hefx_internal.h, galois_index).
__global__ __launch_bounds__(256) void hy_gather_kernel(DevTables T, HyTab H, u64 *__restrict__ xn, u64 *__restrict__ c0p)
{
    const int logn = T.logn, L = H.L;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int m = (int)blockIdx.y, np = H.relin ? 1 : 2;
    const int it = (int)blockIdx.z / np, p = (int)blockIdx.z % np;
    const u64 *item = H.tab + H.items + 4 * (size_t)it;
    const u64 *in = (const u64 *)item[0];
    const uint32_t elt = (uint32_t)item[3];
    const u64 *src = in + ((size_t)((H.relin ? 2 : 1 - p) * L + m) << logn);
    ulonglong2 v;
    if (H.relin || elt == 1) {  // uniform
        v = gld16(src + 2 * w);
    } else {
        const uint32_t i0 = galois_index((uint32_t)(2 * w), elt, logn);
        v = gld16(src + (i0 & ~1u));
        if (i0 & 1u) v = make_ulonglong2(v.y, v.x);
    }
    gst16((p ? c0p : xn) + ((size_t)(it * L + m) << logn) + 2 * w, v);
}

// Digit j = blockIdx.y / split of item blockIdx.z, target rows [r0, r1) of its split part.  y_i = x~_i Dhat_i^-1 mod q_i once
// per lane, then ext_j[m] = sum_i y_i (Dhat_i mod q_m) mod q_m for every row outside the digit.
template <int A>
__global__ __launch_bounds__(256) void hy_convert_kernel(DevTables T, HyTab H, int split, const u64 *__restrict__ xc,
                                                         u64 *__restrict__ extd, u64 *__restrict__ exts)
{
    const int logn = T.logn, L = H.L, R = L + A, k = T.k;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int j = (int)blockIdx.y / split, part = (int)blockIdx.y % split, it = (int)blockIdx.z;
    const int first = j * A, cnt = L - first < A ? L - first : A;  // the digit's rows: first .. first + cnt - 1
    ulonglong2 y[A];
#pragma unroll
    for (int i = 0; i < A; ++i) {
        y[i] = make_ulonglong2(0, 0);
        if (i < cnt) {  // uniform
            const ModConst mc = T.mods[first + i];
            const u64 inv = H.tab[H.inv + 2 * (first + i)], invs = H.tab[H.inv + 2 * (first + i) + 1];
            const ulonglong2 v = gld16(xc + ((size_t)(it * L + first + i) << logn) + 2 * w);
            y[i].x = csub(shoup_lazy(v.x, inv, invs, mc.nq), mc.q);  // shoup_lazy: [0, 2q_i) -> [0, q_i)
            y[i].y = csub(shoup_lazy(v.y, inv, invs, mc.nq), mc.q);
        }
    }
    const int per = (R + split - 1) / split, r0 = part * per, r1 = r0 + per < R ? r0 + per : R;
    for (int r = r0; r < r1; ++r) {
        if (r >= first && r < first + cnt) continue;  // the digit's own rows: x's own NTT rows, nothing to convert
        const ModConst mc = T.mods[hy_row_mod(H, k, r)];
        u64 xl = 0, xh = 0, yl = 0, yh = 0;
#pragma unroll
        for (int i = 0; i < A; ++i) {
            if (i < cnt) {
                const u64 f = H.tab[H.conv + (size_t)(first + i) * R + r];  // Dhat_i mod q_m, canonical
                mac128(xl, xh, y[i].x, f);  // at most HY_ALPHA_MAX products: hefx_hybrid.cuh, ARITHMETIC
                mac128(yl, yh, y[i].y, f);
            }
        }
        const ulonglong2 o = make_ulonglong2(barrett128(xl, xh, mc), barrett128(yl, yh, mc));  // any 128-bit -> [0, q_m)
        u64 *dst = r < L ? extd + ((size_t)((it * H.dn + j) * L + r) << logn) : exts + ((size_t)((it * H.dn + j) * A + (r - L)) << logn);
        gst16(dst + 2 * w, o);
    }
}

// blockIdx.y = row r of R, blockIdx.z = item.  acc[c][r] = sum_j ext_j[m] key[j][c][m] mod q_m over the dn digits; the digit
// that owns a data row reads x's own row from xn.  key [dnum][2][k][N].
__global__ __launch_bounds__(256) void hy_mac_kernel(DevTables T, HyTab H, const u64 *__restrict__ xn, const u64 *__restrict__ extd,
                                                     const u64 *__restrict__ exts, u64 *__restrict__ accd, u64 *__restrict__ accs)
{
    const int logn = T.logn, L = H.L;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int r = (int)blockIdx.y, it = (int)blockIdx.z;
    const int m = hy_row_mod(H, T.k, r);
    const ModConst mc = T.mods[m];
    const u64 *key = (const u64 *)H.tab[H.items + 4 * (size_t)it + 2] + ((size_t)m << logn) + 2 * w;
    HyAcc acc;
    hy_digits_mac(acc, T, H, r, it, xn + ((size_t)(it * L + r) << logn), extd, exts, key, 2 * w, false);
    hy_pair_store(T, H, accd, accs, it, r, w, acc.fold(0, mc), acc.fold(1, mc));
}

// u [c][2][A][N] = INTT of the special rows of acc, canonical.  blockIdx.z = item * 2 + polynomial, blockIdx.y = the split
// part of the L target rows.  z_t = (u_t + floor(P/2) mod q_t) (P/q_t)^-1 mod q_t once per lane, then
// tt[j] = sum_t z_t ((P/q_t) mod q_j) - (floor(P/2) mod q_j)  mod q_j.
template <int A>
__global__ __launch_bounds__(256) void hy_spread_kernel(DevTables T, HyTab H, int split, const u64 *__restrict__ u, u64 *__restrict__ tt)
{
    const int logn = T.logn, L = H.L, k = T.k;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int part = (int)blockIdx.y, z = (int)blockIdx.z;
    ulonglong2 zt[A];
#pragma unroll
    for (int t = 0; t < A; ++t) {
        const ModConst mc = T.mods[k - A + t];
        const u64 half = H.tab[H.halfs + t], inv = H.tab[H.zinv + 2 * t], invs = H.tab[H.zinv + 2 * t + 1];
        const ulonglong2 v = gld16(u + ((size_t)(z * A + t) << logn) + 2 * w);
        zt[t].x = csub(shoup_lazy(csub(v.x + half, mc.q), inv, invs, mc.nq), mc.q);  // u + half < 2q_t -> [0, q_t); shoup_lazy: [0, 2q_t) -> [0, q_t)
        zt[t].y = csub(shoup_lazy(csub(v.y + half, mc.q), inv, invs, mc.nq), mc.q);
    }
    const int per = (L + split - 1) / split, j0 = part * per, j1 = j0 + per < L ? j0 + per : L;
    for (int j = j0; j < j1; ++j) {
        const ModConst mc = T.mods[j];
        u64 xl = 0, xh = 0, yl = 0, yh = 0;
#pragma unroll
        for (int t = 0; t < A; ++t) {
            const u64 f = H.tab[H.phat + (size_t)t * L + j];  // (P/q_t) mod q_j, canonical
            mac128(xl, xh, zt[t].x, f);                       // at most HY_ALPHA_MAX products: hefx_hybrid.cuh, ARITHMETIC
            mac128(yl, yh, zt[t].y, f);
        }
        const u64 half = H.tab[H.halfd + j];
        gst16(tt + ((size_t)(z * L + j) << logn) + 2 * w,
              make_ulonglong2(submod(barrett128(xl, xh, mc), half, mc.q), submod(barrett128(yl, yh, mc), half, mc.q)));
    }
}

// out[c][j] = (acc[c][j] - tt[c][j]) P^-1 mod q_j, plus pi_g(c0) (c == 0 of a Galois item, from c0p) or polynomial c of the
// size-3 input (a relinearisation).  blockIdx.y = j, blockIdx.z = item * 2 + c.
__global__ __launch_bounds__(256) void hy_finish_kernel(DevTables T, HyTab H, const u64 *__restrict__ accd, const u64 *__restrict__ tt,
                                                        const u64 *__restrict__ c0p)
{
    const int logn = T.logn, L = H.L;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int j = (int)blockIdx.y, it = (int)blockIdx.z >> 1, c = (int)blockIdx.z & 1;
    const ModConst mc = T.mods[j];
    const u64 *item = H.tab + H.items + 4 * (size_t)it;
    ulonglong2 v = hy_mod_down(T, H, j, (int)blockIdx.z, w, accd, tt);
    if (H.relin || c == 0) {  // uniform
        const u64 *add = H.relin ? (const u64 *)item[0] + ((size_t)(c * L + j) << logn) : c0p + ((size_t)(it * L + j) << logn);
        const ulonglong2 l = gld16(add + 2 * w);
        v.x = addmod(v.x, l.x, mc.q);
        v.y = addmod(v.y, l.y, mc.q);
    }
    gst16((u64 *)item[1] + ((size_t)(c * L + j) << logn) + 2 * w, v);
}

// hefx_hybrid_keygen's assembly: a uniform [dn][k][N], e noise [dn][k][N] in NTT form.  out[j][1][m] = a_j[m],
// out[j][0][m] = -(a_j[m] sk[m] + e_j[m]) + F_j[m] new_sk[m], F_j[m] = P mod q_m for the data rows of digit j, else 0.
// blockIdx.y = m, blockIdx.z = j.
__global__ __launch_bounds__(256) void hy_keygen_kernel(DevTables T, HyPmod F, int alpha, const u64 *__restrict__ sk,
                                                        const u64 *__restrict__ new_sk, const u64 *__restrict__ a, const u64 *__restrict__ e,
                                                        u64 *__restrict__ out)
{
    const int logn = T.logn, k = T.k;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int m = (int)blockIdx.y, j = (int)blockIdx.z;
    const ModConst mc = T.mods[m];
    const size_t row = ((size_t)m << logn) + 2 * w, at = ((size_t)j * k << logn) + row;
    const ulonglong2 av = gld16(a + at), ev = gld16(e + at), sv = gld16(sk + row);
    ulonglong2 c0;
    c0.x = negmod(addmod(mulmod(av.x, sv.x, mc), ev.x, mc.q), mc.q);  // canonical at every step
    c0.y = negmod(addmod(mulmod(av.y, sv.y, mc), ev.y, mc.q), mc.q);
    if (m < k - alpha && m / alpha == j) {  // uniform: a data row of this digit
        const ulonglong2 ns = gld16(new_sk + row);
        c0.x = addmod(c0.x, mulmod(ns.x, F.v[m], mc), mc.q);
        c0.y = addmod(c0.y, mulmod(ns.y, F.v[m], mc), mc.q);
    }
    gst16(out + ((size_t)(j * 2 + 0) * k << logn) + row, c0);
    gst16(out + ((size_t)(j * 2 + 1) * k << logn) + row, av);
}

// how many ways a lane-loop pass splits its target range: enough workgroups for the chip (about four per CU of 256), at most 4
static int hy_split(const DevTables &T, int groups, int targets)
{
    const size_t wgs = (((size_t)1 << (T.logn - 1)) + 255) / 256 * (size_t)groups;
    int s = 1;
    while (s < 4 && wgs * s < 1024 && 2 * s <= targets) s *= 2;
    return s;
}

hipError_t launch_hy_gather(const DevTables &T, const HyTab &H, int n, u64 *xn, u64 *c0p, hipStream_t s)
{
    hipLaunchKernelGGL(hy_gather_kernel, hy_grid(T, H.L, n * (H.relin ? 1 : 2)), dim3(256), 0, s, T, H, xn, c0p);
    return hipGetLastError();
}

template <int A>
static void hy_convert_a(const DevTables &T, const HyTab &H, int n, int split, const u64 *xc, u64 *extd, u64 *exts, hipStream_t s)
{
    hipLaunchKernelGGL((hy_convert_kernel<A>), hy_grid(T, H.dn * split, n), dim3(256), 0, s, T, H, split, xc, extd, exts);
}
template <int A>
static void hy_spread_a(const DevTables &T, const HyTab &H, int n, int split, const u64 *u, u64 *tt, hipStream_t s)
{
    hipLaunchKernelGGL((hy_spread_kernel<A>), hy_grid(T, split, 2 * n), dim3(256), 0, s, T, H, split, u, tt);
}
#define HY_ALPHA_SWITCH(fn, ...)                    \
    switch (H.alpha) {                              \
    case 1: fn<1>(__VA_ARGS__); break;              \
    case 2: fn<2>(__VA_ARGS__); break;              \
    case 3: fn<3>(__VA_ARGS__); break;              \
    case 4: fn<4>(__VA_ARGS__); break;              \
    case 5: fn<5>(__VA_ARGS__); break;              \
    case 6: fn<6>(__VA_ARGS__); break;              \
    case 7: fn<7>(__VA_ARGS__); break;              \
    case 8: fn<8>(__VA_ARGS__); break;              \
    default: return hipErrorInvalidValue;           \
    }

hipError_t launch_hy_convert(const DevTables &T, const HyTab &H, int n, const u64 *xc, u64 *extd, u64 *exts, hipStream_t s)
{
    const int split = hy_split(T, H.dn * n, H.L + H.alpha);
    HY_ALPHA_SWITCH(hy_convert_a, T, H, n, split, xc, extd, exts, s)
    return hipGetLastError();
}

hipError_t launch_hy_mac(const DevTables &T, const HyTab &H, int n, const u64 *xn, const u64 *extd, const u64 *exts, u64 *accd, u64 *accs,
                         hipStream_t s)
{
    hipLaunchKernelGGL(hy_mac_kernel, hy_grid(T, H.L + H.alpha, n), dim3(256), 0, s, T, H, xn, extd, exts, accd, accs);
    return hipGetLastError();
}

hipError_t launch_hy_spread(const DevTables &T, const HyTab &H, int n, const u64 *u, u64 *tt, hipStream_t s)
{
    const int split = hy_split(T, 2 * n, H.L);
    HY_ALPHA_SWITCH(hy_spread_a, T, H, n, split, u, tt, s)
    return hipGetLastError();
}

hipError_t launch_hy_finish(const DevTables &T, const HyTab &H, int n, const u64 *accd, const u64 *tt, const u64 *c0p, hipStream_t s)
{
    hipLaunchKernelGGL(hy_finish_kernel, hy_grid(T, H.L, 2 * n), dim3(256), 0, s, T, H, accd, tt, c0p);
    return hipGetLastError();
}

hipError_t launch_hy_keygen(const DevTables &T, const HyPmod &F, int alpha, int dn, const u64 *sk, const u64 *new_sk, const u64 *a,
                            const u64 *e, u64 *out, hipStream_t s)
{
    hipLaunchKernelGGL(hy_keygen_kernel, hy_grid(T, T.k, dn), dim3(256), 0, s, T, F, alpha, sk, new_sk, a, e, out);
    return hipGetLastError();
}

}  // namespace hefx
