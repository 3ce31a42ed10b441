// hefx_hybrid_hoist.hip -- the element-wise kernels of hoisted hybrid key switching (include/hefx_hybrid_hoist.h).  The digit
// decomposition of the n sources is hefx_hybrid.hip's (hy_convert between the engine's transforms), the mod-down's spread is
// hy_spread; the host sequence is hefx_capi.cpp's (hybrid_hoist_run).  New here: the term, the combine and a finish that adds
// nothing (P c0 went into the term).
//
// One call, pass by pass (R = L + alpha rows as in hefx_hybrid.hip; T = n m terms, t = i m + k; O outputs):
//   --INTT-->   xc [n][L][N]                                    c1 of every source, straight from the caller's input
//   hy_convert  xc -> extd [n][dn][L][N], exts [n][dn][alpha][N]   --NTT-->
//   hyh_term    inputs, extd, exts, keys -> Ad [T][2][L][N], As [T][2][alpha][N]
//   hyh_combine Ad, As, plaintexts -> Bd [G][2][L][N], Bs [G][2][alpha][N]        (the combine entry; the rotate entry: B = A)
//   --INTT-->   Bs;  hy_spread  Bs -> tt [O][2][L][N]  --NTT-->
//   hyh_finish  Bd, tt -> the outputs
// The inputs are read by the first INTT and by hyh_term, the outputs written by hyh_finish alone: the strict aliasing rule
// of the header is what makes that order safe.
//
// SHAPE.  256 lanes per workgroup, one 16-byte record (two adjacent coefficients) per lane, blockIdx.y = the RNS row (its
// modulus is uniform per workgroup), blockIdx.z = the term or the output.  hyh_term gathers: records 2w, 2w+1 of pi_g(x) come
// from ONE source record, in either order (hefx_internal.h, galois_index), so a gathered row touches the cache lines of a
// straight read.  Neighbouring terms of one source and row read the SAME digit rows but at different records (another
// element, another index), so there is no load to share between them in registers; they meet in the cache.
//
// ARITHMETIC.  Every word read is canonical (the transforms' outputs, the caller's operands by the ABI), every word written
// is canonical.  The sums are lazy 128-bit sums of products of canonical words below 2^61, each product below 2^122, folded
// ONCE per word by barrett128 (any 128-bit value): at most 61 digits + the P c0 term = 62 products in hyh_term, at most
// HEFX_HYBRID_HOIST_MAX_TERMS = 64 in hyh_combine -- 64 * 2^122 = 2^128 is not reached because every factor is at most
// 2^61 - 2: 64 (2^61 - 2)^2 < 2^128.
#include "hefx_internal.h"

namespace hefx {

__device__ __forceinline__ int hyh_row_mod(const HyTab &H, int k, int r) { return r < H.L ? r : k - H.alpha + (r - H.L); }

// blockIdx.y = row r of R, blockIdx.z = term t = i m + k.  A[c][r] = sum_j pi_g(E_j[r]) key[j][c][r] (+ (P mod q_r) pi_g(c0[r])
// for c == 0, r < L); a NULL key (element 1 by the entry's check): A[c][r] = (P mod q_r) c_c[r] for r < L, 0 on the special rows.
// The digit that owns a data row reads c1's own row from the caller's input.
__global__ __launch_bounds__(256) void hyh_term_kernel(DevTables T, HyTab H, HyhTab X, const u64 *__restrict__ extd,
                                                       const u64 *__restrict__ exts, u64 *__restrict__ Ad, u64 *__restrict__ As)
{
    const int logn = T.logn, L = H.L, A = H.alpha, k = T.k;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;  // the grid covers N / 2 records exactly or with whole idle lanes
    const int r = (int)blockIdx.y, t = (int)blockIdx.z;  // r < L + alpha, t < n m (the launch's grid)
    const int i = t / X.m, kk = t % X.m;
    const int m = hyh_row_mod(H, k, r);
    const ModConst mc = T.mods[m];
    const u64 *in = (const u64 *)H.tab[X.srcs + i];      // [2][L][N]
    const u64 *key0 = (const u64 *)H.tab[X.keys + kk];  // [dnum][2][k][N] or NULL
    const uint32_t elt = (uint32_t)H.tab[X.elts + kk];
    ulonglong2 r0, r1;
    if (!key0) {  // uniform: the identity term
        r0 = r1 = make_ulonglong2(0, 0);
        if (r < L) {
            const u64 pm = H.tab[X.pmod + r];
            const ulonglong2 a = gld16(in + ((size_t)r << logn) + 2 * w), b = gld16(in + ((size_t)(L + r) << logn) + 2 * w);
            r0 = make_ulonglong2(mulmod(a.x, pm, mc), mulmod(a.y, pm, mc));  // canonical x canonical -> canonical
            r1 = make_ulonglong2(mulmod(b.x, pm, mc), mulmod(b.y, pm, mc));
        }
    } else {
        // the source record of records 2w, 2w+1: i0 < N, so (i0 & ~1) + 1 < N -- inside the row
        const uint32_t i0 = elt == 1 ? (uint32_t)(2 * w) : galois_index((uint32_t)(2 * w), elt, logn);
        const size_t at = i0 & ~1u;
        const bool swap = i0 & 1u;
        const u64 *key = key0 + ((size_t)m << logn) + 2 * w;
        const size_t poly = (size_t)k << logn, digit = 2 * poly;  // words of one key polynomial / one key digit
        const int own = r < L ? r / A : -1;
        u64 a0xl = 0, a0xh = 0, a0yl = 0, a0yh = 0, a1xl = 0, a1xh = 0, a1yl = 0, a1yh = 0;
        for (int j = 0; j < H.dn; ++j) {
            const u64 *xs = j == own ? in + ((size_t)(L + r) << logn)
                            : r < L  ? extd + ((size_t)((i * H.dn + j) * L + r) << logn)
                                     : exts + ((size_t)((i * H.dn + j) * A + (r - L)) << logn);
            ulonglong2 x = gld16(xs + at);
            if (swap) x = make_ulonglong2(x.y, x.x);
            const ulonglong2 k0 = gld16(key + (size_t)j * digit), k1 = gld16(key + (size_t)j * digit + poly);
            mac128(a0xl, a0xh, x.x, k0.x);  // canonical x canonical < 2^122; dn <= 61 of them
            mac128(a0yl, a0yh, x.y, k0.y);
            mac128(a1xl, a1xh, x.x, k1.x);
            mac128(a1yl, a1yh, x.y, k1.y);
        }
        if (r < L) {  // uniform: + (P mod q_r) pi_g(c0[r]), the 62nd product at most: 62 * 2^122 < 2^128
            const u64 pm = H.tab[X.pmod + r];
            ulonglong2 c = gld16(in + ((size_t)r << logn) + at);
            if (swap) c = make_ulonglong2(c.y, c.x);
            mac128(a0xl, a0xh, c.x, pm);
            mac128(a0yl, a0yh, c.y, pm);
        }
        r0 = make_ulonglong2(barrett128(a0xl, a0xh, mc), barrett128(a0yl, a0yh, mc));  // one fold per word
        r1 = make_ulonglong2(barrett128(a1xl, a1xh, mc), barrett128(a1yl, a1yh, mc));
    }
    if (r < L) {
        gst16(Ad + ((size_t)((t * 2 + 0) * L + r) << logn) + 2 * w, r0);
        gst16(Ad + ((size_t)((t * 2 + 1) * L + r) << logn) + 2 * w, r1);
    } else {
        gst16(As + ((size_t)((t * 2 + 0) * A + (r - L)) << logn) + 2 * w, r0);
        gst16(As + ((size_t)((t * 2 + 1) * A + (r - L)) << logn) + 2 * w, r1);
    }
}

// blockIdx.y = row r of R, blockIdx.z = output o.  B_o[c][r] = sum_t pt[o][t][m(r)] A_t[c][r] over the terms whose plaintext is
// not NULL; pt [k][N], row m(r) of it.  The entry refuses an output with no term, so no sum is empty.
__global__ __launch_bounds__(256) void hyh_combine_kernel(DevTables T, HyTab H, HyhTab X, const u64 *__restrict__ Ad,
                                                          const u64 *__restrict__ As, u64 *__restrict__ Bd, u64 *__restrict__ Bs)
{
    const int logn = T.logn, L = H.L, A = H.alpha, k = T.k;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int r = (int)blockIdx.y, o = (int)blockIdx.z;  // r < L + alpha, o < G (the launch's grid)
    const int m = hyh_row_mod(H, k, r), terms = X.n * X.m;
    const ModConst mc = T.mods[m];
    const u64 *pts = H.tab + X.pts + (size_t)o * terms;
    u64 a0xl = 0, a0xh = 0, a0yl = 0, a0yh = 0, a1xl = 0, a1xh = 0, a1yl = 0, a1yh = 0;
    for (int t = 0; t < terms; ++t) {
        const u64 *pt = (const u64 *)pts[t];
        if (!pt) continue;  // uniform: a structural zero
        const ulonglong2 p = gld16(pt + ((size_t)m << logn) + 2 * w);
        const u64 *a = r < L ? Ad + ((size_t)(t * 2 * L + r) << logn) : As + ((size_t)(t * 2 * A + (r - L)) << logn);
        const size_t poly = (size_t)(r < L ? L : A) << logn;
        const ulonglong2 x0 = gld16(a + 2 * w), x1 = gld16(a + poly + 2 * w);
        mac128(a0xl, a0xh, x0.x, p.x);  // canonical x canonical <= (2^61 - 2)^2; terms <= 64 of them: < 2^128
        mac128(a0yl, a0yh, x0.y, p.y);
        mac128(a1xl, a1xh, x1.x, p.x);
        mac128(a1yl, a1yh, x1.y, p.y);
    }
    const ulonglong2 r0 = make_ulonglong2(barrett128(a0xl, a0xh, mc), barrett128(a0yl, a0yh, mc));  // one fold per word
    const ulonglong2 r1 = make_ulonglong2(barrett128(a1xl, a1xh, mc), barrett128(a1yl, a1yh, mc));
    if (r < L) {
        gst16(Bd + ((size_t)((o * 2 + 0) * L + r) << logn) + 2 * w, r0);
        gst16(Bd + ((size_t)((o * 2 + 1) * L + r) << logn) + 2 * w, r1);
    } else {
        gst16(Bs + ((size_t)((o * 2 + 0) * A + (r - L)) << logn) + 2 * w, r0);
        gst16(Bs + ((size_t)((o * 2 + 1) * A + (r - L)) << logn) + 2 * w, r1);
    }
}

// out[o][c][j] = (Bd[o][c][j] - tt[o][c][j]) P^-1 mod q_j.  blockIdx.y = j, blockIdx.z = o * 2 + c.  hy_finish without its add.
__global__ __launch_bounds__(256) void hyh_finish_kernel(DevTables T, HyTab H, HyhTab X, const u64 *__restrict__ Bd,
                                                         const u64 *__restrict__ tt)
{
    const int logn = T.logn, L = H.L;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int j = (int)blockIdx.y, o = (int)blockIdx.z >> 1, c = (int)blockIdx.z & 1;  // j < L, o < the outputs (the launch's grid)
    const ModConst mc = T.mods[j];
    const u64 pinv = H.tab[H.pinv + 2 * j], pinvs = H.tab[H.pinv + 2 * j + 1];  // {P^-1 mod q_j, its Shoup companion}
    const size_t at = ((size_t)((o * 2 + c) * L + j) << logn) + 2 * w;
    const ulonglong2 a = gld16(Bd + at), t = gld16(tt + at);
    ulonglong2 v;
    v.x = csub(shoup_lazy(submod(a.x, t.x, mc.q), pinv, pinvs, mc.nq), mc.q);  // canonical - canonical -> canonical; shoup_lazy: [0, 2q) -> [0, q)
    v.y = csub(shoup_lazy(submod(a.y, t.y, mc.q), pinv, pinvs, mc.nq), mc.q);
    gst16((u64 *)H.tab[X.outs + o] + ((size_t)(c * L + j) << logn) + 2 * w, v);
}

static dim3 hyh_grid(const DevTables &T, int rows, int z)
{
    const size_t row_pairs = (size_t)1 << (T.logn - 1);
    return dim3((unsigned)((row_pairs + 255) / 256), (unsigned)rows, (unsigned)z);
}

hipError_t launch_hyh_term(const DevTables &T, const HyTab &H, const HyhTab &X, const u64 *extd, const u64 *exts, u64 *Ad, u64 *As,
                           hipStream_t s)
{
    hipLaunchKernelGGL(hyh_term_kernel, hyh_grid(T, H.L + H.alpha, X.n * X.m), dim3(256), 0, s, T, H, X, extd, exts, Ad, As);
    return hipGetLastError();
}

hipError_t launch_hyh_combine(const DevTables &T, const HyTab &H, const HyhTab &X, const u64 *Ad, const u64 *As, u64 *Bd, u64 *Bs,
                              hipStream_t s)
{
    hipLaunchKernelGGL(hyh_combine_kernel, hyh_grid(T, H.L + H.alpha, X.G), dim3(256), 0, s, T, H, X, Ad, As, Bd, Bs);
    return hipGetLastError();
}

hipError_t launch_hyh_finish(const DevTables &T, const HyTab &H, const HyhTab &X, int outs, const u64 *Bd, const u64 *tt, hipStream_t s)
{
    hipLaunchKernelGGL(hyh_finish_kernel, hyh_grid(T, H.L, 2 * outs), dim3(256), 0, s, T, H, X, Bd, tt);
    return hipGetLastError();
}

}  // namespace hefx
