// hefx_hybrid_hoist.hip -- the element-wise kernels of hoisted hybrid key switching (include/hefx_hybrid_hoist.h).  The digit
// decomposition of the n sources is hefx_hybrid.hip's (hy_convert between the engine's transforms), the mod-down's spread is
// hy_spread; the host sequence is hefx_capi.cpp's (hybrid_hoist_run).  The rows, the shape of a launch, the arithmetic ranges
// and the pieces shared with hefx_hybrid.hip are hefx_hybrid.cuh's.  Here: the term, the combine and a finish that adds
// nothing (P c0 went into the term).
//
// One call, pass by pass (T = n m terms, t = i m + k; O outputs):
//   --INTT-->   xc [n][L][N]                                    c1 of every source, straight from the caller's input
//   hy_convert  xc -> extd [n][dn][L][N], exts [n][dn][alpha][N]   --NTT-->
//   hyh_term    inputs, extd, exts, keys -> Ad [T][2][L][N], As [T][2][alpha][N]
//   hyh_combine Ad, As, plaintexts -> Bd [G][2][L][N], Bs [G][2][alpha][N]        (the combine entry; the rotate entry: B = A)
//   --INTT-->   Bs;  hy_spread  Bs -> tt [O][2][L][N]  --NTT-->
//   hyh_finish  Bd, tt -> the outputs
// The inputs are read by the first INTT and by hyh_term, the outputs written by hyh_finish alone: the strict aliasing rule
// of the header is what makes that order safe.
//
// Neighbouring terms of one source and row read the SAME digit rows but at different records (another element, another
// index), so there is no load to share between them in registers; they meet in the cache.
#include "hefx_hybrid.cuh"

namespace hefx {

// blockIdx.y = row r of R, blockIdx.z = term t = i m + k.  A[c][r] = sum_j pi_g(E_j[r]) key[j][c][r] (+ (P mod q_r) pi_g(c0[r])
// for c == 0, r < L); a NULL key (element 1 by the entry's check): A[c][r] = (P mod q_r) c_c[r] for r < L, 0 on the special rows.
// The digit that owns a data row reads c1's own row from the caller's input.
__global__ __launch_bounds__(256) void hyh_term_kernel(DevTables T, HyTab H, HyhTab X, const u64 *__restrict__ extd,
                                                       const u64 *__restrict__ exts, u64 *__restrict__ Ad, u64 *__restrict__ As)
{
    const int logn = T.logn, L = H.L;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int r = (int)blockIdx.y, t = (int)blockIdx.z;  // r < L + alpha, t < n m (the launch's grid)
    const int i = t / X.m, kk = t % X.m;
    const int m = hy_row_mod(H, T.k, r);
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
        HyAcc acc;
        hy_digits_mac(acc, T, H, r, i, in + ((size_t)(L + r) << logn), extd, exts, key0 + ((size_t)m << logn) + 2 * w, at, swap);
        if (r < L) {  // uniform: + (P mod q_r) pi_g(c0[r])
            const u64 pm = H.tab[X.pmod + r];
            acc.mac(0, hy_ld(in + ((size_t)r << logn), at, swap), make_ulonglong2(pm, pm));
        }
        r0 = acc.fold(0, mc), r1 = acc.fold(1, mc);
    }
    hy_pair_store(T, H, Ad, As, t, r, w, r0, r1);
}

// blockIdx.y = row r of R, blockIdx.z = output o.  B_o[c][r] = sum_t pt[o][t][m(r)] A_t[c][r] over the terms whose plaintext is
// not NULL; pt [k][N], row m(r) of it.  The entry refuses an output with no term, so no sum is empty.
__global__ __launch_bounds__(256) void hyh_combine_kernel(DevTables T, HyTab H, HyhTab X, const u64 *__restrict__ Ad,
                                                          const u64 *__restrict__ As, u64 *__restrict__ Bd, u64 *__restrict__ Bs)
{
    const int logn = T.logn;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int r = (int)blockIdx.y, o = (int)blockIdx.z;  // r < L + alpha, o < G (the launch's grid)
    const int m = hy_row_mod(H, T.k, r), terms = X.n * X.m;
    const ModConst mc = T.mods[m];
    const u64 *pts = H.tab + X.pts + (size_t)o * terms;
    HyAcc acc;
    for (int t = 0; t < terms; ++t) {
        const u64 *pt = (const u64 *)pts[t];
        if (!pt) continue;  // uniform: a structural zero
        const ulonglong2 p = gld16(pt + ((size_t)m << logn) + 2 * w);
        size_t poly;
        const u64 *a = hy_pair(T, H, Ad, As, t, r, w, poly);
        acc.mac(0, gld16(a), p);
        acc.mac(1, gld16(a + poly), p);
    }
    hy_pair_store(T, H, Bd, Bs, o, r, w, acc.fold(0, mc), acc.fold(1, mc));
}

// out[o][c][j] = (Bd[o][c][j] - tt[o][c][j]) P^-1 mod q_j.  blockIdx.y = j, blockIdx.z = o * 2 + c.
__global__ __launch_bounds__(256) void hyh_finish_kernel(DevTables T, HyTab H, HyhTab X, const u64 *__restrict__ Bd,
                                                         const u64 *__restrict__ tt)
{
    const int logn = T.logn, L = H.L;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int j = (int)blockIdx.y, o = (int)blockIdx.z >> 1, c = (int)blockIdx.z & 1;  // j < L, o < the outputs (the launch's grid)
    gst16((u64 *)H.tab[X.outs + o] + ((size_t)(c * L + j) << logn) + 2 * w, hy_mod_down(T, H, j, (int)blockIdx.z, w, Bd, tt));
}

hipError_t launch_hyh_term(const DevTables &T, const HyTab &H, const HyhTab &X, const u64 *extd, const u64 *exts, u64 *Ad, u64 *As,
                           hipStream_t s)
{
    hipLaunchKernelGGL(hyh_term_kernel, hy_grid(T, H.L + H.alpha, X.n * X.m), dim3(256), 0, s, T, H, X, extd, exts, Ad, As);
    return hipGetLastError();
}

hipError_t launch_hyh_combine(const DevTables &T, const HyTab &H, const HyhTab &X, const u64 *Ad, const u64 *As, u64 *Bd, u64 *Bs,
                              hipStream_t s)
{
    hipLaunchKernelGGL(hyh_combine_kernel, hy_grid(T, H.L + H.alpha, X.G), dim3(256), 0, s, T, H, X, Ad, As, Bd, Bs);
    return hipGetLastError();
}

hipError_t launch_hyh_finish(const DevTables &T, const HyTab &H, const HyhTab &X, int outs, const u64 *Bd, const u64 *tt, hipStream_t s)
{
    hipLaunchKernelGGL(hyh_finish_kernel, hy_grid(T, H.L, 2 * outs), dim3(256), 0, s, T, H, X, Bd, tt);
    return hipGetLastError();
}

}  // namespace hefx
