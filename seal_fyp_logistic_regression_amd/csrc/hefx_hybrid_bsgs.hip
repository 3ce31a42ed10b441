// hefx_hybrid_bsgs.hip -- the element-wise kernels of the hoisted giant steps (include/hefx_hybrid_bsgs.h).  The baby phase is
// hefx_hybrid_hoist.hip's (hyh_term, hyh_combine), the conversions and the spread are hefx_hybrid.hip's (hy_convert,
// hy_spread), the output's finish is hyh_finish; the host sequence is hefx_capi.cpp's (hybrid_bsgs_run).  Rows, launch shape
// and arithmetic ranges are hefx_hybrid.cuh's.  Here: the mod-down finish of ONE polynomial per giant-rotated inner sum, and
// the giant kernel.
//
// One call, pass by pass (G inner sums, O outputs; a chunk holds C giant-rotated inner sums, s = their slot in the chunk):
//   ... as hefx_hybrid_hoist.hip up to hyh_combine -> Bd [G][2][L][N], Bs [G][2][alpha][N], both in NTT form
//   per chunk:  --INTT-->  us [C][alpha][N] from Bs[o][1];  hy_spread us -> tt1 [C][L][N]  --NTT-->
//               hyb_down   Bd[o][1], tt1 -> dd [C][L][N]                       d_o, NTT form
//               --INTT-->  xc2;  hy_convert xc2 -> ext2d [C][dn][L][N], ext2s [C][dn][alpha][N]  --NTT-->
//               hyb_giant  dd, ext2, giant keys, Bd, Bs -> Wd [O][2][L][N], Ws [O][2][alpha][N] (+= across chunks)
//   --INTT-->   Ws;  hy_spread Ws -> tt [O][2][L][N]  --NTT-->  hyh_finish Wd, tt -> the outputs
//
// The gather of the giant kernel is its only irregular access: records 2w, 2w+1 of pi_g(x) come from ONE source record
// (hefx_hybrid.cuh, SHAPE), so every read is one 16-byte load.  No LDS: nothing is shared between lanes.
//
// THE LAZY RANGE of hyb_giant's accumulator.  HyAcc holds 128-bit sums of products of canonical words, each below 2^122, and
// takes HY_SUM_MAX = 64 of them (hefx_hybrid.cuh, ARITHMETIC).  A canonical word ADDED to the sum (a row of B_o, a carried
// row of W) is below 2^61 < 2^122 and is counted as one product.  A giant-rotated inner sum adds dn products (its digits
// against the key) and one word (pi_g(B_o[0])): dn + 1 <= 62 steps; an unrotated one adds one word.  Up to
// HEFX_HYBRID_HOIST_MAX_OUT = 64 inner sums may feed one output -- 64 * 62 steps -- so the kernel counts: before an inner sum
// whose steps would take the count past HY_SUM_MAX, both sums are folded to canonical words, which then count as ONE step.
// 1 + 62 <= 64, so one inner sum always fits behind a fold (the assertion below).  The count depends on the table alone:
// the fold is uniform over the grid row.
#include "hefx_hybrid.cuh"

namespace hefx {

static_assert(1 + sizeof(HyPmod::v) / sizeof(u64) + 1 <= HY_SUM_MAX, "a folded word, a chain's digits and the B_o[0] word pass HY_SUM_MAX");

// polynomial c of acc += v, word by word: a canonical word, one step of the lazy range above
__device__ __forceinline__ void hyb_add(HyAcc &acc, int c, const ulonglong2 &v)
{
    acc.lo[c][0] += v.x;
    acc.hi[c][0] += acc.lo[c][0] < v.x;
    acc.lo[c][1] += v.y;
    acc.hi[c][1] += acc.lo[c][1] < v.y;
}

// dd[s][j] = (Bd[o][1][j] - tt1[s][j]) P^-1 mod q_j, o = the inner sum in slot s of the chunk that starts at rank c0.
// blockIdx.y = j < L, blockIdx.z = s < the chunk's count (the launch's grid).
__global__ __launch_bounds__(256) void hyb_down_kernel(DevTables T, HyTab H, HybTab Y, int c0, const u64 *__restrict__ Bd,
                                                       const u64 *__restrict__ tt1, u64 *__restrict__ dd)
{
    const int logn = T.logn, L = H.L;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int j = (int)blockIdx.y, s = (int)blockIdx.z;
    const int o = (int)H.tab[Y.sel + c0 + s];  // o >= s: the ranks are taken in the order of o
    // hy_mod_down reads acc and tt at the same z = s: Bd is handed over shifted so that z = s lands on polynomial 1 of o
    gst16(dd + ((size_t)(s * L + j) << logn) + 2 * w, hy_mod_down(T, H, j, s, w, Bd + ((size_t)(2 * o + 1 - s) * L << logn), tt1));
}

// blockIdx.y = row r of R, blockIdx.z = output q.  Over the inner sums o in [o_lo, o_hi) with dest[o] == q:
//   giant key:  W[c][r] += sum_j pi_g(F_{o,j}[r]) K'[j][c][m(r)]  (+ pi_g(B_o[0][r]) for c == 0);   NULL:  W[c][r] += B_o[c][r].
// W[q] is read first when an inner sum below o_lo fed it (an earlier chunk wrote it), and written once; a workgroup row whose
// output has no inner sum in the range leaves W[q] as it is.
__global__ __launch_bounds__(256) void hyb_giant_kernel(DevTables T, HyTab H, HybTab Y, int o_lo, int o_hi, int c0,
                                                        const u64 *__restrict__ Bd, const u64 *__restrict__ Bs, const u64 *__restrict__ dd,
                                                        const u64 *__restrict__ extd, const u64 *__restrict__ exts, u64 *Wd, u64 *Ws)
{
    const int logn = T.logn, L = H.L;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int r = (int)blockIdx.y, q = (int)blockIdx.z;  // r < L + alpha, q < O (the launch's grid)
    const int m = hy_row_mod(H, T.k, r);
    const ModConst mc = T.mods[m];
    const u64 *dest = H.tab + Y.dest, *gkeys = H.tab + Y.gkeys, *gelts = H.tab + Y.gelts, *rank = H.tab + Y.rank;
    bool carried = false, any = false;
    for (int o = 0; o < o_lo; ++o) carried |= (int)dest[o] == q;
    for (int o = o_lo; o < o_hi; ++o) any |= (int)dest[o] == q;
    if (!any) return;  // uniform
    HyAcc acc;
    int steps = 0;  // of the lazy range (the head of this file)
    size_t poly;
    if (carried) {
        const u64 *a = hy_pair(T, H, (const u64 *)Wd, (const u64 *)Ws, q, r, w, poly);
        hyb_add(acc, 0, gld16(a));
        hyb_add(acc, 1, gld16(a + poly));
        steps = 1;
    }
    for (int o = o_lo; o < o_hi; ++o) {
        if ((int)dest[o] != q) continue;  // uniform
        const u64 *key0 = (const u64 *)gkeys[o];
        const int need = key0 ? H.dn + 1 : 1;
        if (steps + need > HY_SUM_MAX) {  // uniform: fold, the folded words are one step
            const ulonglong2 f0 = acc.fold(0, mc), f1 = acc.fold(1, mc);
            acc = HyAcc();
            hyb_add(acc, 0, f0);
            hyb_add(acc, 1, f1);
            steps = 1;
        }
        steps += need;
        if (!key0) {  // uniform: no giant rotation
            const u64 *a = hy_pair(T, H, Bd, Bs, o, r, w, poly);
            hyb_add(acc, 0, gld16(a));
            hyb_add(acc, 1, gld16(a + poly));
            continue;
        }
        // the source record of records 2w, 2w+1: i0 < N, so (i0 & ~1) + 1 < N -- inside the row
        const uint32_t i0 = galois_index((uint32_t)(2 * w), (uint32_t)gelts[o], logn);
        const size_t at = i0 & ~1u;
        const bool swap = i0 & 1u;
        const int s = (int)rank[o] - c0;  // the inner sum's slot in the chunk
        hy_digits_mac(acc, T, H, r, s, dd + ((size_t)(s * L + r) << logn), extd, exts, key0 + ((size_t)m << logn) + 2 * w, at, swap);
        hyb_add(acc, 0, hy_ld(hy_pair(T, H, Bd, Bs, o, r, 0, poly), at, swap));
    }
    hy_pair_store(T, H, Wd, Ws, q, r, w, acc.fold(0, mc), acc.fold(1, mc));
}

hipError_t launch_hyb_down(const DevTables &T, const HyTab &H, const HybTab &Y, int c0, int cnt, const u64 *Bd, const u64 *tt1, u64 *dd,
                           hipStream_t s)
{
    hipLaunchKernelGGL(hyb_down_kernel, hy_grid(T, H.L, cnt), dim3(256), 0, s, T, H, Y, c0, Bd, tt1, dd);
    return hipGetLastError();
}

hipError_t launch_hyb_giant(const DevTables &T, const HyTab &H, const HybTab &Y, int o_lo, int o_hi, int c0, const u64 *Bd, const u64 *Bs,
                            const u64 *dd, const u64 *extd, const u64 *exts, u64 *Wd, u64 *Ws, hipStream_t s)
{
    hipLaunchKernelGGL(hyb_giant_kernel, hy_grid(T, H.L + H.alpha, Y.O), dim3(256), 0, s, T, H, Y, o_lo, o_hi, c0, Bd, Bs, dd, extd, exts, Wd, Ws);
    return hipGetLastError();
}

}  // namespace hefx
