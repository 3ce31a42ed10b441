// hefx_poly.hip -- the kernel of hefx_scalar_combine (include/hefx_poly.h): G scalar combinations of the same m ciphertexts,
//   out_g = sum_k w[g][k] * ct_k + c_g,
// in one pass over the inputs.  The inner loop of a polynomial evaluator (a leaf of Paterson-Stockmeyer, a Chebyshev
// recurrence step, the sum of a node's products): w and c are constants, and the NTT of a constant polynomial is that
// constant in every slot, so a weight is ONE word per RNS row -- block-uniform, a scalar load -- where mulplain_sum_kernel
// reads a plaintext word per ciphertext word.
#include "hefx_internal.h"

namespace hefx {

// TABLE (device words, one descriptor-ring slot per launch; GT = the launch's tile width):
//   [0, m)                 input pointers
//   [m, 2m)                words between two polynomials of input k (its own row count * N): an input of a higher level is
//                          read through its own stride -- its row prefix IS the mod-dropped ciphertext, no copy
//   [2m, 2m + GT)          output pointers, the first G of them valid
//   then [L][m][GT]        weights, row-major per RNS row so that the GT weights of a term are adjacent scalar loads;
//                          outputs g >= G of the tile carry zero weights and are not stored
//   then [L][GT]           constants (has_const)
// One workgroup works on 256 adjacent 16-byte records of ONE row (p, j): blockIdx.y = p * L + j, so the modulus, the weights
// and the constants are uniform per workgroup.  A lane loads 16 bytes of every input once and feeds all G accumulators.
//
// FOLD BOUND.  hefx_context_create refuses primes of 2^61 and above and the entry refuses weights >= q_j, so a weight and a
// (canonical) ciphertext word are both below 2^61 and a product is below 2^122 -- the situation mul_sum_kernel's comment
// derives.  An accumulator starts from the constant (< q < 2^61, or zero) or from a folded residue (< 2^61); the loop
// advances four terms at a time and folds after every 32nd term, and the tail adds at most three terms after a group of
// fewer than 32 unfolded ones: never more than 32 products on top of a residue, 32 * 2^122 + 2^61 < 2^128.  barrett128's
// quotient estimate is short by at most one for ANY 128-bit value, so the final Barrett gives the canonical residue of the
// integer sum: the bits of mod_drop, encode_scalar, multiply_plain, add_many, add_plain.
//
// TILE.  Every output costs a lane four 64-bit accumulator words (8 VGPRs).  Register report of this file
// (-Rpass-analysis=kernel-resource-usage, gfx950, the flags of _build.py):
//     GT = 1:  VGPRs  54, SGPRs 56, scratch 0, occupancy 8 waves/SIMD
//     GT = 2:  VGPRs  60, SGPRs 58, scratch 0, occupancy 8
//     GT = 4:  VGPRs  64, SGPRs 62, scratch 0, occupancy 8
//     GT = 8:  VGPRs 150, SGPRs 80, scratch 0, occupancy 3
//     GT = 16: VGPRs 240, SGPRs 83, scratch 0, occupancy 2   (tried, not instantiated)
// The kernel waits for memory, and what hides that wait is bytes in flight.  GT = 8 at three waves per SIMD still keeps
// 3 * 4 SIMDs * 64 lanes * 4 loads * 16 B = 48 KiB per CU on its way, and reads every input once for eight outputs where two
// tiles of four read it twice; GT = 16 at two waves has a third less in flight and nothing left for the compiler to spill
// into.  So the widest tile is 8, and G = 9 .. 16 runs as two launches: (2m + G) ciphertext volumes instead of (m + G),
// against about 5 m G for the call-by-call sequence.
template <int GT>
__global__ __launch_bounds__(256) void scalar_combine_kernel(DevTables T, int L, int m, int G, const u64 *__restrict__ tab,
                                                             int has_const)
{
    const int logn = T.logn;
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int p = (int)blockIdx.y / L, j = (int)blockIdx.y - p * L;
    const ModConst mc = T.mods[j];
    const u64 *__restrict__ wt = tab + 2 * (size_t)m + GT + (size_t)j * m * GT;
    const size_t off = ((size_t)j << logn) + 2 * w;  // word offset of this lane's pair inside a polynomial
    u64 xl[GT], xh[GT], yl[GT], yh[GT];
#pragma unroll
    for (int g = 0; g < GT; ++g) {
        const u64 c0 = (has_const && p == 0) ? tab[2 * (size_t)m + GT + (size_t)L * m * GT + (size_t)j * GT + g] : 0;
        xl[g] = yl[g] = c0;
        xh[g] = yh[g] = 0;
    }
    int k = 0;
    for (; k + 4 <= m; k += 4) {  // four independent 16-byte loads in flight per lane
        ulonglong2 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = gld16(reinterpret_cast<const u64 *>(tab[k + u]) + (size_t)p * tab[m + k + u] + off);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                const u64 wg = wt[(size_t)(k + u) * GT + g];
                mac128(xl[g], xh[g], x[u].x, wg);
                mac128(yl[g], yh[g], x[u].y, wg);
            }
        }
        if ((k & 31) == 28) {  // 32 terms since the last fold (FOLD BOUND)
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                xl[g] = barrett128(xl[g], xh[g], mc);
                yl[g] = barrett128(yl[g], yh[g], mc);
                xh[g] = yh[g] = 0;
            }
        }
    }
    for (; k < m; ++k) {
        const ulonglong2 x = gld16(reinterpret_cast<const u64 *>(tab[k]) + (size_t)p * tab[m + k] + off);
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            const u64 wg = wt[(size_t)k * GT + g];
            mac128(xl[g], xh[g], x.x, wg);
            mac128(yl[g], yh[g], x.y, wg);
        }
    }
    const size_t oo = ((size_t)blockIdx.y << logn) + 2 * w;  // outputs are [size][L][N]
#pragma unroll
    for (int g = 0; g < GT; ++g) {
        if (g < G) {  // (uniform)
            ulonglong2 r;
            r.x = barrett128(xl[g], xh[g], mc);
            r.y = barrett128(yl[g], yh[g], mc);
            gst16(reinterpret_cast<u64 *>(tab[2 * (size_t)m + g]) + oo, r);
        }
    }
}

size_t scalar_combine_table_words(int L, int m, int gt, bool has_const)
{
    return 2 * (size_t)m + gt + (size_t)L * m * gt + (has_const ? (size_t)L * gt : 0);
}

hipError_t launch_scalar_combine(const DevTables &T, int L, int size, int m, int G, int gt, const u64 *d_tab, bool has_const,
                                 hipStream_t s)
{
    const size_t row_pairs = (size_t)1 << (T.logn - 1);
    const dim3 grid((unsigned)((row_pairs + 255) / 256), (unsigned)(size * L)), block(256);
    const int hc = has_const ? 1 : 0;
    switch (gt) {
    case 1: hipLaunchKernelGGL(scalar_combine_kernel<1>, grid, block, 0, s, T, L, m, G, d_tab, hc); break;
    case 2: hipLaunchKernelGGL(scalar_combine_kernel<2>, grid, block, 0, s, T, L, m, G, d_tab, hc); break;
    case 4: hipLaunchKernelGGL(scalar_combine_kernel<4>, grid, block, 0, s, T, L, m, G, d_tab, hc); break;
    case 8: hipLaunchKernelGGL(scalar_combine_kernel<8>, grid, block, 0, s, T, L, m, G, d_tab, hc); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace hefx
