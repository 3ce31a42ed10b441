// hefx_dft.hip -- the kernel of hefx_plain_combine (include/hefx_dft.h): G plaintext combinations of the same m ciphertexts,
//   out_g = sum_k pt[g][k] (.) ct_k,      pt[g][k] a full plaintext or NULL (a structural zero: no term),
// in one pass over the inputs.  The inner sums of a baby-step/giant-step matrix product (CoeffToSlot, SlotToCoeff: the same few
// rotated ciphertexts meet many different plaintexts): mulplain_sum_kernel reads a ciphertext AND a plaintext per term and per
// polynomial, 4 L N words a term; here a lane owns 16 bytes of BOTH polynomials, so a plaintext word is read once for the two
// of them and a ciphertext word once for a whole tile of outputs.
#include "hefx_internal.h"

namespace hefx {

// TABLE (device words, one descriptor-ring slot per call; GT = the call's tile width, tiles = ceil(G / GT)):
//   [0, m)                      input pointers, [2][L][N] each
//   then per tile  [GT]         output pointers, 0 behind the G-th output
//                  [m][GT]      plaintext pointers ([L][N] each), term-major so that the GT pointers of a term are adjacent
//                               scalar loads; 0 = no term (also every entry of an output behind the G-th)
// One workgroup is ONE wave (nothing is shared between lanes, and single waves spread over all compute units) and works on
// 64 adjacent 16-byte records of row j = blockIdx.y for the tile blockIdx.z, so the modulus and every pointer of the table are
// uniform per workgroup and the NULL test is a scalar branch.  An input no output of the tile uses is not read.
//
// FOLD BOUND.  hefx_context_create refuses primes of 2^61 and above and the words of ciphertexts and plaintexts are taken as
// canonical, so a product is below 2^122 -- the situation mulplain_sum_kernel's and scalar_combine_kernel's comments derive.
// An accumulator starts from zero or from a folded residue (< 2^61); the loop advances four term POSITIONS at a time (a NULL
// counts as a position: the count is uniform and needs no bookkeeping) and folds after every 32nd, and the tail adds at most
// three terms after a group of fewer than 32 unfolded ones: never more than 32 products on top of a residue,
// 32 * 2^122 + 2^61 < 2^128.  barrett128's quotient estimate is short by at most one for ANY 128-bit value, so the final Barrett
// gives the canonical residue of the integer sum: the bits of multiply_plain per term and add_many, and of
// hefx_multiply_plain_sum on the non-null terms of each output.
//
// TILE.  Every output costs a lane eight 64-bit accumulator words (16 VGPRs).  Register report of this file
// (-Rpass-analysis=kernel-resource-usage, gfx950, the flags of _build.py):
//     GT = 1:  VGPRs  82, SGPRs  48, scratch 0, occupancy 5 waves/SIMD
//     GT = 2:  VGPRs  82, SGPRs  47, scratch 0, occupancy 5
//     GT = 4:  VGPRs 122, SGPRs  65, scratch 0, occupancy 4
//     GT = 8:  VGPRs 202, SGPRs 101, scratch 0, occupancy 2
// No tile spills.  What decides between them is not the register file but how many waves the call has: a row has only
// N / 128 of them (640 for all rows at N = 16384, L = 5, on 1024 SIMDs), each a long dependent chain of loads and 128-bit
// products, and the tiles of one call run side by side on blockIdx.z.  The width is chosen per call by plain_combine_tile
// (hefx_capi.cpp): the widest tile that still gives the call 4096 waves.
// MEASURED on the MI355X (tools/dft_bench.py, profiles/dft.json; device us per call, hefx_multiply_plain_sum on the same
// pointers beside it):
//     N = 32768, L = 8   m = G = 8 dense (tile 4)            49.1   against  80.9 (one grouped call)
//                        m = G = 16 dense (tile 8)          161.5   against 311.3
//                        m = 4, G = 16 dense (tile 8)        58.9   against  54.8   <- slower
//                        levels = 3 stage, m = G = 16       107.2   against 320.1 (16 calls: the term counts differ)
//     N = 16384, L = 5   m = G = 8 dense (tile 1)            21.6   against  20.5   <- slower
//                        m = G = 16 dense (tile 2)           45.2   against  58.0
//                        levels = 3 stage, m = 8, G = 16     24.7   against 185.0 (16 calls)
// The old path's re-reads sit in the Infinity Cache at these sizes (it reaches 7 - 11 TB/s of its own byte count), so the
// fused call wins by its launch count and, from about 2^23 words of terms, by its bytes; Evaluator.plain_combine (seal.py)
// keeps the grouped call for the shapes that lose.  DESIGN.md has the whole table.
template <int GT>
__global__ __launch_bounds__(64) void plain_combine_kernel(DevTables T, int L, int m, const u64 *__restrict__ tab)
{
    const int logn = T.logn;
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= ((size_t)1 << (logn - 1))) return;
    const int j = (int)blockIdx.y;
    const ModConst mc = T.mods[j];
    const u64 *__restrict__ otab = tab + (size_t)m + (size_t)blockIdx.z * ((size_t)GT + (size_t)m * GT);
    const u64 *__restrict__ ptab = otab + GT;
    const size_t off = ((size_t)j << logn) + 2 * w;  // word offset of this lane's pair inside a polynomial (and a plaintext)
    const size_t poly = (size_t)L << logn;           // words between the two polynomials of a ciphertext
    u64 al[GT][4], ah[GT][4];                        // [output][c0.x, c0.y, c1.x, c1.y]
#pragma unroll
    for (int g = 0; g < GT; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) al[g][i] = ah[g][i] = 0;
    auto term = [&](int k, const ulonglong2 &c0, const ulonglong2 &c1) {
        ulonglong2 d[GT];
#pragma unroll
        for (int g = 0; g < GT; ++g) {  // the plaintext loads of the term first: GT independent loads in flight
            const u64 p = ptab[(size_t)k * GT + g];
            d[g] = p ? gld16(reinterpret_cast<const u64 *>(p) + off) : make_ulonglong2(0, 0);  // (uniform)
        }
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            if (ptab[(size_t)k * GT + g]) {  // (uniform)
                mac128(al[g][0], ah[g][0], c0.x, d[g].x);
                mac128(al[g][1], ah[g][1], c0.y, d[g].y);
                mac128(al[g][2], ah[g][2], c1.x, d[g].x);
                mac128(al[g][3], ah[g][3], c1.y, d[g].y);
            }
        }
    };
    auto used = [&](int k) {
        u64 any = 0;
#pragma unroll
        for (int g = 0; g < GT; ++g) any |= ptab[(size_t)k * GT + g];
        return any != 0;
    };
    int k = 0;
    for (; k + 4 <= m; k += 4) {
        ulonglong2 c0[4], c1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // up to eight independent 16-byte loads in flight per lane
            if (used(k + u)) {         // (uniform)
                const u64 *in = reinterpret_cast<const u64 *>(tab[k + u]) + off;
                c0[u] = gld16(in);
                c1[u] = gld16(in + poly);
            } else {
                c0[u] = c1[u] = make_ulonglong2(0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) term(k + u, c0[u], c1[u]);
        if ((k & 31) == 28) {  // 32 term positions since the last fold (FOLD BOUND)
#pragma unroll
            for (int g = 0; g < GT; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    al[g][i] = barrett128(al[g][i], ah[g][i], mc);
                    ah[g][i] = 0;
                }
        }
    }
    for (; k < m; ++k) {
        if (!used(k)) continue;  // (uniform)
        const u64 *in = reinterpret_cast<const u64 *>(tab[k]) + off;
        const ulonglong2 c0 = gld16(in), c1 = gld16(in + poly);
        term(k, c0, c1);
    }
#pragma unroll
    for (int g = 0; g < GT; ++g) {
        if (otab[g]) {  // (uniform: 0 behind the G-th output)
            u64 *out = reinterpret_cast<u64 *>(otab[g]) + off;
            ulonglong2 r0, r1;
            r0.x = barrett128(al[g][0], ah[g][0], mc);
            r0.y = barrett128(al[g][1], ah[g][1], mc);
            r1.x = barrett128(al[g][2], ah[g][2], mc);
            r1.y = barrett128(al[g][3], ah[g][3], mc);
            gst16(out, r0);
            gst16(out + poly, r1);
        }
    }
}

size_t plain_combine_table_words(int m, int G, int gt)
{
    const size_t tiles = ((size_t)G + gt - 1) / gt;
    return (size_t)m + tiles * ((size_t)gt + (size_t)m * gt);
}

hipError_t launch_plain_combine(const DevTables &T, int L, int m, int G, int gt, const u64 *d_tab, hipStream_t s)
{
    const size_t row_pairs = (size_t)1 << (T.logn - 1);
    const dim3 grid((unsigned)((row_pairs + 63) / 64), (unsigned)L, (unsigned)((G + gt - 1) / gt)), block(64);
    switch (gt) {
    case 1: hipLaunchKernelGGL(plain_combine_kernel<1>, grid, block, 0, s, T, L, m, d_tab); break;
    case 2: hipLaunchKernelGGL(plain_combine_kernel<2>, grid, block, 0, s, T, L, m, d_tab); break;
    case 4: hipLaunchKernelGGL(plain_combine_kernel<4>, grid, block, 0, s, T, L, m, d_tab); break;
    case 8: hipLaunchKernelGGL(plain_combine_kernel<8>, grid, block, 0, s, T, L, m, d_tab); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace hefx
