// hefx_kernels.hip -- stand-alone NTT (K1/K2, single-workgroup rows up to N=16384) and the dyadic element-wise
// kernels (K3/K4/K10/K11: add, sub, negate, add_plain, multiply_plain, multiply/square, add_many, canonical
// reduce).  Key switching, rescale and the N=32768 NTT live in hefx_keyswitch.hip.
// Pure 64-bit modular integer work: no MFMA.  The NTT is integer-VALU bound (64-bit modmul emulated with
// v_mad_u64_u32), the element-wise kernels are HBM bound.
#include "hefx_internal.h"
#include "hefx_ntt.cuh"

namespace hefx {

// ------------------------------------------------------------------------------------------------
// K1/K2: stand-alone NTT, one workgroup per RNS row, in place.
// ------------------------------------------------------------------------------------------------
template <int LOGN, bool INV>
__global__ __launch_bounds__(NttCfg<LOGN>::T, 4) void ntt_rows_kernel(DevTables T, u64 *data, int nrows, int mod_first)
{
    using C = NttCfg<LOGN>;
    extern __shared__ __align__(16) u64 lds[];
    const int t = threadIdx.x;
    const int row = blockIdx.x, poly = blockIdx.y;
    const int m = mod_first + row;
    u64 *p = data + ((size_t)poly * nrows + row) * C::N;
    const ModConst mc = T.mods[m];
    u64 v[16];
    if (!INV) {
        // The row's arithmetic policy (FP64 for primes below 2^41, integers otherwise) is uniform over the workgroup.  Each
        // policy's branch does its OWN loads -- from its own copy of t, laundered through an empty asm so that the two
        // sets of loads are not recognised as common code and hoisted above the branch.  With the loads in front of the
        // branch the compiler lays the function out as "integer block, then FP64 block if a flag says so", the FP64 block
        // is reachable from the integer block as far as register allocation can tell, and the sixteen loaded words stay
        // live across the whole integer transform for a use that never happens: 12-22 VGPRs in scratch memory at every
        // degree until round 6.
        const ModConstF mf = T.modsf[m];
        int tl = t;
        if (mf.q != 0.0) {
            asm volatile("" : "+v"(tl));
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = p[C::idx_nat(tl, r)];
            ntt_fwd_row<LOGN>(v, lds, ntt_tables(T, m), mc, mf, t);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = p[C::idx_nat(tl, r)];
            ntt_fwd_row<LOGN>(v, lds, ntt_tables(T, m), mc, mf, t);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) p[C::idx_out(t, r)] = v[r];
    } else {
        // (loads per policy branch as above -- at N = 8192 only: that instantiation kept 4 VGPRs in scratch with the loads
        // in front of the branch; the others fit 120-127 that way and LOSE registers with the loads duplicated)
        const ModConstF mf = T.modsf[m];
        int tl = t;
        if (LOGN != 13) {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = p[C::idx_out(t, r)];
            ntt_inv_row<LOGN>(v, lds, ntt_tables(T, m), mc, mf, t);
        } else if (mf.q != 0.0) {
            asm volatile("" : "+v"(tl));
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = p[C::idx_out(tl, r)];
            ntt_inv_row<LOGN>(v, lds, ntt_tables(T, m), mc, mf, t);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = p[C::idx_out(tl, r)];
            ntt_inv_row<LOGN>(v, lds, ntt_tables(T, m), mc, mf, t);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) p[C::idx_nat(t, r)] = v[r];
    }
}

template <int LOGN>
static hipError_t launch_ntt_t(const DevTables &T, bool inverse, u64 *data, int npoly, int nrows, int mod_first,
                               hipStream_t s)
{
    using C = NttCfg<LOGN>;
    dim3 grid(nrows, npoly), block(C::T);
    size_t lds = sizeof(u64) * C::LDS_WORDS;
    if (inverse) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ntt_rows_kernel<LOGN, true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((ntt_rows_kernel<LOGN, true>), grid, block, lds, s, T, data, nrows, mod_first);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ntt_rows_kernel<LOGN, false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((ntt_rows_kernel<LOGN, false>), grid, block, lds, s, T, data, nrows, mod_first);
    }
    return hipGetLastError();
}

#define HEFX_DISPATCH_LOGN(logn, CALL)     \
    switch (logn) {                        \
        case 10: return CALL(10);          \
        case 11: return CALL(11);          \
        case 12: return CALL(12);          \
        case 13: return CALL(13);          \
        case 14: return CALL(14);          \
        default: return hipErrorInvalidValue; \
    }

hipError_t launch_ntt(const DevTables &T, bool inverse, u64 *data, int npoly, int nrows, int mod_first,
                      hipStream_t s)
{
#define CALL(LN) launch_ntt_t<LN>(T, inverse, data, npoly, nrows, mod_first, s)
    HEFX_DISPATCH_LOGN(T.logn, CALL)
#undef CALL
}

// ------------------------------------------------------------------------------------------------
// K3/K4/K10: element-wise ops, two words (16 B) per lane per step, grid-stride.
// word w of a ciphertext batch: row = w / N, modulus j = row % L.  Plaintext operand: [L][N].
// a, b and out carry no __restrict__: the C-ABI serves out == a and out == b (include/hefx.h, "exact in place"), which
// works because a lane reads word w of its operands before it writes word w and touches no other word.  A plaintext b
// can never be the output (refused on the host), but a and b share one parameter list, so the qualifier is off for it too.
// ------------------------------------------------------------------------------------------------
template <int OP>
__global__ __launch_bounds__(256) void elementwise_kernel(DevTables T, int L, int size, size_t total_pairs,
                                                          const ulonglong2 *a, const ulonglong2 *b, ulonglong2 *out,
                                                          int *flag)
{
    const int logn = T.logn;
    const size_t pairs_per_row = (size_t)1 << (logn - 1);
    long long flagged_ct = -1;  // last ciphertext this wave has already marked as not transparent
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total_pairs;
         w += (size_t)gridDim.x * blockDim.x) {
        const size_t row = w >> (logn - 1);
        const int j = (int)(row % (size_t)L);
        const ModConst mc = T.mods[j];
        ulonglong2 x = a[w], r;
        if (OP == EW_ADD) {
            ulonglong2 y = b[w];
            r.x = addmod(x.x, y.x, mc.q);
            r.y = addmod(x.y, y.y, mc.q);
        } else if (OP == EW_SUB) {
            ulonglong2 y = b[w];
            r.x = submod(x.x, y.x, mc.q);
            r.y = submod(x.y, y.y, mc.q);
        } else if (OP == EW_NEG) {
            r.x = negmod(x.x, mc.q);
            r.y = negmod(x.y, mc.q);
        } else if (OP == EW_REDUCE) {
            r.x = barrett64(x.x, mc.q, mc.r1);
            r.y = barrett64(x.y, mc.q, mc.r1);
        } else {
            // plaintext operand: poly index within ciphertext is irrelevant, only (j, i)
            const size_t in_row = w & (pairs_per_row - 1);
            ulonglong2 y = b[(size_t)j * pairs_per_row + in_row];
            const int poly = (int)((row / (size_t)L) % (size_t)size);
            if (OP == EW_MULPLAIN) {
                r.x = mulmod(x.x, y.x, mc);
                r.y = mulmod(x.y, y.y, mc);
                // transparent-ciphertext detection (SEAL is_transparent), PER CIPHERTEXT: flag[1 + ct] is set when any
                // word of a poly beyond c0 is non-zero.  A wave's 64 pairs lie in one row (rows are multiples of 64
                // pairs and the stride is a multiple of the block), so the vote and `ct` are wave-uniform; all writers
                // store the same value.
                if (poly > 0) {
                    const long long ct = (long long)(row / ((size_t)L * size));
                    if (ct != flagged_ct && __any((r.x | r.y) != 0)) {
                        if ((threadIdx.x & 63) == 0) flag[1 + ct] = 1;
                        flagged_ct = ct;
                    }
                }
            } else {  // EW_ADDPLAIN: only c0 gets the plaintext
                if (poly == 0) {
                    r.x = addmod(x.x, y.x, mc.q);
                    r.y = addmod(x.y, y.y, mc.q);
                } else {
                    r = x;
                }
            }
        }
        out[w] = r;
    }
}

hipError_t launch_elementwise(const DevTables &T, EwOp op, int L, int size, int count, const u64 *a,
                              const u64 *b, u64 *out, int *flag, hipStream_t s)
{
    const size_t n = (size_t)1 << T.logn;
    const size_t total_pairs = (size_t)count * size * L * n / 2;
    int blocks = (int)((total_pairs + 255) / 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    const ulonglong2 *pa = reinterpret_cast<const ulonglong2 *>(a);
    const ulonglong2 *pb = reinterpret_cast<const ulonglong2 *>(b);
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(out);
#define LAUNCH(OPC) \
    hipLaunchKernelGGL((elementwise_kernel<OPC>), dim3(blocks), dim3(256), 0, s, T, L, size, total_pairs, pa, pb, po, flag)
    switch (op) {
        case EW_ADD: LAUNCH(EW_ADD); break;
        case EW_SUB: LAUNCH(EW_SUB); break;
        case EW_NEG: LAUNCH(EW_NEG); break;
        case EW_MULPLAIN: LAUNCH(EW_MULPLAIN); break;
        case EW_ADDPLAIN: LAUNCH(EW_ADDPLAIN); break;
        case EW_REDUCE: LAUNCH(EW_REDUCE); break;
    }
#undef LAUNCH
    return hipGetLastError();
}

// add_many: out = (accumulate ? out : 0) + sum_{i<n} in[i]   (n <= ADD_MANY_GROUP pointers by value)
// pt0 != nullptr: the FIRST addend is in[0] (.) pt0 (multiply_plain, plaintext [L][N]) -- Linear_Transform_Plain's
// res[0] = ct_new * diag[0] (helper.h:250) formed inside its final sum (:259) instead of by a launch of its own
// out carries no __restrict__: it may be one of g.p[] (hefx_add_many's in-place form, a single launch) and is read back when
// accumulating; a lane reads its word of every input before it writes that word.  pt0 is never the output.
__global__ __launch_bounds__(256) void add_many_kernel(DevTables T, int L, size_t total_pairs, PtrGroup g, int n,
                                                       int accumulate, const ulonglong2 *__restrict__ pt0,
                                                       ulonglong2 *out)
{
    const int logn = T.logn;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total_pairs;
         w += (size_t)gridDim.x * blockDim.x) {
        const size_t row = w >> (logn - 1);
        const int j = (int)(row % (size_t)L);
        const u64 q = T.mods[j].q;
        ulonglong2 acc = accumulate ? out[w] : make_ulonglong2(0, 0);
        if (pt0) {  // (workgroup-uniform)
            const ModConst mc = T.mods[j];
            const ulonglong2 x = gld16(g.p[0] + 2 * w);
            const ulonglong2 y = pt0[((size_t)j << (logn - 1)) + (w & (((size_t)1 << (logn - 1)) - 1))];
            acc.x = addmod(acc.x, mulmod(x.x, y.x, mc), q);
            acc.y = addmod(acc.y, mulmod(x.y, y.y, mc), q);
        }
        for (int i = pt0 ? 1 : 0; i < n; ++i) {
            ulonglong2 x = gld16(g.p[i] + 2 * w);
            acc.x = addmod(acc.x, x.x, q);
            acc.y = addmod(acc.y, x.y, q);
        }
        out[w] = acc;
    }
}

// First level of a wide add_many: group gi sums inputs [gi*group, min(n, (gi+1)*group)) of a DEVICE pointer table
// into partial[gi]; all groups run in one launch (a chain of 48-input launches over a 0.4 MB ciphertext keeps
// under 100 workgroups in flight).
__global__ __launch_bounds__(256) void add_many_table_kernel(DevTables T, int L, size_t total_pairs,
                                                             const u64 *const *__restrict__ ptrs, int n, int group,
                                                             ulonglong2 *__restrict__ partial)
{
    const int logn = T.logn;
    const int gi = blockIdx.y;
    const int first = gi * group, last = first + group < n ? first + group : n;
    ulonglong2 *__restrict__ out = partial + (size_t)gi * total_pairs;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total_pairs;
         w += (size_t)gridDim.x * blockDim.x) {
        const size_t row = w >> (logn - 1);
        const u64 q = T.mods[(int)(row % (size_t)L)].q;
        ulonglong2 acc = make_ulonglong2(0, 0);
        for (int i = first; i < last; ++i) {
            const ulonglong2 x = gld16(ptrs[i] + 2 * w);
            acc.x = addmod(acc.x, x.x, q);
            acc.y = addmod(acc.y, x.y, q);
        }
        out[w] = acc;
    }
}

hipError_t launch_add_many_table(const DevTables &T, int L, int size, const u64 *const *d_ptrs, int n, int group,
                                 u64 *partial, hipStream_t s)
{
    const size_t total_pairs = (size_t)size * L * ((size_t)1 << T.logn) / 2;
    int blocks = (int)((total_pairs + 255) / 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    const int groups = (n + group - 1) / group;
    hipLaunchKernelGGL(add_many_table_kernel, dim3(blocks, groups), dim3(256), 0, s, T, L, total_pairs, d_ptrs, n, group,
                       reinterpret_cast<ulonglong2 *>(partial));
    return hipGetLastError();
}

// Grouped sum of plaintext products: group gi forms  out[gi] = sum_i ct[i] (.) pt[i]  over its slice [gi*group,
// min(n,(gi+1)*group)) of a DEVICE pointer table laid out as  n ciphertexts | n plaintexts | groups outputs.
// One pass: every operand word is read once and only the sums are written (n multiply_plain + add_many would write
// and re-read 2n ciphertexts).  128-bit lazy accumulation, folded every 32 terms (products < 2^122), one Barrett at
// the end -- the canonical residue of the sum, i.e. the bits of the op-by-op sequence.
__global__ __launch_bounds__(256) void mulplain_sum_kernel(DevTables T, int L, int size, const u64 *const *__restrict__ tab,
                                                           int n, int group)
{
    const int logn = T.logn;
    const size_t row_pairs = (size_t)1 << (logn - 1), poly_pairs = row_pairs * (size_t)L;
    const size_t total_pairs = poly_pairs * (size_t)size;
    const int gi = blockIdx.y;
    const int first = gi * group, last = first + group < n ? first + group : n;
    ulonglong2 *__restrict__ out = reinterpret_cast<ulonglong2 *>((const_cast<u64 *>(tab[2 * n + gi])));
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total_pairs;
         w += (size_t)gridDim.x * blockDim.x) {
        const size_t wp = w % poly_pairs;  // the plaintext word every poly of the ciphertext meets
        const ModConst mc = T.mods[(int)(wp >> (logn - 1))];
        u64 xl = 0, xh = 0, yl = 0, yh = 0;
        int i = first;
        for (; i + 4 <= last; i += 4) {  // eight independent loads in flight per lane
            ulonglong2 c[4], p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                c[u] = gld16(tab[i + u] + 2 * w);
                p[u] = gld16(tab[n + i + u] + 2 * wp);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                mac128(xl, xh, c[u].x, p[u].x);
                mac128(yl, yh, c[u].y, p[u].y);
            }
            if (((i - first) & 31) == 28) {  // every 32 terms: products < 2^122, so 32 + 3 tail terms stay below 2^128
                xl = barrett128(xl, xh, mc);
                yl = barrett128(yl, yh, mc);
                xh = yh = 0;
            }
        }
        for (; i < last; ++i) {
            const ulonglong2 c = gld16(tab[i] + 2 * w);
            const ulonglong2 p = gld16(tab[n + i] + 2 * wp);
            mac128(xl, xh, c.x, p.x);
            mac128(yl, yh, c.y, p.y);
        }
        ulonglong2 r;
        r.x = barrett128(xl, xh, mc);
        r.y = barrett128(yl, yh, mc);
        gst16(out + w, r);
    }
}

hipError_t launch_mulplain_sum(const DevTables &T, int L, int size, const u64 *const *d_tab, int n, int group,
                               hipStream_t s)
{
    const size_t total_pairs = (size_t)size * L * ((size_t)1 << T.logn) / 2;
    int blocks = (int)((total_pairs + 255) / 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    const int groups = (n + group - 1) / group;
    hipLaunchKernelGGL(mulplain_sum_kernel, dim3(blocks, groups), dim3(256), 0, s, T, L, size, d_tab, n, group);
    return hipGetLastError();
}

// Grouped sum of size-2 x size-2 products, the ciphertext twin of mulplain_sum_kernel: group gi forms
//   out3[gi] = sum_i a_i (x) b_i :  c0 = sum a0 b0,  c1 = sum (a0 b1 + a1 b0),  c2 = sum a1 b1
// over its slice [gi*group, min(n,(gi+1)*group)) of a DEVICE pointer table laid out as  n a-pointers | n b-pointers |
// groups outputs ([3][L][N] each).  The body of Linear_Transform_Cipher's product loop and sum (helper.h:222-231) and
// of sum_k A_k (x) B_k (matrix_multiplication.cpp:123-129) in one pass: the 4 L N operand words of a term are read
// once and only the sums are written, where n multiply + add_many write and re-read 3 L N words per term on top.
// A lane owns 16 B of each output poly: six 128-bit accumulators.  a_i == b_i (a square) and operands repeated across
// terms are fine: inputs are only read.
// FOLD INTERVALS.  hefx_context_create refuses primes of 2^61 and above, so a residue is at most q - 1 < 2^61 and a
// product below 2^122; an accumulator that was just folded holds a residue below 2^61.  P products on top of it stay
// below P 2^122 + 2^61 <= 2^128 as long as P <= 63 (barrett128's quotient estimate is short by at most one for ANY
// 128-bit value: the error of r = floor(2^128/q) costs x/2^128 < 1).  c0 and c2 take one product per term, c1 two, so c0
// / c2 could go 63 terms and c1 31; the loop folds at the largest powers of two below that, where the test is a mask:
// c0 / c2 every 32 terms, c1 every 16.  The loop advances four terms at a time and the tail adds at most three more
// terms AFTER a group of fewer than 16 (32) unfolded ones, so no accumulator ever holds more than 32 products.  One final
// Barrett per word gives the canonical residue of the integer sum -- the bits of the op-by-op sequence.
__global__ __launch_bounds__(256) void mul_sum_kernel(DevTables T, int L, const u64 *const *__restrict__ tab, int n, int group)
{
    const int logn = T.logn;
    const size_t poly_pairs = ((size_t)1 << (logn - 1)) * (size_t)L;
    const int gi = blockIdx.y;
    const int first = gi * group, last = first + group < n ? first + group : n;
    ulonglong2 *__restrict__ out = reinterpret_cast<ulonglong2 *>((const_cast<u64 *>(tab[2 * n + gi])));
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < poly_pairs; w += (size_t)gridDim.x * blockDim.x) {
        const ModConst mc = T.mods[(int)(w >> (logn - 1))];
        const size_t w0 = 2 * w, w1 = 2 * (w + poly_pairs);  // word offsets of this lane's pair in poly 0 / poly 1
        u64 c0xl = 0, c0xh = 0, c0yl = 0, c0yh = 0, c1xl = 0, c1xh = 0, c1yl = 0, c1yh = 0, c2xl = 0, c2xh = 0, c2yl = 0,
            c2yh = 0;
        int i = first;
        for (; i + 4 <= last; i += 4) {  // sixteen independent 16-byte loads in flight per lane
            ulonglong2 a0[4], a1[4], b0[4], b1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const u64 *pa = tab[i + u], *pb = tab[n + i + u];
                a0[u] = gld16(pa + w0);
                a1[u] = gld16(pa + w1);
                b0[u] = gld16(pb + w0);
                b1[u] = gld16(pb + w1);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                mac128(c0xl, c0xh, a0[u].x, b0[u].x);
                mac128(c0yl, c0yh, a0[u].y, b0[u].y);
                mac128(c1xl, c1xh, a0[u].x, b1[u].x);
                mac128(c1xl, c1xh, a1[u].x, b0[u].x);
                mac128(c1yl, c1yh, a0[u].y, b1[u].y);
                mac128(c1yl, c1yh, a1[u].y, b0[u].y);
                mac128(c2xl, c2xh, a1[u].x, b1[u].x);
                mac128(c2yl, c2yh, a1[u].y, b1[u].y);
            }
            const int done = i - first;
            if ((done & 15) == 12) {  // 16 terms = 32 products in c1
                c1xl = barrett128(c1xl, c1xh, mc);
                c1yl = barrett128(c1yl, c1yh, mc);
                c1xh = c1yh = 0;
                if ((done & 31) == 28) {  // 32 terms = 32 products in c0 and in c2
                    c0xl = barrett128(c0xl, c0xh, mc);
                    c0yl = barrett128(c0yl, c0yh, mc);
                    c2xl = barrett128(c2xl, c2xh, mc);
                    c2yl = barrett128(c2yl, c2yh, mc);
                    c0xh = c0yh = c2xh = c2yh = 0;
                }
            }
        }
        for (; i < last; ++i) {
            const u64 *pa = tab[i], *pb = tab[n + i];
            const ulonglong2 a0 = gld16(pa + w0), a1 = gld16(pa + w1), b0 = gld16(pb + w0), b1 = gld16(pb + w1);
            mac128(c0xl, c0xh, a0.x, b0.x);
            mac128(c0yl, c0yh, a0.y, b0.y);
            mac128(c1xl, c1xh, a0.x, b1.x);
            mac128(c1xl, c1xh, a1.x, b0.x);
            mac128(c1yl, c1yh, a0.y, b1.y);
            mac128(c1yl, c1yh, a1.y, b0.y);
            mac128(c2xl, c2xh, a1.x, b1.x);
            mac128(c2yl, c2yh, a1.y, b1.y);
        }
        ulonglong2 r0, r1, r2;
        r0.x = barrett128(c0xl, c0xh, mc);
        r0.y = barrett128(c0yl, c0yh, mc);
        r1.x = barrett128(c1xl, c1xh, mc);
        r1.y = barrett128(c1yl, c1yh, mc);
        r2.x = barrett128(c2xl, c2xh, mc);
        r2.y = barrett128(c2yl, c2yh, mc);
        gst16(out + w, r0);
        gst16(out + w + poly_pairs, r1);
        gst16(out + w + 2 * poly_pairs, r2);
    }
}

hipError_t launch_mul_sum(const DevTables &T, int L, const u64 *const *d_tab, int n, int group, hipStream_t s)
{
    const size_t poly_pairs = (size_t)L * ((size_t)1 << T.logn) / 2;
    int blocks = (int)((poly_pairs + 255) / 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    const int groups = (n + group - 1) / group;
    hipLaunchKernelGGL(mul_sum_kernel, dim3(blocks, groups), dim3(256), 0, s, T, L, d_tab, n, group);
    return hipGetLastError();
}

hipError_t launch_add_many(const DevTables &T, int L, int size, const PtrGroup &g, int n, bool accumulate,
                           u64 *out, hipStream_t s, const u64 *pt0)
{
    const size_t total_pairs = (size_t)size * L * ((size_t)1 << T.logn) / 2;
    int blocks = (int)((total_pairs + 255) / 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(add_many_kernel, dim3(blocks), dim3(256), 0, s, T, L, total_pairs, g, n, accumulate ? 1 : 0,
                       reinterpret_cast<const ulonglong2 *>(pt0), reinterpret_cast<ulonglong2 *>(out));
    return hipGetLastError();
}

// tab[i][0..words) = src[i*words ..]: the contiguous results of a batched producer (hefx_ckks_encode over many vectors)
// handed to their separately allocated owners in one launch
__global__ __launch_bounds__(256) void scatter_rows_kernel(const u64 *__restrict__ src, const u64 *const *__restrict__ tab,
                                                           size_t pairs)
{
    const int i = blockIdx.y;
    u64 *dst = const_cast<u64 *>(tab[i]);
    const u64 *from = src + (size_t)i * pairs * 2;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < pairs; w += (size_t)gridDim.x * blockDim.x)
        gst16(dst + 2 * w, *reinterpret_cast<const ulonglong2 *>(from + 2 * w));
}
hipError_t launch_scatter_rows(const u64 *src, const u64 *const *d_tab, int n, size_t words, hipStream_t s)
{
    const size_t pairs = words / 2;
    int blocks = (int)((pairs + 255) / 256);
    if (blocks > 64) blocks = 64;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(blocks, n), dim3(256), 0, s, src, d_tab, pairs);
    return hipGetLastError();
}

// n independent element-wise sums / differences through a DEVICE pointer table  a[0..n) | b[0..n) | out[0..n): the adds
// of n dot-product chains advancing in lockstep (helper.h:464,475 over the rows of logistic_regression_ckks.cpp:217)
// as one launch.  out[i] may be a[i] or b[i] exactly (element-wise: a lane reads word w before it writes word w), so the
// three data pointers carry no __restrict__; the pointer table itself is only read.
template <bool SUB>
__global__ __launch_bounds__(256) void addsub_table_kernel(DevTables T, int L, size_t total_pairs,
                                                           const u64 *const *__restrict__ tab, int n)
{
    const int logn = T.logn;
    const int item = blockIdx.y;
    const ulonglong2 *a = reinterpret_cast<const ulonglong2 *>((tab[item]));
    const ulonglong2 *b = reinterpret_cast<const ulonglong2 *>((tab[n + item]));
    ulonglong2 *out = reinterpret_cast<ulonglong2 *>((const_cast<u64 *>(tab[2 * n + item])));
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total_pairs;
         w += (size_t)gridDim.x * blockDim.x) {
        const u64 q = T.mods[(int)((w >> (logn - 1)) % (size_t)L)].q;
        const ulonglong2 x = gld16(a + w), y = gld16(b + w);
        ulonglong2 r;
        r.x = SUB ? submod(x.x, y.x, q) : addmod(x.x, y.x, q);
        r.y = SUB ? submod(x.y, y.y, q) : addmod(x.y, y.y, q);
        gst16(out + w, r);
    }
}

hipError_t launch_addsub_table(const DevTables &T, bool sub, int L, int size, const u64 *const *d_tab, int n,
                               hipStream_t s)
{
    const size_t total_pairs = (size_t)size * L * ((size_t)1 << T.logn) / 2;
    int blocks = (int)((total_pairs + 255) / 256);
    if (blocks > 64) blocks = 64;  // n items in grid.y fill the chip
    if (sub)
        hipLaunchKernelGGL(addsub_table_kernel<true>, dim3(blocks, n), dim3(256), 0, s, T, L, total_pairs, d_tab, n);
    else
        hipLaunchKernelGGL(addsub_table_kernel<false>, dim3(blocks, n), dim3(256), 0, s, T, L, total_pairs, d_tab, n);
    return hipGetLastError();
}

// General tensor product of ciphertexts of sa and sb polynomials (Evaluator::multiply beyond size 2 x size 2):
//   out[k] = sum_{i+j=k} a_i (.) b_j  mod q_row,   k = 0 .. sa+sb-2.
// A lane owns one 16-byte record of a row in every polynomial.  sa + sb - 1 <= HEFX_CT_SIZE_MAX = 16, so an output word
// sums at most min(sa, sb) <= 8 products below 2^122 each: far inside the 63 products a 128-bit accumulator holds (FOLD
// INTERVALS at mul_sum_kernel).  mac128 per term, ONE barrett128 per output word, no intermediate fold: the canonical
// residue of the integer sum, hence the bits of SEAL's dyadic-product-and-add loop in any order.  Inputs are only read
// (a == b is a square); every output word is written once.
// Two forms of the body, chosen from the resource report (DESIGN.md kernel table):
//   SA, SB > 0  sizes 2..4 on either side at compile time: the sa + sb operand records are loaded once into registers and
//               the k loop is unrolled over them -- every operand word leaves HBM and the caches once;
//   SA == 0     any other legal shape: a loop over k whose inner loop re-reads the records it needs.  A lane re-reads its
//               OWN records (the same addresses from the same lane within a few hundred instructions), so the repeats are
//               cache hits and HBM still sees each operand word once; holding up to 17 records under a run-time index
//               would put them in scratch memory.
// The block size is a constant of the launcher, not blockDim.x: read from the dispatch packet it cost these kernels a
// dependent vector load in front of the first operand load, which the one-product form (a microsecond of work) shows.
constexpr unsigned MUL_BLOCK = 256;
template <int SA, int SB>
__device__ __forceinline__ void multiply_sizes_body(const DevTables &T, size_t pairs_per_poly, int sa, int sb,
                                                    const ulonglong2 *__restrict__ a, const ulonglong2 *__restrict__ b,
                                                    ulonglong2 *__restrict__ out)
{
    const int logn = T.logn;
    for (size_t w = (size_t)blockIdx.x * MUL_BLOCK + threadIdx.x; w < pairs_per_poly; w += (size_t)gridDim.x * MUL_BLOCK) {
        const ModConst mc = T.mods[(int)(w >> (logn - 1))];
        if constexpr (SA > 0) {
            ulonglong2 ra[SA], rb[SB];
#pragma unroll
            for (int i = 0; i < SA; ++i) ra[i] = gld16(a + w + (size_t)i * pairs_per_poly);
#pragma unroll
            for (int j = 0; j < SB; ++j) rb[j] = gld16(b + w + (size_t)j * pairs_per_poly);
#pragma unroll
            for (int k = 0; k < SA + SB - 1; ++k) {
                u64 xl = 0, xh = 0, yl = 0, yh = 0;
#pragma unroll
                for (int i = 0; i < SA; ++i) {
                    const int j = k - i;
                    if (j >= 0 && j < SB) {
                        mac128(xl, xh, ra[i].x, rb[j].x);
                        mac128(yl, yh, ra[i].y, rb[j].y);
                    }
                }
                ulonglong2 r;
                r.x = barrett128(xl, xh, mc);
                r.y = barrett128(yl, yh, mc);
                gst16(out + w + (size_t)k * pairs_per_poly, r);
            }
        } else {
            for (int k = 0; k < sa + sb - 1; ++k) {
                const int i0 = k - (sb - 1) > 0 ? k - (sb - 1) : 0, i1 = k < sa - 1 ? k : sa - 1;
                u64 xl = 0, xh = 0, yl = 0, yh = 0;
                for (int i = i0; i <= i1; ++i) {
                    const ulonglong2 x = gld16(a + w + (size_t)i * pairs_per_poly);
                    const ulonglong2 y = gld16(b + w + (size_t)(k - i) * pairs_per_poly);
                    mac128(xl, xh, x.x, y.x);
                    mac128(yl, yh, x.y, y.y);
                }
                ulonglong2 r;
                r.x = barrett128(xl, xh, mc);
                r.y = barrett128(yl, yh, mc);
                gst16(out + w + (size_t)k * pairs_per_poly, r);
            }
        }
    }
}

template <int SA, int SB>
__global__ __launch_bounds__(MUL_BLOCK) void multiply_sizes_kernel(DevTables T, size_t pairs_per_poly, int sa, int sb,
                                                             const ulonglong2 *__restrict__ a,
                                                             const ulonglong2 *__restrict__ b, ulonglong2 *__restrict__ out)
{
    multiply_sizes_body<SA, SB>(T, pairs_per_poly, sa, sb, a, b, out);
}

// the pointer-table twin (a[0..n) | b[0..n) | out[0..n), one (sa, sb) for all items), item = blockIdx.y
template <int SA, int SB>
__global__ __launch_bounds__(MUL_BLOCK) void multiply_sizes_table_kernel(DevTables T, size_t pairs_per_poly, int sa, int sb,
                                                                   const u64 *const *__restrict__ tab, int n)
{
    const int item = blockIdx.y;
    multiply_sizes_body<SA, SB>(T, pairs_per_poly, sa, sb, reinterpret_cast<const ulonglong2 *>(tab[item]),
                                reinterpret_cast<const ulonglong2 *>(tab[n + item]),
                                reinterpret_cast<ulonglong2 *>(const_cast<u64 *>(tab[2 * n + item])));
}

// d_tab == nullptr: one product a x b -> out; otherwise n products through the table (a, b, out unused)
hipError_t launch_multiply_sizes(const DevTables &T, int L, int sa, int sb, const u64 *a, const u64 *b, u64 *out,
                                 const u64 *const *d_tab, int n, hipStream_t s)
{
    const size_t pairs = (size_t)L * ((size_t)1 << T.logn) / 2;
    int blocks = (int)((pairs + MUL_BLOCK - 1) / MUL_BLOCK);
    const int cap = d_tab ? 64 : 256 * 8;  // n items in grid.y fill the chip
    if (blocks > cap) blocks = cap;
    const ulonglong2 *pa = reinterpret_cast<const ulonglong2 *>(a), *pb = reinterpret_cast<const ulonglong2 *>(b);
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(out);
#define LAUNCH(SA, SB)                                                                                                    \
    do {                                                                                                                  \
        if (d_tab)                                                                                                        \
            hipLaunchKernelGGL((multiply_sizes_table_kernel<SA, SB>), dim3(blocks, n), dim3(MUL_BLOCK), 0, s, T, pairs, sa, sb, \
                               d_tab, n);                                                                                 \
        else                                                                                                              \
            hipLaunchKernelGGL((multiply_sizes_kernel<SA, SB>), dim3(blocks), dim3(MUL_BLOCK), 0, s, T, pairs, sa, sb, pa, pb,  \
                               po);                                                                                       \
    } while (0)
    switch (sa >= 2 && sa <= 4 && sb >= 2 && sb <= 4 ? sa * 8 + sb : 0) {
        case 2 * 8 + 2: LAUNCH(2, 2); break;
        case 2 * 8 + 3: LAUNCH(2, 3); break;
        case 2 * 8 + 4: LAUNCH(2, 4); break;
        case 3 * 8 + 2: LAUNCH(3, 2); break;
        case 3 * 8 + 3: LAUNCH(3, 3); break;
        case 3 * 8 + 4: LAUNCH(3, 4); break;
        case 4 * 8 + 2: LAUNCH(4, 2); break;
        case 4 * 8 + 3: LAUNCH(4, 3); break;
        case 4 * 8 + 4: LAUNCH(4, 4); break;
        default: LAUNCH(0, 0); break;
    }
#undef LAUNCH
    return hipGetLastError();
}

// HIP loads a translation unit's code object at its first kernel launch (milliseconds); hefx_context_create pays
// that once, up front, instead of the first encode / rotation / encryption of a program.
__global__ void warm_kernels_kernel() {}
hipError_t warm_kernels(hipStream_t s)
{
    hipLaunchKernelGGL(warm_kernels_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace hefx
