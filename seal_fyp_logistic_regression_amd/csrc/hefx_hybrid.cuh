// hefx_hybrid.cuh -- what the element-wise kernels of hybrid key switching (hefx_hybrid.hip) and of its hoisted form
// (hefx_hybrid_hoist.hip) have in common: the row rule, the grid, the lazy accumulator of a record, the digit loop against a
// key, the store into a data / special block pair and the mod-down's record.  Included by those two files and by the hoisted
// giant steps (hefx_hybrid_bsgs.hip), which states its own accumulator's range.
//
// ROWS.  R = L + alpha rows: r < L is data prime r, r >= L is special prime k - alpha + r - L (hy_row_mod).  dn = ceil(L / alpha)
// digits, digit j owning the data rows j alpha .. min((j + 1) alpha, L) - 1.  A result over all R rows lives in a BLOCK PAIR:
// the data rows in d [idx][2][L][N], the special rows -- the ones the mod-down transforms -- in s [idx][2][alpha][N] (hy_pair).
//
// SHAPE.  256 lanes per workgroup, one 16-byte record (two adjacent coefficients) per lane; the grid covers the N / 2 records
// of a row exactly or with whole idle lanes (hy_grid).  blockIdx.y = the RNS row wherever a pass writes one row per workgroup
// row, so its modulus is uniform per workgroup; blockIdx.z = the item, term or output.  A Galois gather takes the records
// 2w, 2w+1 of pi_g(x) from ONE source record, in either order (hefx_internal.h, galois_index): a gathered row touches the cache
// lines of a straight read, and hy_ld reads either kind.
//
// ARITHMETIC.  Every word read is canonical (the transforms' outputs, the caller's operands by the ABI) and every word
// written is canonical.  These passes do integer work mod every prime.  Lazy values inside a lane: shoup_lazy's [0, 2q),
// folded by csub at its line; and the 128-bit sums of products of canonical words, folded ONCE per word by barrett128, which
// takes any 128-bit value (hefx_modarith.cuh).  The range of those sums, for every pass of both files: a prime is below
// 2^61, so a canonical word is at most 2^61 - 2 and a product at most (2^61 - 2)^2 < 2^122; HY_SUM_MAX = 64 of them stay
// below 2^128 (64 * 2^122 = 2^128 itself is not reached: the assertion below).  The sums that exist: at most
// HY_ALPHA_MAX = 8 products in a conversion (hy_convert, hy_spread); one per digit in hy_mac, dn <= 61 because a chain
// has at most 62 primes (HyPmod) and one of them is special; the same plus (P mod q_r) pi_g(c0) in hyh_term, 62; and one per
// term in hyh_combine, which the entry bounds by HEFX_HYBRID_HOIST_MAX_TERMS = 64.
#pragma once
#include "hefx_internal.h"

namespace hefx {

constexpr int HY_SUM_MAX = 64;  // products a lazy 128-bit sum may hold
constexpr u64 HY_WORD_MAX = ((u64)1 << 61) - 2;
static_assert((~(unsigned __int128)0) / HY_WORD_MAX / HY_WORD_MAX >= HY_SUM_MAX, "HY_SUM_MAX products of canonical words pass 2^128");
static_assert(sizeof(HyPmod::v) / sizeof(u64) + 1 <= HY_SUM_MAX && HY_ALPHA_MAX <= HY_SUM_MAX, "a chain's digits + the P c0 term pass HY_SUM_MAX");

__device__ __forceinline__ int hy_row_mod(const HyTab &H, int k, int r) { return r < H.L ? r : k - H.alpha + (r - H.L); }

static inline dim3 hy_grid(const DevTables &T, int rows, int z)
{
    const size_t row_pairs = (size_t)1 << (T.logn - 1);
    return dim3((unsigned)((row_pairs + 255) / 256), (unsigned)rows, (unsigned)z);
}

// the record of pi_g(x) whose source record lies `at` words into `row` (at = 2w, swap = false: x itself)
__device__ __forceinline__ ulonglong2 hy_ld(const u64 *row, size_t at, bool swap)
{
    const ulonglong2 v = gld16(row + at);
    return swap ? make_ulonglong2(v.y, v.x) : v;
}

// The lazy sums of one record of polynomials 0 and 1: per polynomial, a 128-bit sum for each of the record's two words.
// At most HY_SUM_MAX steps per polynomial between the zero and the fold.
struct HyAcc {
    u64 lo[2][2] = {}, hi[2][2] = {};  // [polynomial][word]
    // polynomial c += x f, word by word; x and f canonical
    __device__ __forceinline__ void mac(int c, const ulonglong2 &x, const ulonglong2 &f)
    {
        mac128(lo[c][0], hi[c][0], x.x, f.x);
        mac128(lo[c][1], hi[c][1], x.y, f.y);
    }
    // polynomial c, canonical: one fold per word
    __device__ __forceinline__ ulonglong2 fold(int c, const ModConst &mc) const
    {
        return make_ulonglong2(barrett128(lo[c][0], hi[c][0], mc), barrett128(lo[c][1], hi[c][1], mc));
    }
};

// acc[c] += sum_j pi_g(E_j[r]) key[j][c][m(r)] over the H.dn digits of source `src`: E_j[r] is the source's own NTT row
// (own_row, read only when r < L) for the digit that owns data row r, else row r of extd [..][dn][L][N] / exts [..][dn][alpha][N].
// key points at record w of row m(r) of key[0][0] in [dnum][2][k][N]; (at, swap) as in hy_ld.
__device__ __forceinline__ void hy_digits_mac(HyAcc &acc, const DevTables &T, const HyTab &H, int r, int src, const u64 *own_row,
                                              const u64 *extd, const u64 *exts, const u64 *key, size_t at, bool swap)
{
    const int logn = T.logn, L = H.L, A = H.alpha;
    const size_t poly = (size_t)T.k << logn, digit = 2 * poly;  // words of one key polynomial / one key digit
    const int own = r < L ? r / A : -1;
    for (int j = 0; j < H.dn; ++j) {
        const u64 *xs = j == own ? own_row
                        : r < L  ? extd + ((size_t)((src * H.dn + j) * L + r) << logn)
                                 : exts + ((size_t)((src * H.dn + j) * A + (r - L)) << logn);
        const ulonglong2 x = hy_ld(xs, at, swap);
        acc.mac(0, x, gld16(key + (size_t)j * digit));
        acc.mac(1, x, gld16(key + (size_t)j * digit + poly));
    }
}

// record w of row r of polynomial 0 of entry idx in the block pair (d, s); polynomial 1 lies `poly` words behind it
template <class W>
__device__ __forceinline__ W *hy_pair(const DevTables &T, const HyTab &H, W *d, W *s, int idx, int r, size_t w, size_t &poly)
{
    const bool data = r < H.L;
    const int rows = data ? H.L : H.alpha, row = data ? r : r - H.L;
    poly = (size_t)rows << T.logn;
    return (data ? d : s) + ((size_t)(idx * 2 * rows + row) << T.logn) + 2 * w;
}

__device__ __forceinline__ void hy_pair_store(const DevTables &T, const HyTab &H, u64 *d, u64 *s, int idx, int r, size_t w,
                                              const ulonglong2 &r0, const ulonglong2 &r1)
{
    size_t poly;
    u64 *p = hy_pair(T, H, d, s, idx, r, w, poly);
    gst16(p, r0);
    gst16(p + poly, r1);
}

// The mod-down's record of data row j: (a - t) P^-1 mod q_j, a from acc and t from tt, both [..][L][N] with z = entry * 2 +
// polynomial in front.  canonical - canonical -> canonical; shoup_lazy: [0, 2q) -> [0, q).
__device__ __forceinline__ ulonglong2 hy_mod_down(const DevTables &T, const HyTab &H, int j, int z, size_t w, const u64 *acc, const u64 *tt)
{
    const ModConst mc = T.mods[j];
    const u64 pinv = H.tab[H.pinv + 2 * j], pinvs = H.tab[H.pinv + 2 * j + 1];  // {P^-1 mod q_j, its Shoup companion}
    const size_t at = ((size_t)(z * H.L + j) << T.logn) + 2 * w;
    const ulonglong2 a = gld16(acc + at), t = gld16(tt + at);
    return make_ulonglong2(csub(shoup_lazy(submod(a.x, t.x, mc.q), pinv, pinvs, mc.nq), mc.q),
                           csub(shoup_lazy(submod(a.y, t.y, mc.q), pinv, pinvs, mc.nq), mc.q));
}

}  // namespace hefx
