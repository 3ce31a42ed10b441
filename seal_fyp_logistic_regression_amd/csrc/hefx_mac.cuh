// hefx_mac.cuh -- the key MAC's arithmetic policies (MacW / MacL / MacF) and the operand slack the limb policy admits.
// Used by hefx_keyswitch.hip (mac_items, the pair kernels); a header so that the policies can be instantiated on their own.
#pragma once
#include "hefx_ntt.cuh"

namespace hefx {

// How lazy may the words be that the digit transforms hand the key MAC for target modulus (mc, mf) at level L: 0 canonical,
// 1 below 2q, 2 below 4q?  Only the limb policy (MacL: integer-policy prime below 2^60, L <= 8 -- mac_dispatch) has
// headroom.  Its middle column takes xl*kh + xh*kl per digit (xl, kl, kh < 2^30):
//   x < 2q < 2^61: xh < 2^31, (2^60 + 2^61) * L < 2^64 for L <= 5; top column 2^61 * 5; folded sum < 2 L q^2 < q 2^64
//                  (barrett128's domain: 10 q < 2^64)
//   x < 4q < 2^62: xh < 2^32 (still one 32-bit limb), (2^60 + 2^62) * L < 2^64 for L <= 3; top column 2^62 * 3;
//                  folded sum < 4 L q^2 = 12 q^2 < q 2^64
__device__ __forceinline__ int mac_x_slack(const ModConst &mc, const ModConstF &mf, int L)
{
    if (mf.q != 0.0 || (mc.q >> 60) != 0) return 0;
    return L <= 3 ? 2 : (L <= 5 ? 1 : 0);
}

// MAC arithmetic, one policy per target modulus (uniform per workgroup).  Each accumulates sum_i x_i * k_i for the two
// key polynomials (k0, k1) and two adjacent coefficients (.x, .y).  The kernel waits for HBM either way (its own time
// did not change), but the 128-bit form was a quarter of all VALU instructions of the operation (SQ_INSTS_VALU,
// round 2), issue slots it took from the transform kernels of the neighbouring chunk:
//   MacF  FP64-policy moduli (q < 2^41).  Scratch x holds the UNFINISHED transform value as a double (|x| < 2^45,
//         hefx_ntt.cuh: no canonicalisation in the digit NTTs either); x*k mod q is the exact 6-instruction FP64 modmul
//         with a result in (-0.52q, 0.52q), the L results add exactly, one canonicalisation at the end.
//   MacL  q < 2^60 and L <= 8: 30-bit limbs, x = x1*2^30 + x0, k = k1*2^30 + k0, every partial product < 2^60, so the
//         three column sums (x0k0 | x0k1 + x1k0 | x1k1) take up to 16 terms in plain v_mad_u64_u32 accumulators with no
//         carry handling; the columns are put together into 128 bits once, then one Barrett reduction.
//   MacW  anything wider: full 128-bit accumulators (the generic form).
// All three deliver the canonical residue of the same integer sum: bit-identical results.
struct MacW {
    struct Ctx {
        ModConst mc;
    };
    __device__ static __forceinline__ Ctx make(const ModConst &mc, const ModConstF &) { return Ctx{mc}; }
    typedef ulonglong2 X;
    struct K {
        ulonglong2 k0, k1;
    };
    __device__ static __forceinline__ X xin(const ulonglong2 &bits, bool, const Ctx &) { return bits; }
    __device__ static __forceinline__ K kin(const ulonglong2 &k0, const ulonglong2 &k1, const Ctx &) { return K{k0, k1}; }
    // parity cut (mac_items): the last forward stage on (E[w], O[w]).  Canonical words in (parity_fwd_a, MAC_W), the
    // [0,8q) butterfly -- any prime below 2^61 -- and canonical words out, as this policy's mac takes them.
    typedef ulonglong2 LTW;
    __device__ static __forceinline__ LTW ltw(const NttTables &nt, size_t i) { return gld16(nt.tw + i); }
    __device__ static __forceinline__ X xin_cut(u64 e, u64 o, const LTW &w, const Ctx &c, int)
    {
        const ArithU64::Ctx ac = ArithU64::make(c.mc);
        ArithU64::ct(e, o, w, ac, 0);
        return make_ulonglong2(ArithU64::fwd_finish(e, ac), ArithU64::fwd_finish(o, ac));
    }
    u64 a0xl = 0, a0xh = 0, a0yl = 0, a0yh = 0, a1xl = 0, a1xh = 0, a1yl = 0, a1yh = 0;
    __device__ __forceinline__ void mac(const X &x, const K &k, const Ctx &)
    {
        mac128(a0xl, a0xh, x.x, k.k0.x);
        mac128(a0yl, a0yh, x.y, k.k0.y);
        mac128(a1xl, a1xh, x.x, k.k1.x);
        mac128(a1yl, a1yh, x.y, k.k1.y);
    }
    // this += inner * (dg.x, dg.y): the diagonal product of the double-hoisted transform
    __device__ __forceinline__ void mac_diag(const MacW &in, const ulonglong2 &dg, const Ctx &c)
    {
        ulonglong2 r0, r1;
        in.result(r0, r1, c);
        mac128(a0xl, a0xh, r0.x, dg.x);
        mac128(a0yl, a0yh, r0.y, dg.y);
        mac128(a1xl, a1xh, r1.x, dg.x);
        mac128(a1yl, a1yh, r1.y, dg.y);
    }
    // LT2Q: words below 2q instead of canonical ones -- what the regular MAC leaves in the accumulator scratch: both of
    // its readers take them as they are (the inverse transform of the special-prime rows: first stage on words below 2q;
    // the mod-down epilogue: acc + 4q - f < 6q into a Shoup product), one conditional subtraction less per word
    // what a DATA-prime accumulator row holds in scratch (read by the mod-down epilogue only): integer policies their
    // result<LT2Q>; the FP64 policy its unfinished sums as doubles (MacF::result_data)
    template <bool LT2Q = false>
    __device__ __forceinline__ void result_data(ulonglong2 &r0, ulonglong2 &r1, const Ctx &c) const { result<LT2Q>(r0, r1, c); }
    template <bool LT2Q = false>
    __device__ __forceinline__ void result(ulonglong2 &r0, ulonglong2 &r1, const Ctx &c) const
    {
        r0.x = LT2Q ? barrett128_lt2q(a0xl, a0xh, c.mc) : barrett128(a0xl, a0xh, c.mc);
        r0.y = LT2Q ? barrett128_lt2q(a0yl, a0yh, c.mc) : barrett128(a0yl, a0yh, c.mc);
        r1.x = LT2Q ? barrett128_lt2q(a1xl, a1xh, c.mc) : barrett128(a1xl, a1xh, c.mc);
        r1.y = LT2Q ? barrett128_lt2q(a1yl, a1yh, c.mc) : barrett128(a1yl, a1yh, c.mc);
    }
};

struct MacL {
    typedef MacW::Ctx Ctx;
    __device__ static __forceinline__ Ctx make(const ModConst &mc, const ModConstF &) { return Ctx{mc}; }
    struct X {
        uint32_t xl, xh, yl, yh;
    };
    struct K {
        uint32_t k0xl, k0xh, k0yl, k0yh, k1xl, k1xh, k1yl, k1yh;
    };
    __device__ static __forceinline__ uint32_t lo30(u64 v) { return (uint32_t)v & 0x3FFFFFFFu; }
    __device__ static __forceinline__ uint32_t hi30(u64 v) { return (uint32_t)(v >> 30); }
    __device__ static __forceinline__ X xin(const ulonglong2 &b, bool, const Ctx &)
    {
        return X{lo30(b.x), hi30(b.x), lo30(b.y), hi30(b.y)};
    }
    __device__ static __forceinline__ K kin(const ulonglong2 &k0, const ulonglong2 &k1, const Ctx &)
    {
        return K{lo30(k0.x), hi30(k0.x), lo30(k0.y), hi30(k0.y), lo30(k1.x), hi30(k1.x), lo30(k1.y), hi30(k1.y)};
    }
    // parity cut: E, O arrive as the L16 transform left them, below 16q (parity_fwd_a, MAC_L; q < 2^60).  The butterfly in
    // its odd-stage form (E -> below 8q first) is valid for either parity of the stage count: results below 12q.  Then the
    // reductions the producer of a finished row makes (mac_operand_lazy / mac_operand): down to what `slack` allows
    // (mac_x_slack: 2 -> below 4q, 1 -> below 2q, 0 -> canonical).  The MAC's sums see the same residues either way.
    typedef ulonglong2 LTW;
    __device__ static __forceinline__ LTW ltw(const NttTables &nt, size_t i) { return gld16(nt.tw + i); }
    __device__ static __forceinline__ u64 cut_reduce(u64 x, const ArithU64L::Ctx &ac, int slack)
    {
        x = csubn(csubn(x, ac.n8q), ac.n4q);       // < 12q -> < 4q
        if (slack < 2) x = csubn(x, ac.n2q);       // (block-uniform)
        if (slack < 1) x = csubn(x, ac.nq);
        return x;
    }
    __device__ static __forceinline__ X xin_cut(u64 e, u64 o, const LTW &w, const Ctx &c, int slack)
    {
        const ArithU64L::Ctx ac = ArithU64L::make(c.mc);
        ArithU64L::ct(e, o, w, ac, 1);
        return xin(make_ulonglong2(cut_reduce(e, ac, slack), cut_reduce(o, ac, slack)), false, c);
    }
    u64 c[4][3] = {};  // [a0x, a0y, a1x, a1y][column]
    __device__ static __forceinline__ void mad(u64 (&col)[3], uint32_t xl, uint32_t xh, uint32_t kl, uint32_t kh)
    {
        col[0] += (u64)xl * kl;
        col[1] += (u64)xl * kh;
        col[1] += (u64)xh * kl;
        col[2] += (u64)xh * kh;
    }
    __device__ __forceinline__ void mac(const X &x, const K &k, const Ctx &)
    {
        mad(c[0], x.xl, x.xh, k.k0xl, k.k0xh);
        mad(c[1], x.yl, x.yh, k.k0yl, k.k0yh);
        mad(c[2], x.xl, x.xh, k.k1xl, k.k1xh);
        mad(c[3], x.yl, x.yh, k.k1yl, k.k1yh);
    }
    __device__ __forceinline__ void mac_diag(const MacL &in, const ulonglong2 &dg, const Ctx &cx)
    {
        ulonglong2 r0, r1;
        in.result(r0, r1, cx);
        const uint32_t dxl = lo30(dg.x), dxh = hi30(dg.x), dyl = lo30(dg.y), dyh = hi30(dg.y);
        mad(c[0], lo30(r0.x), hi30(r0.x), dxl, dxh);
        mad(c[1], lo30(r0.y), hi30(r0.y), dyl, dyh);
        mad(c[2], lo30(r1.x), hi30(r1.x), dxl, dxh);
        mad(c[3], lo30(r1.y), hi30(r1.y), dyl, dyh);
    }
    template <bool LT2Q>
    __device__ static __forceinline__ u64 fold(const u64 (&col)[3], const ModConst &mc)
    {
        u64 lo = col[0], hi = 0, t = col[1] << 30;
        lo += t;
        hi += (col[1] >> 34) + (lo < t);
        t = col[2] << 60;
        lo += t;
        hi += (col[2] >> 4) + (lo < t);
        return LT2Q ? barrett128_lt2q(lo, hi, mc) : barrett128(lo, hi, mc);
    }
    template <bool LT2Q = false>
    __device__ __forceinline__ void result_data(ulonglong2 &r0, ulonglong2 &r1, const Ctx &cx) const { result<LT2Q>(r0, r1, cx); }
    template <bool LT2Q = false>
    __device__ __forceinline__ void result(ulonglong2 &r0, ulonglong2 &r1, const Ctx &cx) const
    {
        r0.x = fold<LT2Q>(c[0], cx.mc);
        r0.y = fold<LT2Q>(c[1], cx.mc);
        r1.x = fold<LT2Q>(c[2], cx.mc);
        r1.y = fold<LT2Q>(c[3], cx.mc);
    }
};

struct MacF {
    typedef ArithF64::Ctx Ctx;
    __device__ static __forceinline__ Ctx make(const ModConst &, const ModConstF &mf) { return ArithF64::make(mf); }
    typedef double2 X;
    struct K {
        double k0x, k0y, k1x, k1y;
    };
    // own: the digit's own prime -- canonical words of the source ciphertext instead of scratch doubles
    __device__ static __forceinline__ X xin(const ulonglong2 &b, bool own, const Ctx &)
    {
        return own ? make_double2(ArithF64::from_u64(b.x), ArithF64::from_u64(b.y))
                   : make_double2(__longlong_as_double((long long)b.x), __longlong_as_double((long long)b.y));
    }
    __device__ static __forceinline__ K kin(const ulonglong2 &k0, const ulonglong2 &k1, const Ctx &)
    {
        return K{ArithF64::from_u64(k0.x), ArithF64::from_u64(k0.y), ArithF64::from_u64(k1.x), ArithF64::from_u64(k1.y)};
    }
    // parity cut: E, O are unfinished doubles with |E|, |O| < 2^41 + (LOGN-1) * 0.52q < 2^45 (parity_fwd_raw): O is a valid
    // left operand of mm, and the two results are below 2^41 + LOGN * 0.52q < 2^45 -- the very bound of a finished row's
    // unfinished doubles (ArithF64::mac_operand), valid left operands of mac
    typedef double LTW;
    __device__ static __forceinline__ LTW ltw(const NttTables &nt, size_t i) { return nt.twf[i]; }
    __device__ static __forceinline__ X xin_cut(u64 e, u64 o, const LTW &w, const Ctx &c, int)
    {
        double x = ArithF64::unraw(e), y = ArithF64::unraw(o);
        ArithF64::ct(x, y, w, c, 0);
        return make_double2(x, y);
    }
    double a0x = 0.0, a0y = 0.0, a1x = 0.0, a1y = 0.0;
    __device__ __forceinline__ void mac(const X &x, const K &k, const Ctx &c)
    {
        a0x += ArithF64::mm(x.x, k.k0x, c);
        a0y += ArithF64::mm(x.y, k.k0y, c);
        a1x += ArithF64::mm(x.x, k.k1x, c);
        a1y += ArithF64::mm(x.y, k.k1y, c);
    }
    // |inner sums| <= L * 0.52q < 61 * 0.52 * 2^41 < 2^46 (L <= 61; below 2^45 only for L <= 30 at q near 2^41): valid left
    // operands of mm as they are, whose exactness argument holds up to 2^49 (hefx_ntt.cuh, InvRecentre)
    __device__ __forceinline__ void mac_diag(const MacF &in, const ulonglong2 &dg, const Ctx &c)
    {
        const double dx = ArithF64::from_u64(dg.x), dy = ArithF64::from_u64(dg.y);
        a0x += ArithF64::mm(in.a0x, dx, c);
        a0y += ArithF64::mm(in.a0y, dy, c);
        a1x += ArithF64::mm(in.a1x, dx, c);
        a1y += ArithF64::mm(in.a1y, dy, c);
    }
    // Data-prime rows (round 5): the UNFINISHED sums as doubles -- |a| <= L * 0.52 q < 2^46 -- which the mod-down epilogue
    // subtracts its unfinished transform value from as they are (ArithF64::moddown: |acc - f| < 2^47, a valid left operand of
    // the modmul, hefx_ntt.cuh InvRecentre); no canonicalisation here (eight instructions per word) and no u64 -> f64
    // conversion there (two).  The special prime's row stays canonical (result): the inverse transform reads it.
    template <bool LT2Q = false>
    __device__ __forceinline__ void result_data(ulonglong2 &r0, ulonglong2 &r1, const Ctx &) const
    {
        r0.x = ArithF64::raw(a0x), r0.y = ArithF64::raw(a0y), r1.x = ArithF64::raw(a1x), r1.y = ArithF64::raw(a1y);
    }
    template <bool LT2Q = false>  // (canonical either way)
    __device__ __forceinline__ void result(ulonglong2 &r0, ulonglong2 &r1, const Ctx &c) const
    {
        r0.x = ArithF64::canon(a0x, c);
        r0.y = ArithF64::canon(a0y, c);
        r1.x = ArithF64::canon(a1x, c);
        r1.y = ArithF64::canon(a1y, c);
    }
};

}  // namespace hefx
