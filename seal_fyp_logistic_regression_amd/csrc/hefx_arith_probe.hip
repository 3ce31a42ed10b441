// hefx_arith_probe.hip -- a TEST library (libhefx_arith_probe.so), not part of the engine: one C entry that runs ONE device
// primitive of hefx_modarith.cuh / hefx_ntt.cuh / hefx_mac.cuh per thread on caller-supplied operands and constants, so that
// tests/test_gpu_arith_primitives.py can hold every primitive to the lazy range its comment states (tests/arith_cases.py has
// the operand sets and the exact models).  Built with the engine's flags (_build.build_probe); never linked into libhefx.so.
//
// Operand tuple i is in[i*nin .. i*nin + nin), its results out[i*nout .. i*nout + nout); doubles travel as their bit patterns.
// The per-modulus constants come from the caller word for word (ModConst: q r0 r1 ninv ninv_s ilw ilw_s nq; ModConstF: the
// bits of q qinv ninv ninv_r ilw ilw_r c32 c40): nothing here computes one.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "hefx_mac.cuh"

namespace hefx {
namespace probe {

struct Consts {
    ModConst mc;
    ModConstF mf;
};

// op codes (tests/arith_cases.py OPS mirrors this table)
enum {
    OP_MULHI_UNDER2 = 1,  // x ws                -> h
    OP_MUL_SUB_LO64 = 2,  // x w h nq            -> r
    OP_SHOUP_LAZY = 3,    // x w ws              -> r          (nq from ModConst)
    OP_SHOUP_LAZY4 = 4,   // x w ws              -> r
    OP_CSUB = 5,          // x m                 -> r
    OP_CSUBN = 6,         // x nm                -> r
    OP_BARRETT64 = 7,     // x                   -> r
    OP_BARRETT128_LT2Q = 8,  // lo hi            -> r
    OP_BARRETT128 = 9,    // lo hi               -> r
    OP_MULMOD = 10,       // a b                 -> r
    // ArithU64T<L16>, L16 = param & 1; the rest of param is the op's own
    OP_U_CT = 20,         // x y w ws            -> x' y'      stage = param >> 1
    OP_U_HALF_TW = 21,    // w ws                -> w' ws'     h = param >> 1
    OP_U_CT_HALF = 22,    // x y w ws            -> r
    OP_U_CT_SEL = 23,     // x y w ws            -> r
    OP_U_GS = 24,         // x y w ws            -> x' y'
    OP_U_GS_LAST = 25,    // x y                 -> x' y'
    OP_U_GS_HALF_SUM = 26,   // a0 a1            -> r
    OP_U_GS_HALF_DIFF = 27,  // a0 a1 w ws       -> r
    OP_U_INV_ADD = 28,    // x y                 -> r
    OP_U_INV_SUB_MUL = 29,   // x y w ws         -> r
    OP_U_INPUT = 30,      // x sub               -> r          RED = (param >> 1) & 3, has_sub = (param >> 3) & 1
    OP_U_FWD_FINISH = 32,    // x                -> r
    OP_U_MAC_OPERAND = 33,   // x                -> r          SLACK = param >> 1 (0: mac_operand)
    OP_U_INV_FINISH = 36,    // x                -> r
    OP_U_MODDOWN = 37,    // f acc sadd pt pinv pinv_s -> r    has_pt = param >> 1
    // key MAC policies: param = L | LT2Q << 8 | diag << 9 | cut << 10 | slack << 12
    // tuple: w ws dg.x dg.y, then L x (x.x x.y k0.x k0.y k1.x k1.y)  (cut: x.x x.y are E and O)
    // out:   result r0.x r0.y r1.x r1.y, result_data (4), then the accumulators (MacW 8 words, MacL 12 columns, MacF 4 sums)
    OP_MAC_W = 40,
    OP_MAC_L = 41,
    OP_MAC_F = 42,
    // ArithF64 (doubles as bits)
    OP_F_MM = 50,         // y w                 -> r
    OP_F_RED = 51,        // x                   -> r
    OP_F_CANON = 52,      // x                   -> u
    OP_F_FROM_U64 = 53,   // u                   -> x
    OP_F_TO_U64 = 54,     // x                   -> u
    OP_F_REDUCE_WIDE = 55,   // u                -> x
    OP_F_REDUCE_WIDE40 = 56, // u                -> x
    OP_F_CT = 57,         // x y w               -> x' y'
    OP_F_GS = 58,         // x y w               -> x' y'
    OP_F_GS_LAST = 59,    // x y                 -> x' y'
    OP_F_MODDOWN = 60,    // f acc sadd pt pinv  -> u          has_pt = param & 1
};
static constexpr int MAC_HDR = 4, MAC_PER = 6, MAC_OUT = 20, MAC_MAX_L = 61;

// words per tuple in and out; false for an unknown op / parameter
__host__ bool shape(int op, int param, int &nin, int &nout)
{
    switch (op) {
    case OP_MULHI_UNDER2: nin = 2, nout = 1; return true;
    case OP_MUL_SUB_LO64: nin = 4, nout = 1; return true;
    case OP_SHOUP_LAZY:
    case OP_SHOUP_LAZY4: nin = 3, nout = 1; return true;
    case OP_CSUB:
    case OP_CSUBN:
    case OP_BARRETT128_LT2Q:
    case OP_BARRETT128:
    case OP_MULMOD: nin = 2, nout = 1; return true;
    case OP_BARRETT64: nin = 1, nout = 1; return true;
    case OP_U_CT:
    case OP_U_GS: nin = 4, nout = 2; return true;
    case OP_U_HALF_TW: nin = 2, nout = 2; return true;
    case OP_U_CT_HALF:
    case OP_U_CT_SEL:
    case OP_U_GS_HALF_DIFF:
    case OP_U_INV_SUB_MUL: nin = 4, nout = 1; return true;
    case OP_U_GS_LAST: nin = 2, nout = 2; return true;
    case OP_U_GS_HALF_SUM:
    case OP_U_INV_ADD: nin = 2, nout = 1; return true;
    case OP_U_INPUT: nin = 2, nout = 1; return ((param >> 1) & 3) != 2;
    case OP_U_FWD_FINISH:
    case OP_U_INV_FINISH: nin = 1, nout = 1; return true;
    case OP_U_MAC_OPERAND: nin = 1, nout = 1; return (param >> 1) <= 2;
    case OP_U_MODDOWN: nin = 6, nout = 1; return true;
    case OP_MAC_W:
    case OP_MAC_L:
    case OP_MAC_F: {
        const int L = param & 0xFF;
        nin = MAC_HDR + MAC_PER * L, nout = MAC_OUT;
        return L >= 1 && L <= MAC_MAX_L;
    }
    case OP_F_MM: nin = 2, nout = 1; return true;
    case OP_F_RED:
    case OP_F_CANON:
    case OP_F_FROM_U64:
    case OP_F_TO_U64:
    case OP_F_REDUCE_WIDE:
    case OP_F_REDUCE_WIDE40: nin = 1, nout = 1; return true;
    case OP_F_CT:
    case OP_F_GS: nin = 3, nout = 2; return true;
    case OP_F_GS_LAST: nin = 2, nout = 2; return true;
    case OP_F_MODDOWN: nin = 5, nout = 1; return true;
    }
    return false;
}

__device__ __forceinline__ double dbl(u64 b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ u64 bits(double x) { return (u64)__double_as_longlong(x); }

template <bool L16>
__device__ void run_u64(int op, int p, const ModConst &mc, const u64 *a, u64 *o)
{
    using A = ArithU64T<L16>;
    const typename A::Ctx c = A::make(mc);
    switch (op) {
    case OP_U_CT: {
        u64 x = a[0], y = a[1];
        A::ct(x, y, make_ulonglong2(a[2], a[3]), c, p);
        o[0] = x, o[1] = y;
        break;
    }
    case OP_U_HALF_TW: {
        const ulonglong2 r = A::half_twiddle(make_ulonglong2(a[0], a[1]), c, p);
        o[0] = r.x, o[1] = r.y;
        break;
    }
    case OP_U_CT_HALF: o[0] = A::ct_half(a[0], a[1], make_ulonglong2(a[2], a[3]), c); break;
    case OP_U_CT_SEL: o[0] = A::ct_sel(a[0], a[1], make_ulonglong2(a[2], a[3]), c); break;
    case OP_U_GS: {
        u64 x = a[0], y = a[1];
        A::gs(x, y, make_ulonglong2(a[2], a[3]), c);
        o[0] = x, o[1] = y;
        break;
    }
    case OP_U_GS_LAST: {
        u64 x = a[0], y = a[1];
        A::gs_last(x, y, c);
        o[0] = x, o[1] = y;
        break;
    }
    case OP_U_GS_HALF_SUM: o[0] = A::gs_half_sum(a[0], a[1], c); break;
    case OP_U_GS_HALF_DIFF: o[0] = A::gs_half_diff(a[0], a[1], make_ulonglong2(a[2], a[3]), c); break;
    case OP_U_INV_ADD: o[0] = A::inv_add(a[0], a[1], c); break;
    case OP_U_INV_SUB_MUL: o[0] = A::inv_sub_mul(a[0], a[1], make_ulonglong2(a[2], a[3]), c); break;
    case OP_U_INPUT: {
        InMode m{};
        m.red_int = (p & 3) != 0, m.red_f64 = false, m.has_sub = (p >> 2) & 1, m.sub = a[1];
        const int red = p & 3;
        o[0] = red == 3 ? A::template input<3>(a[0], m, c, mc)
                        : red == 1 ? A::template input<1>(a[0], m, c, mc) : A::template input<0>(a[0], m, c, mc);
        break;
    }
    case OP_U_FWD_FINISH: o[0] = A::fwd_finish(a[0], c); break;
    case OP_U_MAC_OPERAND:
        o[0] = p == 0 ? A::mac_operand(a[0], c)
                      : p == 1 ? A::template mac_operand_lazy<1>(a[0], c) : A::template mac_operand_lazy<2>(a[0], c);
        break;
    case OP_U_INV_FINISH: o[0] = A::inv_finish(a[0], c); break;
    case OP_U_MODDOWN: o[0] = A::moddown(a[0], a[1], a[2], a[3], p != 0, c, make_ulonglong2(a[4], a[5]), mc); break;
    }
}

__device__ __forceinline__ ulonglong2 mac_ltw(MacW, const u64 *a) { return make_ulonglong2(a[0], a[1]); }
__device__ __forceinline__ ulonglong2 mac_ltw(MacL, const u64 *a) { return make_ulonglong2(a[0], a[1]); }
__device__ __forceinline__ double mac_ltw(MacF, const u64 *a) { return dbl(a[0]); }
__device__ __forceinline__ void mac_dump(const MacW &m, u64 *o)
{
    o[0] = m.a0xl, o[1] = m.a0xh, o[2] = m.a0yl, o[3] = m.a0yh, o[4] = m.a1xl, o[5] = m.a1xh, o[6] = m.a1yl, o[7] = m.a1yh;
}
__device__ __forceinline__ void mac_dump(const MacL &m, u64 *o)
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = m.c[i][j];
}
__device__ __forceinline__ void mac_dump(const MacF &m, u64 *o)
{
    o[0] = bits(m.a0x), o[1] = bits(m.a0y), o[2] = bits(m.a1x), o[3] = bits(m.a1y);
}

template <class P>
__device__ void run_mac(int param, const Consts &k, const u64 *a, u64 *o)
{
    const int L = param & 0xFF, slack = (param >> 12) & 3;
    const bool lt2q = (param >> 8) & 1, diag = (param >> 9) & 1, cut = (param >> 10) & 1;
    const typename P::Ctx c = P::make(k.mc, k.mf);
    const typename P::LTW w = mac_ltw(P(), a);
    P acc;
    for (int i = 0; i < L; ++i) {
        const u64 *d = a + MAC_HDR + MAC_PER * i;
        const typename P::X x = cut ? P::xin_cut(d[0], d[1], w, c, slack) : P::xin(make_ulonglong2(d[0], d[1]), false, c);
        acc.mac(x, P::kin(make_ulonglong2(d[2], d[3]), make_ulonglong2(d[4], d[5]), c), c);
    }
    P outer;
    if (diag) outer.mac_diag(acc, make_ulonglong2(a[2], a[3]), c);
    const P &fin = diag ? outer : acc;
    ulonglong2 r0, r1, d0, d1;
    if (lt2q) {
        fin.template result<true>(r0, r1, c);
        fin.template result_data<true>(d0, d1, c);
    } else {
        fin.template result<false>(r0, r1, c);
        fin.template result_data<false>(d0, d1, c);
    }
    for (int i = 0; i < MAC_OUT; ++i) o[i] = 0;
    o[0] = r0.x, o[1] = r0.y, o[2] = r1.x, o[3] = r1.y;
    o[4] = d0.x, o[5] = d0.y, o[6] = d1.x, o[7] = d1.y;
    mac_dump(fin, o + 8);
}

__device__ void run_f64(int op, int p, const Consts &k, const u64 *a, u64 *o)
{
    using A = ArithF64;
    const A::Ctx c = A::make(k.mf);
    switch (op) {
    case OP_F_MM: o[0] = bits(A::mm(dbl(a[0]), dbl(a[1]), c)); break;
    case OP_F_RED: o[0] = bits(A::red(dbl(a[0]), c)); break;
    case OP_F_CANON: o[0] = A::canon(dbl(a[0]), c); break;
    case OP_F_FROM_U64: o[0] = bits(A::from_u64(a[0])); break;
    case OP_F_TO_U64: o[0] = A::to_u64(dbl(a[0])); break;
    case OP_F_REDUCE_WIDE: o[0] = bits(A::reduce_wide(a[0], c)); break;
    case OP_F_REDUCE_WIDE40: o[0] = bits(A::reduce_wide40(a[0], c)); break;
    case OP_F_CT: {
        double x = dbl(a[0]), y = dbl(a[1]);
        A::ct(x, y, dbl(a[2]), c, 0);
        o[0] = bits(x), o[1] = bits(y);
        break;
    }
    case OP_F_GS: {
        double x = dbl(a[0]), y = dbl(a[1]);
        A::gs(x, y, dbl(a[2]), c);
        o[0] = bits(x), o[1] = bits(y);
        break;
    }
    case OP_F_GS_LAST: {
        double x = dbl(a[0]), y = dbl(a[1]);
        A::gs_last(x, y, c);
        o[0] = bits(x), o[1] = bits(y);
        break;
    }
    case OP_F_MODDOWN: o[0] = A::moddown(dbl(a[0]), a[1], a[2], a[3], (p & 1) != 0, c, make_double2(dbl(a[4]), 0.0)); break;
    }
}

__global__ void __launch_bounds__(256) probe_kernel(int op, int param, Consts k, const u64 *__restrict__ in, int nin,
                                                    u64 *__restrict__ out, int nout, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 *a = in + i * (size_t)nin;
    u64 *o = out + i * (size_t)nout;
    const ModConst &mc = k.mc;
    switch (op) {
    case OP_MULHI_UNDER2: o[0] = mulhi64_under2(a[0], a[1]); break;
    case OP_MUL_SUB_LO64: o[0] = mul_sub_lo64(a[0], a[1], a[2], a[3]); break;
    case OP_SHOUP_LAZY: o[0] = shoup_lazy(a[0], a[1], a[2], mc.nq); break;
    case OP_SHOUP_LAZY4: o[0] = shoup_lazy4(a[0], a[1], a[2], mc.nq); break;
    case OP_CSUB: o[0] = csub(a[0], a[1]); break;
    case OP_CSUBN: o[0] = csubn(a[0], a[1]); break;
    case OP_BARRETT64: o[0] = barrett64(a[0], mc.q, mc.r1); break;
    case OP_BARRETT128_LT2Q: o[0] = barrett128_lt2q(a[0], a[1], mc); break;
    case OP_BARRETT128: o[0] = barrett128(a[0], a[1], mc); break;
    case OP_MULMOD: o[0] = mulmod(a[0], a[1], mc); break;
    case OP_MAC_W: run_mac<MacW>(param, k, a, o); break;
    case OP_MAC_L: run_mac<MacL>(param, k, a, o); break;
    case OP_MAC_F: run_mac<MacF>(param, k, a, o); break;
    default:
        if (op >= OP_F_MM)
            run_f64(op, param, k, a, o);
        else if (param & 1)
            run_u64<true>(op, param >> 1, mc, a, o);
        else
            run_u64<false>(op, param >> 1, mc, a, o);
    }
}

}  // namespace probe
}  // namespace hefx

// Runs primitive `op` on n operand tuples (host memory in, host memory out).  0 on success, -1 for an unknown op or a tuple
// shape that is not the op's, else the HIP error code.  Allocates, copies, launches, copies back and frees: no context.
extern "C" __attribute__((visibility("default"))) int hefx_arith_probe(int op, int param, const uint64_t *modconst,
                                                                       const uint64_t *modconstf, const uint64_t *in, int nin,
                                                                       uint64_t *out, int nout, size_t n)
{
    using namespace hefx;
    using namespace hefx::probe;
    int want_in = 0, want_out = 0;
    if (!shape(op, param, want_in, want_out) || nin != want_in || nout != want_out) return -1;
    if (n == 0) return 0;
    if (n > ((size_t)1 << 17) || !modconst || !modconstf || !in || !out) return -1;
    static_assert(sizeof(ModConst) == 64 && sizeof(ModConstF) == 64, "eight words each");
    Consts k;
    memcpy(&k.mc, modconst, sizeof(ModConst));
    memcpy(&k.mf, modconstf, sizeof(ModConstF));
    u64 *din = nullptr, *dout = nullptr;
    const size_t bin = n * (size_t)nin * sizeof(u64), bout = n * (size_t)nout * sizeof(u64);
    hipError_t e = hipMalloc(&din, bin);
    if (e == hipSuccess) e = hipMalloc(&dout, bout);
    if (e == hipSuccess) e = hipMemcpy(din, in, bin, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0, bout);
    if (e == hipSuccess) {
        probe_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(op, param, k, din, nin, dout, nout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, bout, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return (int)e;
}
