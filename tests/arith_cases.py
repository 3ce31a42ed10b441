"""Every device arithmetic primitive on its own: primes next to each policy bound, exact integer models, the contract each
source comment states, and directed operand sets (host only, no GPU).

The kernels are built from hefx_modarith.cuh, the policies ArithU64T<false/true> and ArithF64 of hefx_ntt.cuh and the key-MAC
policies MacW / MacL / MacF of hefx_mac.cuh.  None of them keeps its values canonical: each documents a lazy range and the next
one relies on it.  `Model` restates every primitive word for word in Python integers (FP64: IEEE doubles -- float(int) is
correctly rounded, round() is rint, and every fma result is an exact integer by the very claim under test, which the model
asserts); `cases(K)` gives, per primitive, operand tuples at the edges of the documented input range, the model's results and
a `check` that holds ANY results (the model's or the device's) to the contract of the comment it cites.

tests/test_arith_cases_cpu.py runs the models and a table of mutants over the sets, tests/test_gpu_arith_primitives.py the
device through csrc/hefx_arith_probe.hip (the op codes below mirror its table).
"""
from __future__ import annotations

import random
import struct

from tests.policy_sets import C40_LO, primes_above, primes_below

M64 = (1 << 64) - 1
B45, B49, B52, B53 = 1 << 45, 1 << 49, 1 << 52, 1 << 53


class Violation(AssertionError):
    """a stated range, an exactness claim or a congruence does not hold"""


def need(cond, msg):
    if not cond:
        raise Violation(msg() if callable(msg) else msg)


def dbits(v) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def from_dbits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b & M64))[0]


# ---------------------------------------------------------------------------------------------------------------------
# primes and their constants (computed HERE, from Python integers: the probe takes them as plain words)
# ---------------------------------------------------------------------------------------------------------------------
RINGS = (1024, 32768)


def prime_table(N: int) -> dict:
    return {
        "min": primes_above(1, N, 1)[0],              # the smallest q = 1 mod 2N
        "f40": primes_below(1 << 40, N, 1)[0],        # inside the c40 window
        "f40lo": primes_below(C40_LO, N, 1)[0],       # just below the window
        "f41": primes_below(1 << 41, N, 1)[0],        # FP64's top
        "i41": primes_above(1 << 41, N, 1)[0],        # first integer prime
        "i60": primes_below(1 << 60, N, 1)[0],        # [0,16q) / MacL at their top
        "i60hi": primes_above(1 << 60, N, 1)[0],      # first [0,8q)-only / MacW-only prime
        "i61": primes_below(1 << 61, N, 1)[0],        # the widest admissible prime
    }


class K:
    """ModConst / ModConstF of one prime, as hefx_capi.cpp derives them (hefx_modarith.cuh: struct ModConst, ModConstF)"""

    def __init__(self, q: int, N: int, name: str = ""):
        self.q, self.N, self.name = q, N, name or f"q{q}"
        r = (1 << 128) // q
        self.r0, self.r1 = r & M64, r >> 64
        self.nq = (1 << 64) - q
        self.ninv = pow(N, -1, q)
        g = 2
        while True:  # a primitive 2N-th root of unity
            psi = pow(g, (q - 1) // (2 * N), q)
            if pow(psi, N, q) == q - 1:
                break
            g += 1
        self.psi = psi
        self.ilw = pow(psi, -(N // 2), q) * self.ninv % q  # itw[1] * N^-1: tw[bitrev(i)] = psi^i, bitrev(1) = N/2
        self.ninv_s, self.ilw_s = self.shoup(self.ninv), self.shoup(self.ilw)
        self.is_f64 = q >> 41 == 0
        self.qf, self.qinv = float(q), 1.0 / float(q)
        self.c32 = (1 << 32) % q
        c40 = (1 << 40) % q
        self.c40 = c40 if (q >> 39) == 1 and c40 < (1 << 23) else 0

    def shoup(self, w: int) -> int:
        return (w << 64) // self.q

    def tw(self, w: int) -> tuple:
        return (w, self.shoup(w))

    def modconst_words(self) -> list:
        return [self.q, self.r0, self.r1, self.ninv, self.ninv_s, self.ilw, self.ilw_s, self.nq]

    def modconstf_words(self) -> list:
        if not self.is_f64:
            return [0] * 8  # q == 0.0 marks a prime too wide for the FP64 policy
        q = self.qf
        return [dbits(v) for v in (q, self.qinv, float(self.ninv), float(self.ninv) / q, float(self.ilw), float(self.ilw) / q,
                                   float(self.c32), float(self.c40))]

    def __repr__(self):
        return f"K({self.name}, N={self.N}, q={self.q})"


_K = {}


def all_K() -> list:
    if not _K:
        for N in RINGS:
            for name, q in prime_table(N).items():
                _K[(name, N)] = K(q, N, f"{name}/{N}")
    return list(_K.values())


def get_K(name: str, N: int = 1024) -> K:
    all_K()
    return _K[(name, N)]


# ---------------------------------------------------------------------------------------------------------------------
# the exact model
# ---------------------------------------------------------------------------------------------------------------------
class Model:
    """Bit-exact restatement of the device primitives for one prime.  Integer words wrap at 2^64 exactly where the device's do;
    claims the source makes about INTERMEDIATE values are asserted with need() where the comment states them.  Mutants
    override single methods (MUTANTS below)."""

    def __init__(self, k: K):
        self.k = k

    # ---- hefx_modarith.cuh ------------------------------------------------------------------------------------------
    def mulhi64(self, a, b):
        return (a * b) >> 64

    def mulhi64_under2(self, x, ws):
        x0, x1, w0, w1 = x & 0xFFFFFFFF, x >> 32, ws & 0xFFFFFFFF, ws >> 32
        r = x1 * w1 + ((x0 * w1) >> 32) + ((x1 * w0) >> 32)
        need(r <= M64, "mulhi64_under2: 'the sum cannot wrap'")
        return r

    def mul_sub_lo64(self, x, w, h, nq):
        return (x * w + h * nq) & M64

    def shoup_lazy(self, x, w, ws, nq=None):
        return self.mul_sub_lo64(x, w, self.mulhi64(x, ws), self.k.nq if nq is None else nq)

    def shoup_lazy4(self, x, w, ws, nq=None):
        return self.mul_sub_lo64(x, w, self.mulhi64_under2(x, ws), self.k.nq if nq is None else nq)

    def csubn(self, x, nm):
        d = (x + nm) & M64
        return x if d > x else d

    def csub(self, x, m):
        return x if x < m else x - m

    def barrett64(self, x):
        k = self.k
        return self.csub((x - self.mulhi64(x, k.r1) * k.q) & M64, k.q)

    def barrett128_lt2q(self, lo, hi):
        k = self.k
        carry = (lo * k.r0) >> 64
        t = lo * k.r1
        t_lo, t_hi = t & M64, t >> 64
        tmp1 = (t_lo + carry) & M64
        tmp3 = (t_hi + (tmp1 < carry)) & M64
        u = hi * k.r0
        u_lo, u_hi = u & M64, u >> 64
        s = (tmp1 + u_lo) & M64
        carry2 = (u_hi + (s < u_lo)) & M64
        qhat = (hi * k.r1 + tmp3 + carry2) & M64
        return (lo - qhat * k.q) & M64

    def barrett128(self, lo, hi):
        return self.csub(self.barrett128_lt2q(lo, hi), self.k.q)

    def mulmod(self, a, b):
        p = a * b
        return self.barrett128(p & M64, p >> 64)

    # ---- ArithU64T<L16> (hefx_ntt.cuh) ------------------------------------------------------------------------------
    def nmul(self, m):  # Ctx::n2q .. n8q: nq << s, as the device forms them
        return (self.k.nq * m) & M64

    def u_ct(self, L16, x, y, w, ws, stage):
        q = self.k.q
        if L16:
            a = self.csubn(x, self.nmul(8)) if stage & 1 else x
        else:
            a = self.csubn(x, self.nmul(4))
        t = self.shoup_lazy4(y, w, ws)
        return (a + t) & M64, (a + ((4 * q) & M64) - t) & M64

    def u_half_twiddle(self, w, ws, h):
        return (self.k.q - w, ~ws & M64) if h else (w, ws)

    def u_ct_half(self, x, y, w, ws):
        return (x + self.shoup_lazy4(y, w, ws)) & M64

    def u_ct_sel(self, L16, x, y, w, ws):
        return ((x if L16 else self.csubn(x, self.nmul(4))) + self.shoup_lazy4(y, w, ws)) & M64

    def u_gs(self, x, y, w, ws):
        q4 = (4 * self.k.q) & M64
        s = self.csubn((x + y) & M64, self.nmul(4))
        d = (x + q4 - y) & M64
        return s, self.shoup_lazy4(d, w, ws)

    def u_gs_last(self, x, y):
        k = self.k
        s, d = (x + y) & M64, (x + ((4 * k.q) & M64) - y) & M64
        return self.shoup_lazy(s, k.ninv, k.ninv_s), self.shoup_lazy(d, k.ilw, k.ilw_s)

    def u_gs_half_sum(self, a0, a1):
        return (a0 + a1) & M64

    def u_gs_half_diff(self, a0, a1, w, ws):
        return self.shoup_lazy4((a0 + ((2 * self.k.q) & M64) - a1) & M64, w, ws)

    def u_inv_add(self, x, y):
        return self.csubn((x + y) & M64, self.nmul(4))

    def u_inv_sub_mul(self, x, y, w, ws):
        return self.shoup_lazy4((x + ((4 * self.k.q) & M64) - y) & M64, w, ws)

    def u_input(self, red, has_sub, x, sub):
        q = self.k.q
        if red == 3:
            return (x + (q - sub)) & M64 if has_sub else self.csubn(x, self.k.nq)
        if red:
            x = self.barrett64(x)
        if has_sub:
            x = x - sub if x >= sub else (x + q - sub) & M64
        return x

    def u_fwd_finish(self, L16, x):
        if L16:
            x = self.csubn(x, self.nmul(8))
        return self.csubn(self.csubn(self.csubn(x, self.nmul(4)), self.nmul(2)), self.k.nq)

    def u_mac_operand_lazy(self, L16, slack, x):
        if slack == 0:
            return self.u_fwd_finish(L16, x)
        if L16:
            x = self.csubn(x, self.nmul(8))
        x = self.csubn(x, self.nmul(4))
        return x if slack >= 2 else self.csubn(x, self.nmul(2))

    def u_inv_finish(self, x):
        return self.csubn(x, self.k.nq)

    def moddown_z(self, f, acc):
        """acc + 4q - csubn(f, 4q): 'acc < 2q: < 6q (no 9q intermediate: primes may reach 2^61)'"""
        z = acc + 4 * self.k.q - self.csubn(f, self.nmul(4))
        need(0 <= z < 6 * self.k.q, "ArithU64T::moddown: z < 6q")
        return z

    def u_moddown(self, L16, has_pt, f, acc, sadd, pt, pinv, pinv_s):
        q = self.k.q
        if L16:
            f = self.csubn(f, self.nmul(8))
        z = self.moddown_z(f, acc)
        need(z <= M64, "ArithU64T::moddown: z fits a word")
        z = self.shoup_lazy(z, pinv, pinv_s) + sadd
        need(z < 3 * q, "ArithU64T::moddown: shoup + sadd < 3q")
        if has_pt:
            return self.mulmod(z, pt)
        return self.csubn(self.csubn(z, self.nmul(2)), self.k.nq)

    # ---- ArithF64 (hefx_ntt.cuh): values are Python integers, the doubles they are held in are exact --------------------
    def exact(self, v, what):
        need(abs(v) < B53 or float(v) == v, lambda: f"{what}: {v} is not exact in a double")
        return v

    def mm_limit(self):
        return B49  # 'the modmul stays EXACT for a left operand below 2^49' (InvRecentre)

    def f_mm(self, y, w):
        k = self.k
        need(abs(y) < self.mm_limit(), "ArithF64::mm: left operand below 2^49")
        p = y * w
        h = float(p)                     # RN(y*w)
        hi = int(h)
        l = self.exact(p - hi, "mm: l = fma(y, w, -h)")   # an error-free product: always representable
        kq = round(h * k.qinv)           # rint(RN(h * RN(1/q)))
        s = hi - kq * k.q
        need(abs(s) < B53, "ArithF64::mm: h - k q 'exact in the FMA'")
        r = s + l
        need(abs(r) < B53, "ArithF64::mm: s + l exact")
        return r

    def f_red(self, x):
        r = x - round(float(self.exact(x, "red")) * self.k.qinv) * self.k.q
        return self.exact(r, "red: fma(-rint(x/q), q, x)")

    def f_to_u64(self, r):
        need(0 <= r < B52, "ArithF64::to_u64: integer in [0, 2^52)")
        return r

    def f_from_u64(self, x):
        need(0 <= x < B52, "ArithF64::from_u64: integer in [0, 2^52)")
        return x

    def f_canon(self, x):
        r = self.f_red(x)
        return self.f_to_u64(r + self.k.q if r < 0 else r)

    def f_reduce_wide(self, x):
        return self.exact(self.f_mm(x >> 32, self.k.c32) + (x & 0xFFFFFFFF), "reduce_wide")

    def c40(self):
        return self.k.c40

    def f_reduce_wide40(self, x):
        a, r = (x >> 40) & 0xFFFFFFFF, x & 0xFFFFFFFFFF
        v = a * self.c40() + r
        need(v < B53, "ArithF64::reduce_wide40: a*c40 + r exact in ONE fma")
        return v

    def f_ct(self, x, y, w):
        t = self.f_mm(y, w)
        return self.exact(x + t, "ct"), self.exact(x - t, "ct")

    def f_gs(self, x, y, w):
        return self.exact(x + y, "gs"), self.f_mm(self.exact(x - y, "gs"), w)

    def f_gs_last(self, x, y):
        return self.f_mm(self.exact(x + y, "gs_last"), self.k.ninv), self.f_mm(self.exact(x - y, "gs_last"), self.k.ilw)

    def f_moddown(self, has_pt, f, acc, sadd, pt, pinv):
        q = self.k.q
        z = self.exact(acc - f, "moddown: acc - f")
        need(abs(z) < 1 << 47, "ArithF64::moddown: 'z is exact and below 2^47'")
        z = self.exact(self.f_mm(z, pinv) + sadd, "moddown")
        if has_pt:
            z = self.f_mm(z, pt)
            return self.f_to_u64(z + q if z < 0 else z)
        return self.f_canon(z)

    # ---- key MAC policies (hefx_mac.cuh) ----------------------------------------------------------------------------
    @staticmethod
    def lo30(v):
        return v & 0x3FFFFFFF

    @staticmethod
    def hi30(v):
        return (v >> 30) & 0xFFFFFFFF

    def macl_cut_reduce(self, x, slack):
        x = self.csubn(self.csubn(x, self.nmul(8)), self.nmul(4))
        if slack < 2:
            x = self.csubn(x, self.nmul(2))
        if slack < 1:
            x = self.csubn(x, self.k.nq)
        return x

    def mac(self, pol, param, t):
        """the probe's MAC op on one tuple; returns its 20 output words (F: doubles as integers)"""
        L, lt2q, diag, cut, slack = param & 0xFF, (param >> 8) & 1, (param >> 9) & 1, (param >> 10) & 1, (param >> 12) & 3
        w, ws, dg = t[0], t[1], (t[2], t[3])
        xs, ks = [], []
        for i in range(L):
            d = t[4 + 6 * i: 10 + 6 * i]
            e, o = d[0], d[1]
            if cut:
                if pol == "W":
                    e, o = self.u_ct(False, e, o, w, ws, 0)
                    e, o = self.u_fwd_finish(False, e), self.u_fwd_finish(False, o)
                elif pol == "L":
                    e, o = self.u_ct(True, e, o, w, ws, 1)
                    e, o = self.macl_cut_reduce(e, slack), self.macl_cut_reduce(o, slack)
                else:
                    e, o = self.f_ct(e, o, w)
            xs.append((e, o))
            ks.append(d[2:6])
        # lanes: (x.x k0.x) (x.y k0.y) (x.x k1.x) (x.y k1.y)
        lanes = [[(x[j & 1], k[j]) for x, k in zip(xs, ks)] for j in range(4)]
        fin, dump = [self.mac_lane(pol, ln) for ln in lanes], None
        if diag:
            inner = [self.mac_result(pol, a, False) if pol != "F" else a for a in fin]
            fin = [self.mac_lane(pol, [(inner[j], dg[j & 1])], diag=True) for j in range(4)]
        res = [self.mac_result(pol, a, lt2q) for a in fin]
        data = [a if pol == "F" else self.mac_result(pol, a, lt2q) for a in fin]
        if pol == "W":
            dump = [wd for a in fin for wd in (a & M64, a >> 64)]
        elif pol == "L":
            dump = [c for a in fin for c in a]
        else:
            dump = list(fin)
        return res + data + dump + [0] * (12 - len(dump))

    def mac_lane(self, pol, terms, diag=False):
        if pol == "W":
            a = 0
            for x, k in terms:
                a += x * k
            need(a < 1 << 128, "MacW: the 128-bit accumulator holds the sum")
            return a
        if pol == "L":
            c = [0, 0, 0]
            for x, k in terms:
                xl, xh, kl, kh = self.lo30(x), self.hi30(x), self.lo30(k), self.hi30(k)
                need(x >> 62 == 0 and k >> 60 == 0, "MacL: x below 2^62 (one 32-bit high limb), k below 2^60")
                c[0] += xl * kl
                c[1] += xl * kh + xh * kl
                c[2] += xh * kh
            need(max(c) <= M64, lambda: f"MacL: a column sum wraps ({max(c) / 2 ** 64:.3f} * 2^64)")
            return tuple(c)
        a = 0
        for x, k in terms:
            a = self.exact(a + self.f_mm(x, k), "MacF: the results add exactly")
        return a

    def mac_result(self, pol, a, lt2q):
        if pol == "F":
            return self.f_canon(a)
        if pol == "L":
            a = a[0] + (a[1] << 30) + (a[2] << 60)
            need(a < 1 << 128, "MacL::fold: 128 bits hold the columns")
        lo, hi = a & M64, a >> 64
        return self.barrett128_lt2q(lo, hi) if lt2q else self.barrett128(lo, hi)


# ---------------------------------------------------------------------------------------------------------------------
# probe op codes (csrc/hefx_arith_probe.hip)
# ---------------------------------------------------------------------------------------------------------------------
OP = dict(mulhi64_under2=1, mul_sub_lo64=2, shoup_lazy=3, shoup_lazy4=4, csub=5, csubn=6, barrett64=7, barrett128_lt2q=8,
          barrett128=9, mulmod=10, u_ct=20, u_half_twiddle=21, u_ct_half=22, u_ct_sel=23, u_gs=24, u_gs_last=25,
          u_gs_half_sum=26, u_gs_half_diff=27, u_inv_add=28, u_inv_sub_mul=29, u_input=30, u_fwd_finish=32, u_mac_operand=33,
          u_inv_finish=36, u_moddown=37, mac_w=40, mac_l=41, mac_f=42, f_mm=50, f_red=51, f_canon=52, f_from_u64=53,
          f_to_u64=54, f_reduce_wide=55, f_reduce_wide40=56, f_ct=57, f_gs=58, f_gs_last=59, f_moddown=60)
MAC_OUT = 20


class Case:
    """one primitive at one parameter on one prime: `tuples` (integers; slots listed in fin / fout are doubles holding that
    integer), `model(m, t)` -> the output tuple, `check(t, out)` raises Violation when `out` breaks the cited contract.
    `family` groups cases for the reports (largest lazy result per primitive)."""

    def __init__(self, k, name, op, param, nin, nout, tuples, model, check, cite, fin=(), fout=(), family=None, top=None):
        self.k, self.name, self.op, self.param, self.nin, self.nout = k, name, OP[op], param, nin, nout
        self.tuples, self.model, self.check, self.cite = [tuple(t) for t in tuples], model, check, cite
        self.fin, self.fout = frozenset(fin), frozenset(fout)
        self.family, self.top = family or name, top  # top: the stated exclusive bound of out[*] in units of q (reports)
        for t in self.tuples:
            assert len(t) == nin, (name, len(t), nin)
        assert 0 < len(self.tuples) <= 1 << 17, name

    def fin_slot(self, i):
        return i in self.fin

    def pack(self):
        return [[dbits(v) if self.fin_slot(i) else v & M64 for i, v in enumerate(t)] for t in self.tuples]

    def model_words(self, m, outs=None):
        """the model's outputs as the 64-bit words the device must deliver"""
        outs = outs if outs is not None else [self.model(m, t) for t in self.tuples]
        return [[dbits(v) if i in self.fout else v & M64 for i, v in enumerate(o)] for o in outs]

    def decode(self, words):
        """device words -> the integers check() takes; an FP64 output that is no integer is a Violation"""
        out = []
        for i, wd in enumerate(words):
            if i in self.fout:
                f = from_dbits(wd)
                need(f == f and abs(f) != float("inf") and f == int(f), lambda: f"{self.name}: FP64 output {f!r} is no integer")
                out.append(int(f))
            else:
                out.append(int(wd))
        return tuple(out)

    def __repr__(self):
        return f"Case({self.name} @ {self.k.name}, {len(self.tuples)} tuples)"


class MacCase(Case):
    def __init__(self, k, name, pol, param, tuples, check, cite):
        L = param & 0xFF
        self.pol = pol
        super().__init__(k, name, "mac_" + pol.lower(), param, 4 + 6 * L, MAC_OUT, tuples,
                         lambda m, t: m.mac(pol, param, t), check, cite, family="Mac" + pol)
        self.cut = (param >> 10) & 1
        if pol == "F":  # doubles: the twiddle, every x pair, and the result_data / accumulator words
            self.fin = frozenset([0] + [4 + 6 * i + j for i in range(L) for j in (0, 1)])
            self.fout = frozenset(range(4, 12))


# ---------------------------------------------------------------------------------------------------------------------
# operand helpers
# ---------------------------------------------------------------------------------------------------------------------
def _rng(k: K, salt: str):
    return random.Random(f"{k.q}/{k.N}/{salt}")


def edge(rng, top: int, seeded: int = 3) -> list:
    """0, the top of a documented range minus one, and seeded values inside it"""
    return [0, top - 1] + [rng.randrange(top) for _ in range(seeded)]


def twiddles(k: K, rng, seeded: int = 2) -> list:
    """{w, floor(w 2^64 / q)} for w in {1, q-1, (q+-1)/2, seeded}, and the half_twiddle (h = 1) of each; last of the plain
    ones the twiddle whose Shoup companion is shortest of its quotient (w 2^64 mod q = q - 1): the one that lets a lazy
    product lose every carry at once and keeps a butterfly at the top of its range"""
    ws = [1, k.q - 1, (k.q - 1) // 2, (k.q + 1) // 2] + [rng.randrange(1, k.q) for _ in range(seeded)]
    ws.append((k.q - 1) * pow(1 << 64, -1, k.q) % k.q)
    out = [k.tw(w) for w in ws]
    out += [(k.q - w, ~s & M64) for w, s in out]
    return out


def carry_e(x, ws):
    """the dropped carry of mulhi64_under2: exact high word minus the estimate"""
    x0, x1, w0, w1 = x & 0xFFFFFFFF, x >> 32, ws & 0xFFFFFFFF, ws >> 32
    return ((x * ws) >> 64) - (x1 * w1 + ((x0 * w1) >> 32) + ((x1 * w0) >> 32))


def solve_carries(k: K, w, ws, rng) -> list:
    """x with dropped carry e = 0, 1 and 2 for this twiddle (seeded search; e = 2 needs wide low words in ws)"""
    got = {}
    for _ in range(4000):
        x = rng.getrandbits(64)
        got.setdefault(carry_e(x, ws), x)
        if len(got) == 3:
            break
    return list(got.values())


def solve_top(k: K, w, ws, rng, model: Model, lazy4: bool) -> list:
    """x whose exact lazy product is as near the range's top (2q / 4q) as this twiddle allows: residues q-1, q-2, ... at the
    largest x (the quotient estimate's shortfall grows with x), the largest results of a seeded search kept"""
    q, winv = k.q, pow(w, -1, k.q)
    f = model.shoup_lazy4 if lazy4 else model.shoup_lazy
    best = []
    for res in [q - 1 - d for d in range(4)] + [rng.randrange(q) for _ in range(24)]:
        x0 = res * winv % q
        jmax = (M64 - x0) // q
        for j in {jmax, jmax - 1, jmax - rng.randrange(1 + min(jmax, 1 << 20))}:
            if j >= 0:
                x = x0 + j * q
                best.append((f(x, w, ws), x))
    for i in range(800):  # all three carries lost at once: a seeded search over the largest words
        x = M64 - rng.getrandbits(40 if i < 100 else 61)
        best.append((f(x, w, ws), x))
    best.sort(reverse=True)
    return [x for _, x in best[:4]] + [(q - 1) * winv % q]   # ... and the residue q-1 itself at a small x


def solve_top_below(k: K, w, ws, top, rng, model: Model, sign=1) -> int:
    """the y < top whose lazy product w*y is largest (sign = 1) or smallest (sign = -1): what keeps a butterfly's sum (its
    difference) at the top of its range"""
    q, winv = k.q, pow(w, -1, k.q)
    top = min(top, 1 << 64)  # (a range that does not fit a word: the out-of-domain sets of the mutant table)
    cand = [rng.randrange(top) for _ in range(24)] + [top - 1]
    for res in ([q - 1, q - 2] if sign > 0 else [0, 1]):
        y0 = res * winv % q
        jmax = (top - 1 - y0) // q
        cand += [y0 + j * q for j in {jmax, jmax - 1, jmax // 2} if j >= 0]
    return max(cand, key=lambda y: sign * model.shoup_lazy4(y, w, ws))


# ---------------------------------------------------------------------------------------------------------------------
# contracts
# ---------------------------------------------------------------------------------------------------------------------
def chk_range(name, v, top, lo=0):
    need(lo <= v < top, lambda: f"{name}: {v} outside [{lo}, {top})")


def chk_cong(name, v, want, q):
    need((v - want) % q == 0, lambda: f"{name}: {v} is not congruent to the exact result mod q")


def chk_abs(name, v, bound):
    need(abs(v) < bound, lambda: f"{name}: |{v}| not below {bound}")


# ---------------------------------------------------------------------------------------------------------------------
# the cases of one prime
# ---------------------------------------------------------------------------------------------------------------------
def modarith_cases(k: K, model=None) -> list:
    q, C = k.q, []
    m = model or Model(k)
    rng = _rng(k, "modarith")
    TW = twiddles(k, rng)
    xs = sorted({0, 1, q - 1, q, (1 << 32) - 1, (1 << 32) + 1, M64} | {rng.getrandbits(64) for _ in range(6)})
    # mulhi64_under2 / shoup_lazy / shoup_lazy4: hefx_modarith.cuh
    tup = []
    for w, ws in TW:
        for x in xs + solve_carries(k, w, ws, rng) + solve_top(k, w, ws, rng, m, True) + solve_top(k, w, ws, rng, m, False):
            tup.append((x, w, ws))

    def chk_under2(t, o):  # "UNDER-estimated by at most 2 ... the sum cannot wrap"
        need(0 <= ((t[0] * t[1]) >> 64) - o[0] <= 2, f"mulhi64_under2: estimate off by {((t[0] * t[1]) >> 64) - o[0]}")

    C.append(Case(k, "mulhi64_under2", "mulhi64_under2", 0, 2, 1, [(x, ws) for x, _, ws in tup],
                  lambda m, t: (m.mulhi64_under2(*t),), chk_under2, "hefx_modarith.cuh mulhi64_under2: under-estimated by at most 2"))

    def chk_msl(t, o):  # "x*w - h*q mod 2^64 ... Same value, bit for bit"
        need(o[0] == (t[0] * t[1] + t[2] * t[3]) & M64, "mul_sub_lo64: not x*w + h*nq mod 2^64")

    C.append(Case(k, "mul_sub_lo64", "mul_sub_lo64", 0, 4, 1,
                  [(x, w, (x * ws) >> 64, k.nq) for x, w, ws in tup] + [(M64, M64, M64, M64), (rng.getrandbits(64),) * 4],
                  lambda m, t: (m.mul_sub_lo64(*t),), chk_msl, "hefx_modarith.cuh mul_sub_lo64: x*w - h*q mod 2^64"))

    def chk_shoup(top, nm):
        def chk(t, o):
            chk_range(nm, o[0], top * q)
            chk_cong(nm, o[0], t[0] * t[1], q)
        return chk

    C.append(Case(k, "shoup_lazy", "shoup_lazy", 0, 3, 1, tup, lambda m, t: (m.shoup_lazy(*t),), chk_shoup(2, "shoup_lazy"),
                  "hefx_modarith.cuh shoup_lazy: [0,2q), valid for ANY 64-bit x", top=2))
    C.append(Case(k, "shoup_lazy4", "shoup_lazy4", 0, 3, 1, tup, lambda m, t: (m.shoup_lazy4(*t),), chk_shoup(4, "shoup_lazy4"),
                  "hefx_modarith.cuh shoup_lazy4: [0,4q) for ANY 64-bit x", top=4))
    # csub / csubn with nq, n2q, n4q, n8q: x in [0,2m) -> [0,m)
    ms = [q, 2 * q, 4 * q] + ([8 * q] if q >> 60 == 0 else [])   # 16q <= 2^64 needs q <= 2^60 (ArithU64T header)

    def chk_csub(t, o, neg):
        mm_ = ((1 << 64) - t[1]) if neg else t[1]
        chk_range("csub", o[0], mm_)
        chk_cong("csub", o[0], t[0], mm_)

    vals = lambda m_: [0, m_ - 1, m_, m_ + 1, 2 * m_ - 1] + [rng.randrange(2 * m_) for _ in range(3)]
    C.append(Case(k, "csub", "csub", 0, 2, 1, [(x, m_) for m_ in ms for x in vals(m_)], lambda m, t: (m.csub(*t),),
                  lambda t, o: chk_csub(t, o, False), "hefx_modarith.cuh csub: x in [0,2m) -> [0,m)"))
    C.append(Case(k, "csubn", "csubn", 0, 2, 1, [(x, (1 << 64) - m_) for m_ in ms for x in vals(m_)],
                  lambda m, t: (m.csubn(*t),), lambda t, o: chk_csub(t, o, True),
                  "hefx_modarith.cuh csubn: x in [0,2m) -> [0,m), nm = 2^64 - m"))

    def chk_canon(nm, want):
        def chk(t, o):
            chk_range(nm, o[0], q)
            chk_cong(nm, o[0], want(t), q)
        return chk

    b64 = [0, q - 1, q, q + 1, 2 * q - 1, M64, M64 - M64 % q, M64 - M64 % q - 1] + [rng.getrandbits(64) for _ in range(8)]
    C.append(Case(k, "barrett64", "barrett64", 0, 1, 1, [(x,) for x in b64], lambda m, t: (m.barrett64(*t),),
                  chk_canon("barrett64", lambda t: t[0]), "hefx_modarith.cuh barrett64: any 64-bit x -> [0,q)", top=1))
    # barrett128_lt2q / barrett128: ANY 128-bit value; mulmod: products of residues (and of the 3q the mod-down feeds it)
    T128 = (1 << 128) - 1
    v128 = [0, q * q - 1, (q - 1) ** 2, T128, M64 << 64]
    for mlt in [1, 2, (1 << 64) // q, T128 // q, T128 // q - 1] + [rng.randrange(1, T128 // q) for _ in range(6)]:
        v128 += [mlt * q - 1, mlt * q, mlt * q + 1]
    # the short quotient estimate: x = m q + (q - 1 - d) at the top of the 128-bit range, where the error x/2^128 is largest
    for j in range(48):
        mlt = T128 // q - 1 - (j if j < 16 else rng.randrange(1 << 20))
        v128 += [mlt * q + q - 1 - d for d in (0, 1)]
    # the lazy sums of mul_sum_kernel / mulplain_sum_kernel (hefx_kernels.hip FOLD INTERVALS: a folded residue plus up to 63
    # products below 2^122 stay below 2^128; the loops fold after at most 32 + 3): quotients beyond one word
    v128 += [min(T128, n * (q - 1) ** 2 + (q - 1)) for n in (16, 32, 35, 63)]
    v128 = [v for v in v128 if 0 <= v <= T128]

    def chk_b128(top, nm):
        def chk(t, o):
            chk_range(nm, o[0], top * q)
            chk_cong(nm, o[0], t[0] + (t[1] << 64), q)
        return chk

    t128 = [(v & M64, v >> 64) for v in v128]
    C.append(Case(k, "barrett128_lt2q", "barrett128_lt2q", 0, 2, 1, t128, lambda m, t: (m.barrett128_lt2q(*t),),
                  chk_b128(2, "barrett128_lt2q"), "hefx_modarith.cuh barrett128_lt2q: ANY 128-bit (hi:lo) -> [0,2q)", top=2))
    C.append(Case(k, "barrett128", "barrett128", 0, 2, 1, t128, lambda m, t: (m.barrett128(*t),),
                  chk_b128(1, "barrett128"), "hefx_modarith.cuh barrett128: any 128-bit (hi:lo) -> [0,q)", top=1))
    ab = [0, 1, q - 1, (q + 1) // 2] + [rng.randrange(q) for _ in range(4)]
    tmm = [(a, b) for a in ab + [3 * q - 1, 2 * q] for b in ab]
    C.append(Case(k, "mulmod", "mulmod", 0, 2, 1, tmm, lambda m, t: (m.mulmod(*t),), chk_canon("mulmod", lambda t: t[0] * t[1]),
                  "hefx_modarith.cuh mulmod; hefx_ntt.cuh ArithU64T::moddown: product < 3q*q < q*2^64 -> [0,q)", top=1))
    return C


def u64_cases(k: K, L16: bool, model=None) -> list:
    """ArithU64T<L16> (hefx_ntt.cuh).  L16 needs q < 2^60."""
    q, C, b = k.q, [], int(L16)
    rng = _rng(k, f"u64/{b}")
    TW = twiddles(k, rng)
    tag = "U64L" if L16 else "U64"
    fam = lambda s: f"{tag}::{s}"

    m0 = Model(k)

    def two(top_x, top_y=None):
        X, Y = edge(rng, top_x), edge(rng, top_y or top_x)
        return [(x, y) for x in X for y in Y]

    def bf(top_x, top_y=None):
        """(x, y, w, ws): the edges and seeded values against every twiddle, and per twiddle x at its top with the y that makes
        the twiddle product largest and smallest"""
        out = [(x, y, w, ws) for x, y in two(top_x, top_y) for w, ws in TW]
        for w, ws in TW:
            for sign in (1, -1):
                out.append((top_x - 1, solve_top_below(k, w, ws, top_y or top_x, rng, m0, sign), w, ws))
        return out

    def rng_cong(nm, tops, wants):
        def chk(t, o):
            for i, (top, want) in enumerate(zip(tops, wants)):
                chk_range(f"{nm}[{i}]", o[i], top * q)
                chk_cong(f"{nm}[{i}]", o[i], want(t), q)
        return chk

    cite_ct = ("hefx_ntt.cuh ArithU64T: even stage inputs < 12q -> < 16q, odd stage (by 8q) inputs < 16q -> < 12q"
               if L16 else "hefx_ntt.cuh ArithU64T::ct: L16 = false: inputs/outputs in [0,8q)")
    for stage in (0, 1):
        tin, tout = ((12, 16) if stage == 0 else (16, 12)) if L16 else (8, 8)
        C.append(Case(k, fam(f"ct/stage{stage}"), "u_ct", b | stage << 1, 4, 2,
                      bf(tin * q),
                      lambda m, t, s=stage: m.u_ct(L16, *t, s),
                      rng_cong("ct", (tout, tout), (lambda t: t[0] + t[2] * t[1], lambda t: t[0] - t[2] * t[1])), cite_ct,
                      family=fam("ct"), top=tout))
    for h in (0, 1):
        def chk_ht(t, o, h=h):  # "(q - w, ~w') is the Shoup pair of -w"
            wn = (q - t[0]) if h else t[0]
            need(o[0] == wn and o[1] == (wn << 64) // q, "half_twiddle: not the Shoup pair of (-1)^h w")
        C.append(Case(k, fam(f"half_twiddle/{h}"), "u_half_twiddle", b | h << 1, 2, 2, [tw for tw in TW],
                      lambda m, t, h=h: m.u_half_twiddle(*t, h), chk_ht, "hefx_ntt.cuh ArithU64T::half_twiddle"))
    # ct_half: x, y canonical -> < 5q; or the RED == 3 inputs below 3q -> < 7q (ArithU64T::input)
    for nm, tx in (("canon", 1), ("lt3q", 3)):
        C.append(Case(k, fam(f"ct_half/{nm}"), "u_ct_half", b, 4, 1, bf(tx * q),
                      lambda m, t: (m.u_ct_half(*t),), rng_cong("ct_half", (tx + 4,), (lambda t: t[0] + t[2] * t[1],)),
                      "hefx_ntt.cuh ArithU64T::ct_half: < 5q (input<3>: < 3q + 4q = 7q < 8q)", family=fam("ct_half"), top=tx + 4))
    # ct_sel: second stage on values < 5q -> < 8q (L16: 5q + 4q < 12q); of two < 7q values -> < 11q < 12q (L16) / < 8q
    for nm, tx in (("lt5q", 5), ("lt7q", 7)):
        tout = tx + 4 if L16 else 8
        C.append(Case(k, fam(f"ct_sel/{nm}"), "u_ct_sel", b, 4, 1, bf(tx * q),
                      lambda m, t: (m.u_ct_sel(L16, *t),), rng_cong("ct_sel", (tout,), (lambda t: t[0] + t[2] * t[1],)),
                      "hefx_ntt.cuh ArithU64T::ct_sel: values < 5q -> < 8q; L16: 5q + 4q < 12q; input<3>: < 11q < 12q",
                      family=fam("ct_sel"), top=tout))
    if not L16:  # every inverse transform runs ArithU64T<false>
        inv4 = bf(4 * q)
        C.append(Case(k, fam("gs"), "u_gs", b, 4, 2, inv4, lambda m, t: m.u_gs(*t),
                      rng_cong("gs", (4, 4), (lambda t: t[0] + t[1], lambda t: (t[0] - t[1]) * t[2])),
                      "hefx_ntt.cuh ArithU64T::gs: inputs/outputs in [0,4q)", top=4))
        C.append(Case(k, fam("gs_last"), "u_gs_last", b, 2, 2, two(4 * q) + [(rng.randrange(4 * q), rng.randrange(4 * q)) for _ in range(64)],
                      lambda m, t: m.u_gs_last(*t),
                      rng_cong("gs_last", (2, 2), (lambda t: (t[0] + t[1]) * k.ninv, lambda t: (t[0] - t[1]) * k.ilw)),
                      "hefx_ntt.cuh ArithU64T::gs_last: outputs in [0,2q), what inv_finish expects", top=2))
        C.append(Case(k, fam("gs_half_sum"), "u_gs_half_sum", b, 2, 1, two(2 * q), lambda m, t: (m.u_gs_half_sum(*t),),
                      rng_cong("gs_half_sum", (4,), (lambda t: t[0] + t[1],)),
                      "hefx_ntt.cuh ArithU64T::gs_half_sum: words below 2q -> < 4q", top=4))
        C.append(Case(k, fam("gs_half_diff"), "u_gs_half_diff", b, 4, 1, bf(2 * q),
                      lambda m, t: (m.u_gs_half_diff(*t),), rng_cong("gs_half_diff", (4,), (lambda t: (t[0] - t[1]) * t[2],)),
                      "hefx_ntt.cuh ArithU64T::gs_half_diff: a0, a1 below 2q", top=4))
        C.append(Case(k, fam("inv_add"), "u_inv_add", b, 2, 1, two(4 * q), lambda m, t: (m.u_inv_add(*t),),
                      rng_cong("inv_add", (4,), (lambda t: t[0] + t[1],)),
                      "hefx_ntt.cuh ArithU64T::inv_add: two values of [0,4q) -> [0,4q)", top=4))
        C.append(Case(k, fam("inv_sub_mul"), "u_inv_sub_mul", b, 4, 1, inv4, lambda m, t: (m.u_inv_sub_mul(*t),),
                      rng_cong("inv_sub_mul", (4,), (lambda t: (t[0] - t[1]) * t[2],)),
                      "hefx_ntt.cuh ArithU64T::inv_sub_mul: two values of [0,4q) -> [0,4q)", top=4))
        C.append(Case(k, fam("inv_finish"), "u_inv_finish", b, 1, 1, [(x,) for x in edge(rng, 2 * q, 8) + [q - 1, q]],
                      lambda m, t: (m.u_inv_finish(*t),), rng_cong("inv_finish", (1,), (lambda t: t[0],)),
                      "hefx_ntt.cuh ArithU64T::inv_finish: [0,2q) -> canonical", top=1))
    # input<1> (any word), input<3> (below 2q), with and without the constant
    subs = [0, 1, q - 1, rng.randrange(q)]
    any64 = [0, q - 1, q, 2 * q - 1, M64] + [rng.getrandbits(64) for _ in range(6)]
    for red, xs in ((1, any64), (3, edge(rng, 2 * q, 6) + [q - 1, q])):
        for has_sub in (0, 1):
            top = 3 if (red == 3 and has_sub) else 1
            C.append(Case(k, fam(f"input<{red}>/sub{has_sub}"), "u_input", b | red << 1 | has_sub << 3, 2, 1,
                          [(x, s) for x in xs for s in subs], lambda m, t, r=red, hs=has_sub: (m.u_input(r, hs, *t),),
                          rng_cong("input", (top,), (lambda t, hs=has_sub: t[0] - (t[1] if hs else 0),)),
                          "hefx_ntt.cuh ArithU64T::input: RED 1 Barrett -> canonical; RED 3: x + (q - sub) < 3q", family=fam("input"),
                          top=top))
    ftop = 16 if L16 else 8
    fx = [(x,) for x in edge(rng, ftop * q, 8) + [j * q + d for j in range(1, ftop) for d in (-1, 0)]]
    C.append(Case(k, fam("fwd_finish"), "u_fwd_finish", b, 1, 1, fx, lambda m, t: (m.u_fwd_finish(L16, *t),),
                  rng_cong("fwd_finish", (1,), (lambda t: t[0],)), "hefx_ntt.cuh ArithU64T::fwd_finish: < 16q -> < 8q -> canonical", top=1))
    for slack, top in ((0, 1), (1, 2), (2, 4)):
        C.append(Case(k, fam(f"mac_operand/slack{slack}"), "u_mac_operand", b | slack << 1, 1, 1, fx,
                      lambda m, t, s=slack: (m.u_mac_operand_lazy(L16, s, *t),), rng_cong("mac_operand", (top,), (lambda t: t[0],)),
                      "hefx_ntt.cuh ArithU64T::mac_operand / mac_operand_lazy<SLACK>: 1: < 2q, 2: < 4q", family=fam("mac_operand"),
                      top=top))
    # moddown: f unfinished (< 8q / < 16q), acc < 2q, sadd and pt canonical
    fs, accs = edge(rng, ftop * q, 2) + [4 * q - 1, 4 * q], [0, 2 * q - 1, rng.randrange(2 * q)]
    pinvs = [TW[1], TW[4], TW[5]]
    for has_pt in (0, 1):
        tup = [(f, a, s, p, w, ws) for f in fs for a in accs for s in (0, q - 1) for p in (1, q - 1, rng.randrange(q))
               for w, ws in pinvs]
        C.append(Case(k, fam(f"moddown/pt{has_pt}"), "u_moddown", b | has_pt << 1, 6, 1, tup,
                      lambda m, t, hp=has_pt: (m.u_moddown(L16, hp, *t),),
                      rng_cong("moddown", (1,), (lambda t, hp=has_pt: ((t[1] - t[0]) * t[4] + t[2]) * (t[3] if hp else 1),)),
                      "hefx_ntt.cuh ArithU64T::moddown: acc < 2q ... < 6q ... < 3q, canonical out", family=fam("moddown"), top=1))
    return C


def mm_search(k: K, w: int, limit: int, rng, keep: int = 4, tries: int = 600) -> list:
    """left operands y, |y| < limit, whose exact residue y*w mod q lies next to +-q/2 -- within the quotient estimate's own
    error, about 3 |y| 2^-53 -- so that rint() can land on the far side of the tie; the largest |mm|/q in the model kept"""
    q, m, winv = k.q, Model(k), pow(w, -1, k.q)
    span = max(2, (3 * limit * q) >> 53)
    best = []
    for i in range(tries):
        r = (q // 2 + (i % 2) + rng.randrange(-span, span + 1)) % q
        y0 = r * winv % q
        jmax = (limit - 1 - y0) // q
        if jmax < 0:
            continue
        y = y0 + q * (jmax - rng.randrange(1 + min(jmax, 3)))
        for yy in (y, -y):
            best.append((abs(m.f_mm(yy, w)), yy))
    best.sort(reverse=True)
    return [y for _, y in best[:keep]]


def f64_cases(k: K, model=None) -> list:
    """ArithF64 (hefx_ntt.cuh) and MacF; primes below 2^41 only"""
    assert k.is_f64
    q, C = k.q, []
    rng = _rng(k, "f64")
    sg = lambda v: [v, -v]
    ws = [1, q - 1, (q - 1) // 2, (q + 1) // 2] + [rng.randrange(1, q) for _ in range(3)]
    ws = ws + [-w for w in ws]   # half_twiddle(h = 1) = -w
    chk45 = lambda nm, want: lambda t, o: (chk_abs(nm, 100 * o[0], 52 * q), chk_cong(nm, o[0], want(t), q))
    chk49 = lambda nm, want: lambda t, o: (chk_abs(nm, 100 * o[0], 75 * q), chk_cong(nm, o[0], want(t), q))
    for nm, lim, chk in (("2^45", B45, chk45), ("2^49", B49, chk49)):
        ys = [0, 1, -1] + sg(lim - 1) + sg(lim - 2) + [rng.randrange(-lim + 1, lim) for _ in range(8)]
        tup = [(y, w) for w in ws for y in ys + mm_search(k, abs(w), lim, rng)]
        C.append(Case(k, f"F64::mm/{nm}", "f_mm", 0, 2, 1, tup, lambda m, t: (m.f_mm(*t),), chk("mm", lambda t: t[0] * t[1]),
                      "hefx_ntt.cuh ArithF64::mm: exact, (-0.52q, 0.52q) for |y| < 2^45; InvRecentre: < 0.75q up to 2^49",
                      fin=(0, 1), fout=(0,), family=f"F64::mm/{nm}"))
    xs = [0] + sg(1) + sg(q // 2) + sg(q // 2 + 1) + sg(q) + sg(B49 - 1) + [rng.randrange(-B49, B49) for _ in range(16)]
    C.append(Case(k, "F64::red", "f_red", 0, 1, 1, [(x,) for x in xs], lambda m, t: (m.f_red(*t),),
                  lambda t, o: (need(2 * abs(o[0]) <= q, "red: outside [-0.5q, 0.5q]"), chk_cong("red", o[0], t[0], q)),
                  "hefx_ntt.cuh ArithF64::red: exact, result in [-0.5q, 0.5q]", fin=(0,), fout=(0,)))
    C.append(Case(k, "F64::canon", "f_canon", 0, 1, 1, [(x,) for x in xs], lambda m, t: (m.f_canon(*t),),
                  lambda t, o: (chk_range("canon", o[0], q), chk_cong("canon", o[0], t[0], q)),
                  "hefx_ntt.cuh ArithF64::canon", fin=(0,)))
    us = [0, 1, q - 1, B52 - 1, B52 - 2] + [rng.randrange(B52) for _ in range(8)]
    same = lambda t, o: need(o[0] == t[0], "from_u64 / to_u64: not the same integer")
    C.append(Case(k, "F64::from_u64", "f_from_u64", 0, 1, 1, [(u,) for u in us], lambda m, t: (m.f_from_u64(*t),), same,
                  "hefx_ntt.cuh ArithF64::from_u64: integers in [0, 2^52)", fout=(0,)))
    C.append(Case(k, "F64::to_u64", "f_to_u64", 0, 1, 1, [(u,) for u in us], lambda m, t: (m.f_to_u64(*t),), same,
                  "hefx_ntt.cuh ArithF64::to_u64", fin=(0,)))
    w64 = [0, 1, q - 1, q, (1 << 32) - 1, 1 << 32, M64, M64 - 1, (1 << 61) - 1] + [rng.getrandbits(64) for _ in range(24)]

    def chk_wide(t, o):  # "in (-0.52q, 0.52q + 2^32)"
        need(-52 * q < 100 * o[0] < 52 * q + 100 * (1 << 32), "reduce_wide: outside (-0.52q, 0.52q + 2^32)")
        chk_cong("reduce_wide", o[0], t[0], q)

    C.append(Case(k, "F64::reduce_wide", "f_reduce_wide", 0, 1, 1, [(x,) for x in w64], lambda m, t: (m.f_reduce_wide(*t),), chk_wide,
                  "hefx_ntt.cuh ArithF64::reduce_wide: any 64-bit word -> (-0.52q, 0.52q + 2^32)", fout=(0,)))
    if k.c40:
        x40 = [0, (1 << 40) - 1, 1 << 40, (1 << 61) - 1, (1 << 61) - (1 << 40)] + [rng.getrandbits(61) for _ in range(16)]
        C.append(Case(k, "F64::reduce_wide40", "f_reduce_wide40", 0, 1, 1, [(x,) for x in x40],
                      lambda m, t: (m.f_reduce_wide40(*t),),
                      lambda t, o: (chk_range("reduce_wide40", o[0], B45), chk_cong("reduce_wide40", o[0], t[0], q)),
                      "hefx_ntt.cuh ArithF64::reduce_wide40: x < 2^61 -> a*c40 + r < 2^45, ONE fma", fout=(0,)))
    # butterflies: left operands of mm below 2^45, the sum path bounded by the transform's own growth
    v45 = [0] + sg(B45 - 1) + [rng.randrange(-B45 + 1, B45) for _ in range(3)]
    pairs = [(x, y) for x in v45 for y in v45]

    def chk_bf(nm, wants, bounds):
        def chk(t, o):
            for i in range(2):
                chk_abs(f"{nm}[{i}]", 100 * o[i], bounds[i])
                chk_cong(f"{nm}[{i}]", o[i], wants[i](t), q)
        return chk

    C.append(Case(k, "F64::ct", "f_ct", 0, 3, 2, [(x, y, w) for x, y in pairs for w in ws], lambda m, t: m.f_ct(*t),
                  chk_bf("ct", (lambda t: t[0] + t[2] * t[1], lambda t: t[0] - t[2] * t[1]), (100 * B45 + 52 * q,) * 2),
                  "hefx_ntt.cuh ArithF64::ct: growth 0.52q per stage", fin=(0, 1, 2), fout=(0, 1)))
    # gs: |x|, |y| up to 64q (InvRecentre::SMAX = 7): the difference below 128q < 2^48, the sum below 128q
    v64 = [0] + sg(64 * q - 1) + [rng.randrange(-64 * q + 1, 64 * q) for _ in range(3)]
    pg = [(x, y) for x in v64 for y in v64]
    C.append(Case(k, "F64::gs", "f_gs", 0, 3, 2, [(x, y, w) for x, y in pg for w in ws[:7]], lambda m, t: m.f_gs(*t),
                  chk_bf("gs", (lambda t: t[0] + t[1], lambda t: (t[0] - t[1]) * t[2]), (100 * 128 * q, 75 * q)),
                  "hefx_ntt.cuh InvRecentre: a stage entered up to 64q feeds the modmul < 128q < 2^48: |t| < 0.75q",
                  fin=(0, 1, 2), fout=(0, 1)))
    C.append(Case(k, "F64::gs_last", "f_gs_last", 0, 2, 2, pg, lambda m, t: m.f_gs_last(*t),
                  chk_bf("gs_last", (lambda t: (t[0] + t[1]) * k.ninv, lambda t: (t[0] - t[1]) * k.ilw), (75 * q, 75 * q)),
                  "hefx_ntt.cuh ArithF64::gs_last / InvRecentre", fin=(0, 1), fout=(0, 1)))
    # moddown: |acc| up to the stated 2^46, |f| up to 2^45
    accs = [0] + sg((1 << 46) - 1) + [rng.randrange(-(1 << 46) + 1, 1 << 46) for _ in range(2)]
    fs = [0] + sg(B45 - 1) + [rng.randrange(-B45 + 1, B45) for _ in range(2)]
    for has_pt in (0, 1):
        tup = [(f, a, s, p, pv) for f in fs for a in accs for s in (0, q - 1) for p in (1, q - 1, rng.randrange(q)) for pv in ws[1:6:2]]
        C.append(Case(k, f"F64::moddown/pt{has_pt}", "f_moddown", has_pt, 5, 1, tup,
                      lambda m, t, hp=has_pt: (m.f_moddown(hp, t[0], t[1], t[2], t[3], t[4]),),
                      lambda t, o, hp=has_pt: (chk_range("moddown", o[0], q),
                                               chk_cong("moddown", o[0], ((t[1] - t[0]) * t[4] + t[2]) * (t[3] if hp else 1), q)),
                      "hefx_ntt.cuh ArithF64::moddown: |acc| < 2^46, |f| < 2^45, z below 2^47; canonical out",
                      fin=(0, 1, 4), family="F64::moddown"))
    return C


# ---- key MAC ----------------------------------------------------------------------------------------------------------
def mac_param(L, lt2q=0, diag=0, cut=0, slack=0):
    return L | lt2q << 8 | diag << 9 | cut << 10 | slack << 12


def mac_x_slack(k: K, L: int) -> int:
    """hefx_mac.cuh mac_x_slack"""
    if k.is_f64 or k.q >> 60:
        return 0
    return 2 if L <= 3 else (1 if L <= 5 else 0)


def mac_exact(c: MacCase, t):
    """the four exact sums sum_i x_i k_i (after the cut's last stage: E + w O, E - w O), as integers"""
    L, cut, diag = c.param & 0xFF, (c.param >> 10) & 1, (c.param >> 9) & 1
    w, dg = t[0], (t[2], t[3])
    s = [0, 0, 0, 0]
    for i in range(L):
        d = t[4 + 6 * i: 10 + 6 * i]
        x = (d[0] + w * d[1], d[0] - w * d[1]) if cut else (d[0], d[1])
        for j in range(4):
            s[j] += x[j & 1] * d[2 + j]
    return [s[j] * dg[j & 1] for j in range(4)] if diag else s


def mac_check(c: MacCase):
    q, pol = c.k.q, c.pol
    lt2q = (c.param >> 8) & 1
    L, diag = c.param & 0xFF, (c.param >> 9) & 1

    def chk(t, o):
        want = mac_exact(c, t)
        for j in range(4):
            chk_range(f"Mac{pol}::result[{j}]", o[j], (2 if lt2q and pol != "F" else 1) * q)
            chk_cong(f"Mac{pol}::result[{j}]", o[j], want[j], q)
            if pol == "F":   # result_data: the unfinished sum, |a| <= L * 0.52q (mac_diag: one product, < 0.75q)
                chk_abs("MacF::result_data", 100 * o[4 + j], (75 if diag else 52 * L) * q + 1)
                chk_cong("MacF::result_data", o[4 + j], want[j], q)
                need(o[8 + j] == o[4 + j], "MacF: accumulator and result_data differ")
            else:
                need(o[4 + j] == o[j], f"Mac{pol}::result_data is result<LT2Q>")
        if pol == "L":       # the columns put together are the exact sum: no column wrapped
            for j in range(4):
                col = o[8 + 3 * j: 11 + 3 * j]
                chk_cong("MacL columns", col[0] + (col[1] << 30) + (col[2] << 60), want[j], q)
        if pol == "W":
            for j in range(4):
                chk_cong("MacW accumulator", o[8 + 2 * j] + (o[9 + 2 * j] << 64), want[j], q)
    return chk


MACL_LEVELS = (1, 3, 4, 5, 6, 8)
MACW_LEVELS = MACL_LEVELS + (9, 16, 61)
MACF_LEVELS = (1, 8, 30, 61)


def mac_tuple(k, rng, L, xtop, ktop, kind, hdr):
    """kind 'max': every x at xtop - 1 and every k at ktop - 1; 'seeded': inside the ranges"""
    t = list(hdr)
    for _ in range(L):
        if kind == "max":
            t += [xtop - 1, xtop - 1] + [ktop - 1] * 4
        else:
            t += [rng.randrange(xtop), rng.randrange(xtop)] + [rng.randrange(ktop) for _ in range(4)]
    return t


def mac_int_cases(k: K, pol: str, levels=None, slack_of=None) -> list:
    """MacW (any prime) / MacL (q < 2^60, L <= 8): x at the top of what mac_x_slack allows, k = q - 1, both results, the
    diagonal product of a full inner sum, and the parity cut's last stage"""
    q, C = k.q, []
    rng = _rng(k, "mac" + pol)
    slack_of = slack_of or (lambda L: mac_x_slack(k, L) if pol == "L" else 0)
    TW = twiddles(k, rng, 1)
    for L in levels or (MACL_LEVELS if pol == "L" else MACW_LEVELS):
        slack = slack_of(L)
        xtop = (1 << slack) * q
        hdr = (TW[4][0], TW[4][1], q - 1, rng.randrange(q))
        plain = [mac_tuple(k, rng, L, xtop, q, kind, hdr) for kind in ("max", "seeded", "seeded")]
        cite = ("hefx_mac.cuh MacL / mac_x_slack: (2^60 + 2^62) L < 2^64 for L <= 3, (2^60 + 2^61) L for L <= 5; result<LT2Q> below 2q"
                if pol == "L" else "hefx_mac.cuh MacW: full 128-bit accumulators; result<LT2Q>: words below 2q")
        for lt2q in (0, 1):
            for diag in (0, 1):
                c = MacCase(k, f"Mac{pol}/L{L}/lt2q{lt2q}/diag{diag}", pol, mac_param(L, lt2q, diag, 0, slack), plain, None, cite)
                c.check = mac_check(c)
                C.append(c)
        # the cut: E, O as the producer leaves them -- MacL: the L16 transform's unfinished words, below 16q; MacW: canonical
        # words (parity_fwd_a, MAC_W), and the [0,8q) butterfly's own range
        etops = (16 * q,) if pol == "L" else (q, 8 * q)
        cut = []
        for etop in etops:
            for w, ws in (TW[1], TW[4], TW[3]):
                h = (w, ws, 0, 0)
                cut += [mac_tuple(k, rng, L, etop, q, kind, h) for kind in ("max", "seeded")]
        c = MacCase(k, f"Mac{pol}/L{L}/cut", pol, mac_param(L, 0, 0, 1, slack), cut, None,
                    "hefx_mac.cuh xin_cut / cut_reduce: E, O below 16q -> odd-stage butterfly < 12q -> what slack allows"
                    if pol == "L" else "hefx_mac.cuh MacW::xin_cut: the [0,8q) butterfly, canonical words out")
        c.check = mac_check(c)
        C.append(c)
    return C


def macf_cases(k: K) -> list:
    q, C = k.q, []
    rng = _rng(k, "macF")
    for L in MACF_LEVELS:
        def xs(kind, lim):
            t = [rng.randrange(1, q), 0, q - 1, rng.randrange(q)]
            for i in range(L):
                if kind == "max":
                    t += [(lim - 1) * (-1) ** i, -(lim - 1)] + [q - 1] * 4
                else:
                    t += [rng.randrange(-lim + 1, lim) for _ in range(2)] + [rng.randrange(q) for _ in range(4)]
            return t
        # every digit with its own near-tie operand: |mm| at its largest in every term, all of one sign where the search allows
        w = rng.randrange(1, q)
        ys = mm_search(k, w, B45, rng, keep=2 * L, tries=300)
        pos = [y for y in ys if Model(k).f_mm(y, w) > 0] or ys
        tie = [rng.randrange(1, q), 0, q - 1, q - 1]
        for i in range(L):
            tie += [pos[i % len(pos)], pos[(i + 1) % len(pos)]] + [w] * 4
        plain = [xs("max", B45), xs("seeded", B45), xs("seeded", B45), tie]
        for diag in (0, 1):
            c = MacCase(k, f"MacF/L{L}/diag{diag}", "F", mac_param(L, 0, diag), plain, None,
                        "hefx_mac.cuh MacF: |sums| <= L * 0.52q < 2^46; mac_diag: valid left operands of mm as they are")
            c.check = mac_check(c)
            C.append(c)
        # the cut: |E|, |O| < 2^41 + (LOGN-1) * 0.52q < 2^45
        lim = (1 << 41) + 15 * q * 52 // 100
        c = MacCase(k, f"MacF/L{L}/cut", "F", mac_param(L, 0, 0, 1), [xs("max", lim), xs("seeded", lim)], None,
                    "hefx_mac.cuh MacF::xin_cut: |E|, |O| < 2^41 + (LOGN-1) * 0.52q < 2^45, results valid left operands of mac")
        c.check = mac_check(c)
        C.append(c)
    return C


_CASES = {}


def cases(k: K) -> list:
    """every case of prime k, by the policies the engine would run on it"""
    if id(k) not in _CASES:
        C = modarith_cases(k)
        if k.is_f64:
            C += f64_cases(k) + macf_cases(k)
        else:
            C += u64_cases(k, False)
            if k.q >> 60 == 0:
                C += u64_cases(k, True) + mac_int_cases(k, "L")
            C += mac_int_cases(k, "W")
        _CASES[id(k)] = C
    return _CASES[id(k)]


def run_model(c: Case, m: Model = None) -> list:
    """model outputs of every tuple, each held to the case's contract; raises Violation"""
    m = m or Model(c.k)
    outs = []
    for t in c.tuples:
        o = tuple(c.model(m, t))
        c.check(t, o)
        outs.append(o)
    return outs


# ---------------------------------------------------------------------------------------------------------------------
# mutants: a wrong primitive that the committed sets must catch
# ---------------------------------------------------------------------------------------------------------------------
class Under2DropsOne(Model):
    """under2 dropping one more partial product (hi32(x1 w0) too)"""
    def mulhi64_under2(self, x, ws):
        x0, x1, w1 = x & 0xFFFFFFFF, x >> 32, ws >> 32
        return x1 * w1 + ((x0 * w1) >> 32)


class NoOddStageSub(Model):
    """the 16q butterfly without its odd-stage subtraction"""
    def u_ct(self, L16, x, y, w, ws, stage):
        return super().u_ct(L16, x, y, w, ws, 0 if L16 else stage)


class Moddown9q(Model):
    """moddown forming acc + 8q - f on the unreduced f (a 9q intermediate) instead of acc + 4q - csubn(f, 4q)"""
    def moddown_z(self, f, acc):
        return (acc + ((8 * self.k.q) & M64) - f) & M64


class Wide40AnyPrime(Model):
    """reduce_wide40 outside its window: c40 = 2^40 mod q whatever q"""
    def c40(self):
        return (1 << 40) % self.k.q


class MmTakes2p53(Model):
    """mm fed left operands up to 2^53"""
    def mm_limit(self):
        return B53 + 1


def _first_violation(cs, m) -> str:
    for c in cs:
        try:
            run_model(c, m)
        except Violation as e:
            return f"{c.name} @ {c.k.name}: {e}"
    return ""


def _mm_2p53(k):
    rng = _rng(k, "mm53")
    ys = [B53, -B53, B53 - 1] + [rng.randrange(B52, B53) for _ in range(61)]
    base = [c for c in f64_cases(k) if c.name == "F64::mm/2^49"][0]
    ws = sorted({t[1] for t in base.tuples})
    return [Case(k, "F64::mm/2^53", "f_mm", 0, 2, 1, [(y, w) for y in ys for w in ws], base.model, base.check, base.cite,
                 fin=(0, 1), fout=(0,))]


def _reduce40_outside(k):
    rng = _rng(k, "w40")
    x40 = [0, (1 << 40) - 1, 1 << 40, (1 << 61) - 1] + [rng.getrandbits(61) for _ in range(16)]
    return [Case(k, "F64::reduce_wide40", "f_reduce_wide40", 0, 1, 1, [(x,) for x in x40], lambda m, t: (m.f_reduce_wide40(*t),),
                 lambda t, o: (chk_range("reduce_wide40", o[0], B45), chk_cong("reduce_wide40", o[0], t[0], k.q)),
                 "hefx_ntt.cuh ArithF64::reduce_wide40", fout=(0,))]


def mutants() -> dict:
    """name -> (cases, model): the model is wrong (or the policy is applied outside its domain); running it over the cases
    must raise a Violation"""
    i60, i61 = get_K("i60"), get_K("i61")
    f40_min = K(primes_above(1 << 39, 1024, 1)[0], 1024, "f40min/1024")   # the smallest 40-bit prime: outside the c40 window
    by = lambda cs, sub: [c for c in cs if sub in c.name]
    return {
        "under2 drops one more partial product": (by(modarith_cases(i60), "shoup_lazy4"), Under2DropsOne(i60)),
        "16q butterfly without the odd-stage subtraction, q just below 2^60": (by(u64_cases(i60, True), "ct/stage1"), NoOddStageSub(i60)),
        "MacL slack 2 at L = 4": (mac_int_cases(i60, "L", (4,), lambda L: 2), Model(i60)),
        "MacL slack 1 at L = 6": (mac_int_cases(i60, "L", (6,), lambda L: 1), Model(i60)),
        "the [0,16q) form applied to a 61-bit prime": (by(u64_cases(i61, True), "ct/"), Model(i61)),
        "reduce_wide40 outside its window (smallest 40-bit prime)": (_reduce40_outside(f40_min), Wide40AnyPrime(f40_min)),
        "mm fed 2^53": (_mm_2p53(get_K("f41")), MmTakes2p53(get_K("f41"))),
        "moddown forming 9q": (by(u64_cases(i61, False), "moddown"), Moddown9q(i61)),
    }


def mutant_caught(name: str) -> str:
    cs, m = mutants()[name]
    return _first_violation(cs, m)
