"""Polynomial plans on the Python side (include/hefx_poly.h): the planner itself is host-only C++ inside libhefx.so
(csrc/hefx_poly_plan.h) and is READ here through ctypes, never restated -- the Python and the C++ executor run the same step
list.  The one thing with a Python twin is the weight rounding rule, because a backend without the fused kernel (the oracle
twin of the tests) builds its scalar plaintexts from it."""
from __future__ import annotations

import ctypes as C
import math
import struct
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import capi


def weight_residue(value: float, scale: float, q: int) -> int:
    """round_half_away(value * scale) mod q, canonical: hefx_poly_weight_residue, the word hefx_ckks_encode_scalar writes.
    The product is float64; below 2^63 its rounded magnitude is an integer, from there up the float64 m * 2^e itself."""
    x = float(value) * float(scale)
    if not math.isfinite(x):
        return 0
    a = abs(x)
    t = math.trunc(a)  # exact for every float64
    if a - t >= 0.5:   # (a - t is exact too: C's round(), halves away from zero)
        t += 1
    if t >= 1 << 63:
        bits = struct.unpack("<Q", struct.pack("<d", float(t)))[0]
        e, m = (bits >> 52) - 1075, (bits & ((1 << 52) - 1)) | (1 << 52)
        r = (m % q) * pow(2, e, q) % q
    else:
        r = t % q
    return (q - r) % q if x < 0 else r


def weight_residues(values, scales, primes: Sequence[int]):
    """[len(values)][len(primes)] uint64: weight_residue of values[i] at scales[i]"""
    rows = [[weight_residue(v, s, q) for q in primes] for v, s in zip(values, scales)]
    return np.array(rows, dtype=np.uint64) if rows else np.zeros((0, len(primes)), dtype=np.uint64)


MUL, COMBINE, ADD = capi.POLY_MUL, capi.POLY_COMBINE, capi.POLY_ADD   # Step.op


class Term(NamedTuple):
    src: int
    coef: float
    wscale: float


class Step(NamedTuple):
    op: int              # MUL / COMBINE / ADD
    dst: int
    a: int               # MUL / ADD: operand slots (COMBINE: see terms)
    b: int
    level: int           # rows the step runs at
    terms: tuple         # COMBINE: its Terms
    constant: Optional[float]  # COMBINE: the constant, or None
    cscale: float        # COMBINE: S
    scale: float         # scale of dst


class Plan(NamedTuple):
    steps: List[Step]
    nslots: int

    @property
    def muls(self) -> int:
        return sum(1 for s in self.steps if s.op == MUL)

    def deferred(self) -> dict:
        """{index of a MUL step: index of the COMBINE it can be deferred into}: the MULs whose result is read exactly once,
        by a COMBINE, and is not the plan's result.  Relinearisation is linear, so such a product can stay at size 3 inside
        its consumer's sum (Evaluator.product_combine) and the sum be relinearised once."""
        readers: dict = {}
        for i, s in enumerate(self.steps):
            for src in ([t.src for t in s.terms] if s.op == COMBINE else [s.a, s.b]):
                readers.setdefault(src, []).append(i)
        final = self.steps[-1].dst
        out = {}
        for i, s in enumerate(self.steps):
            r = readers.get(s.dst, [])
            if s.op == MUL and s.dst != final and len(r) == 1 and self.steps[r[0]].op == COMBINE:
                out[i] = r[0]
        return out

    def relinearizations(self, lazy: bool = True) -> int:
        """key switches of one run of the plan: one per MUL when every product is relinearised on its own (lazy=False, what
        evaluate_polynomial does); with lazy=True one per MUL that cannot be deferred and one per COMBINE that takes
        deferred products (evaluate_polynomial_many)"""
        if not lazy:
            return self.muls
        d = self.deferred()
        return self.muls - len(d) + len(set(d.values()))

    @property
    def result_level(self) -> int:
        last = self.steps[-1]
        return last.level - 1 if last.op == COMBINE else last.level


def plan(coeffs: Sequence[float], basis: str, primes: Sequence[int], in_scale: float,
         target_scale: Optional[float] = None) -> Plan:
    """hefx_poly_plan for sum_i coeffs[i] x^i (basis "power") or sum_i coeffs[i] T_i(x) ("chebyshev") on an input of
    len(primes) rows at in_scale; target_scale None: in_scale.  ValueError: what the planner refuses."""
    if basis not in capi.POLY_BASIS:
        raise ValueError("basis must be 'power' or 'chebyshev'")
    c = [float(v) for v in coeffs]
    if not c:
        raise ValueError("coeffs cannot be empty")
    cs = (C.c_double * len(c))(*c)
    qs = (C.c_uint64 * len(primes))(*[int(p) for p in primes])
    ns, nt, nsl = C.c_int(0), C.c_int(0), C.c_int(0)
    args = (len(c) - 1, cs, capi.POLY_BASIS[basis], len(primes), qs, float(in_scale),
            float(target_scale) if target_scale is not None else 0.0)
    f = capi.lib().hefx_poly_plan
    rc = f(*args, None, 0, C.byref(ns), None, 0, C.byref(nt), C.byref(nsl))  # sizes the arrays, or says why not
    if ns.value == 0:
        capi.check(rc)
    steps, terms = (capi.PolyStep * ns.value)(), (capi.PolyTerm * max(nt.value, 1))()
    capi.check(f(*args, steps, ns.value, C.byref(ns), terms, nt.value, C.byref(nt), C.byref(nsl)))
    out = []
    for s in steps:
        tms = tuple(Term(t.src, t.coef, t.wscale) for t in terms[s.a:s.a + s.b]) if s.op == COMBINE else ()
        out.append(Step(s.op, s.dst, s.a, s.b, s.level, tms, s.constant if s.has_const else None, s.cscale, s.scale))
    return Plan(out, nsl.value)


def format_plan(p: Plan) -> str:
    """the text drivers/poly_plan_selftest.cpp prints for the same plan, line for line"""
    lines = ["slots %d steps %d" % (p.nslots, len(p.steps))]
    for s in p.steps:
        if s.op == MUL:
            lines.append("MUL %d = %d * %d level %d scale %.17g" % (s.dst, s.a, s.b, s.level, s.scale))
        elif s.op == ADD:
            lines.append("ADD %d = %d + %d level %d scale %.17g" % (s.dst, s.a, s.b, s.level, s.scale))
        else:
            t = " ".join("(%d %.17g %.17g)" % (t.src, t.coef, t.wscale) for t in s.terms)
            c = "const %.17g" % s.constant if s.constant is not None else "const none"
            lines.append("COMBINE %d level %d S %.17g scale %.17g %s terms %s" % (s.dst, s.level, s.cscale, s.scale, c, t))
    return "\n".join(lines) + "\n"
