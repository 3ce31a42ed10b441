"""csrc/hefx_poly_plan.h -- the polynomial planner and the weight rounding rule -- without a GPU.

The plan is read through the library (poly.plan: hefx_poly_plan over ctypes) and
  * executed over exact rationals, as polynomials in x with Fraction coefficients and UNROUNDED weights (coef as the plan
    states it): the outcome is p(x), or sum c_k T_k(x), coefficient for coefficient.  The coefficients of these cases are
    small multiples of 1/8, so the float64 arithmetic the Chebyshev split does on them (2 c_k, r -= c_k) is exact;
  * held to its depth and scale rules for every degree 1 .. 63;
  * compared, line for line, with what drivers/poly_plan_selftest.cpp prints for the same inputs -- the program the C++
    executor's planner is, built with g++ under AddressSanitizer and UBSan as a stand-alone program (nothing loaded into
    Python is sanitised).
The residue rule (poly.weight_residue, hefx_poly_weight_residue) is held to Python-integer arithmetic."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import pytest

from seal_fyp_logistic_regression_amd import _build, capi, poly
from seal_fyp_logistic_regression_amd import seal as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1024
PRIMES = S.CoeffModulus.Create(N, [60] + [40] * 7)   # 8 data primes: degree 63 takes six of the seven below the first
SCALE = 2.0 ** 40
DEGREES = (1, 2, 3, 4, 7, 8, 15, 16, 31, 63)
BASES = ("power", "chebyshev")


@pytest.fixture(scope="module", autouse=True)
def built():
    _build.build()


def coefficients(d, pattern):
    dense = [Fraction((i * 7 + 3) % 11 - 5, 8) or Fraction(3, 8) for i in range(d + 1)]
    if pattern == "dense":
        return dense
    if pattern == "odd":
        return [c if i % 2 else Fraction(0) for i, c in enumerate(dense)]
    if pattern == "ends":
        return [Fraction(1, 2) if i == 0 else Fraction(-5, 4) if i == d else Fraction(0) for i in range(d + 1)]
    assert pattern == "nocst"
    return [Fraction(0) if i == 0 else c for i, c in enumerate(dense)]


def pmul(a, b):
    out = [Fraction(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * y
    return out


def padd(a, b):
    n = max(len(a), len(b))
    return [(a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0) for i in range(n)]


def trim(a):
    a = list(a)
    while a and a[-1] == 0:
        a.pop()
    return a


def expected_polynomial(c, basis):
    if basis == "power":
        return trim(c)
    t0, t1, acc = [Fraction(1)], [Fraction(0), Fraction(1)], [c[0]]
    for ck in c[1:]:
        acc = padd(acc, [ck * v for v in t1])
        t0, t1 = t1, padd(pmul([Fraction(0), Fraction(2)], t1), [-v for v in t0])
    return trim(acc)


def execute_exact(p):
    slots = {0: [Fraction(0), Fraction(1)]}
    for s in p.steps:
        assert s.dst not in slots, "every slot is written once"
        if s.op == capi.POLY_MUL:
            slots[s.dst] = pmul(slots[s.a], slots[s.b])
        elif s.op == capi.POLY_ADD:
            slots[s.dst] = padd(slots[s.a], slots[s.b])
        else:
            acc = [Fraction(s.constant)] if s.constant is not None else [Fraction(0)]
            for t in s.terms:
                acc = padd(acc, [Fraction(t.coef) * v for v in slots[t.src]])
            slots[s.dst] = acc
    return trim(slots[p.steps[-1].dst])


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("pattern", ["dense", "odd", "ends", "nocst"])
@pytest.mark.parametrize("d", DEGREES)
def test_plan_is_the_polynomial_exactly(d, pattern, basis):
    c = coefficients(d, pattern)
    p = poly.plan([float(v) for v in c], basis, PRIMES, SCALE)
    assert execute_exact(p) == expected_polynomial(c, basis)
    # no transparent ciphertext: a zero coefficient is no term, and no weight rounds to zero
    for s in p.steps:
        for t in s.terms:
            assert t.coef != 0 and poly.weight_residue(t.coef, t.wscale, PRIMES[0]) != 0


def walk(p, primes, in_scale):
    """levels and scales of every slot as the steps define them, with the rules of include/hefx_poly.h asserted"""
    tol = 2.0 ** -48   # float64 rounding of a handful of products and quotients of scales
    level, scale = {0: len(primes)}, {0: in_scale}
    for s in p.steps:
        if s.op == capi.POLY_MUL:
            assert s.level == min(level[s.a], level[s.b]) and s.scale == scale[s.a] * scale[s.b]
            level[s.dst], scale[s.dst] = s.level, s.scale
        elif s.op == capi.POLY_ADD:
            assert level[s.a] == level[s.b] == s.level
            assert abs(scale[s.a] - scale[s.b]) <= tol * scale[s.a]
            level[s.dst], scale[s.dst] = s.level, s.scale
        else:
            assert 2 <= s.level <= len(primes) and 1 <= len(s.terms) <= capi.COMBINE_MAX_IN
            for t in s.terms:
                assert level[t.src] >= s.level
                assert abs(scale[t.src] * t.wscale - s.cscale) <= tol * s.cscale, (s, t)
            assert s.scale == s.cscale / float(primes[s.level - 1])
            level[s.dst], scale[s.dst] = s.level - 1, s.scale
    return level, scale


@pytest.mark.parametrize("basis", BASES)
def test_depth_and_scales_for_every_degree(basis):
    for d in range(1, 64):
        for pattern in ("dense", "ends"):
            c = [float(v) for v in coefficients(d, pattern)]
            for target in (None, 2.0 ** 38):
                p = poly.plan(c, basis, PRIMES, SCALE, target)
                level, scale = walk(p, PRIMES, SCALE)
                res = p.steps[-1].dst
                depth = math.ceil(math.log2(d + 1))
                assert len(PRIMES) - level[res] == depth == len(PRIMES) - p.result_level, (d, pattern)
                want = target or SCALE
                assert abs(scale[res] - want) <= 2.0 ** -48 * want


def test_the_planner_takes_fewer_products_where_the_degree_leaves_room():
    """degree 8 fits four baby steps in its four levels (x^2, x^3, x^4, x^8 and one product); degree 7 does not"""
    assert poly.plan([1.0] * 9, "power", PRIMES, SCALE).muls == 5
    assert poly.plan([1.0] * 8, "power", PRIMES, SCALE).muls == 5
    assert poly.plan([0.5, 0, 0, 0, 0, 0, 0, 2.0], "power", PRIMES, SCALE).muls == 4


def test_refusals():
    with pytest.raises(ValueError, match="not enough levels"):
        poly.plan([0.5, 1.0, 0.0, -1.0], "power", PRIMES[:2], SCALE)
    poly.plan([0.5, 1.0, 0.0, -1.0], "power", PRIMES[:3], SCALE)
    with pytest.raises(ValueError, match="constant polynomial"):
        poly.plan([0.5, 0.0, 0.0], "power", PRIMES, SCALE)
    with pytest.raises(ValueError, match="basis"):
        poly.plan([0.5, 1.0], "legendre", PRIMES, SCALE)
    with pytest.raises(ValueError, match="scale out of bounds"):
        poly.plan([0.5, 1.0], "power", PRIMES, 0.0)


def test_the_library_carries_the_new_surface(tmp_path):
    """built from the new source and headers, exported, bound, and the header is plain C like hefx.h"""
    import re
    assert "hefx_poly.hip" in _build.SOURCES and "hefx_poly_plan.h" in _build.HEADERS and "../../include/hefx_poly.h" in _build.HEADERS
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.library_path()], text=True)
    exported = set(re.findall(r" T (hefx_[a-z_0-9]+)", out))
    assert set(capi.POLY_SYMBOLS) <= exported
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hefx_poly.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(hefx_[a-z_0-9]+)\s*\(", src))) == capi.POLY_SYMBOLS
    assert not set(capi.POLY_SYMBOLS) & set(capi.EXPORTED_SYMBOLS)   # hefx.h's table stays as it is
    c = tmp_path / "t.c"
    c.write_text('#include "hefx_poly.h"\nint main(void) { return (int)sizeof(hefx_poly_step) + (int)hefx_poly_weight_residue(0.5, 1.0, 97); }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert C_sizes() == (48, 24)


def C_sizes():
    import ctypes
    return ctypes.sizeof(capi.PolyStep), ctypes.sizeof(capi.PolyTerm)


# ---- the C++ planner as a stand-alone program --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build drivers/poly_plan_selftest.cpp"
    exe = str(tmp_path_factory.mktemp("poly_plan") / "poly_plan_selftest")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "drivers", "poly_plan_selftest.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        return r.stdout
    return run


def test_selftest_under_asan_and_ubsan(selftest):
    out = selftest()
    assert "POLY PLAN SELFTEST PASSED" in out and "FAIL" not in out, out[-3000:]


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("d", [1, 3, 7, 8, 15, 31, 63])
def test_python_reads_the_plan_the_cpp_planner_prints(selftest, d, basis):
    import numpy as np
    from seal_fyp_logistic_regression_amd.algorithms import SIGMOID_COEFFS
    cases = [([float(v) for v in coefficients(d, "dense")], SCALE, None), ([float(v) for v in coefficients(d, "ends")], 2.0 ** 41.5, 2.0 ** 39)]
    if d in SIGMOID_COEFFS:
        c = SIGMOID_COEFFS[d]
        cases.append(([float(v) for v in (np.polynomial.chebyshev.poly2cheb(c) if basis == "chebyshev" else c)], SCALE, None))
    for c, s0, target in cases:
        nprimes = math.ceil(math.log2(d + 1)) + 1
        args = [basis, str(d), float(s0).hex(), float(target or 0.0).hex(), str(nprimes)]
        args += [str(q) for q in PRIMES[:nprimes]] + [float(v).hex() for v in c]
        assert selftest(*args) == poly.format_plan(poly.plan(c, basis, PRIMES[:nprimes], s0, target))


# ---- the weight rounding rule -------------------------------------------------------------------------------------------
def c_round(x):
    """round half away from zero of a float64, in Python integers"""
    f = Fraction(x)
    n = abs(f)
    r = int(n) + (1 if n - int(n) >= Fraction(1, 2) else 0)
    return -r if f < 0 else r


def residue_cases():
    vals = [(0.5, 1.0), (-0.5, 1.0), (1.5, 1.0), (2.5, 1.0), (-2.5, 1.0), (0.49999999999999994, 1.0), (-0.49999999999999994, 1.0),
            (0.0, SCALE), (-1.20069, SCALE), (1e-5, SCALE), (-0.81562, 2.0 ** 80), (1.0, 2.0 ** 80), (-1.0, 2.0 ** 80), (2.0, 2.0 ** 80),
            (1099511627775.5, 1.0), (-4.19407, 2.0 ** 79.3)]
    for bound in (2.0 ** 62, 2.0 ** 63):   # products just below and above 2^62 and 2^63
        vals += [(math.nextafter(1.0, 0.0), bound), (1.0, bound), (math.nextafter(1.0, 2.0), bound), (-math.nextafter(1.0, 0.0), bound),
                 (-math.nextafter(1.0, 2.0), bound)]
    return vals


def test_weight_residue_is_python_integer_arithmetic():
    from tests import policy_sets
    primes = set(PRIMES)
    for name in ("p_min61", "small_p", "mixed2048"):   # the 61-bit and the tiny primes among them
        primes.update(policy_sets.sets()[name].primes)
    assert any(q >> 60 for q in primes) and any(q < 1 << 20 for q in primes)
    f = capi.lib().hefx_poly_weight_residue
    for value, scale in residue_cases():
        integer = c_round(value * scale)   # (the product is the float64 one, as the engine forms it)
        for q in sorted(primes):
            want = integer % q
            assert poly.weight_residue(value, scale, q) == want, (value, scale, q)
            assert f(value, scale, q) == want, (value, scale, q)
