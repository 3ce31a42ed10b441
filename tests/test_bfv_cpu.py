"""The BFV entries without a GPU: the exact model of tests/bfv_cases.py against definitions that share nothing with it,
the crafted values against the remainders they are meant to hit, and the surface of include/hefx_bfv.h (plain C, bound,
exported, an aliasing rule in front of every entry that writes device memory, built into the library and into the
GPU-less stand-ins of the engine)."""
import os
import re
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from tests import bfv_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY_N = 16


# ---- the model against independent definitions
def _schoolbook(A, Bp, n):
    """sum_{i+j=k} A_i * B_j in Z[X]/(X^n + 1), coefficient by coefficient"""
    out = [[0] * n for _ in range(len(A) + len(Bp) - 1)]
    for i, a in enumerate(A):
        for j, b in enumerate(Bp):
            c = out[i + j]
            for x in range(n):
                for y in range(n):
                    if x + y < n:
                        c[x + y] += a[x] * b[y]
                    else:
                        c[x + y - n] -= a[x] * b[y]
    return out


def _round_fraction(z, t, Q):
    """t z / Q to the nearest integer; Q is odd, so the fraction never ends in one half"""
    f = Fraction(t * z, Q)
    assert f.denominator == 1 or (2 * f).denominator != 1
    return round(f)


def _toy_primes(L):
    from tests import policy_sets
    return policy_sets.primes_above(1 << 20, TOY_N, L) if L < 4 else (
        policy_sets.primes_above(1 << 20, TOY_N, 2) + policy_sets.primes_below(1 << 60, TOY_N, 2))


@pytest.mark.parametrize("sizes", B.SIZES + ((2, 5),))
@pytest.mark.parametrize("L,t", [(1, 2), (2, 1024), (3, 65537), (4, B.T_59)])
def test_multiply_model_equals_schoolbook_and_fraction_rounding(L, t, sizes):
    sa, sb = sizes
    primes = _toy_primes(L)
    Q = B.modulus(primes, L)
    kinds = [(B.uniform(primes, L, sa, TOY_N, 1), B.uniform(primes, L, sb, TOY_N, 2)),
             B.identity_operands(primes, L, t, sa, sb, TOY_N, seed=3),
             B.magnitude_operands(primes, L, sa, sb, TOY_N, 1, 1),
             B.magnitude_operands(primes, L, sa, sb, TOY_N, -1, 1)]
    for a, b in kinds:
        got = B.multiply_model(a, b, primes, L, t)
        A = [[B.centre(v, Q) for v in B.compose(p, primes, L)] for p in a]
        Bp = [[B.centre(v, Q) for v in B.compose(p, primes, L)] for p in b]
        for p in list(A) + list(Bp):
            assert all(-(Q // 2) <= v <= Q // 2 for v in p)
        c = _schoolbook(A, Bp, TOY_N)
        assert got.shape == (sa + sb - 1, L, TOY_N)
        for k in range(sa + sb - 1):
            r = [_round_fraction(z, t, Q) for z in c[k]]
            assert [B.R(z, t, Q) for z in c[k]] == r
            for j in range(L):
                assert [int(v) for v in got[k, j]] == [v % primes[j] for v in r]
    # a square through the same object is the product with itself
    a = kinds[0][0]
    assert np.array_equal(B.multiply_model(a, a, primes, L, t), B.multiply_model(a, a.copy(), primes, L, t))


@pytest.mark.parametrize("L,t", [(1, 2), (2, 1024), (3, 65537), (4, B.T_59)])
def test_decrypt_round_model_equals_fraction_rounding(L, t):
    primes = _toy_primes(L)
    Q = B.modulus(primes, L)
    x = B.crafted_poly(primes, L, t, TOY_N, seed=4)
    got = B.decrypt_round_model(x, primes, L, t)
    comp = B.compose(x, primes, L)
    for i, v in enumerate(comp):
        assert all(v % primes[j] == int(x[j][i]) for j in range(L))
        assert int(got[i]) == _round_fraction(B.centre(v, Q), t, Q) % t
        assert int(got[i]) == _round_fraction(v, t, Q) % t  # read uncentred it agrees modulo t


def test_the_identity_operands_put_the_crafted_polynomial_in_front_of_R():
    name = "bfv4096_bits"
    N, primes, L = B.prime_sets()[name]
    t = 65537
    Q = B.modulus(primes, L)
    a, b = B.identity_operands(primes, L, t, 3, 3, N, seed=1)
    got = B.multiply_model(a, b, primes, L, t)
    want = [B.R(z, t, Q) for z in B.centred(b[0], primes, L)]
    for j in range(L):
        assert [int(v) for v in got[0, j]] == [v % primes[j] for v in want]


@pytest.mark.parametrize("t", B.PLAIN_MODULI)
@pytest.mark.parametrize("name", sorted(B.prime_sets()))
def test_the_crafted_values_hit_the_remainders_next_to_one_half(name, t):
    N, primes, L = B.prime_sets()[name]
    Q = B.modulus(primes, L)
    assert Q % 2 == 1 and all(np.gcd(t, q) == 1 for q in primes[:L])
    lo, hi = B.boundary_values(primes, L, t)
    assert (t * lo) % Q == (Q - 1) // 2 and (t * hi) % Q == (Q + 1) // 2
    for x in (lo, hi):
        z = B.centre(x, Q)
        down, up = (t * z) // Q, (t * z) // Q + 1
        assert B.R(z, t, Q) == (down if x == lo else up)   # the first rounds down, the second up
        assert B.R(-z, t, Q) == -B.R(z, t, Q)
    sp = B.special_values(primes, L, t)
    assert {0, 1, -1, Q // 2, -(Q // 2), lo, hi, -lo, -hi} == set(sp)
    x = B.crafted_poly(primes, L, t, N, seed=1)
    comp = B.compose(x[:, :len(sp)], primes, L)
    assert comp == [v % Q for v in sp]
    # the magnitude operands reach the bound the working basis is sized from, with either sign
    a, b = B.magnitude_operands(primes, L, 3, 3, 16, 1, -1)
    c = B.negacyclic_sums([B.centred(p, primes, L) for p in a], [B.centred(p, primes, L) for p in b], 2 * Q.bit_length() + 8)
    assert min(c[2]) == -3 * 16 * (Q // 2) ** 2 and max(c[2]) == 3 * 14 * (Q // 2) ** 2


def test_the_prime_sets_are_what_the_docstring_says():
    from seal_fyp_logistic_regression_amd.seal import CoeffModulus
    S = B.prime_sets()
    assert [q.bit_length() for q in S["one60"][1]] == [60] and S["one60"][2] == 1
    assert [q.bit_length() for q in S["bfv4096_bits"][1]] == [q.bit_length() for q in CoeffModulus.BFVDefault(4096)]
    assert [q.bit_length() for q in S["bfv8192_bits"][1]] == [q.bit_length() for q in CoeffModulus.BFVDefault(8192)]
    m = S["mixed"][1]
    assert m[0] < 1 << 41 < m[1] and m[2] > 1 << 60
    for N, primes, L in S.values():
        assert N == 1024 and L == max(1, len(primes) - 1) and all(q % (2 * N) == 1 for q in primes)
    assert B.T_59.bit_length() == 59 and set(B.PLAIN_MODULI) >= {2, 1024, 65537, 1032193}


# ---- the surface of include/hefx_bfv.h
def _header():
    return open(os.path.join(ROOT, "include", "hefx_bfv.h")).read()


def _header_symbols():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(hefx_bfv_[a-z_0-9]+)\s*\(", src)))


def test_bfv_header_is_plain_c():
    src = ('#include "hefx_bfv.h"\nint main(void) { hefx_bfv *b = 0; int rc = hefx_bfv_create(0, 1, 2, &b);\n'
           'rc += hefx_bfv_multiply(b, 2, 0, 2, 0, 0, 0) + hefx_bfv_decrypt_round(b, 0, 0, 0) + hefx_bfv_aux_count(b);\n'
           'hefx_bfv_destroy(b); return rc == HEFX_OK; }\n')
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
        path = f.name
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), path], capture_output=True, text=True)
    os.unlink(path)
    assert r.returncode == 0, r.stderr


def test_bfv_symbols_are_exported_and_bound():
    from seal_fyp_logistic_regression_amd import _build, capi
    _build.build()
    syms = _header_symbols()
    assert {"hefx_bfv_create", "hefx_bfv_destroy", "hefx_bfv_multiply", "hefx_bfv_decrypt_round"} <= set(syms)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.library_path()], text=True)
    exported = set(re.findall(r" T (hefx_[a-z_0-9]+)", out))
    assert not [s for s in syms if s not in exported]
    assert sorted(capi.BFV_SYMBOLS) == syms
    assert not set(capi.BFV_SYMBOLS) & set(capi.EXPORTED_SYMBOLS)
    assert not set(capi.BFV_SYMBOLS) & set(capi.REFRESH_SYMBOLS)
    lib = capi.lib()
    for s in syms:
        assert getattr(lib, s).argtypes is not None
    assert int(re.search(r"#define HEFX_BFV_MAX_BASIS (\d+)", _header()).group(1)) == capi.BFV_MAX_BASIS
    assert int(re.search(r"#define HEFX_BFV_SIZE_MAX (\d+)", _header()).group(1)) == capi.BFV_SIZE_MAX
    assert "../../include/hefx_bfv.h" in _build.HEADERS and "hefx_crt.cuh" in _build.HEADERS
    assert "hefx_bfv.hip" in _build.SOURCES
    for d in _build.DEPS:
        assert os.path.exists(os.path.join(_build.CSRC, d)), d


def test_bfv_header_states_the_aliasing_rule_in_front_of_each_entry_that_writes():
    src = _header()
    for name in ("hefx_bfv_multiply", "hefx_bfv_decrypt_round"):
        at = src.index("int " + name + "(")
        comment = " ".join(src[src.rindex("/*", 0, at):at].replace("\n *", " ").split())
        assert "overlap" in comment and "HEFX_ERR_INVALID before anything is submitted" in comment, name
    top = " ".join(src[:src.index("#ifndef")].replace("\n *", " ").split())
    assert "ONE object on two streams at once" in top and "caller's error" in top
    assert "HEFX_ERR_UNSUPPORTED" in top


def test_no_division_or_floating_point_in_the_bfv_kernels():
    """device code of the rounding: no `/` or `%` operator and no floating type (comments aside)"""
    for name in ("hefx_bfv.hip", "hefx_crt.cuh"):
        src = open(os.path.join(ROOT, "seal_fyp_logistic_regression_amd", "csrc", name)).read()
        code = re.sub(r"//.*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
        code = re.sub(r'#include\s+"[^"]*"', "", code)
        assert not re.search(r"[/%]", code), name
        assert not re.search(r"\b(double|float)\b", code), name


def test_the_gpu_less_engines_build_with_the_new_prototypes():
    """include/seal/seal.h names the BFV entries: the symbolic engine of the shim fuzzer and the stub of the host probe
    define them (the symbolic one as loud HEFX_ERR_UNSUPPORTED fall-backs), or neither would link"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_symbolic_libhefx.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    gen = open(os.path.join(ROOT, "build", "symbolic", "fallbacks.cpp")).read()
    for s in _header_symbols():
        assert re.search(r"\b" + s + r"\(", gen), s
    assert "hefx_bfv_multiply: not modelled by the symbolic engine" in gen
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "build", "symbolic", "libhefx.so")], text=True)
    assert " T hefx_bfv_create" in out and " T hefx_bfv_multiply" in out
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_stub_libhefx.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_bfv_selftest_driver_compiles():
    """drivers/bfv_selftest.cpp against include/seal/seal.h, in both of its forms (syntax only: no library needed)"""
    for extra in ([], ["-DBFV_SELFTEST_PUBLIC_API_ONLY"]):
        r = subprocess.run(["g++", "-std=c++17", "-w", "-fsyntax-only", "-I", os.path.join(ROOT, "include")] + extra +
                           [os.path.join(ROOT, "drivers", "bfv_selftest.cpp")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    mk = open(os.path.join(ROOT, "drivers", "Makefile")).read()
    assert "$(OUT)/bfv_selftest:" in mk  # its rule ...
    assert "$(OUT)/bfv_selftest " in next(line for line in mk.splitlines() if line.startswith("all:"))  # ... and in `all`
    assert '"_ref/bfv_selftest"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()  # built where there is no reference tree
