"""The wide CKKS encode without a GPU: the C-ABI surface, the routing of seal.CKKSEncoder on both sides of 2^62 and of
2^(bc-3), the stand-in engines of the shim's host tests, and the rule of tests/encode_wide_cases.py tried on a float64
encoder written in numpy."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from seal_fyp_logistic_regression_amd import seal as S
from tests import encode_wide_cases as W
from tests import exact_ckks as X
from tests import policy_sets as ps
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hefx_ckks_encode_wide", "hefx_ckks_encode_wide_batch", "hefx_ckks_encode_scalar"]


def chain(N):
    """tests/test_gpu_frontend_edges.chain: a 60-bit row, a 40-bit row and a special prime"""
    p60 = ps.primes_below(1 << 60, N, 2)
    return [p60[0], ps.primes_below(1 << 40, N, 1)[0], p60[1]]


def test_abi_has_the_new_entries():
    from seal_fyp_logistic_regression_amd import capi
    header = open(os.path.join(ROOT, "include", "hefx.h")).read()
    for n in NEW:
        assert n in capi.EXPORTED_SYMBOLS
        assert re.search(r"\bint " + n + r"\(hefx_context \*ctx, int L,", header), n
    assert "2^max(62, min(bc - 3, 1000))" in header


class Recording(OracleBackend):
    """an oracle backend that offers the three encode entries, records which one the encoder chose and lets the host path
    produce the words (None: "not for this N")"""

    def __init__(self, N, primes):
        super().__init__(N, primes)
        self.calls = []

    def ckks_encode(self, L, values, scale):
        self.calls.append(("narrow", np.asarray(values).shape))
        return None

    def ckks_encode_wide(self, L, values, scale):
        self.calls.append(("wide", np.asarray(values).shape))
        return None

    def ckks_encode_scalar(self, L, value, scale):
        self.calls.append(("scalar", float(value)))
        c = S._c_round(float(value) * float(scale))
        return self.from_host(np.asarray([[c % q] * self.N for q in self.primes[:L]], dtype=np.uint64))


def test_encoder_routing_on_both_sides_of_the_two_bounds():
    N = 1024
    primes = chain(N)
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(primes)
    be = Recording(N, primes)
    ctx = S.SEALContext.Create(parms, backend=be)
    enc, host = S.CKKSEncoder(ctx), S.CKKSEncoder(ctx, device_encode=False)
    L = ctx.first_parms_id()
    bc = S.ContextData(ctx, L).total_coeff_modulus_bit_count()
    assert L == 2 and bc == W.bit_count(primes, L) == 100
    scale = 2.0 ** 50
    v = np.zeros(8)

    def route(top, encoder=enc):
        del be.calls[:]
        v[:] = 0.25
        v[3] = top / scale
        encoder.encode(v, scale)
        encoder.encode_many([v, -v], scale)
        assert len(be.calls) in (0, 4)   # encode; encode_many, then (the fake declines) once per vector
        return sorted({c[0] for c in be.calls})

    assert route(math.nextafter(2.0 ** 62, 0.0)) == ["narrow"]
    assert route(2.0 ** 62) == ["wide"]
    assert route(math.nextafter(2.0 ** (bc - 3), 0.0)) == ["wide"]
    assert route(2.0 ** (bc - 3)) == []                      # beyond the bound: today's host path
    assert route(2.0 ** 70, host) == []                      # device_encode=False
    for bad in (np.nan, np.inf):
        del be.calls[:]
        with pytest.raises((ValueError, OverflowError)):
            enc.encode(np.array([1.0, bad]), scale)
        assert be.calls == []
    # the words are the host path's whichever entry declined
    a, b = enc.encode(v, scale), host.encode(v, scale)
    assert (be.to_host(a.data) == be.to_host(b.data)).all()
    # scalars
    for value, s, want in ((0.3, 2.0 ** 40, True), (-0.3, 2.0 ** 80, True), (math.nextafter(2.0 ** (bc - 3), 0.0) / scale, scale, True),
                           (2.0 ** (bc - 3) / scale, scale, False)):
        del be.calls[:]
        a, b = enc.encode(value, s), host.encode(value, s)
        assert [c[0] for c in be.calls] == (["scalar"] if want else [])
        assert (be.to_host(a.data) == be.to_host(b.data)).all() and a.is_zero == b.is_zero
    with pytest.raises(ValueError, match="scale out of bounds"):
        enc.encode(1.0, 2.0 ** 100)


def test_stand_in_engines_export_what_the_shim_calls(tmp_path):
    """the stub (every prototype of hefx.h) and the symbolic engine (models, not fall-backs) know the new entries, and the
    shim with its new overloads compiles and links against them"""
    sym = open(os.path.join(ROOT, "drivers", "hefx_symbolic.cpp")).read()
    defined = set(re.findall(r"^(?:int|void|const char \*|uint32_t|uint64_t) ?(hefx_[a-z0-9_]+)\(", sym, flags=re.M))
    assert set(NEW) <= defined
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_stub_libhefx.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    stub = os.path.join(ROOT, "build", "stub")
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(stub, "libhefx.so")], text=True)
    assert set(NEW) <= set(re.findall(r" T (hefx_[a-z_0-9]+)", out))
    exe = str(tmp_path / "encode_wide_selftest")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "drivers", "encode_wide_selftest.cpp"), "-o", exe, "-L" + stub, "-lhefx"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_symbolic_libhefx.py")], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        fails = r.stdout[r.stdout.index("fail by name:"):]
        assert not any(n in fails.split() for n in NEW), fails
    finally:  # the stand-in library never outlives the test (it is named like the real one)
        shutil.rmtree(os.path.join(ROOT, "build", "symbolic"), ignore_errors=True)


@pytest.mark.parametrize("name", sorted(W.families(1024)))
def test_rule_accepts_a_numpy_float64_encoder(name):
    """the cases of the GPU test (b) at N = 1024: the rule is one a correct float64 encoder passes"""
    N = 1024
    primes = chain(N)
    v = W.families(N)[name]
    for L, scale in ((2, 2.0 ** 63), (2, 2.0 ** 68), (3, W.FULL_MANTISSA), (2, W.top_scale(primes, 2, v))):
        assert 2.0 ** 62 <= W.max_abs(v) * scale < 2.0 ** W.wide_bits(primes, L)
        x, band = X.exact_coefficients(N, v, scale), X.encode_band(N, v, scale)
        worst = W.check_wide(W.numpy_encode_rows(N, v, scale, primes, L), primes, x, band)
        print(f"{name} at 2^{math.log2(scale):.2f}: largest (|c - x| - 0.5) / band {worst:.3g}")


def test_rule_refuses_what_it_should():
    N = 1024
    primes = chain(N)
    v, scale, L = W.families(N)["uniform_real"], 2.0 ** 68, 2
    x, band = X.exact_coefficients(N, v, scale), X.encode_band(N, v, scale)
    rows = W.numpy_encode_rows(N, v, scale, primes, L)
    rows[1][5] = (rows[1][5] + 1) % primes[1]                 # one row holds another integer
    with pytest.raises(X.Mismatch):
        W.check_wide(rows, primes, x, band)
    rows = W.numpy_encode_rows(N, v, scale, primes, L)
    k = max(range(N), key=lambda i: abs(x[i]))
    c = W.compose(rows, primes, x)[k] + 1                     # the neighbour of a 2^67-sized float64 is no float64
    for j in range(L):
        rows[j][k] = c % primes[j]
    with pytest.raises(X.Mismatch, match="not a float64"):
        W.check_wide(rows, primes, x, band)
    c += int(2 * band) + 2 ** 20                              # outside the band (and a float64 again or not: refused first)
    for j in range(L):
        rows[j][k] = c % primes[j]
    with pytest.raises(X.Mismatch):
        W.check_wide(rows, primes, x, band)
