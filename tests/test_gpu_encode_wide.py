"""hefx_ckks_encode_wide / hefx_ckks_encode_wide_batch / hefx_ckks_encode_scalar on the GPU: the same words as the narrow
entries where both accept the input, the rule of tests/encode_wide_cases.py against the exact reference above 2^62,
exact pins, refusals, the seal.py routing, asynchrony on a gated stream and the C++ shim's selftest.

chainN at L = 2 is a 60-bit and a 40-bit row: bc = 100, so the wide entry accepts |v| * scale < 2^97.  The full-mantissa
scale 0x1F3A5C7E9B2D4F * 2^60 (about 2^113) lies above that bound -- and above 2^bc, which SEAL refuses as "scale out
of bounds" -- so it is exercised at L = 3 (all three rows of the chain, bc = 160) and asserted to be refused at L = 2."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import encode_wide_cases as W
from tests import exact_ckks as X
from tests import policy_sets as ps
from tests.test_gpu_frontend_edges import Ctx, chain

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctxs():
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()  # one parameter set at a time on the device
            cache[name] = Ctx(name)
        return cache[name]

    yield get
    cache.clear()


def wide_one(c, L, v, scale):
    return c.coefficients(c.e.ckks_encode_wide(L, np.asarray(v)[None], scale), 1, L)[0]


# ---------------------------------------------------------------------------------------------------------------------
# a. wide == narrow where the narrow entry accepts the input
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1024, 2048, 4096, 32768))   # LM % 3 = 0, 1, 2 and the SPLIT kernel
def test_wide_entry_writes_the_narrow_words(N, ctxs):
    c, L, scale = ctxs(f"chain{N}"), 2, 2.0 ** 40
    fams = dict(X.unit_family(N))
    fams.update(X.wide_family(N, scale))
    for name, v in fams.items():
        a = np.asarray(v)[None]
        assert (c.e.ckks_encode_wide(L, a, scale).download() == c.e.ckks_encode(L, a, scale).download()).all(), name
    three = np.asarray([fams["uniform_real"], fams["wide_uniform"], fams["alternating"]])
    narrow = c.e.ckks_encode(L, three, scale).download()
    assert (c.e.ckks_encode_wide(L, three, scale).download() == narrow).all()
    for i, o in enumerate(c.e.ckks_encode_wide_batch(L, three, scale)):
        assert (o.download() == narrow[i]).all(), i
    cx = np.asarray([fams["uniform_complex"], fams["wide_complex"]])
    narrow = c.e.ckks_encode(L, cx, scale).download()
    assert (c.e.ckks_encode_wide(L, cx, scale).download() == narrow).all()
    for i, o in enumerate(c.e.ckks_encode_wide_batch(L, cx, scale)):
        assert (o.download() == narrow[i]).all(), i


# ---------------------------------------------------------------------------------------------------------------------
# b. wide against the exact reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1024, 2048, 4096))
def test_wide_against_exact_reference(N, ctxs):
    c, worst = ctxs(f"chain{N}"), 0.0
    fams = W.families(N)
    x68 = X.exact_coefficients(N, fams["uniform_real"], 2.0 ** 68)
    mags = [abs(t) >> X.F for t in x68]
    assert min(mags) < 2 ** 63 < max(mags), "2^68: one vector must put coefficients on both sides of 2^63"
    for name, v in fams.items():
        cases = [(2, 2.0 ** 63), (2, 2.0 ** 68), (3, W.FULL_MANTISSA), (2, W.top_scale(c.primes, 2, v))]
        for L, scale in cases:
            assert 2.0 ** 62 <= W.max_abs(v) * scale < 2.0 ** W.wide_bits(c.primes, L)
            x, band = X.exact_coefficients(N, v, scale), X.encode_band(N, v, scale)
            rows = wide_one(c, L, v, scale)
            worst = max(worst, W.check_wide(rows, c.primes, x, band))
    # the full-mantissa scale at L = 2 is beyond the bound of that level
    with pytest.raises(ValueError, match="out of range"):
        c.e.ckks_encode_wide(2, np.asarray(fams["ones"])[None], W.FULL_MANTISSA)
    # single, contiguous-count and batch forms: the same words
    for L, scale in ((2, 2.0 ** 68), (3, W.FULL_MANTISSA)):
        for names in (("ones", "neg_uniform_real", "alternating", "onehot_short"), ("uniform_complex", "neg_uniform_complex")):
            if len({len(fams[n]) for n in names}) > 1:
                names = [n for n in names if len(fams[n]) == N // 2]
            vals = np.asarray([fams[n] for n in names])
            single = np.stack([c.e.ckks_encode_wide(L, vals[i][None], scale).download()[0] for i in range(len(names))])
            assert (c.e.ckks_encode_wide(L, vals, scale).download() == single).all()
            for i, o in enumerate(c.e.ckks_encode_wide_batch(L, vals, scale)):
                assert (o.download() == single[i]).all(), (names[i], L)
    print(f"\nencode wide N={N}: largest (|c - x| - 0.5) / band {worst:.3g}")


def test_wide_at_32768(ctxs):
    N, L, scale = 32768, 2, 2.0 ** 80
    c = ctxs(f"chain{N}")
    v = X.unit_family(N)["uniform_complex"]
    w = W.check_wide(wide_one(c, L, v, scale), c.primes, X.exact_coefficients(N, v, scale), X.encode_band(N, v, scale))
    outs = c.e.ckks_encode_wide_batch(L, np.asarray(v)[None], scale)
    assert (outs[0].download() == c.e.ckks_encode_wide(L, np.asarray(v)[None], scale).download()[0]).all()
    print(f"\nencode wide N={N} 2^80: largest (|c - x| - 0.5) / band {w:.3g}")


@pytest.mark.parametrize("name,L,log_scale", [("p_min61", 8, 300), ("f41_wide", 61, 900)])
def test_wide_into_61_bit_and_fp64_policy_rows(name, L, log_scale, ctxs):
    """61-bit rows at L = 8; 41-bit FP64-policy rows at L = 61 with exponents near the cap of 1000"""
    c, scale = ctxs(name), 2.0 ** log_scale
    assert log_scale < W.wide_bits(c.primes, L) <= 1000
    v = X.unit_family(c.N)["uniform_complex"]
    w = W.check_wide(wide_one(c, L, v, scale), c.primes, X.exact_coefficients(c.N, v, scale), X.encode_band(c.N, v, scale))
    print(f"\nencode wide {name} L={L} 2^{log_scale}: largest (|c - x| - 0.5) / band {w:.3g}")


# ---------------------------------------------------------------------------------------------------------------------
# c. exact pins
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1024, 4096))
def test_constant_vectors_are_exact(N, ctxs):
    """all 1.0 over the N/2 slots: butterflies on equal values are exact and the twist at k = 0 is 1, so coefficient 0 is
    exactly int(scale) (and -int(scale) for all -1.0)"""
    c = ctxs(f"chain{N}")
    for L, scale in ((3, W.FULL_MANTISSA), (2, 2.0 ** 63), (2, 2.0 ** 64), (2, 2.0 ** 65)):
        for sign in (1.0, -1.0):
            rows = wide_one(c, L, [sign] * (N // 2), scale)
            got = X.crt_centred(c.primes[:L], [r[:1] for r in rows])[0]
            assert got == int(sign) * int(scale), (L, scale, sign)


def test_scalar_words(ctxs):
    from seal_fyp_logistic_regression_amd.seal import _c_round
    N = 2048
    c = ctxs(f"chain{N}")
    for L, scale, vals in ((2, 2.0 ** 40, [0.0, 1.0, -1.0, 0.3, -2.5e-13, 7.25, -4194303.99]),
                           (2, 2.0 ** 68, [0.0, 1.0, -1.0, 0.3, -0.7, 2.0 ** -10, -(2.0 ** 28) * 0.999]),
                           (3, W.FULL_MANTISSA, [1.0, -1.0, 0.123456789, -3e10, 2.0 ** -80])):
        many = c.e.ckks_encode_scalar(L, vals, scale).download().reshape(len(vals), L, N)
        for i, v in enumerate(vals):
            co = _c_round(float(v) * scale)
            one = c.e.ckks_encode_scalar(L, v, scale).download().reshape(L, N)
            for j in range(L):
                assert (many[i, j] == np.uint64(co % c.primes[j])).all(), (v, scale, j)
                assert (one[j] == many[i, j]).all()


# ---------------------------------------------------------------------------------------------------------------------
# d. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ctxs):
    N, L, scale = 1024, 2, 2.0 ** 68
    c = ctxs(f"chain{N}")
    e = c.e
    bits = W.wide_bits(c.primes, L)
    assert bits == W.bit_count(c.primes, L) - 3 == 97
    edge = 2.0 ** bits / scale
    below = math.nextafter(edge, 0.0)
    e.ckks_encode_wide(L, np.full((1, 8), below), scale)
    for bad in (np.full((1, 8), edge), np.full((1, 8), -edge), np.array([[0.0, np.nan, 1.0]]), np.array([[np.inf, 0.0]]),
                np.array([[1.0, -np.inf]]), np.array([[complex(below, below)]]), np.array([[complex(0.0, np.nan)]]),
                np.array([[1.0], [edge]])):
        with pytest.raises(ValueError, match="out of range"):
            e.ckks_encode_wide(L, bad, scale)
        with pytest.raises(ValueError, match="out of range"):
            e.ckks_encode_wide_batch(L, bad, scale)
    for bad in ([edge], [-edge], [1.0, np.nan], [np.inf], [-np.inf, 0.0]):
        with pytest.raises(ValueError, match="out of range"):
            e.ckks_encode_scalar(L, bad, scale)
    # a following valid call still works; the bound is on the modulus of a complex value, not on its parts
    v = np.array([[complex(below, below) * 0.7, 1.0]])
    W.check_wide(wide_one(c, L, v[0], scale), c.primes, X.exact_coefficients(N, v[0], scale), X.encode_band(N, v[0], scale))
    got = e.ckks_encode_scalar(L, [below], scale).download().reshape(L, N)
    assert int(got[0, 0]) == int(below * scale) % c.primes[0]


# ---------------------------------------------------------------------------------------------------------------------
# e. seal.py
# ---------------------------------------------------------------------------------------------------------------------
def _seal(N, primes):
    from seal_fyp_logistic_regression_amd import seal as S
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(primes)
    return S, S.SEALContext.Create(parms)


def _spy(be, name, calls):
    real = getattr(be, name)

    def wrapped(*a, **k):
        calls.append(name)
        return real(*a, **k)

    setattr(be, name, wrapped)


def test_seal_encoder_routes_to_the_wide_and_scalar_entries():
    N = 4096
    primes = ps.primes_below(1 << 60, N, 3) + ps.primes_below(1 << 50, N, 1)
    S, ctx = _seal(N, primes)
    be, L = ctx.backend, 3
    calls = []
    for n in ("ckks_encode", "ckks_encode_wide", "ckks_encode_scalar"):
        _spy(be, n, calls)
    enc, host = S.CKKSEncoder(ctx), S.CKKSEncoder(ctx, device_encode=False)
    coeff = lambda pt: be.to_host(be.ntt_inverse(be.from_host(be.to_host(pt.data)), 1, L, 0)).reshape(L, N)
    fam = X.unit_family(N)
    scale = 2.0 ** 80
    v = fam["uniform_complex"]
    pt = enc.encode(np.asarray(v), scale)
    assert calls == ["ckks_encode_wide"] and pt.scale == scale and not pt.is_zero
    W.check_wide(coeff(pt), primes, X.exact_coefficients(N, v, scale), X.encode_band(N, v, scale))
    del calls[:]
    vs = [fam["uniform_real"], fam["alternating"], fam["ones"]]
    pts = enc.encode_many([np.asarray(t) for t in vs], scale)
    assert calls == ["ckks_encode_wide"]
    for t, p in zip(vs, pts):
        W.check_wide(coeff(p), primes, X.exact_coefficients(N, t, scale), X.encode_band(N, t, scale))
    del calls[:]
    enc.encode(np.asarray(fam["ones"]), 2.0 ** 40)
    assert calls == ["ckks_encode"]
    del calls[:]
    for value, s in ((0.37, 2.0 ** 40), (-0.37, scale), (0.0, scale), (-1.5, W.FULL_MANTISSA)):
        a, b = enc.encode(value, s), host.encode(value, s)
        assert (be.to_host(a.data) == be.to_host(b.data)).all() and a.is_zero == b.is_zero and a.scale == b.scale
    assert calls == ["ckks_encode_scalar"] * 4


def test_add_plain_at_the_scale_of_an_unrescaled_product():
    N = 4096
    primes = ps.primes_below(1 << 60, N, 3) + ps.primes_below(1 << 50, N, 1)
    S, ctx = _seal(N, primes)
    enc, host = S.CKKSEncoder(ctx), S.CKKSEncoder(ctx, device_encode=False)
    keygen = S.KeyGenerator(ctx, seed=7)
    encryptor, decryptor, ev = S.Encryptor(ctx, keygen.public_key(), seed=8), S.Decryptor(ctx, keygen.secret_key()), S.Evaluator(ctx)
    rng = np.random.default_rng(5)
    x, y, z = (rng.uniform(-1, 1, N // 2) for _ in range(3))
    ct = ev.multiply_plain(encryptor.encrypt(enc.encode(x, 2.0 ** 40)), enc.encode(y, 2.0 ** 40))
    assert ct.scale == 2.0 ** 80
    calls = []
    _spy(ctx.backend, "ckks_encode_wide", calls)
    pd, ph = enc.encode(z, ct.scale, parms_id=ct.parms_id()), host.encode(z, ct.scale, parms_id=ct.parms_id())
    assert calls == ["ckks_encode_wide"]
    got = [enc.decode(decryptor.decrypt(ev.add_plain(ct, p))) for p in (pd, ph)]
    # the two plaintexts differ by at most twice the rule per coefficient; a slot is a sum of N coefficients times roots
    bound = N * 2 * (X.encode_band(N, z, ct.scale) + 0.5) / ct.scale
    diff = float(np.abs(got[0] - got[1]).max())
    print(f"\nadd_plain at 2^80: device vs host plaintext, largest slot difference {diff:.3g}, bound {bound:.3g}")
    assert diff <= bound
    assert float(np.abs(got[0].real - (x * y + z)).max()) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# f. the new entries do not wait for their stream
# ---------------------------------------------------------------------------------------------------------------------
def test_new_entries_return_while_their_stream_is_shut():
    from seal_fyp_logistic_regression_amd import Engine
    from tests.hip_stream_gate import Stream
    N, L, scale = 2048, 2, 2.0 ** 68
    primes = chain(N)
    e = Engine(N, primes)
    fam = X.unit_family(N)
    one, many = np.asarray(fam["uniform_real"])[None].copy(), np.asarray([fam["ones"], fam["alternating"], fam["uniform_real"]])
    sc = np.array([0.3, -1.0, 0.0])
    want = [e.ckks_encode_wide(L, one, scale).download(), e.ckks_encode_wide(L, many, scale).download(),
            e.ckks_encode_scalar(L, sc, scale).download()]   # warm-up: tables, staging, scratch
    [o.download() for o in e.ckks_encode_wide_batch(L, many, scale)]
    e.sync()
    with Stream() as S:
        gate = S.gate()
        a = e.ckks_encode_wide(L, one, scale, stream=S.handle)
        assert not gate.opened, "hefx_ckks_encode_wide waited for the stream"
        outs = e.ckks_encode_wide_batch(L, many, scale, stream=S.handle)
        assert not gate.opened, "hefx_ckks_encode_wide_batch waited for the stream"
        b = e.ckks_encode_scalar(L, sc, scale, stream=S.handle)
        assert not gate.opened, "hefx_ckks_encode_scalar waited for the stream"
        e.sync(S.handle)
        assert gate.opened
        assert (a.download() == want[0]).all() and (b.download() == want[2]).all()
        for i, o in enumerate(outs):
            assert (o.download() == want[1][i]).all()
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# g. the C++ shim
# ---------------------------------------------------------------------------------------------------------------------
def test_encode_wide_selftest_driver():
    """drivers/encode_wide_selftest.cpp through include/seal/seal.h: complex encode -> decode, real == complex overloads on
    real input, a wide encode recorded and live, and (second run, SEAL_SHIM_HOST_ENCODE=1) the host fallback above 2^128"""
    exe = os.path.join(ROOT, "drivers", "_ref", "encode_wide_selftest")
    if not os.path.exists(exe):  # our own source: build it where it is missing
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "drivers"), "_ref/encode_wide_selftest"], check=False)
    assert os.path.exists(exe), "drivers/_ref/encode_wide_selftest could not be built (make -C drivers _ref/encode_wide_selftest)"
    for extra in ({}, {"SEAL_SHIM_HOST_ENCODE": "1"}):
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env={**os.environ, **extra})
        assert r.returncode == 0 and "SELFTEST PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
        assert "FAIL" not in r.stdout
