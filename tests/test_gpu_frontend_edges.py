"""The two ends every ciphertext passes through, on the GPU, at the shapes and primes where they could go wrong:
CKKS encode and decode (csrc/hefx_encode.hip) against the exact integer reference of tests/exact_ckks.py, the
counter-mode samplers, key generation, encrypt and decrypt (csrc/hefx_sample.hip) word for word against the CPU oracle
on the arithmetic-policy sets of tests/policy_sets.py -- and the key identities on the engine's own keys in Python
integers, so that they do not rest on the oracle alone.

Encode: for every coefficient an integer within 0.5 + band of the exact p_k * scale (exactly round-half-away at a tie),
the same integer in every RNS row; decode: every slot within the band.  The bands are derived in exact_ckks.py from
float64's unit roundoff; each test prints the largest observed error as a fraction of its band (pytest -s)."""
import math

import numpy as np
import pytest

from tests import exact_ckks as X
from tests import policy_sets as ps
from tests.test_exact_ckks_cpu import (SAMPLER_KEY, check_key_identities, decode_cases, redraw_stream, twin)

pytestmark = pytest.mark.gpu

SETS = ps.sets()
NS = (1024, 2048, 4096, 8192, 16384, 32768)   # FftCfg<9..13> (LM % 3 = 0, 1, 2, 0, 1) and the SPLIT kernel


def chain(N):
    """a 60-bit row (integer transform), a 40-bit row (FP64 transform) and a special prime: L = 2"""
    p60 = ps.primes_below(1 << 60, N, 2)
    return [p60[0], ps.primes_below(1 << 40, N, 1)[0], p60[1]]


class Ctx:
    def __init__(self, name):
        from oracle import oracle as O
        from seal_fyp_logistic_regression_amd import Engine
        if name in SETS:
            self.N, self.primes = SETS[name].N, SETS[name].primes
        else:
            self.N = int(name[5:])
            self.primes = chain(self.N)
        self.k = len(self.primes)
        self.o, self.e = O.Oracle(self.N, self.primes), Engine(self.N, self.primes)

    def coefficients(self, dev, count, L):
        """[count][L][N] NTT-form plaintexts on the device -> host coefficient rows"""
        self.e.ntt_inverse(dev, count, L, 0)
        return dev.download().reshape(count, L, self.N)

    def encode_one(self, L, v, scale):
        return self.coefficients(self.e.ckks_encode(L, np.asarray(v)[None], scale), 1, L)[0]


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


# ---------------------------------------------------------------------------------------------------------------------
# encode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_encode_unit_family_against_exact_reference(N, ctxs):
    c = ctxs(f"chain{N}")
    L, worst = 2, 0.0
    fam = X.unit_family(N)
    for name, v in fam.items():
        for scale in X.SCALES:
            x, band = X.exact_coefficients(N, v, scale), X.encode_band(N, v, scale)
            assert band < 0.25
            worst = max(worst, X.check_encode(c.encode_one(L, v, scale), c.primes, x, band))
    # several vectors in one call, and the batch form with separately allocated outputs: the words of the single calls
    names = [n for n, v in fam.items() if len(v) == N // 2 and not isinstance(v[0], complex)]
    scale = X.SCALES[1]
    single = np.stack([c.e.ckks_encode(L, np.asarray(fam[n])[None], scale).download()[0] for n in names])
    vals = np.asarray([fam[n] for n in names])
    assert (c.e.ckks_encode(L, vals, scale).download() == single).all()
    outs = c.e.ckks_encode_batch(L, vals, scale)
    assert all((o.download() == single[i]).all() for i, o in enumerate(outs))
    cv = np.asarray([fam["uniform_complex"], np.conj(fam["uniform_complex"])])
    both = c.coefficients(c.e.ckks_encode(L, cv, scale), 2, L)
    for i in range(2):
        X.check_encode(both[i], c.primes, X.exact_coefficients(N, cv[i], scale), X.encode_band(N, cv[i], scale))
    print(f"\nencode unit N={N}: band(uniform_complex, 2^40) {X.encode_band(N, fam['uniform_complex'], 2.0 ** 40):.3g}, "
          f"largest (|c - x| - 0.5) / band {worst:.3g}")


@pytest.mark.parametrize("N", NS)
def test_encode_rounds_ties_away_from_zero(N, ctxs):
    c = ctxs(f"chain{N}")
    for scale in X.SCALES:
        for name, v in X.tie_family(N, scale, ms=X.TIE_M if scale == 2.0 ** 40 else (2,)).items():
            x, band = X.exact_coefficients(N, v, scale), X.encode_band(N, v, scale)
            assert X.is_tie(x[0]) and not any(x[1:]) and band < 0.25
            X.check_encode(c.encode_one(2, v, scale), c.primes, x, band)


WIDE = [("small_p", 3), ("small_p", 2), ("p_min61", 8), ("mixed2048", 9), ("mixed16384", 9), ("f41_wide", 61),
        ("f41_wide", 62), ("seal_deep", 20)]


@pytest.mark.parametrize("name,L", WIDE)
def test_encode_wide_values_into_every_row_class(name, L, ctxs):
    """max|v| * scale just under 2^62: 60-bit magnitudes reduced into 12-bit, 40-bit and 61-bit rows"""
    c = ctxs(name)
    scale, worst = 2.0 ** 40, 0.0
    for vname, v in X.wide_family(c.N, scale).items():
        x, band = X.exact_coefficients(c.N, v, scale), X.encode_band(c.N, v, scale)
        worst = max(worst, X.check_encode(c.encode_one(L, v, scale), c.primes, x, band))
    print(f"\nencode wide {name} N={c.N} L={L}: band(wide_uniform) {X.encode_band(c.N, v, scale):.3g}, "
          f"largest (|c - x| - 0.5) / band {worst:.3g}")


def test_encode_guard_at_2_62(ctxs):
    """seal.CKKSEncoder sends max|v| * scale < 2^62 to the kernel and everything else through its exact host path: both
    sides of the boundary meet the rule.  hefx_ckks_encode itself refuses what it cannot hold."""
    from seal_fyp_logistic_regression_amd import seal as S
    N, scale = 4096, 2.0 ** 40
    primes = ps.primes_below(1 << 60, N, 3)
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(primes)
    ctx = S.SEALContext.Create(parms)
    enc, be = S.CKKSEncoder(ctx), ctx.backend
    edge = 2.0 ** 62 / scale
    below = math.nextafter(edge, 0.0)
    rng = np.random.default_rng(4)
    for top in (below, edge, -below, -edge):
        for v in (np.full(N // 2, top), np.concatenate([[top], rng.uniform(-1, 1, N // 2 - 1) * below])):
            pt = enc.encode(v, scale)
            rows = be.to_host(be.ntt_inverse(be.from_host(be.to_host(pt.data)), 1, 2, 0)).reshape(2, N)
            X.check_encode(rows, primes, X.exact_coefficients(N, v, scale), X.encode_band(N, v, scale))
    e = be.engine
    ok = np.full((1, 8), below)
    e.ckks_encode(2, ok, scale)
    for bad in (np.full((1, 8), edge), np.full((1, 8), -edge), np.array([[0.0, np.nan, 1.0]]), np.array([[np.inf, 0.0]]),
                np.array([[1.0, -np.inf]]), np.array([[complex(below, below)]]), np.array([[complex(0.0, np.nan)]]),
                np.array([[1.0], [edge]])):
        with pytest.raises(ValueError, match="out of range"):
            e.ckks_encode(2, bad, scale)
        with pytest.raises(ValueError, match="out of range"):
            e.ckks_encode_batch(2, bad, scale)
    # the bound is on the modulus of a complex value, not on its parts
    e.ckks_encode(2, np.array([[complex(below, below) * 0.7]]), scale)
    e.sync()


# ---------------------------------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------------------------------
def _decode_case(c, L, coeffs, scale):
    primes = c.primes[:L]
    z, band = X.exact_slots(c.N, coeffs, scale), X.decode_band(c.N, primes, coeffs, scale)
    big = max(math.hypot(X.to_float(a), X.to_float(b)) for a, b in z)
    assert band <= 1e-9 * big      # never looser than what tests/test_gpu_encode.py holds
    rows = np.stack([c.o.ntt_fwd(j, np.asarray([t % q for t in coeffs], dtype=np.uint64)) for j, q in enumerate(primes)])
    return rows, z, band


DECODE = ([("lsweep", L) for L in (1, 2, 5, 8, 15, 16)] + [("f41_wide", L) for L in (1, 2, 5, 8, 15, 16)]
          + [(n, L) for n in ("small_p", "p_min61", "mixed2048", "straddle60") for L in range(1, SETS[n].k + 1)]
          + [("seal_deep", L) for L in (1, 2, 16)])


@pytest.mark.parametrize("name,L", DECODE)
def test_decode_against_exact_reference(name, L, ctxs):
    c = ctxs(name)
    worst = 0.0
    cases = decode_cases(c.N, c.primes[:L], 100 * L + c.N)
    if name == "seal_deep":
        cases = cases[:2]
    for cname, coeffs in cases:
        rows, z, band = _decode_case(c, L, coeffs, 2.0 ** 30)
        dev = c.e.to_device(rows[None])
        got = c.e.ckks_decode(L, dev, 2.0 ** 30)[0]
        worst = max(worst, X.check_decode(got, z, band))
        real = c.e.ckks_decode(L, dev, 2.0 ** 30, complex_out=False)[0]     # h_im == NULL
        assert (real == got.real).all()
    both = c.e.ckks_decode(L, c.e.to_device(np.stack([rows, rows])), 2.0 ** 30, count=2)
    assert (both[0] == got).all() and (both[1] == got).all()
    print(f"\ndecode {name} N={c.N} L={L}: largest |got - z| / band {worst:.3g}")


def test_decode_refuses_17_rows_and_the_encoder_falls_back(ctxs):
    from seal_fyp_logistic_regression_amd import seal as S
    from seal_fyp_logistic_regression_amd.capi import HEFX_ERR_UNSUPPORTED, HefxError
    s = SETS["lsweep"]
    assert s.k == 17
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(s.N)
    parms.set_coeff_modulus(s.primes)
    ctx = S.SEALContext.Create(parms)
    c = ctxs("lsweep")
    cname, coeffs = decode_cases(s.N, s.primes, 17)[1]
    rows, z, band = _decode_case(c, 17, coeffs, 2.0 ** 30)
    dev = ctx.backend.from_host(rows)
    with pytest.raises(HefxError, match=f"hefx error {HEFX_ERR_UNSUPPORTED}"):
        ctx.backend.engine.ckks_decode(17, dev, 2.0 ** 30)
    pt = S.Plaintext()
    pt.data, pt._parms_id, pt._scale = dev, 17, 2.0 ** 30
    f = X.check_decode(S.CKKSEncoder(ctx).decode(pt), z, band)
    print(f"\ndecode lsweep L=17 (host path): |got - z| / band {f:.3g}")


# ---------------------------------------------------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------------------------------------------------
SAMPLER_SETS = ("straddle60", "mixed2048", "mixed16384", "small_p", "p_min61", "f41_wide")


@pytest.mark.parametrize("name", SAMPLER_SETS)
def test_samplers_bit_exact_where_words_are_redrawn(name, ctxs):
    c = ctxs(name)
    k = c.k
    redraw = any(q > 1 << 60 and q < 3 << 59 for q in c.primes)
    streams = [redraw_stream(name)[0]] + list(range(101, 109)) if redraw else [1, 2 ** 40 + 5]
    shapes = ((1, k, 0), (3, k - 1, 1), (3, 2, k - 2))
    for i, stream in enumerate(streams):
        for kind in ("uniform", "ternary", "noise") if i < 2 else ("uniform",):
            for npoly, nrows, mod_first in shapes if i < 2 else shapes[1:2]:
                got = c.e.sample(kind, SAMPLER_KEY, stream, npoly, nrows, mod_first).download()
                want = c.o.sample(kind, SAMPLER_KEY, stream, npoly, nrows, mod_first)
                assert (got == want).all(), (kind, stream, npoly, nrows, mod_first)


# ---------------------------------------------------------------------------------------------------------------------
# keys, encrypt, decrypt
# ---------------------------------------------------------------------------------------------------------------------
KEY_SETS = ("p_min", "p_min40", "p_min61", "straddle60", "small_p", "mixed2048", "i42", "c40_edge")


@pytest.mark.parametrize("name", KEY_SETS)
def test_keys_encrypt_decrypt_word_for_word_and_by_identity(name, ctxs):
    """seal.py twins on the set's own primes, HIP engine and oracle backend, same seeds: secret, public, relinearisation
    and three Galois keys (steps 1, -3 and the conjugation; hefx_galois_permute on the engine's side), two encryptions,
    a batch of five with one encryption of zero, decryptions of sizes 2 and 3 -- word for word; then the key identities
    and the fresh-noise bound on the ENGINE's words in Python integers."""
    from seal_fyp_logistic_regression_amd import seal as S
    ctxs("chain1024")  # leave the device to the twin's own engine
    out = {}
    for kind in ("hip", "oracle"):
        s = SETS[name]
        s, ctx, kg = twin(name, backend=S.GpuBackend(s.N, s.primes) if kind == "hip" else None, seed=23)
        be, L = ctx.backend, ctx.first_parms_id()
        sk, pk = kg.secret_key(), kg.public_key()
        rk, gk = kg.relin_keys(), kg.galois_keys(steps=[1, -3, 0])
        rng = np.random.default_rng(9)
        msgs = [np.stack([rng.integers(0, q, s.N, dtype=np.uint64) for q in s.primes[:L]]) for _ in range(4)]
        pts = []
        for m in msgs:
            pt = S.Plaintext()
            pt.data, pt._parms_id, pt._scale = be.from_host(m), L, 1.0
            pts.append(pt)
        enc, dec, ev = S.Encryptor(ctx, pk, 24), S.Decryptor(ctx, sk), S.Evaluator(ctx)
        ct1, ct2 = enc.encrypt(pts[0]), enc.encrypt(pts[1])
        prod = ev.multiply(ct1, ct2)
        key32 = S._key32(25)
        plains = [pts[0].data, pts[1].data, None, pts[2].data, pts[3].data]
        if kind == "hip":
            batch = [b.download() for b in be.engine.encrypt_batch(L, enc._pk_dev, plains, key32, 7)]
        else:
            batch = [be.encrypt(L, enc._pk_dev, p, key32, 7 + i) for i, p in enumerate(plains)]
        out[kind] = dict(sk=sk.host, pk=pk, rk=be.to_host(rk.key(0)), ct1=be.to_host(ct1.data), ct2=be.to_host(ct2.data),
                         prod=be.to_host(prod.data), d2=be.to_host(dec.decrypt(ct1).data),
                         d3=be.to_host(dec.decrypt(prod).data), batch=np.stack(batch),
                         **{f"gk{g}": be.to_host(key) for g, key in gk.keys.items()})
        if kind == "hip":
            g = out["hip"]
            from oracle import oracle as O
            o = O.Oracle(s.N, s.primes)
            shape = (s.k - 1, 2, s.k, s.N)
            check_key_identities(o, s, g["sk"], np.asarray(g["pk"]).reshape(2, s.k, s.N), g["rk"].reshape(shape),
                                 {gg: g[f"gk{gg}"].reshape(shape) for gg in gk.keys})
            # decrypt(encrypt(m)) - m on the engine's words, in Python integers
            diff = [np.asarray([int(t) for t in (X._obj(g["d2"].reshape(L, s.N)[j]) - X._obj(msgs[0][j])) % q], dtype=np.uint64)
                    for j, q in enumerate(s.primes[:L])]
            noise = X.crt_centred(s.primes[:L], [o.ntt_inv(j, diff[j]) for j in range(L)])
            assert math.prod(s.primes[:L]) > 4 * X.fresh_noise_bound(s.N)
            assert 19 < max(abs(t) for t in noise) <= X.fresh_noise_bound(s.N)
        del kg, enc, dec, ev, ctx, be, rk, gk, pts, ct1, ct2, prod
    assert set(out["hip"]) == set(out["oracle"]) and len(out["hip"]) == 12
    for key in out["hip"]:
        assert (np.asarray(out["hip"][key]).reshape(-1) == np.asarray(out["oracle"][key]).reshape(-1)).all(), key
