"""The exact CKKS reference (tests/exact_ckks.py) and what it says about the host side: the transform against its
definition and against mpmath, the checkers against planted faults, the conditions the test inputs must meet, the CPU
oracle's and seal.CKKSEncoder's host encode / decode under the exact rule, the uniform sampler's redraw rule restated in
Python, and the key / encryption identities on the oracle twin's keys.  No GPU.

Observed errors are printed as a fraction of the derived band (pytest -s shows them); they are never used to set it."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from seal_fyp_logistic_regression_amd import seal as S
from seal_fyp_logistic_regression_amd.galois_tables import gather_table
from tests import exact_ckks as X
from tests import policy_sets as ps
from tests.oracle_backend import OracleBackend

GPU_NS = (1024, 2048, 4096, 8192, 16384, 32768)


def _rows_of(ints, primes):
    return np.asarray([[c % q for c in ints] for q in primes], dtype=np.uint64)


def _chain(N):
    """three 60-bit primes: room for every scale of the families at L = 2"""
    return ps.primes_below(1 << 60, N, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 64])
def test_transform_equals_the_definition(N):
    rng = np.random.default_rng(N)
    v = rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2)
    for vals, scale in ((v, 2.0 ** 30), (v[:3], 3.7e9), (v.real, 2.0 ** 40), (v[: N // 2 - 1], 1.0)):
        for sparse in (0, 16):  # through the transform, and term by term where the input is short
            X._CACHE.clear()
            old, X.SPARSE = X.SPARSE, sparse
            try:
                got = X.exact_coefficients(N, vals, scale)
            finally:
                X.SPARSE = old
            assert got == X.naive_coefficients(N, vals, scale)
    c = [int(x) for x in rng.integers(-10 ** 15, 10 ** 15, N)]
    for scale in (2.0 ** 20, 3.0, 1e-3):
        assert X.exact_slots(N, c, scale) == X.naive_slots(N, c, scale)
    # and the two maps invert each other: slots of the (unrounded) coefficients are the values
    x = X.exact_coefficients(N, v, 2.0 ** 30)
    P = 400
    Z, (r1, _) = X.roots(N, P), X.slot_roots(N)
    for i in (0, 1, N // 2 - 1):
        g = 2 * r1[i] + 1
        re = sum(xk * Z[(g * k) % (2 * N)][0] for k, xk in enumerate(x)) >> P
        im = sum(xk * Z[(g * k) % (2 * N)][1] for k, xk in enumerate(x)) >> P
        assert abs(re - X.to_fixed(v[i].real * 2.0 ** 30)) < 1 << 40 and abs(im - X.to_fixed(v[i].imag * 2.0 ** 30)) < 1 << 40


def test_transform_equals_mpmath_at_1024():
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 400
    N = 1024
    tol = mp.mpf(2) ** -120
    Z = X.roots(N, 320)
    for j in list(range(0, 2 * N, 37)) + [1, N - 1, N + 1, 2 * N - 1]:
        w = mp.expjpi(mp.mpf(j) / N)
        assert abs(mp.mpf(Z[j][0]) / mp.mpf(2) ** 320 - w.real) < tol and abs(mp.mpf(Z[j][1]) / mp.mpf(2) ** 320 - w.imag) < tol
    rng = np.random.default_rng(7)
    v = rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2)
    scale = 2.0 ** 40
    x = X.exact_coefficients(N, v, scale)
    r1, r2 = X.slot_roots(N)
    A = [mp.mpc(0)] * N
    for i, z in enumerate(v):
        A[r1[i]] = mp.mpc(float(z.real), float(z.imag))
        A[r2[i]] = mp.mpc(float(z.real), -float(z.imag))
    for k in (0, 1, 2, 511, 512, 1023):
        want = sum(a * mp.expjpi(-mp.mpf((2 * r + 1) * k % (2 * N)) / N) for r, a in enumerate(A)).real / N * scale
        assert abs(mp.mpf(x[k]) / mp.mpf(2) ** X.F - want) < tol, k
    c = [int(t) for t in rng.integers(-10 ** 17, 10 ** 17, N)]
    z = X.exact_slots(N, c, 2.0 ** 30)
    for i in (0, 1, 300, 511):
        g = pow(3, i, 2 * N)
        want = sum(ck * mp.expjpi(mp.mpf(g * k % (2 * N)) / N) for k, ck in enumerate(c)) / mp.mpf(2) ** 30
        assert abs(mp.mpf(z[i][0]) / mp.mpf(2) ** X.F - want.real) < tol and abs(mp.mpf(z[i][1]) / mp.mpf(2) ** X.F - want.imag) < tol


def test_rounding_and_ties():
    one = X.ONE
    for num, den, want, tie in ((5, 2, 3, True), (-5, 2, -3, True), (13, 2, 7, True), (1, 2, 1, True), (-1, 2, -1, True),
                                (3, 1, 3, False), (9, 4, 2, False), (-11, 4, -3, False), (0, 1, 0, False)):
        x = num * one // den
        assert X.round_half_away(x) == want and X.is_tie(x) == tie
    assert X.round_half_away(one // 2 - 1) == 0 and not X.is_tie(one // 2 - 1)


def test_references_are_cached():
    X._CACHE.clear()
    v = X.unit_family(1024)["uniform_complex"]
    n0 = X.STATS["transforms"]
    a = X.exact_coefficients(1024, v, 2.0 ** 20)
    b = X.exact_coefficients(1024, list(v), 2.0 ** 40)   # another scale: the same transform, rescaled exactly
    assert X.STATS["transforms"] == n0 + 1 and all(abs((t << 20) - w) <= 1 << 20 for t, w in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# the checkers catch what they are for
# ---------------------------------------------------------------------------------------------------------------------
def _fft32(a):
    """radix-2 FFT in complex64 (numpy's own transform always works in double)"""
    a = np.asarray(a, dtype=np.complex64)
    n = a.size
    if n == 1:
        return a
    e, o = _fft32(a[0::2]), _fft32(a[1::2])
    w = np.exp(-2j * np.pi * np.arange(n // 2) / n).astype(np.complex64)
    return np.concatenate([e + w * o, e - w * o]).astype(np.complex64)


def test_a_wrong_coefficient_row_fft_tie_or_sign_is_caught():
    N, scale = 1024, 2.0 ** 30
    primes = _chain(N)[:2]
    v = np.asarray(X.unit_family(N)["uniform_complex"])
    x, band = X.exact_coefficients(N, v, scale), X.encode_band(N, v, scale)
    good = [X.round_half_away(t) for t in x]
    assert X.check_encode(_rows_of(good, primes), primes, x, band) == 0.0
    # one coefficient off by one where x_k lies within 0.25 of an integer
    k = next(i for i, t in enumerate(x) if abs(t - (X.round_half_away(t) << X.F)) < X.ONE // 4)
    for d in (1, -1):
        bad = list(good)
        bad[k] += d
        with pytest.raises(X.Mismatch, match=f"coefficient {k}"):
            X.check_encode(_rows_of(bad, primes), primes, x, band)
    # one row disagrees with the other
    rows = _rows_of(good, primes)
    rows[1, 77] = (int(rows[1, 77]) + 1) % primes[1]
    with pytest.raises(X.Mismatch, match="coefficient 77"):
        X.check_encode(rows, primes, x, band)
    # a word that is not reduced
    rows = _rows_of(good, primes)
    rows[0, 5] += np.uint64(primes[0])
    with pytest.raises(X.Mismatch, match="not reduced"):
        X.check_encode(rows, primes, x, band)
    # the same encoding through a float32 FFT
    r1, r2 = X.slot_roots(N)
    A = np.zeros(N, dtype=np.complex128)
    A[r1], A[r2] = v, np.conj(v)
    zeta = np.exp(1j * np.pi * np.arange(N) / N)
    c32 = np.round(np.real(_fft32(A).astype(np.complex128) / N * np.conj(zeta)) * scale)
    c64 = np.round(np.real(np.fft.fft(A) / N * np.conj(zeta)) * scale)
    X.check_encode(_rows_of([int(t) for t in c64], primes), primes, x, band)
    with pytest.raises(X.Mismatch):
        X.check_encode(_rows_of([int(t) for t in c32], primes), primes, x, band)
    # a tie rounded to even
    tv = X.tie_family(N, scale, ms=(2,))["tie_2"]
    tx, tband = X.exact_coefficients(N, tv, scale), X.encode_band(N, tv, scale)
    assert X.is_tie(tx[0]) and X.round_half_away(tx[0]) == 3
    X.check_encode(_rows_of([3] + [0] * (N - 1), primes), primes, tx, tband)
    with pytest.raises(X.Mismatch, match="tie"):
        X.check_encode(_rows_of([2] + [0] * (N - 1), primes), primes, tx, tband)
    # decode: the sign of one centred coefficient flipped
    z, dband = X.exact_slots(N, good, scale), X.decode_band(N, primes, good, scale)
    as_float = lambda zz: np.asarray([complex(X.to_float(a), X.to_float(b)) for a, b in zz])
    assert X.check_decode(as_float(z), z, dband) < 0.1
    k = max(range(N), key=lambda i: abs(good[i]))
    flipped = list(good)
    flipped[k] = -flipped[k]
    with pytest.raises(X.Mismatch, match="slot"):
        X.check_decode(as_float(X.exact_slots(N, flipped, scale)), z, dband)
    with pytest.raises(X.Mismatch):   # and a decode done in float32
        X.check_decode(as_float(z).astype(np.complex64), z, dband)


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the inputs, from the reference alone
# ---------------------------------------------------------------------------------------------------------------------
def test_unit_inputs_leave_no_room_for_an_off_by_one():
    for N in GPU_NS:
        for name, v in X.unit_family(N).items():
            for scale in X.SCALES:
                assert X.encode_band(N, v, scale) < 0.25, (N, name, scale)


@pytest.mark.parametrize("N", [1024, 8192, 32768])
def test_tie_inputs_are_ties(N):
    for scale in X.SCALES:
        for name, v in X.tie_family(N, scale, ms=X.TIE_M if scale == 2.0 ** 40 else (2,)).items():
            x = X.exact_coefficients(N, v, scale)
            m = int(name.split("_")[1])
            assert X.is_tie(x[0]) and x[0] == (2 * m + 1) * X.HALF, (N, name, scale)
            assert not any(x[1:]), (N, name, scale)
            assert X.round_half_away(x[0]) == (m + 1 if m >= 0 else m)
            assert X.encode_band(N, v, scale) < 0.25


def test_wide_inputs_stay_below_2_62():
    for N, scale in ((2048, 2.0 ** 40), (4096, 2.0 ** 30)):
        for name, v in X.wide_family(N, scale).items():
            top = max(abs(complex(t)) for t in v) * scale
            assert 2.0 ** 61 < top < 2.0 ** 62, (name, top)


# ---------------------------------------------------------------------------------------------------------------------
# C's round() in the host encoder
# ---------------------------------------------------------------------------------------------------------------------
def test_c_round_for_every_double():
    cases = {2.5: 3, -2.5: -3, 6.5: 7, 3.5: 4, 0.5: 1, -0.5: -1, 0.49999999999999994: 0, -0.49999999999999994: 0,
             1.4999999999999998: 1, 2.0 ** 52 + 1: 2 ** 52 + 1, -(2.0 ** 52 + 1): -(2 ** 52 + 1), 2.0 ** 52 - 0.5: 2 ** 52,
             2.0 ** 53 + 2: 2 ** 53 + 2, 2.0 ** 62: 2 ** 62, 2.0 ** 80: 2 ** 80, 0.0: 0, -0.0: 0, 7.0: 7}
    arr = S._c_round(np.asarray(list(cases), dtype=np.float64))
    for (x, want), got in zip(cases.items(), arr):
        assert S._c_round(x) == want and isinstance(S._c_round(x), int), x
        assert got == float(want), x


# ---------------------------------------------------------------------------------------------------------------------
# the host encoders under the exact rule
# ---------------------------------------------------------------------------------------------------------------------
def _host(N):
    primes = _chain(N)
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(primes)
    ctx = S.SEALContext.Create(parms, backend=OracleBackend(N, primes))
    return ctx, S.CKKSEncoder(ctx, device_encode=False), ctx.backend.o, primes


def _coeff_rows(o, pt_rows):
    return np.stack([o.ntt_inv(j, pt_rows[j]) for j in range(pt_rows.shape[0])])


def _inputs(N, full):
    fam = [(n, v, s) for n, v in X.unit_family(N).items() for s in (X.SCALES if full else X.SCALES[2:])
           if full or n in ("onehot_last", "diag_eps", "uniform_complex")]
    fam += [(n, v, s) for s in X.SCALES for n, v in X.tie_family(N, s, ms=X.TIE_M if s == 2.0 ** 40 else (2,)).items()]
    if full:
        fam += [(n, v, 2.0 ** 40) for n, v in X.wide_family(N, 2.0 ** 40).items()]
    return fam


@pytest.mark.parametrize("N", [1024, 8192, 32768])
def test_oracle_and_host_encoder_meet_the_exact_rule(N):
    """Oracle.encode and seal.CKKSEncoder(device_encode=False).encode on the whole input family; the ties are the cases
    np.rint / Python's round() got wrong (2 where SEAL's std::round gives 3) before seal._c_round."""
    ctx, enc, o, primes = _host(N)
    L = 2
    worst = {"oracle": 0.0, "host": 0.0}
    for name, v, scale in _inputs(N, full=N < 32768):
        x, band = X.exact_coefficients(N, v, scale), X.encode_band(N, v, scale)
        fo = X.check_encode(_coeff_rows(o, o.encode(L, v, scale)), primes, x, band)
        fh = X.check_encode(_coeff_rows(o, enc.encode(np.asarray(v), scale).data), primes, x, band)
        worst["oracle"], worst["host"] = max(worst["oracle"], fo), max(worst["host"], fh)
        assert fo < 1 and fh < 1
    print(f"\nencode N={N}: largest (|c - x| - 0.5) / band: oracle {worst['oracle']:.3g}, host encoder {worst['host']:.3g}")


def test_scalar_encode_rounds_like_c():
    N = 1024
    ctx, enc, o, primes = _host(N)
    for scale in X.SCALES:
        for m in X.TIE_M + (0, 7):
            for v in ((m + 0.5) / scale, (m + 0.25) / scale, float(m)):
                x = X.exact_coefficients(N, [v] * (N // 2), scale)
                X.check_encode(_coeff_rows(o, enc.encode(v, scale).data), primes, x, 0.0)
    pt = enc.encode(2.5 / 2.0 ** 30, 2.0 ** 30)
    assert (pt.data == 3).all()     # every NTT word of the constant polynomial 3: SEAL's std::round(2.5)


def decode_cases(N, primes, seed):
    """(name, integer polynomial) over Q = prod(primes): the centring edges 0, 1, -1, floor(Q/2), floor(Q/2) + 1 (whose
    centred value is -floor(Q/2)), uniform in (-Q/2, Q/2], small values (noise alone), a message with noise-sized low
    bits, and X^0"""
    import random
    rng = random.Random(seed)
    Q = math.prod(primes)
    half = Q // 2
    edge = [0, 1, -1, half, -half]
    mbits = max(0, min(40, Q.bit_length() - 15))   # a message of up to 40 bits above 12 noise bits, inside Q/2
    return [("edges", [edge[i % 5] for i in range(N)]),
            ("uniform", [rng.randrange(-half, half + 1) for _ in range(N)]),
            ("noisy", [rng.randrange(-(1 << 12), 1 << 12) for _ in range(N)]),
            ("message_plus_noise", [rng.randrange(-(1 << mbits), 1 << mbits) * (1 << 12) + rng.randrange(-64, 64)
                                    for _ in range(N)]),
            ("one", [1] + [0] * (N - 1))]


@pytest.mark.parametrize("N", [1024, 8192])
def test_oracle_and_host_decoder_meet_the_exact_rule(N):
    ctx, enc, o, primes = _host(N)
    worst = {"oracle": 0.0, "host": 0.0}
    for L in (1, 2, 3):
        for name, c in decode_cases(N, primes[:L], N + L):
            for scale in (2.0 ** 30,) if name != "noisy" else (2.0 ** 30, 1.0):
                z, band = X.exact_slots(N, c, scale), X.decode_band(N, primes[:L], c, scale)
                big = max(math.hypot(X.to_float(a), X.to_float(b)) for a, b in z)
                assert band <= 1e-9 * big
                rows = np.stack([o.ntt_fwd(j, r) for j, r in enumerate(_rows_of(c, primes[:L]))])
                fo = X.check_decode(o.decode(rows, scale), z, band)
                pt = S.Plaintext()
                pt.data, pt._parms_id, pt._scale = rows.copy(), L, scale
                fh = X.check_decode(enc.decode(pt), z, band)
                worst["oracle"], worst["host"] = max(worst["oracle"], fo), max(worst["host"], fh)
    print(f"\ndecode N={N}: largest |got - z| / band: oracle {worst['oracle']:.3g}, host decoder {worst['host']:.3g}")


# ---------------------------------------------------------------------------------------------------------------------
# the uniform sampler's redraw rule
# ---------------------------------------------------------------------------------------------------------------------
SAMPLER_KEY = bytes(range(32))


def redraw_stream(name):
    """(stream, row): the first stream id at which the first row of this set with a prime just above 2^60 (1 word in 16
    rejected) shows, by the Python restatement alone, a word accepted at attempt 2 and a block whose words are accepted
    at different attempts"""
    s = ps.sets()[name]
    rows = [j for j, q in enumerate(s.primes) if q > 1 << 60 and q < (1 << 60) + (1 << 59)]
    assert rows, "the set has no prime just above 2^60"
    row = rows[0]
    for stream in range(1, 64):
        _, att = X.uniform_restated(O.chacha20_block, SAMPLER_KEY, stream, s.primes[row], row, s.N)
        blocks = [att[i:i + 8] for i in range(0, s.N, 8)]
        if max(att) >= 2 and any(len({a for a in b}) > 1 for b in blocks):
            return stream, row
    raise AssertionError("no stream id below 64 reaches attempt 2")


@pytest.mark.parametrize("name", ["straddle60", "mixed2048"])
def test_uniform_redraw_rule_restated(name):
    s = ps.sets()[name]
    stream, row = redraw_stream(name)
    o = O.Oracle(s.N, s.primes)
    got = o.sample("uniform", SAMPLER_KEY, stream, 1, s.k)
    redrawn = 0
    for j, q in enumerate(s.primes):
        vals, att = X.uniform_restated(O.chacha20_block, SAMPLER_KEY, stream, q, j, s.N)
        assert got[0, j].tolist() == vals, (name, j)
        redrawn += sum(a > 0 for a in att)
        if j == row:   # the condition, from the restatement alone
            assert max(att) >= 2 and any(len(set(att[i:i + 8])) > 1 for i in range(0, s.N, 8))
    print(f"\n{name}: stream {stream}, {redrawn} redrawn words over {s.k} rows")
    # a second polynomial continues the row numbering: row index p * nrows + j
    mf = max(0, row - 1)
    two = o.sample("uniform", SAMPLER_KEY, stream, 2, 2, mod_first=mf)
    vals, _ = X.uniform_restated(O.chacha20_block, SAMPLER_KEY, stream, s.primes[mf + 1], 3, s.N)
    assert two[1, 1].tolist() == vals


# ---------------------------------------------------------------------------------------------------------------------
# key and encryption identities on the oracle twin
# ---------------------------------------------------------------------------------------------------------------------
KEY_SETS = ("p_min", "p_min40", "p_min61", "straddle60", "small_p", "mixed2048")


def twin(name, backend=None, seed=11):
    s = ps.sets()[name]
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(s.N)
    parms.set_coeff_modulus(s.primes)
    ctx = S.SEALContext.Create(parms, backend=backend if backend is not None else OracleBackend(s.N, s.primes))
    return s, ctx, S.KeyGenerator(ctx, seed)


def check_key_identities(o, s, sk, pk, rk, gks):
    """sk [k][N], pk [2][k][N], rk [k-1][2][k][N], gks {elt: key}: all host arrays, NTT form"""
    primes = s.primes
    sko = [X._obj(sk[m]) for m in range(s.k)]
    X.public_key_error(o, primes, sk, pk)
    s2 = np.asarray([[int(t) for t in (sko[m] * sko[m]) % q] for m, q in enumerate(primes)], dtype=np.uint64)
    errs = X.kswitch_key_errors(o, primes, sk, s2, rk)
    assert any(int(abs(e).max()) > 0 for e in errs)
    for g, key in gks.items():
        X.kswitch_key_errors(o, primes, sk, sk[:, gather_table(s.N, g)], key)


@pytest.mark.parametrize("name", KEY_SETS)
def test_key_and_encryption_identities_on_the_oracle_twin(name):
    s, ctx, kg = twin(name)
    o, be = ctx.backend.o, ctx.backend
    sk, pk = kg.secret_key().host, kg.public_key()
    # the secret key is ternary, the same polynomial in every row
    cen = X.centred_coefficients(o, s.primes, sk)
    assert set(int(t) for t in cen[0]) <= {-1, 0, 1} and all((c == cen[0]).all() for c in cen)
    gk = kg.galois_keys(steps=[1, -3])
    rk = kg.relin_keys().key(0)
    check_key_identities(o, s, sk, pk, rk, {g: k for g, k in gk.keys.items()})
    for where in ((0, 0, s.k - 1, 5), (s.k - 2, 1, 0, 0)):      # and one wrong word in a key is seen
        bad = rk.copy()
        bad[where] = (int(bad[where]) + 1) % s.primes[where[2]]
        with pytest.raises(AssertionError):
            check_key_identities(o, s, sk, pk, bad, {})
    with pytest.raises(AssertionError):
        wrong = np.asarray(pk).copy()
        wrong[1, 0, 3] = (int(wrong[1, 0, 3]) + 1) % s.primes[0]
        X.public_key_error(o, s.primes, sk, wrong)
    # decrypt(encrypt(m)) - m, centred, within 19 (2N + 1): see exact_ckks.fresh_noise_bound
    L = ctx.first_parms_id()
    rng = np.random.default_rng(3)
    m = np.stack([rng.integers(0, q, s.N, dtype=np.uint64) for q in s.primes[:L]])
    pt = S.Plaintext()
    pt.data, pt._parms_id, pt._scale = m, L, 1.0
    ct = S.Encryptor(ctx, pk, 5).encrypt(pt)
    dec = S.Decryptor(ctx, kg.secret_key()).decrypt(ct)
    diff = np.stack([(dec.data[j].astype(object) - m[j].astype(object)) % q for j, q in enumerate(s.primes[:L])])
    coef = [o.ntt_inv(j, np.asarray([int(t) for t in diff[j]], dtype=np.uint64)) for j in range(L)]
    noise = X.crt_centred(s.primes[:L], coef)
    bound = X.fresh_noise_bound(s.N)
    Q = math.prod(s.primes[:L])
    assert Q > 4 * bound and max(abs(t) for t in noise) <= bound
    assert max(abs(t) for t in noise) > 19   # and it is the product noise, not just e0
