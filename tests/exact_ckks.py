"""Exact CKKS encode / decode in Python integers, and the float64 error bands the encoders are held to (host only,
standard library only: no numpy, no mpmath).

Numbers
-------
A real number x is the Python integer round(x * 2^F), F = 192 fractional bits ("fixed point").  Complex numbers are
pairs.  Inside a transform the data and the roots of unity carry P >= F + 64 + log2(N) + (bits of the largest input)
fractional bits, so that the sum of all rounding errors of the integer arithmetic stays below 2^-(F+1) and a result is
the correctly rounded F-bit value of the exact one (checked against the O(N^2) definition and against mpmath in
tests/test_exact_ckks_cpu.py).  zeta = exp(2 pi i / 2N); the table zeta^j comes from cos(pi/2) = 0, sin(pi/2) = 1 by the
half-angle recurrences cos(t/2) = sqrt((1 + cos t)/2) (math.isqrt), sin(t/2) = sin t / (2 cos(t/2)) and one complex
product per entry and level -- no math.cos.

The maps
--------
encode: the real polynomial p of degree < N with p(zeta^(3^i)) = v_i and p(conj root) = conj(v_i), i < nvalues, zero at
the other slots.  With A_r = p(zeta^(2r+1)): p_k = (1/N) sum_{r<N} A_r zeta^(-(2r+1)k).  `exact_coefficients` returns
x_k = p_k * scale.  decode: z_i = p(zeta^(3^i)) / scale for an integer polynomial p (`exact_slots`).

The bands (derived here; nothing below was fitted to an encoder's output)
--------------------------------------------------------------------------
u = 2^-53, the unit roundoff of float64.

(a) Roots of unity.  A float64 encoder computes a root as (cos a^, sin a^) of a rounded angle a^ = fl(2 pi j / n).
    Forming a^ costs up to three roundings (the constant pi, one product, one quotient): |a^ - a| <= 3u|a| <= 3 pi u for
    |a| <= pi, which moves the root by the same amount; a libm evaluates cos and sin to less than one ulp (2u) per
    component, 2 sqrt(2) u on the complex value.  mu = (3 pi + 2 sqrt(2)) u < 13u.  We take mu = 13u.
(b) One FFT stage.  Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 24.2: for the radix-2
    Cooley-Tukey FFT of n = 2^t points with roots accurate to mu, ||y^ - y||_2 <= t eta / (1 - t eta) ||y||_2 with
    eta = mu + gamma_4 (sqrt(2) + mu), gamma_4 = 4u / (1 - 4u).  The proof bounds every butterfly stage (one complex
    product with a root, one complex sum) by the factor (1 + eta) in the 2-norm; decimation in frequency and higher radices
    are regroupings of the same butterflies.  A twist (an element-wise product with roots: zeta^(-k) after the encode
    transform, exp(-2 pi i r / N) in front of a half-size transform, zeta^k in front of the decode transform) is a stage
    without the sum, so it costs at most another (1 + eta).  An encoder runs at most log2(N) butterfly stages and two
    twists: T = log2(N) + 2, E = T eta / (1 - T eta).
(c) encode_band.  By Parseval ||FFT(A)||_2 = sqrt(N) ||A||_2 and ||A||_2^2 = 2 sum |v_i|^2, so every transformed value is
    off by at most E sqrt(N) ||A||_2, and after the factor scale / N every x_k by at most E B with
    B = scale ||A||_2 / sqrt(N) (an error in one coefficient is bounded by the 2-norm of the error vector).  |x_k| <= B as
    well (Parseval again: sum x_k^2 = B^2), and the factors 2/N (exact), scale and the final product cost at most three
    more roundings of x_k:  band = ((1 + E)(1 + u)^3 - 1) B.  The final rounding to an integer is exact.
(d) decode_band.  The centred integer c_k enters as a float64 built by Horner's rule over L mixed-radix digits (or over
    64-bit limbs, never more of them): per step the conversions of digit and radix, one product and one sum, 4 roundings,
    all terms of one sign, so a relative error below (1 + u)^(4L); the division by the scale (or the product with its
    rounded reciprocal) adds two more.  Then one twist and the transform, as in (b), on a vector of 2-norm
    ||c||_2 / scale whose transform has 2-norm sqrt(N) ||c||_2 / scale:
    band = ((1 + E)(1 + u)^(4L + 2) - 1) sqrt(N) ||c||_2 / scale, for every slot.
    The N/2 slots and their conjugates are all N values of the transform, so sqrt(N) ||c||_2 / scale = sqrt(2) ||z||_2
    <= sqrt(N) max|z_i|:  band <= sqrt(N) (E + (4L + 2) u) max|z_i|, which is 181 * 4.2e-14 < 1e-11 max|z_i| at N = 32768,
    L = 16 -- never looser than the 1e-9 max|v| the suite held before (the GPU tests assert this for every case).

The rule
--------
check_encode: for EVERY coefficient k there is an integer c with |c - x_k| <= 0.5 + band -- exactly round_half_away(x_k)
where x_k is a tie -- such that EVERY row j holds c mod q_j.  check_decode: |got_i - z_i| <= band for every slot.
Both return the largest observed error as a fraction of the band (reported by the tests, never used to set the band).
"""
from __future__ import annotations

import hashlib
import math
from fractions import Fraction

F = 192                 # fractional bits of every number this module hands out
ONE = 1 << F
HALF = 1 << (F - 1)
U = 2.0 ** -53
MU = 13 * U
ETA = MU + (4 * U / (1 - 4 * U)) * (math.sqrt(2.0) + MU)
SPARSE = 16             # at most this many nonzero values: summed term by term instead of transformed

STATS = {"transforms": 0, "hits": 0}   # how often a reference was computed / served from the cache
_ROOTS = {}
_CACHE = {}


# ---------------------------------------------------------------------------------------------------------------------
# fixed point
# ---------------------------------------------------------------------------------------------------------------------
def _shr(x: int, s: int) -> int:
    """x / 2^s rounded to nearest (s may be negative)"""
    if s <= 0:
        return x << -s
    return (x + (1 << (s - 1))) >> s


def to_fixed(v, bits: int = F) -> int:
    """a float (exactly, when its exponent allows) or an int as a fixed-point number of `bits` fractional bits"""
    if isinstance(v, int):
        return v << bits
    num, den = float(v).as_integer_ratio()
    return _shr(num << bits, den.bit_length() - 1)


def to_float(x: int, bits: int = F) -> float:
    return float(Fraction(x, 1 << bits))


def round_half_away(x: int) -> int:
    """the integer nearest to the fixed-point number x, halves away from zero (C's round())"""
    r = (abs(x) + HALF) >> F
    return -r if x < 0 else r


def is_tie(x: int) -> bool:
    """x is a half-integer (to the 2^-F this module resolves)"""
    return abs(x) & (ONE - 1) == HALF


# ---------------------------------------------------------------------------------------------------------------------
# roots of unity and the transform
# ---------------------------------------------------------------------------------------------------------------------
def roots(N: int, P: int):
    """[(re, im)] of zeta^j = exp(2 pi i j / 2N), j < 2N, with P fractional bits"""
    key = (N, P)
    if key in _ROOTS:
        return _ROOTS[key]
    W = P + 48                       # working precision: one unit lost per level, log2(2N) <= 16 levels
    one = 1 << W
    c, s = 0, one                    # the primitive 4th root: cos(pi/2), sin(pi/2)
    tab = [(one, 0), (0, one), (-one, 0), (0, -one)]
    while len(tab) < 2 * N:
        c2 = math.isqrt(((one + c) << W) >> 1)          # cos(t/2) = sqrt((1 + cos t) / 2)
        s2 = ((s << W) + c2) // (2 * c2)                # sin(t/2) = sin t / (2 cos(t/2))
        c, s = c2, s2
        new = [None] * (2 * len(tab))
        for j, (a, b) in enumerate(tab):
            new[2 * j] = (a, b)
            new[2 * j + 1] = (_shr(a * c - b * s, W), _shr(a * s + b * c, W))
        tab = new
    out = [(_shr(a, 48), _shr(b, 48)) for a, b in tab]
    if len(_ROOTS) >= 6:
        _ROOTS.clear()
    _ROOTS[key] = out
    return out


def _precision(N: int, magnitude_bits: int) -> int:
    need = F + 64 + N.bit_length() + max(0, magnitude_bits)
    return -(-need // 64) * 64


def _fft(re, im, N: int, P: int, sign: int):
    """in place: X_k = sum_r x_r exp(sign * 2 pi i r k / N); data and roots with P fractional bits"""
    Z = roots(N, P)
    logn = N.bit_length() - 1
    for i in range(N):
        j = int(format(i, "0%db" % logn)[::-1], 2) if logn else 0
        if i < j:
            re[i], re[j] = re[j], re[i]
            im[i], im[j] = im[j], im[i]
    half = 1 << (P - 1)
    length = 2
    while length <= N:
        h, step = length >> 1, 2 * (N // length)
        for j in range(h):
            if j == 0:
                for i in range(0, N, length):
                    a, b = re[i], im[i]
                    tr, ti = re[i + h], im[i + h]
                    re[i], im[i], re[i + h], im[i + h] = a + tr, b + ti, a - tr, b - ti
                continue
            wr, wi = Z[j * step]
            if sign < 0:
                wi = -wi
            for i in range(j, N, length):
                br, bi = re[i + h], im[i + h]
                tr = (br * wr - bi * wi + half) >> P
                ti = (br * wi + bi * wr + half) >> P
                a, b = re[i], im[i]
                re[i], im[i], re[i + h], im[i + h] = a + tr, b + ti, a - tr, b - ti
        length <<= 1
    STATS["transforms"] += 1


def slot_roots(N: int):
    """r1[i] = (3^i - 1) / 2 and r2[i] = (2N - 3^i - 1) / 2: slot i sits at zeta^(2 r1 + 1), its conjugate at zeta^(2 r2 + 1)"""
    r1, r2, p = [], [], 1
    for _ in range(N // 2):
        r1.append((p - 1) >> 1)
        r2.append((2 * N - p - 1) >> 1)
        p = p * 3 % (2 * N)
    return r1, r2


def _as_pairs(values):
    out = []
    for v in values:
        v = complex(v)
        out.append((v.real, v.imag))
    return out


def _unscaled(N: int, pairs, P: int):
    """p_k (scale 1) with P fractional bits"""
    r1, r2 = slot_roots(N)
    nz = [(i, a, b) for i, (a, b) in enumerate(pairs) if a != 0.0 or b != 0.0]
    logn = N.bit_length() - 1
    if len(nz) <= SPARSE:  # p_k = (2/N) sum_i Re(v_i zeta^(-(2 r1_i + 1) k))
        Z = roots(N, P)
        acc = [0] * N
        for i, a, b in nz:
            vr, vi, g = to_fixed(a, P), to_fixed(b, P), 2 * r1[i] + 1
            for k in range(N):
                zr, zi = Z[(g * k) % (2 * N)]
                acc[k] += vr * zr + vi * zi          # Re((vr + i vi)(zr - i zi))
        return [_shr(x, P + logn - 1) for x in acc]
    re, im = [0] * N, [0] * N
    for i, a, b in nz:
        vr, vi = to_fixed(a, P), to_fixed(b, P)
        re[r1[i]], im[r1[i]] = vr, vi
        re[r2[i]], im[r2[i]] = vr, -vi
    _fft(re, im, N, P, -1)
    Z = roots(N, P)
    return [_shr(re[k] * Z[k][0] + im[k] * Z[k][1], P + logn) for k in range(N)]   # Re(a_k zeta^-k) / N


def exact_coefficients(N: int, values, scale: float):
    """x_k = p_k * scale, k < N, as fixed-point integers.  Cached by (N, the values' bits): the transform runs once per
    input pattern, whatever the scale."""
    pairs = _as_pairs(values)
    if not 0 < len(pairs) <= N // 2:
        raise ValueError("values has invalid size")
    sm, sd = float(scale).as_integer_ratio()
    big = max((max(abs(a), abs(b)) for a, b in pairs), default=0.0)
    mag = (math.frexp(big)[1] if big else 0) + max(0, sm.bit_length() - sd.bit_length() + 1)
    P = _precision(N, mag)
    key = ("enc", N, P, hashlib.sha1(repr(pairs).encode()).hexdigest())
    if key in _CACHE:
        STATS["hits"] += 1
    else:
        _CACHE[key] = _unscaled(N, pairs, P)
    shift = P - F + sd.bit_length() - 1
    return [_shr(p * sm, shift) for p in _CACHE[key]]


def exact_slots(N: int, int_coeffs, scale: float):
    """z_i = sum_k c_k zeta^(3^i k) / scale, i < N/2, as (re, im) fixed-point pairs"""
    c = [int(x) for x in int_coeffs]
    if len(c) != N:
        raise ValueError("need N coefficients")
    sm, sd = float(scale).as_integer_ratio()
    mag = max((abs(x).bit_length() for x in c), default=0)
    P = _precision(N, mag + max(0, sd.bit_length() - sm.bit_length() + 1))
    key = ("dec", N, P, hashlib.sha1(repr(c).encode()).hexdigest())
    if key in _CACHE:
        STATS["hits"] += 1
    else:
        Z = roots(N, P)
        re = [x * Z[k][0] for k, x in enumerate(c)]      # c_k zeta^k: an integer times a root, exact to P bits
        im = [x * Z[k][1] for k, x in enumerate(c)]
        _fft(re, im, N, P, +1)
        r1, _ = slot_roots(N)
        _CACHE[key] = [(re[r], im[r]) for r in r1]
    # / scale = * sd / sm, then P -> F bits
    def div(x):
        y = x * sd << 8
        return _shr((2 * y + sm) // (2 * sm), P - F + 8)
    return [(div(a), div(b)) for a, b in _CACHE[key]]


def naive_coefficients(N: int, values, scale: float):
    """exact_coefficients by the O(N^2) definition (test of the transform; small N only)"""
    pairs = _as_pairs(values)
    P = _precision(N, 64)
    Z, (r1, r2) = roots(N, P), slot_roots(N)
    A = [(0, 0)] * N
    for i, (a, b) in enumerate(pairs):
        A[r1[i]] = (to_fixed(a, P), to_fixed(b, P))
        A[r2[i]] = (to_fixed(a, P), -to_fixed(b, P))
    sm, sd = float(scale).as_integer_ratio()
    out = []
    for k in range(N):
        acc = 0
        for r, (ar, ai) in enumerate(A):
            zr, zi = Z[((2 * r + 1) * k) % (2 * N)]
            acc += ar * zr + ai * zi
        out.append(_shr(acc * sm, P + (N.bit_length() - 1) + P - F + sd.bit_length() - 1))
    return out


def naive_slots(N: int, int_coeffs, scale: float):
    """exact_slots by the O(N^2) definition"""
    P = _precision(N, max(abs(int(x)).bit_length() for x in int_coeffs) + 64)
    Z = roots(N, P)
    sm, sd = float(scale).as_integer_ratio()
    out, g = [], 1
    for _ in range(N // 2):
        ar = sum(int(c) * Z[(g * k) % (2 * N)][0] for k, c in enumerate(int_coeffs))
        ai = sum(int(c) * Z[(g * k) % (2 * N)][1] for k, c in enumerate(int_coeffs))
        out.append(tuple(_shr((2 * (x * sd << 8) + sm) // (2 * sm), P - F + 8) for x in (ar, ai)))
        g = g * 3 % (2 * N)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the bands
# ---------------------------------------------------------------------------------------------------------------------
def _fft_factor(N: int) -> float:
    T = (N.bit_length() - 1) + 2
    return T * ETA / (1 - T * ETA)


def encode_band(N: int, values, scale: float) -> float:
    """worst-case |x^_k - x_k| of a float64 encoder before its final rounding; (c) of the module docstring"""
    s2 = sum(a * a + b * b for a, b in _as_pairs(values))
    B = float(scale) * math.sqrt(2.0 * s2 / N)
    return ((1 + _fft_factor(N)) * (1 + U) ** 3 - 1) * B * (1 + 2.0 ** -30)   # the last factor: this line's own roundings


def decode_band(N: int, primes, int_coeffs, scale: float) -> float:
    """worst-case |z^_i - z_i| of a float64 decoder over len(primes) RNS rows; (d) of the module docstring"""
    L = len(primes)
    s2 = sum(int(c) * int(c) for c in int_coeffs)
    norm = Fraction(math.isqrt(N * s2 << 128) + 1, 1 << 64) / Fraction(float(scale))
    return ((1 + _fft_factor(N)) * (1 + U) ** (4 * L + 2) - 1) * float(norm) * (1 + 2.0 ** -30)


# ---------------------------------------------------------------------------------------------------------------------
# the checkers
# ---------------------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def check_encode(rows, primes, x, band: float) -> float:
    """rows[j][k]: coefficient k of RNS row j (canonical residues mod primes[j]); x: exact_coefficients; band:
    encode_band.  Raises Mismatch unless every coefficient k has an integer c, |c - x_k| <= 0.5 + band (exactly
    round_half_away(x_k) at a tie), with rows[j][k] == c mod primes[j] in every row.  Returns the largest
    (|c - x_k| - 0.5) / band that was seen (0 when band is 0)."""
    L, N = len(rows), len(x)
    q = [int(p) for p in primes[:L]]
    rows = [[int(w) for w in (r.tolist() if hasattr(r, "tolist") else r)] for r in rows]
    if any(len(r) != N for r in rows):
        raise Mismatch("row length")
    for j in range(L):
        if max(rows[j]) >= q[j]:
            raise Mismatch(f"row {j} holds a word that is not reduced mod its prime")
    Q = 1
    for p in q:
        Q *= p
    crt = [(Q // p) * pow(Q // p, -1, p) for p in q]
    bandx = int(Fraction(band) * ONE) + 1
    lim = HALF + bandx
    jm = max(range(L), key=lambda j: q[j])
    fast = q[jm] * ONE > 2 * (lim + ONE)       # the largest row alone pins c
    worst = 0
    for k in range(N):
        xk = x[k]
        c0 = round_half_away(xk)
        if is_tie(xk):
            bad = [j for j in range(L) if rows[j][k] != c0 % q[j]]
            if bad:
                raise Mismatch(f"coefficient {k} is the tie {to_float(xk)}: rows {bad} do not hold round() = {c0}")
            continue
        if fast:
            d = (rows[jm][k] - c0) % q[jm]
            c = c0 + (d - q[jm] if d > q[jm] // 2 else d)
            cands = [c]
        else:
            r = sum(rows[j][k] * crt[j] for j in range(L)) % Q
            c = r + Q * ((c0 - r + Q // 2) // Q)
            cands = [c, c - Q, c + Q]
        best = None
        for c in cands:
            if all(rows[j][k] == c % q[j] for j in range(L)):
                e = abs((c << F) - xk)
                best = e if best is None else min(best, e)
        if best is None:
            raise Mismatch(f"coefficient {k}: the rows hold no common integer near {to_float(xk)} "
                           f"(residues {[rows[j][k] for j in range(L)]})")
        if best > lim:
            raise Mismatch(f"coefficient {k}: holds an integer {to_float(best)} away from the exact {to_float(xk)}; "
                           f"allowed 0.5 + {band}")
        worst = max(worst, best - HALF)
    return to_float(worst) / band if band else 0.0


def check_decode(got, z, band: float) -> float:
    """got[i]: decoded complex slot values; z: exact_slots; band: decode_band.  Raises Mismatch unless
    |got_i - z_i| <= band for every slot; returns the largest |got_i - z_i| / band."""
    if len(got) != len(z):
        raise Mismatch("slot count")
    bandx = int(Fraction(band) * ONE) + 1
    worst = 0
    for i, (g, (zr, zi)) in enumerate(zip(got, z)):
        g = complex(g)
        if not (math.isfinite(g.real) and math.isfinite(g.imag)):
            raise Mismatch(f"slot {i} is not finite")
        dr, di = to_fixed(g.real) - zr, to_fixed(g.imag) - zi
        e2 = dr * dr + di * di
        if e2 > bandx * bandx:
            raise Mismatch(f"slot {i}: got {g}, exact ({to_float(zr)}, {to_float(zi)}), "
                           f"off by {to_float(math.isqrt(e2))}; allowed {band}")
        worst = max(worst, e2)
    return to_float(math.isqrt(worst)) / band if band else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the input families of the encode tests (standard library only)
# ---------------------------------------------------------------------------------------------------------------------
SCALES = (2.0 ** 20, 2.0 ** 30, 2.0 ** 40)
TIE_M = (2, 3, 6, -3, (1 << 40) - 3)


def unit_family(N: int):
    """name -> slot values of magnitude about one: what the reference encodes in its hot loops (one-hot masks,
    logistic_regression_ckks.cpp:222-225; 0/1 diagonals + 1e-8, matrix_multiplication.cpp:239; block masks,
    helper.h:333-343) and the usual suspects.  Real lists stay real (an encoder is then called without imaginary parts)."""
    import random
    rng = random.Random(N)
    h, d = N // 2, 8
    ur = lambda n: [rng.uniform(-1, 1) for _ in range(n)]
    uc = lambda n: [complex(rng.uniform(-1, 1), rng.uniform(-1, 1)) for _ in range(n)]
    return {
        "onehot_first": [1.0] + [0.0] * (h - 1),
        "onehot_last": [0.0] * (h - 1) + [1.0],
        "onehot_short": [0.0] * 6 + [1.0],
        "block_mask": [1.0 if 3 * d <= i < 4 * d else 0.0 for i in range(d * d)],
        "diag_eps": [(1.0 if (i * 7) % 16 < 5 else 0.0) + 1e-8 for i in range(h)],
        "ones": [1.0] * h,
        "ones_complex": [complex(1.0, 0.0)] * h,
        "alternating": [1.0 if i % 2 == 0 else -1.0 for i in range(h)],
        "uniform_real": ur(h),
        "uniform_complex": uc(h),
        "complex_1": uc(1),
        "complex_2": uc(2),
        "complex_7": uc(7),
        "real_7": ur(7),
        "complex_h-1": uc(h - 1),
    }


def tie_family(N: int, scale: float, ms=TIE_M):
    """name -> the constant vector (m + 0.5) / scale: coefficient 0 is exactly m + 0.5, every other one exactly 0"""
    return {"tie_%d" % m: [(m + 0.5) / scale] * (N // 2) for m in ms}


def wide_family(N: int, scale: float):
    """name -> values with max|v| * scale just under 2^62, both signs: constants (coefficient 0 carries the whole
    magnitude), a one-hot, uniform values"""
    import random
    rng = random.Random(N + 1)
    top = math.nextafter(2.0 ** 62 / scale, 0.0)
    h = N // 2
    uni = [rng.uniform(-1, 1) * top for _ in range(h)]
    uni[0], uni[1] = top, -top
    return {
        "wide_const_pos": [top] * h,
        "wide_const_neg": [-top] * h,
        "wide_onehot_neg": [0.0] * 5 + [-top],
        "wide_uniform": uni,
        "wide_complex": [complex(a, b) * 0.7 for a, b in zip(uni, reversed(uni))],
    }


# ---------------------------------------------------------------------------------------------------------------------
# helpers of the sampler and key tests (numpy; `o` is an oracle.Oracle, used for ChaCha20 and the inverse NTT only)
# ---------------------------------------------------------------------------------------------------------------------
NOISE_MAX = 19          # the clipped normal: |e| <= floor(19.2)


def uniform_restated(chacha20_block, key32: bytes, stream: int, q: int, row: int, N: int):
    """The uniform sampler's rule in plain Python: word (index & 7) of ChaCha20 block
    `attempt << 48 | row << 16 | index >> 3` with nonce `stream`; accept r < q * floor(2^64 / q), else the same word of
    the next attempt's block; value r mod q.  Returns (values, attempt at which each word was accepted)."""
    bound = q * ((1 << 64) // q)
    vals, att = [], []
    for blk in range(N // 8):
        blocks = {}
        for w in range(8):
            a = 0
            while True:
                if a not in blocks:
                    b = chacha20_block(key32, (a << 48) | (row << 16) | blk, stream)
                    blocks[a] = [int(b[2 * i]) | (int(b[2 * i + 1]) << 32) for i in range(8)]
                r = blocks[a][w]
                if r < bound:
                    break
                a += 1
            vals.append(r % q)
            att.append(a)
    return vals, att


def _obj(a):
    import numpy as np
    return np.asarray(a).astype(object)


def centred_coefficients(o, primes, rows_ntt):
    """rows_ntt[j][N] (NTT form, row j mod primes[j]) -> per row the centred coefficients (object arrays of ints)"""
    out = []
    for j, q in enumerate(primes):
        c = _obj(o.ntt_inv(j, rows_ntt[j]))
        out.append(c - (c > q // 2) * q)
    return out


def kswitch_key_errors(o, primes, sk, new_sk, key):
    """key [k-1][2][k][N], sk / new_sk [k][N], all NTT form.  For digit i and row m:
    k0 + k1 * sk - [m == i] (P mod q_i) new_sk  ==  -e_i  in coefficient form.  Returns e[i] (object array of N ints)
    after asserting that it is the same small polynomial in every row."""
    import numpy as np
    k, P = len(primes), primes[-1]
    out = []
    for i in range(k - 1):
        rows = []
        for m, q in enumerate(primes):
            t = (_obj(key[i][0][m]) + _obj(key[i][1][m]) * _obj(sk[m])) % q
            if m == i:
                t = (t - (P % q) * _obj(new_sk[m])) % q
            rows.append(np.asarray([int(x) for x in t], dtype=np.uint64))
        cen = centred_coefficients(o, primes, rows)
        e = -cen[0]
        assert max(abs(int(x)) for x in e) <= NOISE_MAX, ("digit", i, "noise out of range")
        for m in range(1, k):
            assert (cen[m] == cen[0]).all(), ("digit", i, "row", m, "holds another error polynomial")
        out.append(e)
    return out


def public_key_error(o, primes, sk, pk):
    """pk [2][k][N]: pk0 + pk1 * sk == -e, the same |e| <= 19 in every row"""
    import numpy as np
    rows = [np.asarray([int(x) for x in (_obj(pk[0][m]) + _obj(pk[1][m]) * _obj(sk[m])) % q], dtype=np.uint64)
            for m, q in enumerate(primes)]
    cen = centred_coefficients(o, primes, rows)
    assert max(abs(int(x)) for x in cen[0]) <= NOISE_MAX
    for m in range(1, len(primes)):
        assert (cen[m] == cen[0]).all(), ("row", m)
    return -cen[0]


def fresh_noise_bound(N: int) -> int:
    """decrypt(encrypt(m)) - m = e0 + e1 s - e u with (pk0, pk1) = (-(a s + e), a): s and u ternary, e, e0, e1 clipped
    at 19; a product of two polynomials mod X^N + 1 sums N terms, so every coefficient is at most 19 (2N + 1)"""
    return NOISE_MAX * (2 * N + 1)


def crt_centred(primes, rows):
    """rows[j][N] coefficient form -> the integers in (-Q/2, Q/2] they represent (list of ints)"""
    Q = 1
    for p in primes:
        Q *= p
    acc = [0] * len(rows[0])
    for p, r in zip(primes, rows):
        M = (Q // p) * pow(Q // p, -1, p)
        acc = [(a + int(w) * M) % Q for a, w in zip(acc, r.tolist() if hasattr(r, "tolist") else r)]
    return [a - Q if a > Q // 2 else a for a in acc]
