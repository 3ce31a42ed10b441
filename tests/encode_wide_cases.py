"""The rule for CKKS coefficients of any magnitude, and the cases of the wide-encode tests (host only; numpy only for
the float64 model encoder).

The rule (check_wide)
---------------------
x_k = exact_ckks.exact_coefficients(N, v, scale)[k], band = exact_ckks.encode_band(N, v, scale).  For every coefficient k
the rows are CRT-composed to the integer c nearest x_k, and
  * rows[j][k] == c mod q_j in EVERY row,
  * |c - x_k| <= 0.5 + band,
  * c is representable as a float64 (a float64 encoder stores the double its transform produced, nothing else).
exact_ckks.check_encode cannot be used unchanged at wide magnitudes: its tie rule demands the exact round() wherever x_k
is a half-integer, which no float64 encoder can resolve once the band exceeds a fraction of one.  Below a band of 0.25 the
rule IS check_encode (ties included).

The bound of the wide entries: |v| * scale < 2^max(62, min(bc - 3, 1000)), bc = bit length of q_0 ... q_(L-1).
"""
from __future__ import annotations

import math
from fractions import Fraction

from tests import exact_ckks as X

FULL_MANTISSA = float(0x1F3A5C7E9B2D4F) * 2.0 ** 60     # 53 significant bits, about 2^112.97
FAMILIES = ("onehot_short", "ones", "uniform_real", "uniform_complex", "alternating")


def bit_count(primes, L: int) -> int:
    Q = 1
    for p in primes[:L]:
        Q *= int(p)
    return Q.bit_length()


def wide_bits(primes, L: int) -> int:
    """log2 of the wide entries' bound at level L"""
    return max(62, min(bit_count(primes, L) - 3, 1000))


def max_abs(v) -> float:
    return max(abs(complex(a)) for a in v)


def top_scale(primes, L: int, v) -> float:
    """the largest scale the wide entry accepts for v: nextafter(2^(bc-3) / max|v|, 0)"""
    return math.nextafter(2.0 ** (bit_count(primes, L) - 3) / max_abs(v), 0.0)


def families(N: int):
    """name -> values: the five families of exact_ckks.unit_family and their negations"""
    fam = X.unit_family(N)
    out = {}
    for n in FAMILIES:
        out[n] = list(fam[n])
        out["neg_" + n] = [-a for a in fam[n]]
    return out


def compose(rows, primes, x):
    """rows[j][k] -> [c_k]: the integer congruent to the rows of coefficient k that lies nearest x_k (fixed point)"""
    L, N = len(rows), len(x)
    q = [int(p) for p in primes[:L]]
    rows = [[int(w) for w in (r.tolist() if hasattr(r, "tolist") else r)] for r in rows]
    for j in range(L):
        if len(rows[j]) != N:
            raise X.Mismatch("row length")
        if max(rows[j]) >= q[j]:
            raise X.Mismatch(f"row {j} holds a word that is not reduced mod its prime")
    Q = 1
    for p in q:
        Q *= p
    crt = [(Q // p) * pow(Q // p, -1, p) for p in q]
    out = []
    for k in range(N):
        r = sum(rows[j][k] * crt[j] for j in range(L)) % Q
        x0 = X.round_half_away(x[k])
        c = r + Q * ((x0 - r + Q // 2) // Q)
        c = min((c - Q, c, c + Q), key=lambda t: abs((t << X.F) - x[k]))
        bad = [j for j in range(L) if rows[j][k] != c % q[j]]
        if bad:
            raise X.Mismatch(f"coefficient {k}: rows {bad} do not hold {c}")
        out.append(c)
    return out


def check_wide(rows, primes, x, band: float) -> float:
    """The rule of the module docstring; raises exact_ckks.Mismatch, returns the largest (|c - x_k| - 0.5) / band."""
    if band < 0.25:
        return X.check_encode(rows, primes, x, band)
    lim = X.HALF + int(Fraction(band) * X.ONE) + 1
    worst = 0
    for k, c in enumerate(compose(rows, primes, x)):
        e = abs((c << X.F) - x[k])
        if e > lim:
            raise X.Mismatch(f"coefficient {k}: holds an integer {X.to_float(e)} away from the exact {X.to_float(x[k])}; "
                             f"allowed 0.5 + {band}")
        if int(float(c)) != c:
            raise X.Mismatch(f"coefficient {k}: {c} is not a float64")
        worst = max(worst, e - X.HALF)
    return X.to_float(worst) / band


def c_round(x: float) -> int:
    """C's round() of a finite double as a Python integer"""
    t = math.trunc(x)
    return t + (0 if abs(x - t) < 0.5 else (1 if x > 0 else -1))


def numpy_encode_rows(N: int, v, scale: float, primes, L: int):
    """a float64 encoder in numpy (full-size FFT, rounding half away, exact reduction of the rounded double): rows[L][N]
    in coefficient form -- the model the rule is tried on without a GPU"""
    import numpy as np
    r1, r2 = X.slot_roots(N)
    A = np.zeros(N, dtype=np.complex128)
    vv = np.asarray(v, dtype=np.complex128)
    A[np.asarray(r1[: vv.size])] = vv
    A[np.asarray(r2[: vv.size])] = np.conj(vv)
    a = np.fft.fft(A) / N
    co = np.real(a * np.exp(-1j * np.pi * np.arange(N) / N)) * scale
    ints = [c_round(float(c)) for c in co]
    return [[c % int(primes[j]) for c in ints] for j in range(L)]
