"""Host-only planner of CKKS bootstrapping ("Bootstrapping"): the two homomorphic DFTs with their factors, the
Chebyshev interpolant of EvalMod's scaled cosine, the levels, and a float64 model of the whole pipeline.  Nothing here touches
a device; algorithms.eval_mod and algorithms.bootstrap run a plan.

A ciphertext at the last prime q_0 and scale D encrypts an integer polynomial m.  Raised to the top of the chain
(Evaluator.mod_raise) it encrypts t = m + q_0 I with a small integer polynomial I, |I| <= K.  Then
    CoeffToSlot, factor D / (q_0 K')      slots u = t / (q_0 K') = (I + eps) / K' in [-1, 1],   eps = m / q_0
    EvalMod                               g(u) = cos((2 pi K' u - pi / 2) / 2^r) by its Chebyshev interpolant on [-1, 1], then r
                                          double angles cos 2x = 2 cos^2 x - 1:  cos(2 pi (I + eps) - pi / 2) = sin(2 pi eps)
    SlotToCoeff, factor q_0 / (2 pi D)    coefficients D q_0 sin(2 pi eps) / (2 pi D) = m (1 - (2 pi eps)^2 / 6 + ...)
K' = K + 1/4 leaves room for eps next to the outermost integers.  The sine's own error is (2 pi eps)^2 / 6 relative, which is why
q_0 / D must be large (2^10: 6e-6) and the chain starts with a prime ten bits above the scale."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

from . import dft


def chebyshev_interpolant(f, degree: int) -> np.ndarray:
    """coefficients c_0 .. c_degree of the polynomial that meets f at the degree + 1 Chebyshev nodes of [-1, 1]"""
    k = np.arange(degree + 1)
    nodes = np.cos(np.pi * (k + 0.5) / (degree + 1))
    return np.polynomial.chebyshev.chebfit(nodes, f(nodes), degree)


class Plan:
    def __init__(self, N, primes, scale, K, r, degree, c2s, s2c, coeffs, poly_target_scale, max_value, model_error, slots=None, special=1):
        self.N, self.primes, self.scale, self.K, self.r, self.degree = N, [int(p) for p in primes], float(scale), K, r, degree
        self.Kp = K + 0.25
        self.sparse_slots = slots   # None: all N / 2 slots; ns: plan(..., slots=ns).  (slots() is the embedding below.)
        self.c2s, self.s2c, self.coeffs = c2s, s2c, coeffs
        self.poly_target_scale, self.max_value, self.model_error = poly_target_scale, max_value, model_error
        self.special = int(special)   # the special primes at the end of the chain: 1, or the alpha of hybrid keys
        self.top_level = len(self.primes) - self.special
        self.depth = int(math.ceil(math.log2(degree + 1)))
        self.evalmod_level = self.top_level - c2s.levels
        self.s2c_level = self.evalmod_level - self.depth - r
        self.result_level = self.s2c_level - s2c.levels

    def levels(self) -> int:
        """levels one bootstrap spends below the top of the chain: CoeffToSlot, the polynomial, the double angles, SlotToCoeff"""
        return self.c2s.levels + self.depth + self.r + self.s2c.levels

    def galois_steps(self) -> List[int]:
        """every rotation step either transform needs a direct Galois key for; the conjugation key on top:
        KeyGenerator.galois_keys(plan.galois_steps(), conjugate=True)"""
        return sorted(set(self.c2s.galois_steps()) | set(self.s2c.galois_steps()) | set(self.subsum_steps()))

    def subsum_steps(self) -> List[int]:
        """the rotation steps of SubSum, ns 2^i for i < log2 g, g = N / (2 ns): none in a dense plan"""
        if self.sparse_slots is None:
            return []
        g = self.N // (2 * self.sparse_slots)
        return [self.sparse_slots << i for i in range(g.bit_length() - 1)]

    def key_switches(self, lazy: bool = True) -> int:
        """key switches of one bootstrap: SubSum (sparse plans), both transforms, the polynomial's relinearisations on
        both chains (on the one chain of a sparse plan), the double angles"""
        from . import poly
        p = poly.plan(self.coeffs, "chebyshev", self.primes[:self.evalmod_level], self.scale, self.poly_target_scale)
        chains = 2 if self.sparse_slots is None else 1
        return (len(self.subsum_steps()) + self.c2s.key_switches() + self.s2c.key_switches()
                + chains * (p.relinearizations(lazy) + self.r))

    def encode(self, encoder, extended: bool = False):
        """(CoeffToSlot's plaintexts at the top level, SlotToCoeff's at plan.s2c_level): the `encoded` of algorithms.bootstrap.
        extended=True: key-level diagonals for both transforms (dft.Plan.encode's extended form), the `encoded` of
        algorithms.bootstrap_hybrid"""
        if not extended:
            return self.c2s.encode(encoder, self.top_level), self.s2c.encode(encoder, self.s2c_level)
        return self.c2s.encode(encoder, self.top_level, extended=True), self.s2c.encode(encoder, self.s2c_level, extended=True)

    # ---- the float64 model
    def eval_mod(self, u: np.ndarray) -> np.ndarray:
        """what EvalMod computes on plain slots: the interpolant, then r double angles"""
        y = np.polynomial.chebyshev.chebval(u, self.coeffs)
        for _ in range(self.r):
            y = 2.0 * y * y - 1.0
        return y

    def _roots(self) -> np.ndarray:
        M = 2 * self.N
        r, out = 1, np.empty(self.N // 2, dtype=np.int64)
        for j in range(self.N // 2):
            out[j] = r
            r = r * 3 % M
        return out

    def slots(self, coeffs: Sequence[float]) -> np.ndarray:
        """the N / 2 slot values the encoder decodes from N real coefficients at plan.scale: z_j = sum_i t_i zeta^(r_j i) / scale"""
        t = np.asarray(coeffs, dtype=np.float64)
        if t.shape != (self.N,):
            raise ValueError("need the N coefficients of one plaintext")
        return np.conj(np.fft.fft(t, 2 * self.N)[self._roots()]) / self.scale

    def coefficients(self, z: np.ndarray) -> np.ndarray:
        """the inverse of slots(): m_i = (1 / N) sum over the odd k of Z_k zeta^(-k i), Z at the roots and their conjugates"""
        N, roots = self.N, self._roots()
        full = np.zeros(2 * N, dtype=np.complex128)
        full[roots], full[2 * N - roots] = z, np.conj(z)
        return np.real(np.fft.fft(full)[:N]) / N * self.scale

    def apply(self, coeffs: Sequence[float]) -> np.ndarray:
        """The whole pipeline in float64 on the N coefficients t = m + q_0 I of a mod-raised plaintext: the encoder's
        embedding (slot j <-> root zeta^(3^j)) divided by the scale, CoeffToSlot, EvalMod with its approximation error,
        SlotToCoeff, and the embedding back.  Returns the N coefficients the bootstrapped ciphertext's plaintext has (noise
        aside), at plan.scale: about m = t centred mod q_0.  A sparse plan expects m in the subring (coefficients at
        multiples of g = N / (2 ns) only) under a general I: SubSum first, the packed transforms on one vector, and the
        result is about m on the stride and about 0 elsewhere."""
        if self.sparse_slots is not None:
            x = self.slots(coeffs)
            for step in self.subsum_steps():
                x = x + np.roll(x, -step)
            (u,) = self.c2s.apply([x])
            (zz,) = self.s2c.apply([self.eval_mod(np.real(u)).astype(np.complex128)])
            return self.coefficients(zz)
        ua, ub = (np.real(x) for x in self.c2s.apply([self.slots(coeffs)]))
        (zz,) = self.s2c.apply([self.eval_mod(ua).astype(np.complex128), self.eval_mod(ub).astype(np.complex128)])
        return self.coefficients(zz)


def model_error(coeffs: np.ndarray, K: int, r: int, band: float) -> float:
    """max over the integers I in [-K, K] and |f| <= band of |sin-model(I + f) / (2 pi) - f|, as a fraction of band: the error
    of EvalMod's float model (interpolation, double angles and the sine's own cubic term) relative to the largest message"""
    Kp = K + 0.25
    f = np.linspace(-band, band, 33)
    x = (np.arange(-K, K + 1)[:, None] + f[None, :])
    y = np.polynomial.chebyshev.chebval(x / Kp, coeffs)
    for _ in range(r):
        y = 2.0 * y * y - 1.0
    return float(np.abs(y / (2.0 * np.pi) - f[None, :]).max() / band)


def plan(N: int, primes: Sequence[int], scale: float, K: int = 12, r: int = 3, degree: int = 31, c2s_levels: int = 2,
         s2c_levels: int = 2, max_value: float = 1.0, precision: float = 1e-4, slots: Optional[int] = None, special: int = 1) -> Plan:
    """The bootstrap of a ciphertext at primes[0] and `scale` on the chain `primes` (the context's coeff_modulus, the special
    prime last).  K: the integer part |I| the secret key allows (12 for Hamming weight 32); r double angles; `degree` of the
    interpolant; levels of the two transforms.  max_value: the largest |coefficient| / scale of a message (1.0 covers slots of
    magnitude up to 1).  ValueError when the chain is too short (the result must keep at least one prime) or when the float
    model's own error on the band |frac| <= scale max_value / q_0 around every integer in [-K, K] exceeds `precision`
    (relative to max_value).
    slots=ns (a power of two, 2 <= ns <= N/4; ValueError otherwise): the sparse plan of a message of ns slots, whose plaintext
    is a polynomial in X^g, g = N / (2 ns).  SubSum (plan.subsum_steps(): log2 g rotate-and-adds) brings the raised plaintext
    back into that subring, times g; the transforms are dft.plan_packed's, of dimension 2 ns on ONE ciphertext, 1 / g folded
    into CoeffToSlot's diagonals, their levels clipped to log2(ns); EvalMod runs on one chain.  plan.sparse_slots is ns.
    special: the special primes at the end of the chain -- 1, or the alpha of the hybrid keys algorithms.bootstrap_hybrid is
    given (1 <= special <= HYBRID_ALPHA_MAX, ValueError otherwise); the top level is len(primes) - special and every level
    below follows from it."""
    primes = [int(p) for p in primes]
    from .seal import HYBRID_ALPHA_MAX
    special = int(special)
    if not 1 <= special <= HYBRID_ALPHA_MAX:
        raise ValueError("bootstrap plan: special must be in 1 .. %d" % HYBRID_ALPHA_MAX)
    top = len(primes) - special
    if top < 1:
        raise ValueError("bootstrap plan: the chain needs data primes and a special prime")
    if K < 1 or r < 0 or degree < 1:
        raise ValueError("bootstrap plan: K >= 1, r >= 0, degree >= 1")
    g = 1
    if slots is not None:
        slots = int(slots)
        if slots < 2 or slots & (slots - 1) or 4 * slots > N:
            raise ValueError("bootstrap plan: slots must be a power of two in 2 .. N/4")
        g = N // (2 * slots)
        c2s_levels, s2c_levels = (min(int(v), slots.bit_length() - 1) for v in (c2s_levels, s2c_levels))
    q0, Kp = float(primes[0]), K + 0.25
    depth = int(math.ceil(math.log2(degree + 1)))
    evalmod_level = top - int(c2s_levels)
    s2c_level = evalmod_level - depth - r
    if s2c_level - int(s2c_levels) < 1:
        raise ValueError("bootstrap plan: not enough levels: %d primes below the special one, %d + %d + %d + %d needed and one to keep"
                         % (top, c2s_levels, depth, r, s2c_levels))
    coeffs = chebyshev_interpolant(lambda u: np.cos((2.0 * np.pi * Kp * u - 0.5 * np.pi) / 2.0 ** r), degree)
    band = float(scale) * float(max_value) / q0
    err = model_error(coeffs, K, r, band)
    if not err <= precision:
        raise ValueError("bootstrap plan: the float model misses the precision: error %.3g of the largest message, %.3g asked "
                         "(K = %d, r = %d, degree = %d, q_0 / scale = %.3g)" % (err, precision, K, r, degree, q0 / float(scale)))
    # the r double angles take scale s to s^2 / q (weight 2 at scale 1): the polynomial's target scale is the one from which
    # they end at `scale`
    target = float(scale)
    for i in range(r):
        target = math.sqrt(target * float(primes[s2c_level + i]))
    make = dft.plan if slots is None else (lambda N_, *a, **kw: dft.plan_packed(N_, slots, *a, **kw))
    # (sparse: 1 / g next to the small plan's 1 / (2 ns) is the dense 1 / N; in the diagonals, not in a relabelled scale --
    # a scale of g 2^50 entering the polynomial would outgrow the primes)
    c2s = make(N, c2s_levels, dft.C2S, [primes[top - 1 - i] for i in range(c2s_levels)], factor=float(scale) / (q0 * Kp * g))
    s2c = make(N, s2c_levels, dft.S2C, [primes[s2c_level - 1 - i] for i in range(s2c_levels)],
               factor=q0 / (2.0 * np.pi * float(scale)))
    return Plan(N, primes, scale, K, r, degree, c2s, s2c, coeffs, target, max_value, err, slots, special)
