"""Exact models and inputs of the BFV entries beyond multiply and decrypt_round (include/hefx_bfv.h): the message scaled by
Delta and added to c_0, the centred lift, the noise budget and BatchEncoder's slot transform.  Python integers only, on
top of tests/bfv_cases.py; the models follow the header's definitions literally and share nothing with the engine's
method (Delta from an integer division of Q, the budget from a composed and centred integer, the slots by evaluating
the polynomial at psi^(e_i) power by power).

    scale_plain_add_model(m, ncoeff, c0, primes, L, t)   [ncoeff], [L][N] or None -> [L][N]
    lift_plain_model(m, ncoeff, primes, L, t, n)         [ncoeff] -> [L][n]
    noise_budget_model(x, primes, L, t)                  [L][N] -> int
    x_for_noise(v, primes, L, t)                         N signed integers v -> x [L][N] with t x^ = v mod Q
    batch_encode_model(values, t, n) / batch_decode_model(m, t, n)
"""
import functools

import numpy as np

from tests import bfv_cases as B

N = B.N


def scale_plain_add_model(m, ncoeff, c0, primes, L, t, n=N):
    delta = B.modulus(primes, L) // t
    out = np.zeros((L, n), dtype=np.uint64) if c0 is None else np.array(c0, dtype=np.uint64).copy()
    for j in range(L):
        q = int(primes[j])
        dq = delta % q
        for i in range(ncoeff):
            out[j, i] = (int(out[j, i]) + dq * (int(m[i]) % q)) % q
    return out


def lift_plain_model(m, ncoeff, primes, L, t, n=N):
    """the header's words: m mod q_j up to floor(t/2), q_j - ((t - m) mod q_j) above it -- which is q_j itself, not 0,
    when q_j divides t - m"""
    out = np.zeros((L, n), dtype=np.uint64)
    for j in range(L):
        q = int(primes[j])
        for i in range(ncoeff):
            v = int(m[i])
            out[j, i] = v % q if v <= t // 2 else q - ((t - v) % q)
    return out


def noise_budget_model(x, primes, L, t):
    Q = B.modulus(primes, L)
    W = max(abs(B.centre((t * v) % Q, Q)) for v in B.compose(x, primes, L))
    return max(0, Q.bit_length() - W.bit_length() - 1)


def x_for_noise(v, primes, L, t):
    """x = v t^-1 mod Q per coefficient: the centred representative of t x^ mod Q is v (|v| <= (Q-1)/2)"""
    Q = B.modulus(primes, L)
    ti = pow(t, -1, Q)
    return B.residues([(int(c) * ti) % Q for c in v], primes, L)


def budget_of(v, primes, L):
    """closed form for a polynomial whose largest noise magnitude is |v|"""
    Q = B.modulus(primes, L)
    return max(0, Q.bit_length() - abs(v).bit_length() - 1)


def noise_values(primes, L):
    """+-1, +-(2^k - 1) and +-2^k for every k < bits(Q) - 1, +-(Q-1)/2"""
    Q = B.modulus(primes, L)
    mags = {1, (Q - 1) // 2}
    for k in range(Q.bit_length() - 1):
        mags |= {(1 << k) - 1, 1 << k}
    mags.discard(0)
    assert all(w <= (Q - 1) // 2 for w in mags)
    return [s * w for w in sorted(mags) for s in (1, -1)]


# ---- batching
def is_prime(t):
    if t < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if t % p == 0:
            return t == p
    d, r = t - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, t)
        if x in (1, t - 1):
            continue
        for _ in range(r - 1):
            x = x * x % t
            if x == t - 1:
                break
        else:
            return False
    return True


def allows_batching(t, n=N):
    return is_prime(t) and t % (2 * n) == 1


@functools.lru_cache(maxsize=None)
def minimal_root(t, n=N):
    """the smallest element of order exactly 2n modulo the prime t, by search over all of them"""
    g = next(c for c in (pow(a, (t - 1) // (2 * n), t) for a in range(2, 2000)) if pow(c, n, t) == t - 1)
    best, cur, sq = g, g, g * g % t
    for _ in range(n):
        best = min(best, cur)
        cur = cur * sq % t
    return best


@functools.lru_cache(maxsize=None)
def _powers(t, n):
    psi, out, p = minimal_root(t, n), [], 1
    for _ in range(2 * n):
        out.append(p)
        p = p * psi % t
    return out


@functools.lru_cache(maxsize=None)
def slot_exponents(n=N):
    """e_i = 3^i mod 2n for i < n/2, e_(n/2+i) = -3^i mod 2n"""
    e, pos = [0] * n, 1
    for i in range(n // 2):
        e[i], e[n // 2 + i] = pos, 2 * n - pos
        pos = pos * 3 % (2 * n)
    return e


def batch_decode_model(m, t, n=N):
    """values[i] = m(psi^(e_i)) = sum_k m[k] psi^(e_i k)"""
    pw, two_n = _powers(t, n), 2 * n
    mm = [int(c) % t for c in m] + [0] * (n - len(m))
    nz = [(k, c) for k, c in enumerate(mm) if c]
    return np.array([sum(c * pw[e * k % two_n] for k, c in nz) % t for e in slot_exponents(n)], dtype=np.uint64)


def batch_encode_model(values, t, n=N):
    """the polynomial of degree < n through (psi^(e_i), values[i]), zeros in the slots behind len(values): the points are
    the n odd powers of psi, so m[k] = n^-1 sum_i values[i] psi^(-e_i k)"""
    pw, two_n = _powers(t, n), 2 * n
    ninv = pow(n, -1, t)
    e = slot_exponents(n)
    nz = [(e[i], int(v) % t) for i, v in enumerate(values) if int(v) % t]
    return np.array([ninv * sum(v * pw[-ei * k % two_n] for ei, v in nz) % t for k in range(n)], dtype=np.uint64)


def batching_moduli(n=N):
    """the plain moduli of tests/bfv_cases.py that allow batching at ring size n, and the largest such prime below 2^59"""
    from tests import policy_sets
    ts = [t for t in B.PLAIN_MODULI if allows_batching(t, n)]
    top = policy_sets.primes_below(1 << 59, n, 1)[0]
    return ts + ([top] if top not in ts else [])


def message_values(t, n, seed):
    """the values at and next to the lift's threshold, then seeded uniform ones below t"""
    rng = np.random.default_rng(seed)
    special = [0, 1, t - 1, t // 2, min(t // 2 + 1, t - 1)]
    m = [int(v) for v in rng.integers(0, t, n, dtype=np.uint64)]
    m[:len(special)] = special
    m[n - 1] = t - 1
    return np.array(m, dtype=np.uint64)
