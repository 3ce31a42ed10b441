"""Exact model and inputs of the BFV entries (include/hefx_bfv.h), Python integers only.

The model follows the header's definitions literally and shares nothing with the engine's method (which never centres,
never composes and never divides: csrc/hefx_bfv.hip): CRT-compose every coefficient, centre it, multiply the polynomials
in Z[X]/(X^N + 1) by Kronecker substitution into one big integer, and round with Python's integer division.

    centre(x, Q)   x when x <= Q // 2, else x - Q
    R(z, t, Q)     sign(z) * ((t |z| + (Q - 1) // 2) // Q)
    multiply_model(a, b, primes, L, t)      [sa][L][N], [sb][L][N] -> [sa + sb - 1][L][N]
    decrypt_round_model(x, primes, L, t)    [L][N] -> [N]
"""
import numpy as np

from seal_fyp_logistic_regression_amd.seal import CoeffModulus
from tests import policy_sets as P

N = 1024

# plain moduli: the smallest, a power of two (1_bfv.cpp), the usual batching prime, vector_ops.cpp's, and a 59-bit prime
T_59 = P.primes_below(1 << 59, 8192, 1)[0]
PLAIN_MODULI = (2, 1024, 65537, 1032193, T_59)
SIZES = ((2, 2), (2, 3), (3, 3), (3, 4))


def _mixed_set():
    """from policy_sets' mixed chain at N = 1024: a prime just below 2^41 (FP64 transform), one just above it, one just
    above 2^60 and a 60-bit one; special prime just below 2^61"""
    m = P._mixed(N)
    data = [m[2], m[6], m[7], m[0]]
    assert data[0] < 1 << 41 < data[1] and data[2] > 1 << 60 and data[3] < 1 << 60
    return data + [m[9]]


def prime_sets():
    """name -> (N, primes incl. the special prime, L)"""
    b4096 = [q.bit_length() for q in CoeffModulus.BFVDefault(4096)]
    b8192 = [q.bit_length() for q in CoeffModulus.BFVDefault(8192)]
    return {
        "one60": (N, CoeffModulus.Create(N, [60]), 1),
        "bfv4096_bits": (N, CoeffModulus.Create(N, b4096), 2),
        "bfv8192_bits": (N, CoeffModulus.Create(N, b8192), 4),
        "mixed": (N, _mixed_set(), 4),
    }


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def modulus(primes, L):
    Q = 1
    for q in primes[:L]:
        Q *= int(q)
    return Q


def centre(x, Q):
    return x if x <= Q // 2 else x - Q


def R(z, t, Q):
    m = (t * abs(z) + (Q - 1) // 2) // Q
    return -m if z < 0 else m


def compose(rows, primes, L):
    """[L][N] residues -> N integers in [0, Q)"""
    Q = modulus(primes, L)
    n = len(rows[0])
    x = [0] * n
    for j in range(L):
        q = int(primes[j])
        w = (Q // q) * pow(Q // q, -1, q)
        r = rows[j]
        for i in range(n):
            x[i] += int(r[i]) * w
    return [v % Q for v in x]


def centred(rows, primes, L):
    Q = modulus(primes, L)
    return [centre(v, Q) for v in compose(rows, primes, L)]


def _pack(p, B):
    """sum_i p[i] 2^(B i) for signed p[i], |p[i]| < 2^(B-1), B a multiple of 8: through bytes, offset by 2^(B-1) per digit"""
    half, step = 1 << (B - 1), B // 8
    raw = b"".join((v + half).to_bytes(step, "little") for v in p)
    return int.from_bytes(raw, "little") - int.from_bytes((half.to_bytes(step, "little")) * len(p), "little")


def _unpack(v, count, B):
    """the signed digits of v in base 2^B, each |digit| < 2^(B-1)"""
    half, step = 1 << (B - 1), B // 8
    v += int.from_bytes((half.to_bytes(step, "little")) * count, "little")  # every digit non-negative: no borrows
    raw = v.to_bytes(count * step + 8, "little")
    return [int.from_bytes(raw[i * step:(i + 1) * step], "little") - half for i in range(count)]


def negacyclic_sums(A, Bp, bound_bits):
    """A[sa][N], Bp[sb][N] signed integers -> c_k = sum_{i+j=k} A_i * B_j in Z[X]/(X^N + 1), by Kronecker substitution:
    every polynomial becomes one integer (X = 2^B, B wide enough for a signed sum of 3 N products), the sums are formed
    on those, and the digits come back out"""
    n = len(A[0])
    B = -(-(bound_bits + 3) // 8) * 8
    pa, pb = [_pack(p, B) for p in A], [_pack(p, B) for p in Bp]
    out = []
    for k in range(len(A) + len(Bp) - 1):
        s = sum(pa[i] * pb[k - i] for i in range(len(A)) if 0 <= k - i < len(Bp))
        d = _unpack(s, 2 * n, B)
        out.append([d[i] - d[i + n] for i in range(n)])
    return out


def multiply_model(a, b, primes, L, t):
    sa, sb = len(a), len(b)
    n = len(a[0][0])
    Q = modulus(primes, L)
    A = [centred(p, primes, L) for p in a]
    Bp = A if b is a else [centred(p, primes, L) for p in b]
    c = negacyclic_sums(A, Bp, 2 * Q.bit_length() + n.bit_length() + 2)
    out = np.zeros((sa + sb - 1, L, n), dtype=np.uint64)
    for k, poly in enumerate(c):
        r = [R(z, t, Q) for z in poly]
        for j in range(L):
            q = int(primes[j])
            out[k, j] = np.array([v % q for v in r], dtype=np.uint64)
    return out


def decrypt_round_model(x, primes, L, t):
    Q = modulus(primes, L)
    return np.array([R(z, t, Q) % t for z in centred(x, primes, L)], dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def residues(values, primes, L):
    """integers (any sign) -> [L][len] canonical residues"""
    return np.array([[v % int(primes[j]) for v in values] for j in range(L)], dtype=np.uint64)


def boundary_values(primes, L, t):
    """the two neighbours of a rounding boundary: x with t x = (Q - 1)/2 and (Q + 1)/2 mod Q -- the first rounds down,
    the second up"""
    Q = modulus(primes, L)
    ti = pow(t, -1, Q)
    return ((Q - 1) // 2 * ti) % Q, ((Q + 1) // 2 * ti) % Q


def special_values(primes, L, t):
    """what is placed in front of R: 0, +-1, +-floor(Q/2), both neighbours of a rounding boundary and their negatives"""
    Q = modulus(primes, L)
    lo, hi = boundary_values(primes, L, t)
    return [0, 1, -1, Q // 2, -(Q // 2), lo, hi, -lo, -hi]


def uniform(primes, L, size, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.integers(0, int(primes[j]), n, dtype=np.uint64) for j in range(L)])
                     for _ in range(size)])


def crafted_poly(primes, L, t, n, seed):
    """[L][n]: the special values in the first coefficients, seeded uniform residues behind them"""
    x = uniform(primes, L, 1, n, seed)[0]
    sp = residues(special_values(primes, L, t), primes, L)
    x[:, :sp.shape[1]] = sp
    return x


def identity_operands(primes, L, t, sa, sb, n, seed):
    """a = (1, 0, ..., 0) and b_0 = crafted_poly: output polynomial 0 of the product is R(b^_0) itself"""
    a = np.zeros((sa, L, n), dtype=np.uint64)
    a[0, :, 0] = 1
    b = uniform(primes, L, sb, n, seed + 1)
    b[0] = crafted_poly(primes, L, t, n, seed)
    return a, b


def magnitude_operands(primes, L, sa, sb, n, sign_a, sign_b):
    """every coefficient of every polynomial +-floor(Q/2), one sign per operand: coefficient N-1 of the middle output
    polynomials is a sum of min(sa, sb) N products of magnitude floor(Q/2)^2, all of one sign -- the bound the working
    basis is sized from (3 N (Q/2)^2 at 3 x 3 and 3 x 4)"""
    Q = modulus(primes, L)
    one = lambda sign, size: np.broadcast_to(residues([sign * (Q // 2)], primes, L)[None, :, :], (size, L, n)).copy()
    return one(sign_a, sa), one(sign_b, sb)
