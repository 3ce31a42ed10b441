"""Pure-Python (big-int, O(N^2)) restatement of the path's math for TOY sizes only.

Independent of oracle/ckks_oracle.c: used to pin the C oracle at N<=64.
Follows SURVEY.md Appendix A.5/A.7/A.8/A.9 (SEAL 3.4.5 semantics); test infrastructure only.
"""


def bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


def is_prime(n):
    if n < 2:
        return False
    i = 2
    while i * i <= n:
        if n % i == 0:
            return False
        i += 1
    return True


def min_primitive_root(two_n, q):
    """smallest integer of exact multiplicative order two_n (a power of two) mod q"""
    for x in range(2, q):
        if pow(x, two_n // 2, q) == q - 1:
            return x
    raise ValueError


_VDM = {}


def _vandermonde(psi, q, n, inverse):
    """rows [x_i^k for k < n] with x_i = psi^(2 bitrev(i) + 1) (its inverse for the inverse transform): the definition's
    matrix, built once per (psi, q, n) with plain big-int products"""
    key = (psi, q, n, inverse)
    if key not in _VDM:
        logn = n.bit_length() - 1
        rows = []
        for i in range(n):
            x = pow(psi, 2 * bitrev(i, logn) + 1, q)
            if inverse:
                x = pow(x, -1, q)
            row, p = [], 1
            for _ in range(n):
                row.append(p)
                p = p * x % q
            rows.append(row)
        _VDM[key] = rows
    return _VDM[key]


def ntt_def(a, psi, q):
    """out[i] = a(psi^(2 bitrev(i) + 1)) mod q"""
    a = [int(v) for v in a]
    return [sum(x * y for x, y in zip(a, row)) % q for row in _vandermonde(psi, q, len(a), False)]


def intt_def(A, psi, q):
    """out[k] = n^-1 sum_i A[i] psi^-(2 bitrev(i) + 1) k mod q"""
    n = len(A)
    ninv = pow(n, -1, q)
    A = [int(v) for v in A]
    M = _vandermonde(psi, q, n, True)
    return [sum(A[i] * M[i][k] for i in range(n)) * ninv % q for k in range(n)]


def galois_table(n, elt):
    logn = n.bit_length() - 1
    tab = []
    for i in range(n):
        raw = (elt * (2 * bitrev(i, logn) + 1)) % (2 * n)
        tab.append(bitrev((raw - 1) >> 1, logn))
    return tab


def switch_key(ct, target, key, primes, psis, L):
    """App. A.8.  ct [2][L][n], target [L][n], key [L_key][2][k][n] (lists of ints). Returns new ct."""
    k = len(primes)
    n = len(target[0])
    P = primes[k - 1]
    mods = list(range(L)) + [k - 1]
    acc = [[[0] * n for _ in mods] for _ in range(2)]
    for i in range(L):
        d = intt_def(target[i], psis[i], primes[i])
        for jj, mi in enumerate(mods):
            m = primes[mi]
            if mi == i:
                x = [int(v) for v in target[i]]
            else:
                x = ntt_def([v % m for v in d], psis[mi], m)
            for c in range(2):
                kr = key[i][c][mi]
                for a in range(n):
                    acc[c][jj][a] += x[a] * int(kr[a])
    out = [[list(map(int, ct[c][j])) for j in range(L)] for c in range(2)]
    half = P >> 1
    for c in range(2):
        u = intt_def([v % P for v in acc[c][L]], psis[k - 1], P)
        u = [(v + half) % P for v in u]
        for j in range(L):
            q = primes[j]
            r = [((v % q) - (half % q)) % q for v in u]
            rh = ntt_def(r, psis[j], q)
            pinv = pow(P % q, -1, q)
            for a in range(n):
                out[c][j][a] = (out[c][j][a] + (acc[c][j][a] - rh[a]) * pinv) % q
    return out


def rescale_floor(ct, primes, psis, L):
    """App. A.9, SEAL 3.4.x floor variant.  ct [size][L][n] -> [size][L-1][n]"""
    last = L - 1
    ql = primes[last]
    out = []
    for poly in ct:
        d = intt_def(poly[last], psis[last], ql)
        rows = []
        for j in range(last):
            q = primes[j]
            x = ntt_def([v % q for v in d], psis[j], q)
            qinv = pow(ql % q, -1, q)
            rows.append([((int(poly[j][a]) - x[a]) * qinv) % q for a in range(len(d))])
        out.append(rows)
    return out


def rescale_round(ct, primes, psis, L):
    """App. A.9, the rounded division (SEAL >= 3.5 divide_and_round_q_last; csrc/hefx_keyswitch.hip K8):
    out_j = (c_j - ([c_l + floor(q_l/2)]_(q_l) mod q_j - (floor(q_l/2) mod q_j))) * q_l^-1 mod q_j,
    i.e. round(c / q_l) in every row.  ct [size][L][n] -> [size][L-1][n]"""
    last = L - 1
    ql = primes[last]
    half = ql >> 1
    out = []
    for poly in ct:
        d = [(v + half) % ql for v in intt_def(poly[last], psis[last], ql)]
        rows = []
        for j in range(last):
            q = primes[j]
            x = ntt_def([(v - half) % q for v in d], psis[j], q)
            qinv = pow(ql % q, -1, q)
            rows.append([((int(poly[j][a]) - x[a]) * qinv) % q for a in range(len(d))])
        out.append(rows)
    return out


def galois_coef(a, elt, q):
    """a(X) -> a(X^elt) in Z_q[X]/(X^n + 1), coefficient domain (X^n = -1)"""
    n = len(a)
    out = [0] * n
    for i, v in enumerate(a):
        e = i * elt % (2 * n)
        if e < n:
            out[e] = (out[e] + int(v)) % q
        else:
            out[e - n] = (out[e - n] - int(v)) % q
    return out


def apply_galois(ct, elt, key, primes, psis, L):
    """App. A.7: each NTT row is taken to the coefficient domain, mapped X -> X^elt there and transformed back (no
    permutation table), then c1's image is key-switched onto c0's.  ct [2][L][n] NTT form."""
    rot = [[ntt_def(galois_coef(intt_def(ct[c][j], psis[j], primes[j]), elt, primes[j]), psis[j], primes[j])
            for j in range(L)] for c in range(2)]
    zero = [[0] * len(rot[0][0]) for _ in range(L)]
    return switch_key([rot[0], zero], rot[1], key, primes, psis, L)
