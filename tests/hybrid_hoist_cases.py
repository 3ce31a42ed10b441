"""Shared cases of tests/test_hybrid_hoist_cpu.py and tests/test_gpu_hybrid_hoist.py (TEST INFRASTRUCTURE): hoisted hybrid key
switching -- the integer statement of include/hefx_hybrid_hoist.h in Python integers over the oracle twin's row transforms,
written from the header and independent of seal.py's host code, and the operands of the word cases.  Sets, operands, keys and
the noise bound are those of tests/hybrid_cases.py."""
import numpy as np

from tests import hybrid_cases as HC


def _consts(primes, alpha, L):
    q = [int(p) for p in primes]
    k = len(q)
    S = list(range(k - alpha, k))
    P = int(np.prod([q[t] for t in S], dtype=object))
    return q, k, S, list(range(L)) + S, P


def digits_model(be, primes, alpha, L, c1):
    """E[j][m] for m in R: steps 1-3 of hefx_hybrid.h on x = c1 ([L][N], NTT form), NOT permuted; c1's own row inside the digit"""
    q, k, S, rows, P = _consts(primes, alpha, L)
    c1 = np.asarray(c1, dtype=np.uint64).reshape(L, -1)
    xt = [HC._inv(be, i, c1[i]) for i in range(L)]
    E = []
    for G in HC.digits(alpha, L):
        Dj = int(np.prod([q[i] for i in G], dtype=object))
        y = {i: xt[i] * pow(Dj // q[i] % q[i], -1, q[i]) % q[i] for i in G}
        E.append({m: c1[m].astype(object) if m in G else HC._fwd(be, m, sum(y[i] * (Dj // q[i] % q[m]) for i in G) % q[m], q[m])
                  for m in rows})
    return E


def term_model(primes, alpha, L, ct, E, elt, key):
    """A[c, m] for m in R; key None: the identity term (element 1)"""
    q, k, S, rows, P = _consts(primes, alpha, L)
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, L, -1)
    n = ct.shape[2]
    if key is None:
        assert elt == 1
        return {(c, m): ct[c, m].astype(object) * (P % q[m]) % q[m] if m < L else np.zeros(n, dtype=object) for c in range(2) for m in rows}
    key = np.asarray(key, dtype=np.uint64).reshape(-1, 2, k, n)
    A = {}
    for c in range(2):
        for m in rows:
            acc = np.zeros(n, dtype=object)
            for j in range(len(E)):
                acc = (acc + HC.gather(n, elt, E[j][m]) * key[j, c, m].astype(object)) % q[m]
            if c == 0 and m < L:
                acc = (acc + (P % q[m]) * HC.gather(n, elt, ct[0, m]).astype(object)) % q[m]
            A[c, m] = acc
    return A


def mod_down_model(be, primes, alpha, L, B):
    """step 5 of hefx_hybrid.h on the pair B[c, m], m in R -> [2][L][N] uint64"""
    q, k, S, rows, P = _consts(primes, alpha, L)
    half = P // 2
    n = len(B[0, 0])
    out = np.empty((2, L, n), dtype=np.uint64)
    for c in range(2):
        z = {}
        for t in S:
            u = (HC._inv(be, t, (B[c, t] % q[t]).astype(np.uint64)) + half % q[t]) % q[t]
            z[t] = u * pow(P // q[t] % q[t], -1, q[t]) % q[t]
        for j in range(L):
            v = sum(z[t] * (P // q[t] % q[j]) for t in S) % q[j]
            tj = (v - half % q[j]) % q[j]
            out[c, j] = ((B[c, j] - HC._fwd(be, j, tj, q[j])) * pow(P % q[j], -1, q[j]) % q[j]).astype(np.uint64)
    return out


def terms_model(be, primes, alpha, L, cts, elts, keys):
    """A_t for t = i m + k"""
    out = []
    for ct in cts:
        ct = np.asarray(ct, dtype=np.uint64).reshape(2, L, -1)
        E = digits_model(be, primes, alpha, L, ct[1])
        out += [term_model(primes, alpha, L, ct, E, elt, key) for elt, key in zip(elts, keys)]
    return out


def rotate_model(be, primes, alpha, L, cts, elts, keys):
    """the n m hoisted rotations, [i m + k] = [2][L][N]"""
    return [mod_down_model(be, primes, alpha, L, A) for A in terms_model(be, primes, alpha, L, cts, elts, keys)]


def combine_model(be, primes, alpha, L, cts, elts, keys, pts):
    """pts[o][t] = [k][N] or None -> the G outputs"""
    q, k, S, rows, P = _consts(primes, alpha, L)
    terms = terms_model(be, primes, alpha, L, cts, elts, keys)
    outs = []
    for row in pts:
        assert len(row) == len(terms) and any(p is not None for p in row)
        B = {}
        for c in range(2):
            for m in rows:
                acc = 0
                for p, A in zip(row, terms):
                    if p is not None:
                        acc = (acc + np.asarray(p)[m].astype(object) * A[c, m]) % q[m]
                B[c, m] = acc
        outs.append(mod_down_model(be, primes, alpha, L, B))
    return outs


# ---------------------------------------------------------------------------------------------------------------------
# the word cases of both entries: n = 2 sources, the elements {1 with no key, 3, 2N - 1}, G = 2 with one structural zero per row
# ---------------------------------------------------------------------------------------------------------------------
def plaintext(s, kind, seed):
    """[k][N] canonical words: uniform, or every word q_m - 1, or the constant 1"""
    rng = np.random.default_rng(seed)
    out = np.empty((s.k, s.N), dtype=np.uint64)
    for m, q in enumerate(s.primes):
        out[m] = q - 1 if kind == "max" else 1 if kind == "one" else rng.integers(0, q, s.N, dtype=np.uint64)
    return out


def case(s, L, kind="uniform"):
    """(cts [2 sources], elts, keys (host arrays or None), pts [2][6])"""
    cts = [HC.operand(s, kind, L, 2, seed=HC.SEED + 31 * L + i) for i in range(2)]
    elts = [1, 3, 2 * s.N - 1]
    keys = [None, HC.case_key(s, kind if kind == "max" else "uniform"), HC.random_key(s, HC.SEED + 1)]
    pts = [[plaintext(s, kind, 100 * L + 6 * o + t) for t in range(6)] for o in range(2)]
    pts[0][4] = None
    pts[1][0] = None
    return cts, elts, keys, pts


_MODEL = {}


def case_models(s, L, kind="uniform"):
    """(the 6 rotations, the 2 combined outputs) of case(s, L, kind), once per process"""
    key_ = (s.name, L, kind)
    if key_ not in _MODEL:
        cts, elts, keys, pts = case(s, L, kind)
        be = HC.twin(s)
        terms = terms_model(be, s.primes, s.alpha, L, cts, elts, keys)
        q, k, S, rows, P = _consts(s.primes, s.alpha, L)
        rot = [mod_down_model(be, s.primes, s.alpha, L, A) for A in terms]
        comb = []
        for row in pts:
            B = {(c, m): sum(p[m].astype(object) * A[c, m] for p, A in zip(row, terms) if p is not None) % q[m] for c in range(2) for m in rows}
            comb.append(mod_down_model(be, s.primes, s.alpha, L, B))
        _MODEL[key_] = (rot, comb)
    return _MODEL[key_]


def full_case(s, L):
    """the accumulator at its bound: 64 terms (n = 8 sources of the max operand, m = 8 elements, every key the max key) and one
    output whose 64 plaintexts are all q_m - 1.  Every source is the same words and there are two distinct elements, so the
    model computes two terms: (cts, elts, keys, pts, the model's output)."""
    ct = HC.operand(s, "max", L, 2, seed=0)
    key = HC.max_key(s)
    elts = [3, 2 * s.N - 1] * 4
    pt = plaintext(s, "max", 0)
    key_ = (s.name, L, "full")
    if key_ not in _MODEL:
        be = HC.twin(s)
        q, k, S, rows, P = _consts(s.primes, s.alpha, L)
        two = terms_model(be, s.primes, s.alpha, L, [ct], elts[:2], [key, key])
        B = {(c, m): 32 * sum(pt[m].astype(object) * A[c, m] for A in two) % q[m] for c in range(2) for m in rows}
        _MODEL[key_] = mod_down_model(be, s.primes, s.alpha, L, B)
    return [ct] * 8, elts, [key] * 8, [[pt] * 64], _MODEL[key_]


# ---------------------------------------------------------------------------------------------------------------------
# the hybrid DFT: the plans of both test files on k7a2-p50_60, on the oracle twin or on the engine (same seeds, same words)
# ---------------------------------------------------------------------------------------------------------------------
DFT_SET = "k7a2-p50_60"
DFT_LEVELS = 2
DFT_SCALE = 2.0 ** 40
KEY_SEED = 3
_DFT = {}


def dft_env(kind):
    """N = 2048: the ciphertext starts at level k - alpha = 5; CoeffToSlot takes DFT_LEVELS = 2 levels, SlotToCoeff two more (the
    dense plans of two stages: radix 32, a few seconds on the CPU), and the packed plans (ns = 16, two levels each) run the same
    chain.  kind: "oracle" or "gpu"."""
    from seal_fyp_logistic_regression_amd import dft
    from seal_fyp_logistic_regression_amd import seal as S
    if kind not in _DFT:
        s = HC.sets()[DFT_SET]
        ctx = HC.context(s, kind)
        kg = S.KeyGenerator(ctx, KEY_SEED)
        top, q, N = s.k - s.alpha, ctx.primes, s.N
        drop = lambda L: [q[L - 1 - i] for i in range(DFT_LEVELS)]
        plans = {"c2s": dft.plan(N, DFT_LEVELS, dft.C2S, drop(top)), "s2c": dft.plan(N, DFT_LEVELS, dft.S2C, drop(top - DFT_LEVELS)),
                 "pc2s": dft.plan_packed(N, 16, 2, dft.C2S, drop(top)), "ps2c": dft.plan_packed(N, 16, 2, dft.S2C, drop(top - 2))}
        steps = sorted({st for p in plans.values() for st in p.galois_steps()})
        _DFT[kind] = dict(s=s, ctx=ctx, kg=kg, ev=S.Evaluator(ctx), gk=kg.hybrid_galois_keys(s.alpha, steps, conjugate=True), plans=plans,
                          top=top, enc=S.Encryptor(ctx, kg.public_key(), KEY_SEED + 1), dec=S.Decryptor(ctx, kg.secret_key()),
                          encoder=S.CKKSEncoder(ctx, device_encode=False))
    return _DFT[kind]


def dft_program(e, which):
    """(the hybrid round trip as a function of the input ciphertext that returns (CoeffToSlot's results, the final ciphertext),
    the two plans, the input values, the values plan.apply expects) of the "dense" or the "packed" plans"""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    ev, gk, plans, n = e["ev"], e["gk"], e["plans"], e["s"].N // 2
    rng = np.random.default_rng(2026)
    if which == "dense":
        z = np.sqrt(rng.uniform(0, 1, n)) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
        c2s, s2c = plans["c2s"], plans["s2c"]

        def hybrid(ct):
            a, b = alg.coeffs_to_slots_hybrid(ev, ct, c2s, gk)
            return (a, b), alg.slots_to_coeffs_hybrid(ev, a, b, s2c, gk)
    else:
        z = np.tile(np.sqrt(rng.uniform(0, 1, 16)) * np.exp(2j * np.pi * rng.uniform(0, 1, 16)), n // 16)
        c2s, s2c = plans["pc2s"], plans["ps2c"]

        def hybrid(ct):
            mid = alg.coeffs_to_slots_packed_hybrid(ev, ct, c2s, gk)
            return (mid,), alg.slots_to_coeffs_packed_hybrid(ev, mid, s2c, gk)
    return hybrid, c2s, s2c, z, s2c.apply(c2s.apply([z]))[0]
