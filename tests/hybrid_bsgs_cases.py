"""Shared cases of tests/test_hybrid_bsgs_cpu.py and tests/test_gpu_hybrid_bsgs.py (TEST INFRASTRUCTURE): the hoisted giant
steps -- the integer statement of include/hefx_hybrid_bsgs.h in Python integers over the oracle twin's row transforms, written
from the header over the pieces of tests/hybrid_cases.py and tests/hybrid_hoist_cases.py (digits_model, terms_model,
mod_down_model, gather) and independent of seal.py's host code; the operands of the word cases; the environment of the
EvalMod and bootstrap tests."""
import numpy as np

from tests import hybrid_cases as HC
from tests import hybrid_hoist_cases as HH


def sums_model(primes, alpha, L, terms, pts):
    """B_o[c, m] for m in R: the combine's sums of hefx_hybrid_hoist.h, before any mod-down"""
    q, k, S, rows, P = HH._consts(primes, alpha, L)
    out = []
    for row in pts:
        assert len(row) == len(terms) and any(p is not None for p in row)
        out.append({(c, m): sum(np.asarray(p)[m].astype(object) * A[c, m] for p, A in zip(row, terms) if p is not None) % q[m]
                    for c in range(2) for m in rows})
    return out


def giant_model(be, primes, alpha, L, B, elt, key):
    """W_o[c, m] for m in R of one inner sum B with the giant element elt and key (None: W_o = B_o, the element must be 1)"""
    q, k, S, rows, P = HH._consts(primes, alpha, L)
    if key is None:
        assert elt == 1
        return B
    n = len(B[0, 0])
    key = np.asarray(key, dtype=np.uint64).reshape(-1, 2, k, n)
    # d_o = MD(B_o[1]): step 5 on that ONE polynomial (mod_down_model takes a pair: B_o[1] stands in both places)
    d = HH.mod_down_model(be, primes, alpha, L, {(c, m): B[1, m] for c in range(2) for m in rows})[1]
    F = HH.digits_model(be, primes, alpha, L, d)
    W = {}
    for c in range(2):
        for m in rows:                                             # EVERY row of R, the special rows included
            acc = np.zeros(n, dtype=object)
            for j in range(len(F)):
                acc = (acc + HC.gather(n, elt, F[j][m]) * key[j, c, m].astype(object)) % q[m]
            if c == 0:
                acc = (acc + HC.gather(n, elt, B[0, m])) % q[m]    # no factor P: B_o[0] carries it
            W[c, m] = acc
    return W


def outputs_model(be, primes, alpha, L, Ws, dest, weights=None):
    """out[q] = MD(sum over dest[o] == q of weights[o] W_o) (weights: how many equal inner sums a W stands for)"""
    q, k, S, rows, P = HH._consts(primes, alpha, L)
    O = max(dest) + 1
    assert set(dest) == set(range(O))
    weights = weights or [1] * len(Ws)
    outs = []
    for out in range(O):
        acc = {(c, m): sum(w * W[c, m] for W, d, w in zip(Ws, dest, weights) if d == out) % q[m] for c in range(2) for m in rows}
        outs.append(HH.mod_down_model(be, primes, alpha, L, acc))
    return outs


def bsgs_model(be, primes, alpha, L, cts, elts, keys, pts, giant_elts, giant_keys, dest):
    """the statement: the O outputs, [2][L][N] each"""
    sums = sums_model(primes, alpha, L, HH.terms_model(be, primes, alpha, L, cts, elts, keys), pts)
    Ws = [giant_model(be, primes, alpha, L, B, g, K) for B, g, K in zip(sums, giant_elts, giant_keys)]
    return outputs_model(be, primes, alpha, L, Ws, list(dest))


# ---------------------------------------------------------------------------------------------------------------------
# the word cases: 2 sources, the baby elements {1 with no key, 3, 2N - 1}, G = 4 inner sums with one structural zero each, O = 2
# outputs; each output has one inner sum without a giant rotation and one rotated, by the giant elements 3 and 2N - 1
# ---------------------------------------------------------------------------------------------------------------------
WORD_CASES = [("k7a2-p50_60", 5), ("k7a2-p50_60", 4), ("k7a2-p50_60", 3), ("k8a3-above60", 5), ("k7a4-d40_s60", 3), ("k4a1-p50_60", 3),
              ("k12a5-p50_60", 7), ("big", 2)]
KINDS = ("uniform", "max")
DEST = [0, 1, 1, 0]


def case(s, L, kind="uniform"):
    """(cts, elts, keys, pts [4][6], giant_elts, giant_keys, dest)"""
    cts, elts, keys, _ = HH.case(s, L, kind)
    pts = [[HH.plaintext(s, kind, 1000 * L + 6 * o + t) for t in range(6)] for o in range(4)]
    pts[0][4] = pts[1][0] = pts[2][3] = pts[3][1] = None
    giant_elts = [1, 3, 1, 2 * s.N - 1]
    if kind == "max":
        giant_keys = [None, HC.max_key(s), None, HC.max_key(s)]
    else:
        giant_keys = [None, HC.random_key(s, HC.SEED + 2), None, HC.random_key(s, HC.SEED + 3)]
    return cts, elts, keys, pts, giant_elts, giant_keys, list(DEST)


_MODEL = {}


def case_model(s, L, kind="uniform"):
    """the 2 outputs of case(s, L, kind), once per process"""
    key_ = (s.name, L, kind)
    if key_ not in _MODEL:
        _MODEL[key_] = bsgs_model(HC.twin(s), s.primes, s.alpha, L, *case(s, L, kind))
    return _MODEL[key_]


def full_case(s, L):
    """the accumulator at its bound: G = 64 inner sums into ONE output, each giant-rotated with the max key, alternately by 3
    and 2N - 1; one source of the max operand, the baby elements 3 and 2N - 1 with the max key, every plaintext q_m - 1.  All
    inner sums are the same words and there are two giant elements, so the model computes two W:
    (cts, elts, keys, pts, giant_elts, giant_keys, dest, the model's output)."""
    ct, key, pt = HC.operand(s, "max", L, 2, seed=0), HC.max_key(s), HH.plaintext(s, "max", 0)
    elts, gelts = [3, 2 * s.N - 1], [3, 2 * s.N - 1] * 32
    key_ = (s.name, L, "full")
    if key_ not in _MODEL:
        be = HC.twin(s)
        (B,) = sums_model(s.primes, s.alpha, L, HH.terms_model(be, s.primes, s.alpha, L, [ct], elts, [key, key]), [[pt, pt]])
        Ws = [giant_model(be, s.primes, s.alpha, L, B, g, key) for g in gelts[:2]]
        _MODEL[key_] = outputs_model(be, s.primes, s.alpha, L, Ws, [0, 0], [32, 32])[0]
    return [ct], elts, [key, key], [[pt, pt]] * 64, gelts, [key] * 64, [0] * 64, _MODEL[key_]


# ---------------------------------------------------------------------------------------------------------------------
# EvalMod and the bootstrap on hybrid keys: [60] + [50] * 13 + [60, 60] bits at N = 2048, alpha = 2, scale 2^50, the secret of
# tests/bootstrap_cases.py (Hamming weight 32, seed 1); on the oracle twin or on the engine (same seeds, same words)
# ---------------------------------------------------------------------------------------------------------------------
BOOT_BITS = [60] + [50] * 13 + [60, 60]
BOOT_ALPHA = 2
BOOT_NS = 16
_BOOT = {}


def boot_primes():
    """the 15 primes of tests/bootstrap_cases.py's chain and one more 60-bit prime behind them: the 14 data primes are those of
    the one-special-prime bootstrap the tests compare with"""
    from seal_fyp_logistic_regression_amd import seal as S
    from tests import bootstrap_cases as BC
    base = [int(p) for p in S.CoeffModulus.Create(BC.N, BC.CHAIN_BITS)]
    more = [int(p) for p in S.CoeffModulus.Create(BC.N, [60, 60, 60]) if int(p) not in base]
    assert [p.bit_length() for p in base + more[:1]] == BOOT_BITS
    return base + more[:1]


def boot_env(kind, sparse=True):
    """the environment of BC.make on the alpha = 2 chain, on `kind` ("oracle" or "gpu"), with e["plan"] = bootstrap.plan(...,
    special=2) (sparse: ns = 16, else dense), e["hgk"], e["hrk"] its hybrid Galois and relinearisation keys and e["encoded"]
    the plan's key-level diagonals"""
    from seal_fyp_logistic_regression_amd import bootstrap
    from seal_fyp_logistic_regression_amd import seal as S
    from tests import bootstrap_cases as BC
    from tests import encaps_cases as EC
    key_ = (kind, sparse)
    if key_ not in _BOOT:
        ctx = EC.context(kind, BC.N, boot_primes())
        kg = S.KeyGenerator(ctx, BC.KEY_SEED, hamming_weight=BC.HAMMING_WEIGHT)
        plan = bootstrap.plan(BC.N, ctx.primes, BC.SCALE, slots=BOOT_NS if sparse else None, special=BOOT_ALPHA)
        e = dict(ctx=ctx, kg=kg, enc=S.Encryptor(ctx, kg.public_key(), BC.KEY_SEED + 1), dec=S.Decryptor(ctx, kg.secret_key()),
                 encoder=S.CKKSEncoder(ctx, device_encode=False), ev=S.Evaluator(ctx), plan=plan)
        e.update(hgk=kg.hybrid_galois_keys(BOOT_ALPHA, plan.galois_steps(), conjugate=True), hrk=kg.hybrid_relin_keys(BOOT_ALPHA),
                 encoded=plan.encode(e["encoder"], extended=True))
        _BOOT[key_] = e
    return _BOOT[key_]
