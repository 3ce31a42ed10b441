"""Shared cases of tests/test_hybrid_encaps_cpu.py and tests/test_gpu_hybrid_encaps.py (TEST INFRASTRUCTURE): sparse-secret
encapsulation on hybrid keys -- the integer statement of hefx_hybrid_collapse_key / hefx_hybrid_raise_switch
(include/ext/hefx_hybrid_encaps.h) in Python integers over a backend's own row transforms, written from the header and independent
of seal.py's host code; the sets (tests/hybrid_cases.py's, by import), the inputs, the noise bound and the bootstrap environment.

THE TABLE (set -> the levels L_out).  N = 2048 unless named otherwise: the smallest shapes at which a pass can still go wrong.
    k7a2-p50_60      5, 4, 2   last digit partial, full digits, one digit
    k8a3-d40_s60     5, 2      data primes below 2^40 (the transforms' FP64 policy), q_0 below the specials
    k7a2-d60_s40     5, 2      q_0 above every special prime: the lift must reduce
    k4a1-d60_s40     3, 2      the same at alpha = 1
    k7a2-above60     5         a data prime just above 2^60
    k7a4-p50_60      3, 2      alpha > D, fewer rows than alpha
    k4a1-p50_60      3, 2      alpha = 1: also the words of hefx_collapse_key / hefx_raise_switch
    k18a8-p50_60     10, 8     alpha = HEFX_HYBRID_ALPHA_MAX
    k24a4-top61      20        the digit structure of the bench shape, the largest primes
    n16384, big7     5         N = 16384 and N = 32768, the uniform input only: the large-ring transforms

THE INPUTS, a ciphertext [2][1][N] at q_0 and a key [dnum][2][k][N] (any canonical words are an input of the statement):
    "uniform"   seeded uniform words, the set's random key
    "boundary"  c0 and c1 whose first coefficients are 0, 1, h - 1, h, h + 1, q_0 - 1 (h = floor(q_0 / 2): both sides of the
                lift's rule), the rest uniform, taken to NTT form by the twin; the set's random key
    "maxkey"    the uniform ciphertext on the key whose every word is q_m - 1

THE NOISE BOUND, the header's: dec_s(out) - (y + x s'), centred mod Q_L, has infinity norm at most
    B = ceil(ceil(L/alpha) * N * 19 * floor(q_0/2) / P) + alpha * (1 + N).

THE BOOTSTRAP.  The chain of tests/hybrid_bsgs_cases.boot_primes(), alpha = 2, ns = 16, the main secret KeyGenerator(ctx,
BC.KEY_SEED) WITHOUT hamming_weight: dense.  The auxiliary secret has Hamming weight 32 and seed AUX_SEED = 7: on this chain the
raised plaintext of the tests' ciphertext under it has max |I| = 6 <= 12 = plan.K (asserted by the tests before the run)."""
import numpy as np

from tests import hybrid_cases as HC

TABLE = {"k7a2-p50_60": (5, 4, 2), "k8a3-d40_s60": (5, 2), "k7a2-d60_s40": (5, 2), "k4a1-d60_s40": (3, 2), "k7a2-above60": (5,),
         "k7a4-p50_60": (3, 2), "k4a1-p50_60": (3, 2), "k18a8-p50_60": (10, 8), "k24a4-top61": (20,), "n16384": (5,), "big7": (5,)}
INPUTS = ("uniform", "boundary", "maxkey")
ALPHA_ONE = ("k4a1-p50_60", "k4a1-d60_s40")
NOISE_SETS = ("k7a2-p50_60", "k8a3-d40_s60")
SEED = 23
AUX_SEED = 7
AUX_MAX_I = 6          # measured on the twin for AUX_SEED on the bootstrap chain (the tests assert it is <= plan.K)
HAMMING_WEIGHT = 32


def sets():
    return {name: HC.sets()[name] for name in TABLE}


def inputs_of(s):
    return INPUTS if s.N == HC.N else ("uniform",)


def rows_of(primes, alpha, L):
    """m(r) for the R = L + alpha rows"""
    k = len(primes)
    return list(range(L)) + list(range(k - alpha, k))


def word_cases():
    """[(set name, L, input)] over the whole table"""
    return [(name, L, kind) for name, levels in TABLE.items() for L in levels for kind in inputs_of(HC.sets()[name])]


def case_id(case):
    return f"{case[0]}-L{case[1]}-{case[2]}"


_INPUT = {}


def uniform_ct(s, seed):
    return np.random.default_rng(seed).integers(0, s.primes[0], (2, 1, s.N), dtype=np.uint64)


def boundary_ct(s, seed):
    q0 = s.primes[0]
    h = q0 // 2
    coef = np.random.default_rng(seed).integers(0, q0, (2, s.N), dtype=np.uint64)
    coef[0, :6] = [0, 1, h - 1, h, h + 1, q0 - 1]
    coef[1, :6] = [q0 - 1, h + 1, h, h - 1, 1, 0]
    be = HC.twin(s)
    return np.stack([HC._fwd(be, 0, coef[p], q0).astype(np.uint64) for p in range(2)])[:, None, :]


def case_input(s, kind, side=0):
    """(ct [2][1][N], key [dnum][2][k][N]); side 1: the decoys of the stream-order cases (other seeds, same kinds)"""
    key_ = (s.name, kind, side)
    if key_ not in _INPUT:
        seed = SEED + 100 * side
        ct = boundary_ct(s, seed + 1) if kind == "boundary" else uniform_ct(s, seed)
        key = HC.max_key(s) if kind == "maxkey" else HC.random_key(s, seed + 2)
        _INPUT[key_] = (ct, key)
    return _INPUT[key_]


# ---------------------------------------------------------------------------------------------------------------------
# the statement of include/ext/hefx_hybrid_encaps.h
# ---------------------------------------------------------------------------------------------------------------------
def collapse_model(key, primes, alpha, L):
    """out[c][r] = sum_{j < ceil(L/alpha)} key[j][c][m(r)] mod q_m(r): [2][L + alpha][N]"""
    q = [int(p) for p in primes]
    key = np.asarray(key)
    key = key.reshape(-1, 2, len(q), key.shape[-1])
    dn = (L + alpha - 1) // alpha
    out = np.empty((2, L + alpha, key.shape[3]), dtype=np.uint64)
    for r, m in enumerate(rows_of(q, alpha, L)):
        out[:, r] = (key[:dn, :, m].astype(object).sum(axis=0) % q[m]).astype(np.uint64)
    return out


def centred_lift(be, q0, row):
    """the integer polynomial an NTT row at q_0 stands for: v <= floor(q_0 / 2) -> v, otherwise v - q_0"""
    v = HC._inv(be, 0, row)
    return np.where((v > q0 // 2).astype(bool), v - q0, v)


def raise_switch_model(be, primes, alpha, L, ct, ckey):
    """the statement, line by line: ct [2][1][N] words, ckey [2][L + alpha][N] -> [2][L][N]"""
    q = [int(p) for p in primes]
    k = len(q)
    S = list(range(k - alpha, k))
    rows = rows_of(q, alpha, L)
    P = int(np.prod([q[t] for t in S], dtype=object))
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, -1)
    n = ct.shape[1]
    ckey = np.asarray(ckey, dtype=np.uint64).reshape(2, L + alpha, n).astype(object)
    y, x = centred_lift(be, q[0], ct[0]), centred_lift(be, q[0], ct[1])                       # the lift
    xn = {m: ct[1].astype(object) if m == 0 else HC._fwd(be, m, x, q[m]) for m in rows}       # row 0: the input's own row
    acc = {(c, m): xn[m] * ckey[c, r] % q[m] for c in range(2) for r, m in enumerate(rows)}   # the product
    half = P // 2
    out = np.empty((2, L, n), dtype=np.uint64)
    for c in range(2):                                                                        # the mod-down
        z = {}
        for t in S:
            u = (HC._inv(be, t, acc[c, t].astype(np.uint64)) + half % q[t]) % q[t]
            z[t] = u * pow(P // q[t] % q[t], -1, q[t]) % q[t]
        for j in range(L):
            v = sum(z[t] * (P // q[t] % q[j]) for t in S) % q[j]
            tj = (v - half % q[j]) % q[j]
            ks = (acc[c, j] - HC._fwd(be, j, tj, q[j])) * pow(P % q[j], -1, q[j]) % q[j]
            if c == 0:                                                                        # the result
                ks = (ks + (ct[0].astype(object) if j == 0 else HC._fwd(be, j, y, q[j]))) % q[j]
            out[c, j] = ks.astype(np.uint64)
    return out


_MODEL = {}


def case_model(case, side=0):
    """(the collapsed key, the output) of a word case by the model on the oracle twin, once per process"""
    key_ = (case, side)
    if key_ not in _MODEL:
        name, L, kind = case
        s = HC.sets()[name]
        ct, key = case_input(s, kind, side)
        ckey = collapse_model(key, s.primes, s.alpha, L)
        _MODEL[key_] = (ckey, raise_switch_model(HC.twin(s), s.primes, s.alpha, L, ct, ckey))
    return _MODEL[key_]


def noise_bound(s, L):
    """(B, Q_L) as exact integers (B rounded up): the header's bound"""
    q = s.primes
    P = int(np.prod(q[s.k - s.alpha:], dtype=object))
    dn = (L + s.alpha - 1) // s.alpha
    B = -(-(dn * s.N * 19 * (q[0] // 2)) // P) + s.alpha * (1 + s.N)
    return B, int(np.prod(q[:L], dtype=object))


# ---------------------------------------------------------------------------------------------------------------------
# the stream-order cases (tests/stream_ext_cases.Case): real operands and decoys of the same kinds from other seeds
# ---------------------------------------------------------------------------------------------------------------------
STREAM_CASES = [("k8a3-d40_s60", 5, "uniform"), ("big7", 5, "uniform")]


def stream_cases(case):
    """(collapse, raise_switch) under the decoy protocol.  hefx_hybrid_raise_switch reads the collapsed key that the collapse
    case writes on the same stream just before: its call takes that buffer as a fifth argument; until the stream runs the buffer
    holds the collapse case's output decoy."""
    from tests import stream_ext_cases as SX
    name, L, kind = case
    s = HC.sets()[name]
    (cr, kr), (cd, kd) = case_input(s, kind, 0), case_input(s, kind, 1)
    (ckr, outr), (ckd, outd) = case_model(case, 0), case_model(case, 1)
    dn = (L + s.alpha - 1) // s.alpha
    collapse = SX.Case(f"hybrid_collapse_key at {name}, L = {L}", "hefx_hybrid_collapse_key", [kr[:dn]], [kd[:dn]], [ckr], [ckd],
                       lambda e, i, t, st: e.hybrid_collapse_key(s.alpha, L, i[0], out=t[0], stream=st))
    rs = SX.Case(f"hybrid_raise_switch at {name}, L = {L}", "hefx_hybrid_raise_switch", [cr], [cd], [outr], [outd],
                 lambda e, i, t, st, ckey: e.hybrid_raise_switch(s.alpha, L, i[0], ckey, out=t[0], stream=st))
    return collapse, rs


# ---------------------------------------------------------------------------------------------------------------------
# the bootstrap under a dense secret on hybrid keys
# ---------------------------------------------------------------------------------------------------------------------
_BOOT = {}


def boot_env(kind):
    """tests/hybrid_bsgs_cases.boot_env's sparse environment with a DENSE main secret (no hamming_weight) and e["keys"], the
    hybrid encapsulation keys of AUX_SEED; e["dec_sparse"]: a Decryptor under the auxiliary secret, rebuilt from its seed"""
    from seal_fyp_logistic_regression_amd import bootstrap
    from seal_fyp_logistic_regression_amd import seal as S
    from tests import bootstrap_cases as BC
    from tests import encaps_cases as EC
    from tests import hybrid_bsgs_cases as HB
    if kind not in _BOOT:
        ctx = EC.context(kind, BC.N, HB.boot_primes())
        kg = S.KeyGenerator(ctx, BC.KEY_SEED)
        plan = bootstrap.plan(BC.N, ctx.primes, BC.SCALE, slots=HB.BOOT_NS, special=HB.BOOT_ALPHA)
        e = dict(ctx=ctx, kg=kg, enc=S.Encryptor(ctx, kg.public_key(), BC.KEY_SEED + 1), dec=S.Decryptor(ctx, kg.secret_key()),
                 encoder=S.CKKSEncoder(ctx, device_encode=False), ev=S.Evaluator(ctx), plan=plan)
        e.update(hgk=kg.hybrid_galois_keys(HB.BOOT_ALPHA, plan.galois_steps(), conjugate=True), hrk=kg.hybrid_relin_keys(HB.BOOT_ALPHA),
                 encoded=plan.encode(e["encoder"], extended=True),
                 keys=kg.hybrid_encapsulation_keys(HB.BOOT_ALPHA, HAMMING_WEIGHT, seed=AUX_SEED))
        _BOOT[kind] = e
    return _BOOT[kind]


def boot_input(e):
    from tests import bootstrap_cases as BC
    from tests import hybrid_bsgs_cases as HB
    from tests import sparse_bootstrap_cases as SC
    v = SC.sparse_input(HB.BOOT_NS)
    return v, e["enc"].encrypt(e["encoder"].encode(SC.tiled(v), BC.SCALE, parms_id=1))


def dense(e):
    """does the main secret have more than N / 2 nonzero coefficients?"""
    be = e["ctx"].backend
    coef = np.asarray(be.to_host(be.ntt_inverse(be.from_host(e["kg"].secret_key().host[:1].copy()), 1, 1, 0))).reshape(-1)
    return np.count_nonzero(coef) > e["ctx"].N // 2
