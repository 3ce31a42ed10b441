"""Shared cases of tests/test_encaps_cpu.py and tests/test_gpu_encaps.py (TEST INFRASTRUCTURE): sparse-secret encapsulation --
the integer statement of hefx_collapse_key / hefx_raise_switch (include/hefx_encaps.h) in Python integers over a backend's
own transforms, the chains, the keys and the noise prediction.

THE CHAINS.  N = 2048, the smallest ring with key switching.
    "wide0"   [60, 50, 50, 50, 60] bits: q_0 > q_j, x mod q_j is a real reduction
    "narrow0" [40, 50, 50, 60] bits:     q_0 < q_j, it is only a sign fix
The end-to-end runs take the chain of tests/bootstrap_cases.py with the sparse plan ns = 16 of tests/sparse_bootstrap_cases.py.

THE KEYS.  The main secret is KeyGenerator(ctx, DENSE_SEED): uniform ternary, DENSE.  The auxiliary secret of the encapsulation
keys has Hamming weight 32 and seed SPARSE_SEED = 7: on the bootstrap chain the integer part I of the raised plaintext of the
tests' ciphertext under it has max |I| = 6 <= 12 = plan.K (asserted by the tests before the end-to-end run).

THE NOISE.  The result of raise_switch, decrypted under s, against mod_raise of the same ciphertext decrypted under s': as centred
coefficients mod q_0 they differ by the key-switch noise.  Predicted deviation
    (q_0 / P) * 3.2 * sqrt(L * N / 12) + sqrt((2 N / 3 + 1) / 12):
the collapsed key's noise (L digits of sigma 3.2) times x (uniform below q_0 / 2 in magnitude: variance q_0^2 / 12) over N
terms, divided by P; and the mod-down's rounding (uniform in [-1/2, 1/2) per polynomial) seen through a uniform ternary secret
(2 N / 3 nonzero entries) plus c0's own.  The bound is NOISE_FACTOR = 8 times that: 94 -> 754 on "wide0" at the top."""
import numpy as np

from tests import bootstrap_cases as BC

N = 2048
CHAINS = {"wide0": [60, 50, 50, 50, 60], "narrow0": [40, 50, 50, 60]}
SCALES = {"wide0": 2.0 ** 50, "narrow0": 2.0 ** 30}
DENSE_SEED = 1
SPARSE_SEED = 7
HAMMING_WEIGHT = 32
NOISE_FACTOR = 8


def make(kind, N_=N, bits=None, galois_steps=(), conjugate=False):
    """BC.make under the DENSE secret, plus `keys` (the encapsulation keys) and `dec_sparse` (a Decryptor under the auxiliary
    secret, rebuilt here from its seed: the generator does not keep it)"""
    from seal_fyp_logistic_regression_amd import seal as S
    e = BC.make(N_, bits, kind, seed=DENSE_SEED, hamming_weight=None, galois_steps=galois_steps, conjugate=conjugate)
    e["keys"] = e["kg"].encapsulation_keys(HAMMING_WEIGHT, seed=SPARSE_SEED)
    e["dec_sparse"] = S.Decryptor(e["ctx"], sparse_secret(e["ctx"], SPARSE_SEED, HAMMING_WEIGHT))
    return e


def sparse_secret(ctx, seed, h):
    from seal_fyp_logistic_regression_amd import seal as S
    be, k = ctx.backend, ctx.k
    coef = S.sparse_ternary_secret(S._key32(seed), ctx.N, h)
    dev = be.from_host(np.stack([(coef % int(q)).astype(np.uint64) for q in ctx.primes[:k]])[None])
    be.ntt_forward(dev, 1, k, 0)
    return S.SecretKey(np.array(be.to_host(dev), dtype=np.uint64).reshape(k, ctx.N), dev)


def context(kind, N_, primes):
    """a bare context over a given prime list (no keys): for word-for-word cases on random operands"""
    from seal_fyp_logistic_regression_amd import seal as S
    from tests.oracle_backend import OracleBackend
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N_)
    parms.set_coeff_modulus([int(p) for p in primes])
    return S.SEALContext.Create(parms, backend=OracleBackend(N_, [int(p) for p in primes]) if kind == "oracle" else None)


def random_operands(N_, primes, seed):
    """(ct [2][1][N] canonical words mod q_0, key [k-1][2][k][N] canonical words): uniform, seeded -- any words are a valid
    input of the integer statement"""
    rng = np.random.default_rng(seed)
    k = len(primes)
    ct = rng.integers(0, int(primes[0]), (2, 1, N_), dtype=np.uint64)
    key = np.empty((k - 1, 2, k, N_), dtype=np.uint64)
    for m, q in enumerate(primes):
        key[:, :, m] = rng.integers(0, int(q), (k - 1, 2, N_), dtype=np.uint64)
    return ct, key


def as_ciphertext(ctx, words, scale=1.0):
    from seal_fyp_logistic_regression_amd import seal as S
    return S.Ciphertext()._set(ctx.backend.from_host(words), 2, 1, scale)


def as_keys(ctx, key):
    from seal_fyp_logistic_regression_amd import seal as S
    return S.EncapsKeys(None, ctx.backend.from_host(key), HAMMING_WEIGHT)


def collapse_model(key, primes, L):
    """hefx_collapse_key's statement in Python integers: [2][L+1][N], rows 0 .. L-1 and the special prime's"""
    k = len(primes)
    key = np.asarray(key).reshape(k - 1, 2, k, -1)
    out = np.empty((2, L + 1, key.shape[3]), dtype=np.uint64)
    for r in range(L + 1):
        m = r if r < L else k - 1
        out[:, r] = (key[:L, :, m].astype(object).sum(axis=0) % int(primes[m])).astype(np.uint64)
    return out


def _fwd(be, m, row):
    return np.asarray(be.to_host(be.ntt_forward(be.from_host(np.asarray(row, dtype=np.uint64)[None, None]), 1, 1, m))).reshape(-1).astype(object)


def _inv(be, m, row):
    return np.asarray(be.to_host(be.ntt_inverse(be.from_host(np.asarray(row, dtype=np.uint64)[None, None]), 1, 1, m))).reshape(-1).astype(object)


def raise_switch_model(be, primes, L, ct, key):
    """hefx_raise_switch's statement, line by line, in Python integers over the backend's own transforms: ct [2][1][N] words,
    key [k-1][2][k][N] (collapsed here) -> [2][L][N]"""
    q = [int(p) for p in primes]
    k, P, half = len(q), q[-1], q[-1] // 2
    kc = collapse_model(key, q, L).astype(object)
    ct = np.asarray(ct).reshape(2, -1)
    c0, c1 = (_inv(be, 0, ct[p]) for p in range(2))
    centred = lambda v: np.where((v > q[0] // 2).astype(bool), v - q[0], v)
    x, y = centred(c1), centred(c0)
    mods = list(range(L)) + [k - 1]
    acc = [[_fwd(be, m, x % q[m]) * kc[c][r] % q[m] for r, m in enumerate(mods)] for c in range(2)]
    out = np.empty((2, L, ct.shape[1]), dtype=np.uint64)
    for c in range(2):
        u = (_inv(be, k - 1, acc[c][L]) + half) % P
        for j in range(L):
            t = (u % q[j] - half % q[j]) % q[j]
            md = (acc[c][j] - _fwd(be, j, t)) * pow(P, -1, q[j]) % q[j]
            if c == 0:
                md = (md + _fwd(be, j, y % q[j])) % q[j]
            out[c, j] = md.astype(np.uint64)
    return out


def predicted_deviation(primes, L, N_):
    q0, P = float(primes[0]), float(primes[-1])
    return (q0 / P) * 3.2 * np.sqrt(L * N_ / 12.0) + np.sqrt((2.0 * N_ / 3.0 + 1.0) / 12.0)


def centred_q0(e, pt):
    """the coefficients of a decrypted plaintext, row 0, as centred integers mod q_0"""
    ctx, be = e["ctx"], e["ctx"].backend
    rows = np.array(be.to_host(pt.data), dtype=np.uint64).reshape(pt.parms_id(), ctx.N)
    q0 = int(ctx.primes[0])
    v = _inv(be, 0, rows[0])
    return np.where((v > q0 // 2).astype(bool), v - q0, v)


def centred_difference(a, b, q0):
    d = (a - b) % q0
    return np.where((d > q0 // 2).astype(bool), d - q0, d)


def input_values(N_=N):
    return np.random.default_rng(11).uniform(-1.0, 1.0, N_ // 2)
