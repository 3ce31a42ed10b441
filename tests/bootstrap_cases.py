"""Shared cases of tests/test_bootstrap_cpu.py and tests/test_gpu_bootstrap.py (TEST INFRASTRUCTURE): the integer statement
of hefx_product_combine (include/hefx_bootstrap.h), the bootstrap chain and its inputs, and the environment builder.

THE CHAIN.  N = 2048, primes of [60, 50 x 13, 60] bits, scale 2^50: q_0 / scale = 2^10 (the sine's own error: 6e-6 relative),
2 + 5 + 3 + 2 levels spent, one left above the bottom.  The 40-bit stages the issue suggests were measured on the oracle twin at
1.2e-2 of the largest expected value (cap 1e-3): an error e of EvalMod reaches the message as e q_0 / (2 pi scale) = 163 e and an
error of CoeffToSlot as 2 pi K' 163 = 12500 times itself, so the rescale noise at 40 bits is too much; at 50 bits the twin
decodes to 1.2e-5.  DESIGN.md, "Bootstrapping", has the figures.

THE KEY.  Hamming weight 32, seed KEY_SEED = 1: the integer part I of the mod-raised plaintext of the test's ciphertext has
max |I| = 6 (required <= 12 = plan.K, checked by the tests before anything else)."""
import numpy as np

N = 2048
CHAIN_BITS = [60] + [50] * 13 + [60]
SCALE = 2.0 ** 50
KEY_SEED = 1
HAMMING_WEIGHT = 32
CAP = 1e-3   # the project's DFT gate: decode error as a fraction of the largest expected value


def evalmod_interpolant(degree, r, K=12):
    """Chebyshev coefficients of g(u) = cos(2 pi (K' u - 1/4) / 2^r) on [-1, 1], K' = K + 1/4: the issue's interpolant"""
    k = np.arange(degree + 1)
    nodes = np.cos(np.pi * (k + 0.5) / (degree + 1))
    return np.polynomial.chebyshev.chebfit(nodes, np.cos(2.0 * np.pi * ((K + 0.25) * nodes - 0.25) / 2.0 ** r), degree)


def product_model(As, Bs, lins, ures, wres, cres, L, primes):
    """the header's statement in Python integers for ONE item: As[p], Bs[p] [2][rows][N], lins[k] [2][rows][N]; ures [P][L],
    wres [m][L], cres [L] or None -> [3][L][N]"""
    Nn = As[0].shape[2]
    out = np.empty((3, L, Nn), dtype=np.uint64)
    for j in range(L):
        c0 = np.zeros(Nn, dtype=object) + (int(cres[j]) if cres is not None else 0)
        c1, c2 = np.zeros(Nn, dtype=object), np.zeros(Nn, dtype=object)
        for p, (a, b) in enumerate(zip(As, Bs)):
            u = int(ures[p][j])
            a0, a1, b0, b1 = (x.astype(object) for x in (a[0, j], a[1, j], b[0, j], b[1, j]))
            c0 = c0 + u * a0 * b0
            c1 = c1 + u * (a0 * b1 + a1 * b0)
            c2 = c2 + u * a1 * b1
        for k, l in enumerate(lins):
            w = int(wres[k][j])
            c0 = c0 + w * l[0, j].astype(object)
            c1 = c1 + w * l[1, j].astype(object)
        q = int(primes[j])
        out[0, j], out[1, j], out[2, j] = (c0 % q).astype(np.uint64), (c1 % q).astype(np.uint64), (c2 % q).astype(np.uint64)
    return out


def make(N_, bits, backend_kind, seed=KEY_SEED, hamming_weight=None, galois_steps=(), conjugate=False):
    """context, keys and tools on the HIP engine ("gpu") or the oracle-backed twin ("oracle"); galois_steps=() makes no Galois
    key"""
    import os
    from seal_fyp_logistic_regression_amd import seal as S
    from tests.oracle_backend import OracleBackend
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N_)
    parms.set_coeff_modulus(S.CoeffModulus.Create(N_, bits))
    backend = OracleBackend(N_, parms.coeff_modulus()) if backend_kind == "oracle" else None
    ctx = S.SEALContext.Create(parms, backend=backend)
    assert ctx.backend.rescale_rounded == (os.environ.get("HEFX_RESCALE", "round") != "floor"), backend_kind
    kg = S.KeyGenerator(ctx, seed, hamming_weight=hamming_weight)
    gk = kg.galois_keys(list(galois_steps), conjugate=conjugate) if (galois_steps or conjugate) else None
    return dict(ctx=ctx, kg=kg, enc=S.Encryptor(ctx, kg.public_key(), seed + 1), dec=S.Decryptor(ctx, kg.secret_key()),
                encoder=S.CKKSEncoder(ctx, device_encode=False), ev=S.Evaluator(ctx), rk=kg.relin_keys(), gk=gk)


def words(e, ct):
    return np.asarray(e["ctx"].backend.to_host(ct.data)).reshape(ct.size(), ct.parms_id(), e["ctx"].N)


def bootstrap_input():
    """the slot values of the bootstrap tests: N / 2 reals in [-1, 1]"""
    return np.random.default_rng(5).uniform(-1.0, 1.0, N // 2)


def raised_coefficients(e, ct, top_level):
    """(t, I): the integer coefficients t = m + q_0 I of the plaintext of mod_raise(ct) as Python integers, computed on the
    host from the secret key, and its integer part I = round(t / q_0)"""
    be, ctx = e["ctx"].backend, e["ctx"]
    pt = e["dec"].decrypt(e["ev"].mod_raise(ct, top_level))
    rows = np.array(be.to_host(pt.data), dtype=np.uint64).reshape(top_level, ctx.N)[:2].copy()
    coef = np.asarray(be.to_host(be.ntt_inverse(be.from_host(rows), 1, 2, 0))).reshape(2, ctx.N)
    q0, q1 = int(ctx.primes[0]), int(ctx.primes[1])
    a0, a1 = coef[0].astype(object), coef[1].astype(object)
    t = a0 + q0 * (((a1 - a0) * pow(q0, -1, q1)) % q1)     # |t| < q_0 (K + 1) is far below q_0 q_1 / 2
    t = np.where((t > q0 * q1 // 2).astype(bool), t - q0 * q1, t)
    I = np.array([(int(x) + q0 // 2) // q0 for x in t], dtype=np.int64)
    return t, I
