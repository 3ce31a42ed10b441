"""GPU parity of the composite algorithms: the SAME host code (seal.py + algorithms.py)
runs once on the HIP engine and once on the oracle-backed twin with identical seeds; final ciphertexts must be
bit-identical, and decrypted values must match plaintext math (tolerance written per test)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def make(N, bits, backend_kind, seed=1, galois_steps=None):
    from seal_fyp_logistic_regression_amd import seal as S
    from tests.oracle_backend import OracleBackend
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(S.CoeffModulus.Create(N, bits))
    backend = OracleBackend(N, parms.coeff_modulus()) if backend_kind == "oracle" else None
    ctx = S.SEALContext.Create(parms, backend=backend)
    # both twins rescale the way the environment says (the `rescale_mode` fixture of tests/conftest.py; default: round)
    import os
    assert ctx.backend.rescale_rounded == (os.environ.get("HEFX_RESCALE", "round") != "floor"), backend_kind
    kg = S.KeyGenerator(ctx, seed)
    return dict(ctx=ctx, kg=kg, enc=S.Encryptor(ctx, kg.public_key(), seed + 1), dec=S.Decryptor(ctx, kg.secret_key()),
                encoder=S.CKKSEncoder(ctx, device_encode=False), ev=S.Evaluator(ctx), rk=kg.relin_keys(), gk=kg.galois_keys(galois_steps))


def bits(e, ct):
    return e["ctx"].backend.to_host(ct.data).reshape(ct.size(), ct.parms_id(), e["ctx"].N)


def decode(e, ct, n):
    return e["encoder"].decode(e["dec"].decrypt(ct))[:n].real


def both(N, bits_, fn, **kw):
    outs = {}
    for kind in ("gpu", "oracle"):
        e = make(N, bits_, kind, **kw)
        outs[kind] = (e, fn(e))
    return outs


def test_keys_and_encryption_are_bit_identical():
    """keygen/encrypt arithmetic (NTT, dyadic ops) runs on the backend: same seeds -> same key and ct bits"""
    g, o = make(4096, [50, 30, 30, 50], "gpu"), make(4096, [50, 30, 30, 50], "oracle")
    assert (g["kg"].secret_key().host == o["kg"].secret_key().host).all()
    for elt in o["gk"].keys:
        assert (g["ctx"].backend.to_host(g["gk"].key(elt)) == o["gk"].key(elt)).all()
    assert (g["ctx"].backend.to_host(g["rk"].key(0)) == o["rk"].key(0)).all()
    v = np.arange(16) / 7.0
    cg = g["enc"].encrypt(g["encoder"].encode(v, 2.0 ** 30))
    co = o["enc"].encrypt(o["encoder"].encode(v, 2.0 ** 30))
    assert (bits(g, cg) == bits(o, co)).all()


def test_linear_transform_plain_c2_bit_exact():
    """config 2: linear_transformation2.cpp 4x4 diagonal-method matvec at N=8192 {60,40,40,60}"""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    M = np.arange(1, 17, dtype=float).reshape(4, 4)
    v = np.array([1.0, 5.0, 9.0, 13.0])

    def run(e):
        scale = 2.0 ** 40
        diags = [e["encoder"].encode(d, scale) for d in alg.get_all_diagonals(M)]
        ct = e["enc"].encrypt(e["encoder"].encode(v, scale))
        return alg.linear_transform_plain(e["ev"], ct, diags, e["gk"])

    r = both(8192, [60, 40, 40, 60], run)
    (eg, cg), (eo, co) = r["gpu"], r["oracle"]
    assert cg.parms_id() == co.parms_id() and cg.scale == co.scale
    assert (bits(eg, cg) == bits(eo, co)).all()
    assert np.allclose(decode(eg, cg, 4), [90, 202, 314, 426], atol=1e-4)  # CKKS at scale 2^40


def test_linear_transform_d16_and_cipher_variant_bit_exact():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    rng = np.random.default_rng(5)
    d = 16
    M, v = rng.standard_normal((d, d)), rng.standard_normal(d)

    def run(e):
        scale = 2.0 ** 30
        diags = [e["encoder"].encode(x, scale) for x in alg.get_all_diagonals(M)]
        ct = e["enc"].encrypt(e["encoder"].encode(v, scale))
        a = alg.linear_transform_plain(e["ev"], ct, diags, e["gk"])
        b = alg.linear_transform_cipher(e["ev"], ct, [e["enc"].encrypt(p) for p in diags], e["gk"])
        return a, b

    r = both(4096, [50, 30, 30, 50], run)
    (eg, (ag, bg)), (eo, (ao, bo)) = r["gpu"], r["oracle"]
    assert (bits(eg, ag) == bits(eo, ao)).all()
    assert bg.size() == 3 and (bits(eg, bg) == bits(eo, bo)).all()
    assert np.allclose(decode(eg, ag, d), M @ v, atol=1e-2)  # scale 2^30, 30 key switches
    assert np.allclose(decode(eg, bg, d), M @ v, atol=1e-2)


def test_dot_product_powers_bit_exact(rescale_mode):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    a, b = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]), np.linspace(-1, 1, 8)

    def run(e):
        scale = 2.0 ** 30
        ca = e["enc"].encrypt(e["encoder"].encode(a, scale))
        cb = e["enc"].encrypt(e["encoder"].encode(b, scale))
        dp = alg.cipher_dot_product(e["ev"], ca, cb, 8, e["rk"], e["gk"])
        pw = alg.compute_all_powers(e["ev"], cb, 5, e["rk"])
        return dp, pw

    r = both(4096, [50, 30, 30, 30, 30, 50], run)
    (eg, (dg, pg)), (eo, (do, po)) = r["gpu"], r["oracle"]
    assert (bits(eg, dg) == bits(eo, do)).all()
    for i in range(2, 6):
        assert pg[i].parms_id() == po[i].parms_id()
        assert (bits(eg, pg[i]) == bits(eo, po[i])).all()
        assert np.allclose(decode(eg, pg[i], 8), b ** i, atol=1e-2)
    assert abs(decode(eg, dg, 1)[0] - float(a @ b)) < 0.05


def test_cc_matrix_multiplication_n4_known_answer(rescale_mode):
    """config 3: matrix_multiplication.cpp n=4 at N=16384 {60,40,40,40,40,60}; A = 1..16, A*A known."""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    n = 4
    A = np.arange(1, n * n + 1, dtype=float).reshape(n, n)
    want = A @ A

    u_matrices = lambda: alg.matmul_permutation_matrices(n)  # helper.h:702-851

    def run(e):
        scale = 2.0 ** 40
        enc = lambda U: [e["encoder"].encode(dg + 1e-8, scale) for dg in alg.get_all_diagonals(U)]  # epsilon: :239
        Us, Ut, V, W = u_matrices()
        ctA = e["enc"].encrypt(e["encoder"].encode(A.reshape(-1), scale))
        ctB = e["enc"].encrypt(e["encoder"].encode(A.reshape(-1), scale))
        return alg.cc_matrix_multiplication(e["ev"], ctA, ctB, n, enc(Us), enc(Ut), [enc(v) for v in V],
                                            [enc(w) for w in W], e["gk"])

    r = both(16384, [60, 40, 40, 40, 40, 60], run)
    (eg, cg), (eo, co) = r["gpu"], r["oracle"]
    assert cg.size() == 3 and cg.parms_id() == co.parms_id() == 4
    assert (bits(eg, cg) == bits(eo, co)).all()
    got = decode(eg, cg, n * n).reshape(n, n)
    assert np.allclose(got, want, rtol=1e-4, atol=1e-2), got


def _driver(name):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = os.path.join(root, "drivers", "_ref", name)
    if not os.path.exists(p) and name == "shim_selftest":  # our own source: build it where it is missing
        import subprocess
        subprocess.run(["make", "-s", "-C", os.path.join(root, "drivers"), "_ref/shim_selftest"], check=False)
    if not os.path.exists(p):
        pytest.skip(f"{name} not built (make -C drivers needs /root/reference, absent on the GPU box unless prebuilt)")
    return p


def test_cpp_shim_selftest(rescale_mode):
    """include/seal/seal.h over the C-ABI: values, levels, NAF rotations, SEAL's exceptions (drivers/shim_selftest.cpp)"""
    import subprocess
    r = subprocess.run([_driver("shim_selftest")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SELFTEST PASSED" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_sparse_matrix_product_bit_exact_and_at_config5_size():
    """cc_matrix_multiplication_sparse (the zero diagonals skipped): the same composition on the
    oracle twin gives the same bits at n = 4 (config 3's ring); and BASELINE config 5 -- a 64 x 64 product at
    N = 32768 {60,40,40,40,40,60}, 4096 of the 16384 slots, 380 rotations instead of 524 288 -- decrypts to A.B."""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import seal as S
    n = 4
    rng = np.random.default_rng(4)
    A, B = rng.standard_normal((n, n)), rng.standard_normal((n, n))

    def run(e):
        scale = 2.0 ** 40
        sig, tau, phi, psi = alg.matmul_permutation_diagonals(n)
        enc = lambda dd: {l: e["encoder"].encode(v, scale) for l, v in dd.items()}
        ctA = e["enc"].encrypt(e["encoder"].encode(A.reshape(-1), scale))
        ctB = e["enc"].encrypt(e["encoder"].encode(B.reshape(-1), scale))
        return alg.cc_matrix_multiplication_sparse(e["ev"], ctA, ctB, n, enc(sig), enc(tau), [enc(x) for x in phi],
                                                   [enc(x) for x in psi], e["gk"])

    r = both(16384, [60, 40, 40, 40, 40, 60], run)
    (eg, cg), (eo, co) = r["gpu"], r["oracle"]
    assert cg.size() == 3 and (bits(eg, cg) == bits(eo, co)).all()
    assert np.allclose(decode(eg, cg, n * n).reshape(n, n), A @ B, atol=1e-4)

    def run_hoisted(e):  # direct keys, sigma / tau rotations on a shared digit decomposition
        scale = 2.0 ** 40
        sig, tau, phi, psi = alg.matmul_permutation_diagonals(n)
        enc = lambda dd: {l: e["encoder"].encode(v, scale) for l, v in dd.items()}
        ctA = e["enc"].encrypt(e["encoder"].encode(A.reshape(-1), scale))
        ctB = e["enc"].encrypt(e["encoder"].encode(B.reshape(-1), scale))
        return alg.cc_matrix_multiplication_sparse(e["ev"], ctA, ctB, n, enc(sig), enc(tau), [enc(x) for x in phi],
                                                   [enc(x) for x in psi], e["gk"], hoisted=True)

    sig, tau, phi, psi = alg.matmul_permutation_diagonals(n)
    steps = sorted({-n * n} | {l for dd in [sig, tau] + phi + psi for l in dd if l})
    r = both(16384, [60, 40, 40, 40, 40, 60], run_hoisted, galois_steps=steps)
    (eg, hg), (eo, ho) = r["gpu"], r["oracle"]
    assert (bits(eg, hg) == bits(eo, ho)).all()
    assert np.allclose(decode(eg, hg, n * n).reshape(n, n), A @ B, atol=1e-4)

    def run_hoisted2(e):  # sigma / tau double-hoisted: key-level diagonals, one mod-down per transform
        scale = 2.0 ** 40
        enc = lambda dd, lvl=None: {l: e["encoder"].encode(v, scale, parms_id=lvl) for l, v in dd.items()}
        ctA = e["enc"].encrypt(e["encoder"].encode(A.reshape(-1), scale))
        ctB = e["enc"].encrypt(e["encoder"].encode(B.reshape(-1), scale))
        k = e["ctx"].k
        return alg.cc_matrix_multiplication_sparse(e["ev"], ctA, ctB, n, enc(sig, k), enc(tau, k),
                                                   [enc(x) for x in phi], [enc(x) for x in psi], e["gk"], hoisted=2)

    r = both(16384, [60, 40, 40, 40, 40, 60], run_hoisted2, galois_steps=steps)
    (eg, h2g), (eo, h2o) = r["gpu"], r["oracle"]
    assert (bits(eg, h2g) == bits(eo, h2o)).all()
    assert np.allclose(decode(eg, h2g, n * n).reshape(n, n), A @ B, atol=1e-4)
    # config 5 at full size, GPU only
    n, N = 64, 32768
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(S.CoeffModulus.Create(N, [60, 40, 40, 40, 40, 60]))
    ctx = S.SEALContext.Create(parms)
    kg = S.KeyGenerator(ctx, 31)
    enc_, dec_ = S.Encryptor(ctx, kg.public_key(), 32), S.Decryptor(ctx, kg.secret_key())
    encoder, ev, gk = S.CKKSEncoder(ctx), S.Evaluator(ctx), kg.galois_keys()
    A, B = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    scale = 2.0 ** 40
    sig, tau, phi, psi = alg.matmul_permutation_diagonals(n)
    enc = lambda dd: dict(zip(dd, encoder.encode_many(list(dd.values()), scale)))
    ctA, ctB = enc_.encrypt(encoder.encode(A.reshape(-1), scale)), enc_.encrypt(encoder.encode(B.reshape(-1), scale))
    res = alg.cc_matrix_multiplication_sparse(ev, ctA, ctB, n, enc(sig), enc(tau), [enc(x) for x in phi],
                                              [enc(x) for x in psi], gk)
    got = encoder.decode(dec_.decrypt(res))[:n * n].real.reshape(n, n)
    assert np.abs(got - A @ B).max() < 1e-3, np.abs(got - A @ B).max()  # entries of A.B are O(5); CKKS at 2^40


def test_reference_matrix_multiplication_driver_unchanged():
    """The reference's own matrix_multiplication.cpp (config 3), compiled unchanged against the shim, prints A*A."""
    import re
    import subprocess
    r = subprocess.run([_driver("matrix_multiplication")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    tail = r.stdout[r.stdout.rindex("Resulting matrix"):]
    nums = [float(x) for x in re.findall(r"-?\d+\.?\d*(?:e-?\d+)?", tail)][:16]
    want = (np.arange(1, 17).reshape(4, 4) @ np.arange(1, 17).reshape(4, 4)).reshape(-1)
    assert np.allclose(nums, want, atol=0.05), nums  # the driver adds 1e-8 to every diagonal entry (:239)


def test_matrix_encode_decode_and_ciphermatrix_plainvector_bit_exact():
    """rows a3-a5: Linear_Transform_CipherMatrix_PlainVector, C_Matrix_Encode, C_Matrix_Decode"""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    n = 3
    rows = [np.arange(n) + 10.0 * i for i in range(n)]

    def run(e):
        scale = 2.0 ** 30
        cts = [e["enc"].encrypt(e["encoder"].encode(r, scale)) for r in rows]
        packed = alg.c_matrix_encode(e["ev"], cts, e["gk"])
        back = alg.c_matrix_decode(e["ev"], e["encoder"], packed, n, scale, e["gk"])
        pv = alg.linear_transform_ciphermatrix_plainvector(
            e["ev"], [e["encoder"].encode(r[::-1].copy(), scale) for r in rows], cts)
        return packed, back, pv

    r = both(4096, [50, 30, 30, 50], run)
    (eg, (pg, bg, vg)), (eo, (po, bo, vo)) = r["gpu"], r["oracle"]
    assert (bits(eg, pg) == bits(eo, po)).all() and (bits(eg, vg) == bits(eo, vo)).all()
    for i in range(n):
        assert (bits(eg, bg[i]) == bits(eo, bo[i])).all()
        assert np.allclose(decode(eg, bg[i], n), rows[i], atol=1e-2)
    assert np.allclose(decode(eg, vg, n), sum(r * r[::-1] for r in rows), atol=1e-2)


def test_logistic_regression_step_bit_exact(rescale_mode):
    """rows a9-a11 on the reference's LR chain {60,40x7,60}: Tree/Horner sigmoid, predict_cipher_weights (dot products
    of all rows advanced in lockstep as batched key switches), update_weights raising where SEAL raises (:336) -- what it
    computes before that is held to the twin and to plaintext math in tests/test_gpu_lr_gradient.py."""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    X = np.array([[0.5, -1.0, 0.2, 0.1], [1.5, 0.25, -0.3, 0.4], [-0.75, 0.5, 0.6, -0.2]])
    w = np.array([0.3, -0.6, 0.5, 0.25])
    y = np.array([1.0, 0.0, 1.0])
    c = alg.SIGMOID_COEFFS[3]

    def run(e):
        scale = 2.0 ** 40
        feats = [e["enc"].encrypt(e["encoder"].encode(r, scale)) for r in X]
        featsT = [e["enc"].encrypt(e["encoder"].encode(col, scale)) for col in X.T]
        cw = e["enc"].encrypt(e["encoder"].encode(w, scale))
        cy = e["enc"].encrypt(e["encoder"].encode(y, scale))
        x = e["enc"].encrypt(e["encoder"].encode([0.8, -0.3], scale))
        t = alg.tree_cipher(e["ev"], e["encoder"], e["enc"], x, 3, scale, c, e["rk"])
        pred = alg.predict_cipher_weights(e["ev"], e["encoder"], e["enc"], feats, cw, 4, scale, e["gk"], e["rk"])
        with pytest.raises(ValueError, match="scale out of bounds"):
            alg.update_weights(e["ev"], e["encoder"], e["enc"], feats, featsT, cy, cw, 0.1, e["gk"], e["rk"], scale)
        return t, pred

    r = both(4096, [60, 40, 40, 40, 40, 40, 40, 40, 60], run, seed=4)
    (eg, (tg, pg)), (eo, (to, po)) = r["gpu"], r["oracle"]
    assert (bits(eg, tg) == bits(eo, to)).all()
    assert pg.parms_id() == po.parms_id() and (bits(eg, pg) == bits(eo, po)).all()
    z = X @ w
    assert np.allclose(decode(eg, pg, 3), c[0] + c[1] * z + c[2] * z ** 2 + c[3] * z ** 3, atol=5e-3)
    xs = np.array([0.8, -0.3])
    assert np.allclose(decode(eg, tg, 2), c[0] + c[1] * xs + c[2] * xs ** 2 + c[3] * xs ** 3, atol=1e-3)


def test_lr_prediction_fast_window_sum_bit_exact_against_the_twin():
    """predict_cipher_weights(log_sum=True): the dot products' window sums by doubling (4 instead of 9 key switches per
    row at 8 weights).  Same composition on the oracle twin -> same bits; same predictions as the reference's chain."""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    rng = np.random.default_rng(77)
    X, w = rng.uniform(-1, 1, (6, 8)), rng.uniform(-0.5, 0.5, 8)
    c = alg.SIGMOID_COEFFS[3]

    def run(e):
        scale = 2.0 ** 40
        feats = [e["enc"].encrypt(e["encoder"].encode(r, scale)) for r in X]
        cw = e["enc"].encrypt(e["encoder"].encode(w, scale))
        return (alg.predict_cipher_weights(e["ev"], e["encoder"], e["enc"], feats, cw, 8, scale, e["gk"], e["rk"],
                                           log_sum=True),
                alg.predict_cipher_weights(e["ev"], e["encoder"], e["enc"], feats, cw, 8, scale, e["gk"], e["rk"]))

    r = both(4096, [60, 40, 40, 40, 40, 40, 40, 40, 60], run, seed=6)
    (eg, (fg, rg)), (eo, (fo, ro)) = r["gpu"], r["oracle"]
    assert (bits(eg, fg) == bits(eo, fo)).all() and (bits(eg, rg) == bits(eo, ro)).all()
    z = X @ w
    want = c[0] + c[1] * z + c[2] * z ** 2 + c[3] * z ** 3
    assert np.allclose(decode(eg, fg, 6), want, atol=5e-3) and np.allclose(decode(eg, rg, 6), want, atol=5e-3)
    assert (bits(eg, fg) != bits(eg, rg)).any()


def test_linear_transform_with_direct_galois_keys_and_hoisted_fast_mode():
    """Direct keys for every step (keygen.galois_keys(steps)): SEAL then applies ONE key switch per rotation and the
    regular path stays bit-exact.  hoisted=True shares the digit decomposition of ct_new across the d-1 rotations
    explicitly (at this d = 12 the regular call would not: batches of <= 32 items take the latency path) -- with the
    flip-mask term of round 4 (ks_mac_exact_kernel) that is the SAME words: hoisted == regular == the oracle twin."""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    rng = np.random.default_rng(9)
    d = 12
    M, v = rng.standard_normal((d, d)), rng.standard_normal(d)
    steps = [-d] + list(range(1, d))

    def run(e):
        scale = 2.0 ** 40
        diags = [e["encoder"].encode(x, scale) for x in alg.get_all_diagonals(M)]
        ct = e["enc"].encrypt(e["encoder"].encode(v, scale))
        assert all(len(e["ev"].rotation_plan(s, e["gk"])) == 1 for s in steps)
        return (alg.linear_transform_plain(e["ev"], ct, diags, e["gk"]),
                alg.linear_transform_plain(e["ev"], ct, diags, e["gk"], hoisted=True))

    r = both(8192, [60, 40, 40, 60], run, galois_steps=steps)
    (eg, (cg, hg)), (eo, (co, ho)) = r["gpu"], r["oracle"]
    assert (bits(eg, cg) == bits(eo, co)).all()
    assert (bits(eg, hg) == bits(eo, ho)).all()
    assert (bits(eg, hg) == bits(eg, cg)).all()
    assert np.allclose(decode(eg, cg, d), M @ v, atol=1e-5)
    assert np.allclose(decode(eg, hg, d), M @ v, atol=1e-5)
    # (the GPU side ran hefx_linear_transform_plain_hoisted in one call, the oracle twin the Python composition)
    e = eg
    scale = 2.0 ** 40
    # without direct keys the hoisted mode refuses
    e2 = make(8192, [60, 40, 40, 60], "gpu")
    with pytest.raises(ValueError):
        alg.linear_transform_plain(e2["ev"], e2["enc"].encrypt(e2["encoder"].encode(v, scale)),
                                   [e2["encoder"].encode(x, scale) for x in alg.get_all_diagonals(M)], e2["gk"],
                                   hoisted=True)


@pytest.mark.parametrize("d,n1,hoisted", [(12, None, True), (13, 3, True), (12, None, False)])
def test_bsgs_linear_transform_bit_exact_against_the_twin(d, n1, hoisted):
    """Baby-step / giant-step Linear_Transform_Plain: n1-1 hoisted (exactly: SEAL's words) + n2-1 regular
    key switches, inner sums through hefx_multiply_plain_sum.  Same composition on the oracle twin -> same bits; M.v to CKKS precision; and
    with regular (non-hoisted) baby steps every primitive is SEAL's, so the twin's bits are op-by-op SEAL bits."""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    rng = np.random.default_rng(100 + d)
    M, v = rng.standard_normal((d, d)), rng.standard_normal(d)

    def run(e):
        scale = 2.0 ** 40
        sd = [e["encoder"].encode(x, scale) for x in alg.bsgs_diagonals(alg.get_all_diagonals(M), n1)]
        ct = e["enc"].encrypt(e["encoder"].encode(v, scale))
        return alg.linear_transform_plain_bsgs(e["ev"], ct, sd, e["gk"], n1, hoisted=hoisted)

    r = both(8192, [60, 40, 40, 60], run, galois_steps=alg.bsgs_steps(d, n1))
    (eg, cg), (eo, co) = r["gpu"], r["oracle"]
    assert cg.parms_id() == co.parms_id() and cg.scale == co.scale
    assert (bits(eg, cg) == bits(eo, co)).all()
    assert np.allclose(decode(eg, cg, d), M @ v, atol=1e-5)


@pytest.mark.parametrize("N,bits_", [(16384, [60, 40, 40, 40, 40, 60]), (32768, [60, 40, 40, 40, 40, 60])])
def test_full_size_properties(N, bits_):
    """BASELINE configs 3 and 5 at full size, through size-independent properties (the oracle twin is not run here):
    rotate(s) then rotate(-s) is the identity, rotation moves slots, a plain linear transform equals M.v, the
    dot product of the LR step is right, and GPU encode/encrypt/decrypt/decode round-trips -- all to CKKS precision."""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import seal as S
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(S.CoeffModulus.Create(N, bits_))
    ctx = S.SEALContext.Create(parms)
    kg = S.KeyGenerator(ctx, 21)
    enc, dec = S.Encryptor(ctx, kg.public_key(), 22), S.Decryptor(ctx, kg.secret_key())
    encoder, ev = S.CKKSEncoder(ctx), S.Evaluator(ctx)
    d = 8
    gk = kg.galois_keys([-d] + list(range(1, d)) + [-3, 1024, -1024])
    rk = kg.relin_keys()
    rng = np.random.default_rng(N)
    v = rng.uniform(-1, 1, N // 2)
    scale = 2.0 ** 40
    ct = enc.encrypt(encoder.encode(v, scale))
    assert np.abs(encoder.decode(dec.decrypt(ct)).real - v).max() < 1e-6
    r = ev.rotate_vector(ct, 3, gk)
    assert np.abs(encoder.decode(dec.decrypt(r)).real - np.roll(v, -3)).max() < 1e-5
    back = ev.rotate_vector(r, -3, gk)
    assert np.abs(encoder.decode(dec.decrypt(back)).real - v).max() < 1e-5
    far = ev.rotate_vector(ev.rotate_vector(ct, 1024, gk), -1024, gk)
    assert np.abs(encoder.decode(dec.decrypt(far)).real - v).max() < 1e-5
    M, w = rng.standard_normal((d, d)), rng.standard_normal(d)
    cw = enc.encrypt(encoder.encode(w, scale))
    diags = encoder.encode_many(list(alg.get_all_diagonals(M)), scale)
    for hoisted in (False, True):
        out = alg.linear_transform_plain(ev, cw, diags, gk, hoisted=hoisted)
        assert np.abs(encoder.decode(dec.decrypt(out))[:d].real - M @ w).max() < 1e-4
    a, b = rng.uniform(-1, 1, d), rng.uniform(-1, 1, d)
    ca, cb = enc.encrypt(encoder.encode(a, scale)), enc.encrypt(encoder.encode(b, scale))
    prod = ev.multiply(ca, cb)
    ev.relinearize_inplace(prod, rk)
    ev.rescale_to_next_inplace(prod)
    assert np.abs(encoder.decode(dec.decrypt(prod))[:d].real - a * b).max() < 1e-5


def _vec(line):
    import re
    return [float(x) for x in re.findall(r"-?\d+\.\d+", line)]


def test_reference_linear_transformation_benchmark_unchanged():
    """The reference's benchmark driver behind its chart (linear_transformation.cpp: N=8192, d = 10/100/1000, plain
    and cipher diagonals), compiled unchanged: every printed result row equals the expected row it prints next to it.
    Runs through the shim's deferred rotations (batched submission of the loop's rotate/multiply calls)."""
    import subprocess
    r = subprocess.run([_driver("linear_transformation")], capture_output=True, text=True, timeout=900, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    checked = 0
    for i, ln in enumerate(lines):
        if ln.startswith("Linear Transformation Set") and "Result" in ln:
            got = _vec(lines[i + 1])
            j = next(k for k in range(i + 1, i + 8) if lines[k].startswith("Expected output Set"))
            want = _vec(lines[j + 1])
            assert len(got) == len(want) == 6
            assert np.allclose(got, want, rtol=1e-7, atol=2e-3), (ln, got, want)
            checked += 1
    assert checked == 6  # three sizes x (plain, cipher) diagonals


def test_reference_polynomial_driver_unchanged():
    import re
    import subprocess
    r = subprocess.run([_driver("polynomial")], input="3\n0.5\n1\n2\n0\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    act = [float(x) for x in re.findall(r"Actual : (-?[\d.]+)", r.stdout)]
    exp = [float(x) for x in re.findall(r"Expected : (-?[\d.]+)", r.stdout)]
    assert len(act) == len(exp) == 2 and np.allclose(act, exp, atol=1e-4)   # Horner and Tree, degree 3 at x = 0.5


@pytest.mark.parametrize("N,bits_,d", [(8192, [60, 40, 40, 60], 12), (4096, [50, 30, 30, 50], 21), (16384, [60, 40, 40, 40, 40, 60], 9)])
def test_double_hoisted_linear_transform_bit_exact_against_its_oracle(N, bits_, d):
    """hefx_linear_transform_plain_hoisted2: shared decomposition AND one mod-down for the whole transform (key-level
    diagonals).  Not the bits of the rotation-by-rotation sum; bit-exact against the oracle's statement of this
    algorithm (orc_lt_double_hoisted_core), same decrypted values to CKKS precision.  d > 8 spans several chunks."""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    rng = np.random.default_rng(d)
    M, v = rng.standard_normal((d, d)), rng.standard_normal(d)
    steps = [-d] + list(range(1, d))

    def run(e):
        scale = 2.0 ** 30
        ctx = e["ctx"]
        dk = [e["encoder"].encode(x, scale, parms_id=ctx.k) for x in alg.get_all_diagonals(M)]
        dd = [e["encoder"].encode(x, scale) for x in alg.get_all_diagonals(M)]
        ct = e["enc"].encrypt(e["encoder"].encode(v, scale))
        return (alg.linear_transform_plain(e["ev"], ct, dk, e["gk"], hoisted=2),
                alg.linear_transform_plain(e["ev"], ct, dd, e["gk"]))

    r = both(N, bits_, run, galois_steps=steps)
    (eg, (hg, cg)), (eo, (ho, co)) = r["gpu"], r["oracle"]
    assert (bits(eg, hg) == bits(eo, ho)).all()
    assert (bits(eg, cg) == bits(eo, co)).all()
    assert (bits(eg, hg) != bits(eg, cg)).any()
    assert np.allclose(decode(eg, hg, d), M @ v, atol=1e-2)
    assert np.abs(decode(eg, hg, d) - decode(eg, cg, d)).max() < 1e-2  # 30-bit primes at scale 2^30: noise ~1e-3
