"""Round-3 GPU parity: the configuration bench.py times, checked output by output; config 4's own
workload (pulsar rows x 8 weights) bit for bit against the oracle twin and against the plaintext polynomial; the
reference's LR driver, unchanged, up to the exception SEAL throws at logistic_regression_ckks.cpp:336."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3 = (16384, [0xffffffffffd8001, 0xffffb20001, 0xffffc40001, 0xffffca8001, 0xffffe80001, 0xffffffffffe8001])
C4_BITS = [60, 40, 40, 40, 40, 40, 40, 40, 60]


def _pulsar_rows(n):
    """first n rows of the reference's data file (tests/golden/pulsar_rows_head400.csv: a data fixture): features [n][8],
    labels [n]"""
    rows = np.loadtxt(os.path.join(ROOT, "tests", "golden", "pulsar_rows_head400.csv"), delimiter=",", skiprows=1)
    assert rows.shape[1] == 9 and rows.shape[0] >= n
    return rows[:n, :8], rows[:n, 8]


def test_bench_configuration_default_chunking_every_output_bit_exact():
    """What bench.py times, in the default environment: C3 (N=16384, L=5), a batch that spans several 256-item chunks
    on the two internal streams (600 items: 256 + 256 + 88), digit x modulus products streamed (a chunk's x exceeds the
    Infinity Cache), three Galois keys round-robin (so ks_run's key-grouped order differs from the caller's), device-drawn
    inputs as in the bench -- and EVERY output compared word for word with the oracle."""
    from oracle import oracle as O
    from seal_fyp_logistic_regression_amd import Engine
    from seal_fyp_logistic_regression_amd.seal import galois_elt_from_step
    for v in ("HEFX_CHUNK", "HEFX_STREAMS", "HEFX_NO_FP64", "HEFX_QUARTER"):
        if v in os.environ:
            pytest.skip(f"{v} is set: this test is about the DEFAULT launch structure (the knob runs have their own tests)")
    N, primes = C3
    k, L, n, nk = len(primes), len(primes) - 1, 600, 3
    o, e = O.Oracle(N, primes), Engine(N, primes)
    key32 = lambda tag: hashlib.sha256(f"round3:{tag}".encode()).digest()
    big_ct = e.sample("uniform", key32("ct"), 1, 2 * n, L, 0)
    big_pt = e.sample("uniform", key32("pt"), 2, n, L, 0)
    big_key = e.sample("uniform", key32("key"), 3, 2 * L * nk, k, 0)
    kw = L * 2 * k * N
    keyv = [big_key.view(i * kw, (L, 2, k, N)) for i in range(nk)]
    cts = [big_ct.view(i * 2 * L * N, (2, L, N)) for i in range(n)]
    pts = [big_pt.view(i * L * N, (L, N)) for i in range(n)]
    elts = [galois_elt_from_step(1 + (i % nk), N) for i in range(n)]
    outs = e.rotate_multiply_plain_batch(L, cts, elts, [keyv[i % nk] for i in range(n)], pts)
    e.sync()
    hkeys = [kv.download() for kv in keyv]
    hct, hpt = big_ct.download().reshape(n, 2, L, N), big_pt.download().reshape(n, L, N)
    bad = [i for i in range(n) if not (outs[i].download() == o.rotate_mulplain(hct[i], elts[i], hkeys[i % nk], hpt[i])).all()]
    assert not bad, f"{len(bad)} of {n} outputs differ from the oracle, first: {bad[:8]}"


def test_config4_pulsar_rows_eight_weights_bit_exact(rescale_mode):
    """BASELINE config 4's own shape (logistic_regression_ckks.cpp:208-266 with num_weights = 8): 16 observation rows of
    the pulsar data set -- raw values, as the reference encodes them (:590 encodes `features`, not the standardised copy)
    -- times 8 encrypted weights at the full parameter set (N=16384, {60,40x7,60}); the row-batched engine path against
    the same composition on the oracle-backed twin, bit for bit, at every level the chain passes through."""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from tests.test_gpu_composites import both, bits
    X, _ = _pulsar_rows(16)
    w = np.array([0.31, -0.62, 1.5, -1.25, 0.05, -0.4, 0.9, -0.07])   # "random numbers" in (-2, 2), :551

    def run(e):
        scale = 2.0 ** 40
        feats = [e["enc"].encrypt(e["encoder"].encode(r, scale)) for r in X]
        cw = e["enc"].encrypt(e["encoder"].encode(w, scale))
        dots = alg.cipher_dot_product_many(e["ev"], feats, [cw] * len(feats), 8, e["rk"], e["gk"])
        pred = alg.predict_cipher_weights(e["ev"], e["encoder"], e["enc"], feats, cw, 8, scale, e["gk"], e["rk"])
        return dots, pred

    r = both(16384, C4_BITS, run, seed=44)
    (eg, (dg, pg)), (eo, (do, po)) = r["gpu"], r["oracle"]
    for i in range(16):
        assert dg[i].parms_id() == do[i].parms_id() and (bits(eg, dg[i]) == bits(eo, do[i])).all(), i
    assert pg.parms_id() == po.parms_id() and pg.size() == po.size() and (bits(eg, pg) == bits(eo, po)).all()
    # the dot products themselves are exact to CKKS precision (slot 0 of each row's result; values up to ~1e2)
    z = X @ w
    got = np.array([eg["encoder"].decode(eg["dec"].decrypt(d))[0].real for d in dg])
    assert np.allclose(got, z, rtol=1e-6, atol=1e-4), np.abs(got - z).max()


def test_config4_400_pulsar_rows_predict_against_the_plaintext_polynomial():
    """predict_cipher_weights (logistic_regression_ckks.cpp:208-266) over the 400 fixture rows x 8 weights on the engine
    (3600 key switches in row-batched chunks at L = 8 ... 4), decrypted, against the same algorithm in the clear.
    What the reference computes: cipher_dot_product (helper.h:416-502) leaves in slot s the product p_s plus the window
    dup[s+1 .. s+size-1] of the duplicated product vector [p_0..p_7, p_0..p_7, 0, ...] -- the full dot product for s < 8, a
    partial sum for 8 <= s < 16, zero beyond -- and the one-hot mask of row i (:222-229) picks slot i of ITS result; the
    degree-3 sigmoid polynomial follows.  (So only the first num_weights rows see their full dot product: the
    reference's behaviour, reproduced, not repaired.)  Every row's full dot product is checked on its own as well.
    Standardised features (what the reference meant to encode, :570) keep the cubic inside CKKS range."""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from tests.test_gpu_composites import make
    X, _ = _pulsar_rows(400)
    X = (X - X.mean(axis=0)) / X.std(axis=0)
    w = np.array([0.31, -0.62, 0.5, -0.25, 0.05, -0.4, 0.3, -0.07])
    e = make(16384, C4_BITS, "gpu", seed=45)
    scale = 2.0 ** 40
    feats = [e["enc"].encrypt(p) for p in e["encoder"].encode_many(list(X), scale)]
    cw = e["enc"].encrypt(e["encoder"].encode(w, scale))
    dots = alg.cipher_dot_product_many(e["ev"], feats, [cw] * len(feats), 8, e["rk"], e["gk"])
    z = X @ w
    got_z = np.array([e["encoder"].decode(e["dec"].decrypt(d))[0].real for d in dots])
    assert np.abs(got_z - z).max() < 1e-4, np.abs(got_z - z).max()          # all 400 dot products, slot 0
    pred = alg.predict_cipher_weights(e["ev"], e["encoder"], e["enc"], feats, cw, 8, scale, e["gk"], e["rk"])
    got = e["encoder"].decode(e["dec"].decrypt(pred))[:400].real
    c = alg.SIGMOID_COEFFS[3]
    lin = np.zeros(400)
    for i in range(400):
        p_ = X[i] * w
        dup = np.concatenate([p_, p_, np.zeros(400 + 8)])                     # helper.h:455-462
        lin[i] = (p_[i] if i < 8 else 0.0) + dup[i + 1:i + 8].sum()           # :472-476: mult += rot^j(dup), j = 1..7
    assert np.allclose(lin[:8], z[:8])
    want = c[0] + c[1] * lin + c[2] * lin ** 2 + c[3] * lin ** 3
    assert np.abs(got - want).max() < 5e-3, (np.abs(got - want).max(), int(np.abs(got - want).argmax()))


@pytest.mark.parametrize("devices", ["1", "2"])
def test_reference_lr_driver_unchanged_runs_to_the_scale_exception(tmp_path, devices):
    """The reference's logistic_regression_ckks.cpp, compiled unchanged against include/seal/seal.h, on 400 pulsar rows:
    it encrypts, runs predict_cipher_weights (:282 -> 3600 recorded key switches), the eight gradient dot products
    (:295-300, 400-long rotate-by-1 chains) and the masks, and stops where SEAL itself stops -- evaluator.multiply_plain
    at :336 throws std::invalid_argument("scale out of bounds") at the last level (rows a9-a11 -- the words of
    the gradient the reference's update_weights holds at that throw are checked by tests/test_gpu_xcheck.py).
    devices = 2: the same unchanged binary with SEAL_SHIM_DEVICES=2 -- the recorded rows are dealt over two engine
    contexts (both on this box's one GPU; on a node: one per GPU) -- must behave identically (the bit-for-bit comparison
    of that path is drivers/shim_selftest.cpp's)."""
    from tests.test_gpu_composites import _driver
    exe = _driver("logistic_regression_ckks")
    shutil.copy(os.path.join(ROOT, "tests", "golden", "pulsar_rows_head400.csv"), tmp_path / "pulsar_stars_copy.csv")
    env = dict(os.environ, SEAL_SHIM_DEVICES=devices, SEAL_SHIM_STATS="1")
    r = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert "num obs = 400" in out and "num weights = 8" in out, out[-1500:]
    assert "->335" in out, out[-1500:]                      # the driver's own trace line before the failing call
    assert "scale out of bounds" in out, out[-1500:]
    assert r.returncode != 0                                # terminate() on the uncaught throw, as with real SEAL
