"""Inputs, plaintext expectation and comparison for the LR gradient tests (row a11: algorithms.lr_gradient), shared by
tests/test_host_api_cpu.py (oracle twin alone, prints the decode error it measures), tests/test_gpu_lr_gradient.py and
tests/test_gpu_round2.py (engine against twin).  TEST INFRASTRUCTURE: nothing here is imported by the package.

What slot j of the gradient must hold, from the test's own X, w, y in float64:
    g_j = sum_i X[i, j] * (c0 + c1 z_i + c2 z_i^2 + c3 z_i^3 - y_i),   z = X @ w
-- where the reference's dot product delivers the whole sum.  cipher_dot_product (helper.h:416-502) of size s forms
m = a * b, dup = m + rotate(m, -s), and adds rotate(dup, t) for t = 1 .. s-1 to m ITSELF (:472-476 accumulate into
`mult`, not into `dup`), so slot k of its result is m_k + sum_{t=1..s-1} dup_(k+t): the whole sum for k < s, the products
k-s+1 .. s-1 only for s <= k < 2s - 1, nothing beyond.  predict_cipher_weights reads slot i of row i (size num_weights) and
the gradient reads slot j of column j (size num_obs), so
    z_i is (X @ w)_i for i < num_weights          and a tail of that sum for the observations after them,
    g_j is the whole sum over i for j < num_obs   and a tail of it for the weights after them.
That is the reference's arithmetic (the oracle twin, the engine and the reference's own C++ agree on it word for word),
reproduced and not fixed; tests/test_host_api_cpu.py has carried the note since the first LR test.  The closed form above
therefore holds in every slot only for num_obs == num_weights, and expected_gradient() evaluates the operation sequence
itself on plain float64 vectors (plain_dot_product), which IS the closed form wherever the sums are whole --
closed_form_gradient() and the mask `whole` say where, and the tests assert the agreement there."""
import numpy as np

LR_BITS = [60, 40, 40, 40, 40, 40, 40, 40, 60]  # logistic_regression_ckks.cpp:421
SCALE = 2.0 ** 40
KEY_SEED = 4

# (num_obs, num_weights) -> seed of the inputs; (3, 4) takes the inputs the LR tests have used since the first one.  Inputs
# are accepted when ALLOWANCE <= 0.1 * min_j |g_j| (test_host_api_cpu.py asserts it for every shape), so a missing term,
# a wrong sign or a wrong slot cannot hide in the allowance
INPUT_SEED = {(5, 3): 11, (8, 8): 11, (40, 8): 11}
TODAY = (np.array([[0.5, -1.0, 0.2, 0.1], [1.5, 0.25, -0.3, 0.4], [-0.75, 0.5, 0.6, -0.2]]),
         np.array([0.3, -0.6, 0.5, 0.25]), np.array([1.0, 0.0, 1.0]))

# Largest |decoded - g_j| of the ORACLE TWIN ALONE at N = 4096, rescale division "round", as printed by
# tests/test_host_api_cpu.py::test_lr_gradient_on_the_oracle_twin ("c4": the (3, 4) inputs at N = 16384, the same
# computation run once by hand: 6 s of key generation on the CPU); the GPU tests allow 8x that.  The figures are the scale
# snaps' (helper.h:489, logistic_regression_ckks.cpp:242, :195, :323: each replaces 2^80 / q by 2^40, a relative 1e-6 to
# 1e-5 for the chain's 40-bit primes), far above the key switches' noise, so they grow with |g| and not with the chain length.
TWIN_ERROR = {(3, 4): 3.261e-06, (5, 3): 3.635e-06, (8, 8): 5.437e-06, (40, 8): 2.286e-05, "c4": 2.013e-05}
ALLOWANCE = {k: 8 * v for k, v in TWIN_ERROR.items()}


def inputs(num_obs, num_weights):
    if (num_obs, num_weights) == (3, 4):
        return tuple(a.copy() for a in TODAY)
    rng = np.random.default_rng(INPUT_SEED[(num_obs, num_weights)])
    X = rng.uniform(-1, 1, (num_obs, num_weights))
    w = rng.uniform(-0.5, 0.5, num_weights)
    y = rng.integers(0, 2, num_obs).astype(float)
    return X, w, y


def plain_dot_product(a, b, size, slots=256):
    """helper.h:432-476 on plain vectors: every slot of cipher_dot_product(a, b, size)"""
    m = np.zeros(slots)
    m[:len(a)] = np.asarray(a) * np.asarray(b)[:len(a)]
    dup = m + np.roll(m, size)        # :455, :464  rotate_vector(mult, -size) moves slot k to slot k + size
    acc = m.copy()
    for _ in range(1, size):          # :472-476
        dup = np.roll(dup, -1)
        acc += dup
    return acc


def expected_pred_labels(X, w, y, coeffs):
    """slots 0 .. num_obs-1 of the operand of :288"""
    n, s = X.shape
    z = np.array([plain_dot_product(X[i], w, s)[i] for i in range(n)])   # :220-229: slot i of row i
    return sum(c * z ** k for k, c in enumerate(coeffs)) - y, z


def expected_gradient(X, w, y, coeffs):
    n, s = X.shape
    pl, z = expected_pred_labels(X, w, y, coeffs)
    g = np.array([plain_dot_product(X[:, j], pl, n)[j] for j in range(s)])   # :299-310: slot j of column j
    # where the reference's sums are whole this is the closed form of the module docstring
    assert np.abs(z[:s] - (X @ w)[:s]).max() < 1e-13
    if n <= s:
        assert np.abs(g[:n] - closed_form_gradient(X, w, y, coeffs)[:n]).max() < 1e-12
    return g


def closed_form_gradient(X, w, y, coeffs):
    z = X @ w
    return X.T @ (sum(c * z ** k for k, c in enumerate(coeffs)) - y)


def encrypt_inputs(e, X, w, y):
    enc = lambda v: e["enc"].encrypt(e["encoder"].encode(np.asarray(v, dtype=float), SCALE))
    return [enc(r) for r in X], [enc(c) for c in X.T], enc(y), enc(w)


def run_gradient(e, X, w, y, then_update=True):
    """(gradient, pred_labels) of algorithms.lr_gradient on the environment `e` (make() of the calling module), then
    update_weights on the same inputs, which must still stop where SEAL stops (:336)"""
    import pytest
    from seal_fyp_logistic_regression_amd import algorithms as alg
    feats, featsT, cy, cw = encrypt_inputs(e, X, w, y)
    out = alg.lr_gradient(e["ev"], e["encoder"], e["enc"], feats, featsT, cy, cw, e["gk"], e["rk"], SCALE)
    if then_update:
        with pytest.raises(ValueError, match="scale out of bounds"):
            alg.update_weights(e["ev"], e["encoder"], e["enc"], feats, featsT, cy, cw, 0.1, e["gk"], e["rk"], SCALE)
    return out


def check_shape_of_results(gradient, pred_labels):
    assert gradient.size() == 2 and gradient.parms_id() == 1 and gradient.scale == 2.0 ** 40
    assert pred_labels.size() == 2 and pred_labels.parms_id() == 3


def words(e, ct):
    return np.asarray(e["ctx"].backend.to_host(ct.data)).reshape(ct.size(), ct.parms_id(), e["ctx"].N)


def compare(ea, a, eb, b):
    """what differs between two ciphertexts of two environments: a list out of 'size', 'level', 'scale', 'words'"""
    diff = [name for name, x, y in (("size", a.size(), b.size()), ("level", a.parms_id(), b.parms_id()),
                                    ("scale", a.scale, b.scale)) if x != y]
    if "size" in diff or "level" in diff or not np.array_equal(words(ea, a), words(eb, b)):
        diff.append("words")
    return diff


def decode_error(e, gradient, want):
    got = e["encoder"].decode(e["dec"].decrypt(gradient))[:len(want)].real
    return float(np.abs(got - want).max())
