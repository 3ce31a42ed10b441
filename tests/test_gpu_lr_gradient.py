"""Row a11 before its exception: the LR gradient (algorithms.lr_gradient = update_weights up to its manual rescale,
logistic_regression_ckks.cpp:269-323), engine against oracle twin word for word and against plaintext math.

update_weights itself can only be tested for the exception SEAL raises at :336, and many wrong gradients still raise it.
Here the same host code runs on the HIP engine and on the oracle-backed twin (make / both / bits of
tests/test_gpu_composites.py) on the reference's LR chain {60, 40 x 7, 60} at scale 2^40, N = 4096 (the config-4 case at
N = 16384 is tests/test_gpu_round2.py::test_lr_gradient_at_n16384_c4_chain), in both rescale divisions.  The engine runs each
dot product's rotate-and-add loop as ONE hefx_rotate_add_chain call when rotate-by-1 is a single key; the twin has no such
entry and runs the loop of helper.h:472-476, so the chain is judged by an independent path -- at L = 2, and up to 39 steps.

Shapes (num_obs, num_weights), the smallest at which each path can still go wrong:
    (3, 4)   default keys        today's inputs; the window rotation -3 is a NAF plan
    (5, 3)   default keys        more rows than weights, neither a power of two: the two dot-product sizes differ, a swap of
                                 them cannot pass; -3 and -5 are both NAF plans; 4-step chains
    (8, 8)   keys for 1, -8 only every rotation is one key
    (40, 8)  default keys        predict runs 40 rows in lockstep (past the 34/35 batch cut of test_gpu_parity_cut.py); the
                                 gradient runs 8 chains of 39 steps at L = 2

The slot check.  Slots 0 .. num_weights-1 of the decrypted gradient against g_j, computed in float64 from the test's own
X, w, y by tests/lr_gradient_cases.py (its docstring says where g_j is the closed form X^T (sigmoid(X w) - y) and what the
reference's window sum leaves elsewhere; (8, 8) is the closed form in every slot).  The tolerance is derived, not chosen:
the largest |decoded - g_j| of the ORACLE TWIN ALONE (tests/test_host_api_cpu.py::test_lr_gradient_on_the_oracle_twin prints
it, CPU only), times 8 -- the engine's decode differs from the twin's only by the float decode kernel, whose band
tests/exact_ckks.py bounds far below this, and the factor leaves room for the other rescale division:

    shape            twin, round   twin, floor   allowance (8 x round)   min |g_j|   allowance / min |g_j|
    (3, 4)           3.261e-06     3.037e-06     2.609e-05               0.2140      1.2e-04
    (5, 3)           3.635e-06     3.660e-06     2.908e-05               1.3793      2.1e-05
    (8, 8)           5.437e-06     5.564e-06     4.350e-05               0.0278      1.6e-03
    (40, 8)          2.286e-05     2.332e-05     1.829e-04               0.1769      1.0e-03
    (3, 4) N=16384   2.013e-05     1.971e-05     1.610e-04               0.2140      7.5e-04

Every allowance is below a tenth of the smallest |g_j| (asserted on the CPU), so a missing term, a wrong sign or a wrong
slot cannot hide in it."""
import numpy as np
import pytest

from tests import lr_gradient_cases as C
from tests.test_gpu_composites import make

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4), (5, 3), (8, 8), (40, 8)]
_twin = {}  # (shape, division) -> (environment, gradient, pred_labels): computed once, read by every test, never changed


def _keys(shape):
    return [1, -8] if shape == (8, 8) else None


def twin(shape, mode, N=4096):
    if (shape, mode, N) not in _twin:
        e = make(N, C.LR_BITS, "oracle", seed=C.KEY_SEED, galois_steps=_keys(shape))
        _twin[(shape, mode, N)] = (e,) + tuple(C.run_gradient(e, *C.inputs(*shape), then_update=shape != (40, 8)))
    return _twin[(shape, mode, N)]


def check_gradient_against_twin_and_plain_math(shape, mode, N, allowance):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    X, w, y = C.inputs(*shape)
    want = C.expected_gradient(X, w, y, alg.SIGMOID_COEFFS[3])
    assert allowance <= 0.1 * np.abs(want).min()
    eo, go, po = twin(shape, mode, N)
    eg = make(N, C.LR_BITS, "gpu", seed=C.KEY_SEED, galois_steps=_keys(shape))
    if shape == (8, 8):  # the engine's chain entry and every other rotation on one key each
        assert len(eg["ev"].rotation_plan(1, eg["gk"])) == 1 and len(eg["ev"].rotation_plan(-8, eg["gk"])) == 1
        assert sorted(eg["gk"].keys) == sorted(eo["gk"].keys) and len(eg["gk"].keys) == 2
    else:
        assert len(eg["ev"].rotation_plan(-shape[0], eg["gk"])) > 1  # the window sums open with a NAF plan
    gg, pg = C.run_gradient(eg, X, w, y)   # ... and update_weights on the same inputs still raises at :336
    for e, g, p in ((eg, gg, pg), (eo, go, po)):
        C.check_shape_of_results(g, p)
    assert C.compare(eg, pg, eo, po) == [], "pred_labels (the operand of :288)"
    assert C.compare(eg, gg, eo, go) == [], "gradient (after :323)"
    err_g, err_o = C.decode_error(eg, gg, want), C.decode_error(eo, go, want)
    print(f"lr_gradient {shape} N={N} {mode}: max |decoded - g_j| engine {err_g:.3e}, twin {err_o:.3e}, allowance {allowance:.3e}")
    assert err_g <= allowance and err_o <= allowance, (err_g, err_o, allowance)


@pytest.mark.parametrize("shape", SHAPES)
def test_lr_gradient_same_words_as_the_twin_and_plain_math(shape, rescale_mode):
    check_gradient_against_twin_and_plain_math(shape, rescale_mode, 4096, C.ALLOWANCE[shape])


def test_a_wrong_word_or_a_wrong_scale_of_the_gradient_is_caught(rescale_mode):
    """the comparison is not vacuous (as test_gpu_xcheck.py::test_a_wrong_word_or_a_wrong_scale_is_caught): one word of the
    twin's gradient flipped, one bit of its scale flipped -- on copies, the shared twin stays as it is"""
    from seal_fyp_logistic_regression_amd import seal as S
    shape = (3, 4)
    eo, go, po = twin(shape, rescale_mode)
    eg = make(4096, C.LR_BITS, "gpu", seed=C.KEY_SEED)
    gg, pg = C.run_gradient(eg, *C.inputs(*shape), then_update=False)
    assert C.compare(eg, gg, eo, go) == [] and C.compare(eg, pg, eo, po) == []
    flipped = C.words(eo, go).copy()
    flipped[1, 0, 7] ^= 1
    bad_word = S.Ciphertext()._set(flipped, go.size(), go.parms_id(), go.scale)
    assert C.compare(eg, gg, eo, bad_word) == ["words"]
    bad_scale = go.copy()
    bad_scale.scale = float(np.frombuffer((np.array([go.scale]).view(np.uint64) ^ np.uint64(1)).tobytes(), dtype=np.float64)[0])
    assert bad_scale.scale != go.scale and abs(bad_scale.scale / go.scale - 1) < 1e-15
    assert C.compare(eg, gg, eo, bad_scale) == ["scale"]
    both_bad = bad_word.copy()
    both_bad.scale = bad_scale.scale
    assert C.compare(eg, gg, eo, both_bad) == ["scale", "words"]
    assert C.compare(eg, gg, eo, go) == []  # the twin's own gradient was not touched
