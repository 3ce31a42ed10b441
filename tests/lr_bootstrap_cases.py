"""Shared cases of tests/test_lr_bootstrap_cpu.py and tests/test_gpu_lr_bootstrap.py (TEST INFRASTRUCTURE): logistic-regression
training with evaluation keys only, algorithms.update_weights_bootstrapped / train_cipher_bootstrapped.

THE CHAIN.  N = 2048, scale 2^50, key seed and Hamming weight of tests/bootstrap_cases.py; primes of
[60] + [50] * (12 + lr_step_levels(3, "ps")) + [60] bits from CoeffModulus.Create, as the bootstrap cases take theirs: the
bootstrap's 12 levels above the 7 of one step, 21 primes, the key switch at k = 21.  Degree 3, poly "ps".

THE SHAPES.  (rows, weights, ns, iterations):
    A = (3, 4, 4, 2)   ns = num_weights; the second iteration starts from bootstrapped weights
    B = (4, 3, 8, 1)   num_weights no power of two, ns > num_weights, more rows than weights (the reference's window sum leaves a
                       tail of the dot product in row 3: tests/lr_gradient_cases.py states it, and the model here is built from it)
A takes the inputs the LR tests have used since the first one (lr_gradient_cases.TODAY); B's are drawn here.

THE MODEL.  w <- w - (LEARNING_RATE / num_obs) * lr_gradient_cases.expected_gradient(X, w, y, coeffs) in float64, per iteration.
MAX_VALUE = 1.0 is the plan's promise on |w|: the models' weights stay below 0.75 (asserted by the CPU test).

TWIN_ERROR: largest |decoded - tiled model| over ALL N / 2 slots after any iteration, of the ORACLE TWIN ALONE, the larger of the two
rescale divisions, as printed by tests/test_lr_bootstrap_cpu.py::test_twin_against_the_float_model; the tests allow 8 times that
(the convention of lr_gradient_cases.ALLOWANCE).  REFRESH_ERROR: the same for train_cipher (the Decryptor's refresh) on the same
inputs and chain, after the last iteration, first num_weights slots, division round.  The condition, not a measurement: the twin's error stays under bootstrap_cases.CAP = 1e-3 of MAX_VALUE."""
import numpy as np

from tests import bootstrap_cases as BC
from tests import lr_gradient_cases as LG

N = BC.N
SCALE = BC.SCALE
DEGREE, POLY = 3, "ps"
STEP_LEVELS = 7                                   # lr_step_levels(3, "ps"), asserted by the CPU test
CHAIN_BITS = [60] + [50] * (12 + STEP_LEVELS) + [60]
START_LEVEL = 1 + STEP_LEVELS
LEARNING_RATE = 0.5
MAX_VALUE = 1.0

SHAPES = {"A": (3, 4, 4, 2), "B": (4, 3, 8, 1)}
B_SEED = 23

TWIN_ERROR = {"A": 1.706e-06, "B": 1.578e-06}
REFRESH_ERROR = {"A": 1.670e-10, "B": 1.047e-10}
ALLOWANCE = {k: 8 * v for k, v in TWIN_ERROR.items()}
REFRESH_ALLOWANCE = {k: 8 * v for k, v in REFRESH_ERROR.items()}


def coeffs():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    return alg.SIGMOID_COEFFS[DEGREE]


def inputs(shape):
    rows, weights, _, _ = SHAPES[shape]
    if shape == "A":
        return LG.inputs(rows, weights)
    rng = np.random.default_rng(B_SEED)
    X = rng.uniform(-1, 1, (rows, weights))
    w = rng.uniform(-0.5, 0.5, weights)
    y = rng.integers(0, 2, rows).astype(float)
    return X, w, y


def model(shape):
    """the weights after every iteration, in float64: [w_1, .., w_iters], each padded with zeros to ns values"""
    X, w, y = inputs(shape)
    rows, _, ns, iters = SHAPES[shape]
    out = []
    for _ in range(iters):
        w = w - (LEARNING_RATE / rows) * LG.expected_gradient(X, w, y, coeffs())
        out.append(padded(w, ns))
    return out


def padded(w, ns):
    v = np.zeros(ns)
    v[:len(w)] = w
    return v


def tiled(v):
    return np.tile(v, (N // 2) // len(v))


def plan(ns):
    from seal_fyp_logistic_regression_amd import bootstrap as B
    from seal_fyp_logistic_regression_amd import seal as S
    return B.plan(N, S.CoeffModulus.Create(N, CHAIN_BITS), SCALE, slots=ns, max_value=MAX_VALUE)


def galois_steps(plans):
    """one key set for every shape: the steps of all the plans and of all the dot products"""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    steps = set()
    for name, (rows, weights, ns, _) in SHAPES.items():
        steps |= set(alg.lr_bootstrap_galois_steps(plans[ns], rows, weights))
    return sorted(steps)


def make(kind, steps):
    return BC.make(N, CHAIN_BITS, kind, seed=BC.KEY_SEED, hamming_weight=BC.HAMMING_WEIGHT, galois_steps=tuple(steps),
                   conjugate=True)


def fresh(e, seed=BC.KEY_SEED + 1):
    """`e` with a new Encryptor: a seeded Encryptor replays its i-th ciphertext, so runs whose WORDS are compared start from one"""
    from seal_fyp_logistic_regression_amd import seal as S
    return dict(e, enc=S.Encryptor(e["ctx"], e["kg"].public_key(), seed))


def encrypt_inputs(e, shape, level=None):
    """(features, features_T, labels, weights) at the first level (level=None) or at `level`: rows zero-padded, weights TILED"""
    X, w, y = inputs(shape)
    ns = SHAPES[shape][2]
    enc = lambda v: e["enc"].encrypt(e["encoder"].encode(np.asarray(v, dtype=float), SCALE, parms_id=level))
    return [enc(r) for r in X], [enc(c) for c in X.T], enc(y), enc(tiled(padded(w, ns)))


def run(e, shape, plan_):
    """the ciphertexts after every iteration: the first through train_cipher_bootstrapped from first-level operands (it
    mod-switches them, once), every later one through update_weights_bootstrapped on operands already at the start level"""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    rows, weights, ns, iters = SHAPES[shape]
    e = fresh(e)
    ev, encoded = e["ev"], plan_.encode(e["encoder"])
    feats, featsT, cy, cw = encrypt_inputs(e, shape)
    outs = [alg.train_cipher_bootstrapped(ev, e["encoder"], e["enc"], feats, featsT, cy, cw, LEARNING_RATE, 1, e["gk"],
                                          e["rk"], SCALE, plan_, DEGREE, POLY, encoded)]
    low = lambda c: ev.mod_switch_to_inplace(c.copy(), START_LEVEL)
    feats, featsT, cy = [low(c) for c in feats], [low(c) for c in featsT], low(cy)
    for _ in range(1, iters):
        outs.append(alg.update_weights_bootstrapped(ev, e["encoder"], e["enc"], feats, featsT, cy, outs[-1], LEARNING_RATE,
                                                    e["gk"], e["rk"], SCALE, plan_, DEGREE, POLY, encoded))
    return outs


def decode(e, ct):
    return e["encoder"].decode(e["dec"].decrypt(ct)).real


def errors(e, ct, want_ns):
    """(error over the first ns slots, error over all slots against the tiled expectation)"""
    got = decode(e, ct)
    ns = len(want_ns)
    return float(np.abs(got[:ns] - want_ns).max()), float(np.abs(got - tiled(want_ns)).max())


words = BC.words
