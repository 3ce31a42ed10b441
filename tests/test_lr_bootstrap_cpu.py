"""Logistic-regression training with evaluation keys only, without a GPU: algorithms.lr_step_levels,
lr_bootstrap_galois_steps, the level= keyword of predict_cipher_weights / lr_gradient, update_weights_bootstrapped and
train_cipher_bootstrapped on the oracle-backed twin.  Chain, shapes, model and allowances: tests/lr_bootstrap_cases.py.

Measured here on the twin (printed by test_twin_against_the_float_model; |decoded - model| over ALL slots against the tiled
model, largest over the iterations):
    shape A (3 rows, 4 weights, ns = 4, 2 iterations)   round 1.669e-06   floor 1.706e-06
    shape B (4 rows, 3 weights, ns = 8, 1 iteration)    round 1.531e-06   floor 1.578e-06
    train_cipher (the Decryptor's refresh) on the same inputs and chain, after the last iteration: A 1.670e-10, B 1.047e-10
The bootstrap's own error (1.5e-06 of the largest value at ns = 16: tests/test_sparse_bootstrap_cpu.py) is all of it; the
condition is bootstrap_cases.CAP = 1e-3 of MAX_VALUE, six hundred times above."""
import hashlib

import numpy as np
import pytest

from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import seal as S
from tests import bootstrap_cases as BC
from tests import lr_bootstrap_cases as LB
from tests import lr_gradient_cases as LG
from tests.oracle_backend import OracleBackend

_ENV = {}


def plans():
    if "plans" not in _ENV:
        _ENV["plans"] = {ns: LB.plan(ns) for ns in sorted({s[2] for s in LB.SHAPES.values()})}
    return _ENV["plans"]


def twin():
    """one environment for both rescale divisions: the twin reads its division at every rescale, and no key depends on it"""
    if "twin" not in _ENV:
        _ENV["twin"] = LB.make("oracle", LB.galois_steps(plans()))
    return _ENV["twin"]


def twin_run(shape):
    key = ("run", shape, OracleBackend.rescale_rounded)
    if key not in _ENV:
        _ENV[key] = LB.run(twin(), shape, plans()[LB.SHAPES[shape][2]])
    return _ENV[key]


def lr_env():
    """the LR chain of tests/lr_gradient_cases.py at N = 2048, with SEAL's default Galois keys"""
    if "lr" not in _ENV:
        parms = S.EncryptionParameters("ckks")
        parms.set_poly_modulus_degree(2048)
        parms.set_coeff_modulus(S.CoeffModulus.Create(2048, LG.LR_BITS))
        ctx = S.SEALContext.Create(parms, backend=OracleBackend(2048, parms.coeff_modulus()))
        kg = S.KeyGenerator(ctx, LG.KEY_SEED)
        _ENV["lr"] = dict(ctx=ctx, kg=kg, enc=S.Encryptor(ctx, kg.public_key(), LG.KEY_SEED + 1),
                          dec=S.Decryptor(ctx, kg.secret_key()), encoder=S.CKKSEncoder(ctx, device_encode=False),
                          ev=S.Evaluator(ctx), rk=kg.relin_keys(), gk=kg.galois_keys())
    return _ENV["lr"]


# ---- 1. the level bookkeeping ---------------------------------------------------------------------------------------------------
def test_lr_step_levels_and_the_chain_of_the_cases():
    assert alg.lr_step_levels(3, "ps") == LB.STEP_LEVELS == 7
    assert alg.lr_step_levels(3, "horner") == 8 and alg.lr_step_levels(7, "ps") == 8 and alg.lr_step_levels(7, "horner") == 12
    assert alg.lr_step_levels(5, "ps") == 8 and alg.lr_step_levels(1, "ps") == 6 and alg.lr_step_levels(3) == 8
    assert len(LB.CHAIN_BITS) == 21 and LB.START_LEVEL == 8
    for p in plans().values():
        assert p.result_level == LB.START_LEVEL and p.top_level == 20 and p.sparse_slots in (4, 8)
    with pytest.raises(ValueError, match="poly must be"):
        alg.lr_step_levels(3, "tree")
    with pytest.raises(ValueError, match="degree"):
        alg.lr_step_levels(0, "ps")


@pytest.mark.parametrize("poly,degree", [("horner", 3), ("ps", 3), ("ps", 7)])
def test_lr_step_levels_is_what_the_twin_spends(poly, degree):
    """lr_gradient spends every level of the step but the learning-rate product's"""
    e = lr_env()
    top = e["ctx"].first_parms_id()
    feats, featsT, cy, cw = LG.encrypt_inputs(e, *LG.inputs(3, 4))
    g, _ = alg.lr_gradient(e["ev"], e["encoder"], e["enc"], feats, featsT, cy, cw, e["gk"], e["rk"], LG.SCALE, degree, poly)
    assert top - g.parms_id() == alg.lr_step_levels(degree, poly) - 1
    # ... and from a lower start level the same count: the reference's degree 3 leaves one level of its chain unused with "ps"
    if top - alg.lr_step_levels(degree, poly) >= 1:
        s = top - 1
        low = lambda c: e["ev"].mod_switch_to_inplace(c.copy(), s)
        g2, _ = alg.lr_gradient(e["ev"], e["encoder"], e["enc"], [low(c) for c in feats], [low(c) for c in featsT], low(cy),
                                low(cw), e["gk"], e["rk"], LG.SCALE, degree, poly, level=s)
        assert s - g2.parms_id() == alg.lr_step_levels(degree, poly) - 1


def test_galois_steps():
    p = plans()[8]
    steps = alg.lr_bootstrap_galois_steps(p, 4, 3)
    assert steps == sorted(set(steps)) and set(steps) == set(p.galois_steps()) | {1, -3, -4}
    assert set(p.subsum_steps()) <= set(steps)       # the update's tiling takes SubSum's own keys


# ---- 2. level=None: the words of the parent commit ------------------------------------------------------------------------------
def digest(e, ct):
    return hashlib.sha256(np.ascontiguousarray(LG.words(e, ct)).tobytes()).hexdigest()[:32]


# sha256 (first 32 hex digits) of the words the commit BEFORE the level keyword produced on the twin: lr_gradient_cases' (3, 4)
# inputs, LR chain, N = 2048, rescale division round
PARENT_WORDS = {"prediction": "f78c196a72a2a029f967c2357fc0a0ce", "gradient": "30e2f3ca90c57ab9dc1f354a6d480123",
                "pred_labels": "7354c341bc6a73463e87ae8d3daa185a"}


def parity_outputs(**kw):
    e = LB.fresh(lr_env(), LG.KEY_SEED + 1)
    feats, featsT, cy, cw = LG.encrypt_inputs(e, *LG.inputs(3, 4))
    pred = alg.predict_cipher_weights(e["ev"], e["encoder"], e["enc"], feats, cw, 4, LG.SCALE, e["gk"], e["rk"], **kw)
    g, pl = alg.lr_gradient(e["ev"], e["encoder"], e["enc"], feats, featsT, cy, cw, e["gk"], e["rk"], LG.SCALE, **kw)
    return e, {"prediction": pred, "gradient": g, "pred_labels": pl}


def test_without_level_the_words_are_the_parents():
    """passes on both sides of the change"""
    assert OracleBackend.rescale_rounded
    e, outs = parity_outputs()
    got = {k: digest(e, c) for k, c in outs.items()}
    print("[lr bootstrap cpu] words without level:", got)
    assert got == PARENT_WORDS
    LG.check_shape_of_results(outs["gradient"], outs["pred_labels"])


def test_level_none_and_the_first_level_are_one_path():
    e, a = parity_outputs(level=None)
    _, b = parity_outputs(level=e["ctx"].first_parms_id())
    for k in a:
        assert digest(e, a[k]) == digest(e, b[k]) == PARENT_WORDS[k], k
        assert (a[k].parms_id(), a[k].scale) == (b[k].parms_id(), b[k].scale)


# ---- 3. the loop on the twin against the float model ----------------------------------------------------------------------------
def test_the_models_weights_fit_the_plan():
    for shape in LB.SHAPES:
        _, w, _ = LB.inputs(shape)
        assert max(np.abs(w).max(), max(np.abs(m).max() for m in LB.model(shape))) <= 0.75 * LB.MAX_VALUE
        assert LB.ALLOWANCE[shape] <= BC.CAP * LB.MAX_VALUE
        # a missing update cannot hide in the allowance: every step moves some weight by a thousand times more
        before = LB.padded(w, LB.SHAPES[shape][2])
        for m in LB.model(shape):
            assert np.abs(m - before).max() >= 1000 * LB.ALLOWANCE[shape]
            before = m


@pytest.mark.parametrize("shape", sorted(LB.SHAPES))
def test_twin_against_the_float_model(shape, rescale_mode):
    e = twin()
    rows, weights, ns, iters = LB.SHAPES[shape]
    p = plans()[ns]
    outs, want = twin_run(shape), LB.model(shape)
    assert len(outs) == len(want) == iters
    for i, (ct, w) in enumerate(zip(outs, want)):
        assert ct.size() == 2 and ct.parms_id() == LB.START_LEVEL and abs(ct.scale / LB.SCALE - 1.0) < 1e-12
        first, everywhere = LB.errors(e, ct, w)
        got = LB.decode(e, ct)
        period = float(np.abs(got - LB.tiled(got[:ns])).max())
        _, I = BC.raised_coefficients(e, e["ev"].mod_switch_to_inplace(ct.copy(), 1), p.top_level)
        print(f"[lr bootstrap cpu] shape {shape} ({rescale_mode}), iteration {i + 1}: error {first:.3e} in the first {ns} slots, "
              f"{everywhere:.3e} in all, off the period {period:.3e}; max |I| of a next bootstrap {int(np.abs(I).max())}")
        assert everywhere <= BC.CAP * LB.MAX_VALUE                    # the condition
        assert first <= LB.ALLOWANCE[shape] and everywhere <= LB.ALLOWANCE[shape] and period <= LB.ALLOWANCE[shape]
        assert np.abs(got[weights:ns]).max(initial=0.0) <= LB.ALLOWANCE[shape]     # the padding stays zero
        assert np.abs(I).max() <= p.K


@pytest.mark.parametrize("shape", sorted(LB.SHAPES))
def test_refresh_and_bootstrap_agree(shape):
    e = twin()
    rows, weights, ns, iters = LB.SHAPES[shape]
    feats, featsT, cy, cw = LB.encrypt_inputs(e, shape)
    boot = LB.decode(e, twin_run(shape)[-1])
    ref = alg.train_cipher(e["ev"], e["encoder"], e["enc"], e["dec"], feats, featsT, cy, cw, LB.LEARNING_RATE, iters, e["gk"],
                           e["rk"], LB.SCALE, LB.DEGREE, LB.POLY)
    assert ref.parms_id() == e["ctx"].first_parms_id()
    got = LB.decode(e, ref)
    own = float(np.abs(got[:weights] - LB.model(shape)[-1][:weights]).max())
    apart = float(np.abs(got[:weights] - boot[:weights]).max())
    print(f"[lr bootstrap cpu] shape {shape}: train_cipher's own error {own:.3e}, apart from train_cipher_bootstrapped {apart:.3e}")
    assert own <= LB.REFRESH_ALLOWANCE[shape]
    assert apart <= LB.ALLOWANCE[shape] + LB.REFRESH_ALLOWANCE[shape]


def test_iterations_through_the_loop_are_the_steps_one_by_one():
    """train_cipher_bootstrapped(iters = 2) from first-level operands: the words of shape A's two steps"""
    e = twin()
    p = plans()[4]
    feats, featsT, cy, cw = LB.encrypt_inputs(LB.fresh(e), "A")
    out = alg.train_cipher_bootstrapped(e["ev"], e["encoder"], e["enc"], feats, featsT, cy, cw, LB.LEARNING_RATE, 2, e["gk"],
                                        e["rk"], LB.SCALE, p, LB.DEGREE, LB.POLY)       # (encoded=None: made inside)
    assert np.array_equal(LB.words(e, out), LB.words(e, twin_run("A")[-1]))
    assert feats[0].parms_id() == cw.parms_id() == e["ctx"].first_parms_id()              # the operands are only read


# ---- 4. the refusals ------------------------------------------------------------------------------------------------------------
class NothingSubmitted:
    """an Evaluator stand-in that fails the test on any use but the checks"""

    def __init__(self, ev):
        self.ctx, self._close = ev.ctx, ev._close

    def __getattr__(self, name):
        raise AssertionError("Evaluator.%s was reached before the refusal" % name)


def test_refusals():
    from seal_fyp_logistic_regression_amd import bootstrap as B
    e = twin()
    ev, s = NothingSubmitted(e["ev"]), LB.START_LEVEL
    p = plans()[4]
    primes = S.CoeffModulus.Create(LB.N, LB.CHAIN_BITS)
    top_ops = LB.encrypt_inputs(e, "A")
    feats, featsT, cy, cw = LB.encrypt_inputs(e, "A", level=s)

    def step(plan_=p, ops=(feats, featsT, cy, cw), scale=LB.SCALE, degree=LB.DEGREE, poly=LB.POLY, f=alg.update_weights_bootstrapped):
        a, b, c, d = ops
        mid = (LB.LEARNING_RATE,) if f is alg.update_weights_bootstrapped else (LB.LEARNING_RATE, 1)
        return f(ev, e["encoder"], e["enc"], a, b, c, d, *mid, e["gk"], e["rk"], scale, plan_, degree, poly)

    for f in (alg.update_weights_bootstrapped, alg.train_cipher_bootstrapped):
        with pytest.raises(ValueError, match="needs a sparse plan"):
            step(B.plan(LB.N, primes, LB.SCALE), f=f)
        with pytest.raises(ValueError, match="slots do not hold 4 weights"):
            step(LB.plan(2), f=f)
        with pytest.raises(ValueError, match="returns at level 8 and a step needs 9"):
            step(degree=7, f=f)                                           # lr_step_levels(7, "ps") = 8
        with pytest.raises(ValueError, match="returns at level 8 and a step needs 9"):
            step(poly="horner", f=f)
        with pytest.raises(ValueError, match="scale mismatch"):
            step(scale=2.0 ** 40, f=f)
        with pytest.raises(ValueError, match="another ring or chain"):
            step(B.plan(LB.N, S.CoeffModulus.Create(LB.N, BC.CHAIN_BITS), LB.SCALE, slots=4), f=f)
    with pytest.raises(ValueError, match="must already be at level 8"):
        step(ops=top_ops)
    for i in range(4):                                                    # each operand on its own
        ops = [feats, featsT, cy, cw]
        ops[i] = [top_ops[i][0]] + list(feats[1:]) if i == 0 else top_ops[i]
        with pytest.raises(ValueError, match="must already be at level 8"):
            step(ops=ops)
    below = lambda c: e["ev"].mod_switch_to_inplace(c.copy(), s - 1)
    with pytest.raises(ValueError, match="at level 8 or above"):
        step(ops=(feats, featsT, cy, below(cw)), f=alg.train_cipher_bootstrapped)
    off = cw.copy()
    off.scale = LB.SCALE * 1.001
    with pytest.raises(ValueError, match="weights are not at the plan's scale"):
        step(ops=(feats, featsT, cy, off))
    # the level keyword itself
    for bad in (top_ops[3], below(cw)):
        with pytest.raises(ValueError, match="predict_cipher_weights: .* already be at level 8"):
            alg.predict_cipher_weights(ev, e["encoder"], e["enc"], feats, bad, 4, LB.SCALE, e["gk"], e["rk"], 3, poly="ps", level=s)
    with pytest.raises(ValueError, match="lr_gradient: .* already be at level 8"):
        alg.lr_gradient(ev, e["encoder"], e["enc"], feats, featsT, top_ops[2], cw, e["gk"], e["rk"], LB.SCALE, 3, "ps", level=s)
    for bad in (1, 21, 0):
        with pytest.raises(ValueError, match="level must lie between"):
            alg.lr_gradient(ev, e["encoder"], e["enc"], feats, featsT, cy, cw, e["gk"], e["rk"], LB.SCALE, 3, "ps", level=bad)
