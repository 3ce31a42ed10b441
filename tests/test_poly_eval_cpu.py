"""algorithms.evaluate_polynomial and Evaluator.scalar_combine end to end on the oracle-backed twin (no GPU): toy ring size
N = 1024, {60,40,40,40,60} for the sigmoid polynomials of degree 3, 5 and 7, {60,40x5,60} for degrees 15 and 31.

PRECISION.  Slot values in [-1, 1]; the error is the largest |decoded - float64 polynomial| over the slots.  The baseline is
the smaller of the errors of the existing horner_cipher and tree_cipher on the same slot values, and evaluate_polynomial
must stay within 2x of it (a different but equally long noise path; the expectation is far below 1x, because the reference's
evaluators overwrite their scales -- about 2^-20 relative per level -- and the plan tracks them).
  The baseline's parameters: at {60,40,40,40,60} Horner_cipher has levels for degree 3 only (it takes `degree` of them) and
Tree_cipher for degree 3 only as well: it multiplies every power by its coefficient AFTER computing it, ceil(log2 d) + 1
levels, four for degrees 5 and 7 where the chain has three.  For those two degrees the baseline therefore runs Tree_cipher
alone on the chain with ONE more 40-bit prime, {60,40,40,40,40,60} -- same N, same slot values, same seeds -- while
evaluate_polynomial runs on {60,40,40,40,60} as stated: the baseline gets more room, the gate asks no less.
  Measured here (rescale division round; written to profiles/poly_eval.json with POLY_EVAL_RECORD=1):
      degree 3: horner 3.1e-08, tree 6.6e-08, evaluate_polynomial 1.1e-08 (power), 1.1e-08 (chebyshev)
      degree 5: tree 5.5e-08, evaluate_polynomial 1.2e-08 / 1.3e-08;  degree 7: tree 3.9e-08, 1.2e-08 / 1.2e-08
      degree 15: 1.1e-08 (chebyshev), 2.8e-08 (power);  degree 31: 1.1e-08 (chebyshev)
Degrees 15 and 31 have no counterpart in the reference: their error is recorded, nothing is gated on it (their criteria are
the plan's algebra, tests/test_poly_plan_cpu.py, and bit equality with the engine, tests/test_gpu_poly.py)."""
import json
import os

import numpy as np
import pytest

from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import poly
from seal_fyp_logistic_regression_amd import seal as S
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1024
SCALE = 2.0 ** 40
BITS7 = [60, 40, 40, 40, 60]
BITS31 = [60, 40, 40, 40, 40, 40, 60]
_ENVS = {}
RECORD = {}


def env(bits):
    key = tuple(bits)
    if key not in _ENVS:
        parms = S.EncryptionParameters("ckks")
        parms.set_poly_modulus_degree(N)
        parms.set_coeff_modulus(S.CoeffModulus.Create(N, list(bits)))
        ctx = S.SEALContext.Create(parms, backend=OracleBackend(N, parms.coeff_modulus()))
        kg = S.KeyGenerator(ctx, 3)
        e = dict(ctx=ctx, kg=kg, enc=S.Encryptor(ctx, kg.public_key(), 4), dec=S.Decryptor(ctx, kg.secret_key()),
                 encoder=S.CKKSEncoder(ctx, device_encode=False), ev=S.Evaluator(ctx), rk=kg.relin_keys())
        e["x"] = np.linspace(-1.0, 1.0, N // 2)
        e["ct"] = e["enc"].encrypt(e["encoder"].encode(e["x"], SCALE))
        _ENVS[key] = e
    return _ENVS[key]


def error(e, ct, want):
    return float(np.abs(e["encoder"].decode(e["dec"].decrypt(ct)).real - want).max())


def baseline(d, coeffs, want):
    """{name: error} of the reference's evaluators, on the issue's chain where they have the levels, else Tree_cipher alone
    on the chain with one more prime (module docstring)"""
    e = env(BITS7)
    if d == 3:
        return {"horner": error(e, alg.horner_cipher(e["ev"], e["encoder"], e["enc"], e["ct"], d, coeffs, SCALE, e["rk"]), want),
                "tree": error(e, alg.tree_cipher(e["ev"], e["encoder"], e["enc"], e["ct"], d, SCALE, coeffs, e["rk"]), want)}
    for name, f in (("horner", lambda: alg.horner_cipher(e["ev"], e["encoder"], e["enc"], e["ct"], d, coeffs, SCALE, e["rk"])),
                    ("tree", lambda: alg.tree_cipher(e["ev"], e["encoder"], e["enc"], e["ct"], d, SCALE, coeffs, e["rk"]))):
        with pytest.raises(ValueError, match="scale out of bounds|end of modulus switching chain"):
            f()   # neither has the levels on {60,40,40,40,60}
    e1 = env([60, 40, 40, 40, 40, 60])
    return {"tree": error(e1, alg.tree_cipher(e1["ev"], e1["encoder"], e1["enc"], e1["ct"], d, SCALE, coeffs, e1["rk"]), want)}


@pytest.mark.parametrize("d", [3, 5, 7])
def test_sigmoid_precision_against_horner_and_tree(d):
    e = env(BITS7)
    coeffs = alg.SIGMOID_COEFFS[d]
    want = sum(c * e["x"] ** k for k, c in enumerate(coeffs))
    base = baseline(d, coeffs, want)
    got = {}
    for basis, c in (("power", coeffs), ("chebyshev", np.polynomial.chebyshev.poly2cheb(coeffs))):
        r = alg.evaluate_polynomial(e["ev"], e["ct"], c, e["rk"], basis=basis)
        depth = int(np.ceil(np.log2(d + 1)))
        assert r.size() == 2 and r.parms_id() == len(BITS7) - 1 - depth
        assert abs(r.scale - SCALE) <= 2.0 ** -48 * SCALE   # tracked to the target, not set
        got[basis] = error(e, r, want)
    print(f"[poly_eval] degree {d}: baseline {base}, evaluate_polynomial {got}")
    RECORD[f"sigmoid_degree_{d}"] = {"baseline": base, "evaluate_polynomial": got}
    for basis, err in got.items():
        assert err <= 2 * min(base.values()), (d, basis, err, base)


def chebyshev_interpolant(f, d):
    k = np.arange(d + 1)
    nodes = np.cos(np.pi * (k + 0.5) / (d + 1))
    return np.polynomial.chebyshev.chebfit(nodes, f(nodes), d)


@pytest.mark.parametrize("d", [15, 31])
def test_degrees_15_and_31_run_and_are_recorded(d):
    """the Chebyshev interpolant of a steep sigmoid (what EvalMod-sized degrees look like); degree 15 in the power basis too"""
    e = env(BITS31)
    cheb = chebyshev_interpolant(lambda t: 1.0 / (1.0 + np.exp(-6.0 * t)), d)
    want = np.polynomial.chebyshev.chebval(e["x"], cheb)
    depth = int(np.ceil(np.log2(d + 1)))
    got = {}
    cases = [("chebyshev", cheb)] + ([("power", np.polynomial.chebyshev.cheb2poly(cheb))] if d == 15 else [])
    for basis, c in cases:
        r = alg.evaluate_polynomial(e["ev"], e["ct"], c, e["rk"], basis=basis)
        assert r.size() == 2 and r.parms_id() == len(BITS31) - 1 - depth and abs(r.scale - SCALE) <= 2.0 ** -48 * SCALE
        w = want if basis == "chebyshev" else np.polynomial.polynomial.polyval(e["x"], c)
        got[basis] = error(e, r, w)
        assert np.isfinite(got[basis])
    print(f"[poly_eval] degree {d}: evaluate_polynomial {got} (recorded, not gated)")
    RECORD[f"degree_{d}"] = {"evaluate_polynomial": got}


def test_record_the_measured_errors():
    """POLY_EVAL_RECORD=1: the figures of this run go into the precision section of profiles/poly_eval.json"""
    for d in (3, 5, 7):   # (run on its own, this test measures what the tests above have not yet)
        if f"sigmoid_degree_{d}" not in RECORD:
            test_sigmoid_precision_against_horner_and_tree(d)
    for d in (15, 31):
        if f"degree_{d}" not in RECORD:
            test_degrees_15_and_31_run_and_are_recorded(d)
    assert {"sigmoid_degree_3", "sigmoid_degree_5", "sigmoid_degree_7", "degree_15", "degree_31"} <= set(RECORD)
    if os.environ.get("POLY_EVAL_RECORD"):
        path = os.path.join(ROOT, "profiles", "poly_eval.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["precision_oracle_twin_n1024"] = {"scale": "2^40", "slots": "linspace(-1, 1, 512)",
                                              "rescale": "round" if OracleBackend.rescale_rounded else "floor", **RECORD}
        json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
        open(path, "a").write("\n")


# ---- Evaluator.scalar_combine on a backend without the fused kernel: the composition, its words and its checks -----------
def test_scalar_combine_is_the_integer_combination():
    e = env(BITS7)
    ev, be, q = e["ev"], e["ctx"].backend, e["ctx"].primes
    a = e["ct"]                                     # level 4, scale 2^40
    b = ev.rescale_to_next_inplace(ev.relinearize_inplace(ev.multiply(a, a), e["rk"]))   # level 3, scale 2^80 / q_3
    L, S_ = 2, a.scale * 2.0 ** 40
    wscales = [S_ / a.scale, S_ / b.scale]
    weights = [[0.25, -1.5], [-0.81562, 1e-5], [1.0, 1.0]]
    consts = [0.5, -0.5, 0.0]
    outs = ev.scalar_combine([a, b], weights, wscales, consts, scale=S_, parms_id=L)
    A, B = (np.asarray(x.data).reshape(2, x.parms_id(), N).astype(object) for x in (a, b))
    for g, o in enumerate(outs):
        assert o.parms_id() == L and o.size() == 2 and o.scale == S_
        got = np.asarray(o.data).reshape(2, L, N)
        for j in range(L):
            w = [poly.weight_residue(weights[g][k], wscales[k], q[j]) for k in range(2)]
            c = poly.weight_residue(consts[g], S_, q[j])
            for p in range(2):
                want = (w[0] * A[p, j] + w[1] * B[p, j] + (c if p == 0 else 0)) % q[j]
                assert (got[p, j].astype(object) == want).all(), (g, j, p)
    assert np.array_equal(np.asarray(ev.scalar_combine([a, b], weights[0], wscales, parms_id=L)[0].data).reshape(2, L, N),
                          np.asarray(ev.scalar_combine([a, b], [weights[0]], wscales, None, scale=S_, parms_id=L)[0].data).reshape(2, L, N))
    # the checks of the op-by-op sequence
    with pytest.raises(ValueError, match="scale mismatch"):
        ev.scalar_combine([a, b], weights[0], [wscales[0], wscales[1] * 1.001], parms_id=L)
    with pytest.raises(ValueError, match="cannot switch to higher level modulus"):
        ev.scalar_combine([a, b], weights[0], wscales, parms_id=4)
    with pytest.raises(RuntimeError, match="transparent"):
        ev.scalar_combine([a, b], [0.25, 1e-30], wscales, parms_id=L)
    with pytest.raises(ValueError, match="scale out of bounds"):
        ev.scalar_combine([a, b], weights[0], [w * 2.0 ** 30 for w in wscales], parms_id=L)
    assert not hasattr(be, "scalar_combine")   # (this file runs the composition; the fused call is tests/test_gpu_poly.py)


def test_predict_ps_option_is_validated():
    with pytest.raises(ValueError, match="poly must be"):
        alg.predict_cipher_weights(None, None, None, [], None, 0, SCALE, None, None, poly="estrin")
