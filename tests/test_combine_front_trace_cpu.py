"""The Python front end of the combine family -- Evaluator.scalar_combine, product_combine and plain_combine, and their drivers
evaluate_polynomial, evaluate_polynomial_many and eval_mod -- must give the same words, refuse with the same exception and hand
the native entries the same arguments whatever its own shape: every scenario below is run on two backends and must equal
tests/golden/combine_front_traces.json, recorded before the front end was folded.

Backends: (a) the oracle twin, which has none of the three entries, so every call is composed op by op: the digest of every
result's words, its size, level and scale, or the type and message of the refusal (the sequence of backend calls is not
compared); (b) the twin plus stubs of scalar_combine, plain_combine, product_combine and multiply_plain_sum that return zeros
of the result's shape: which of them is called, with every integer and row-list argument, the digests of the residue
arrays, the None pattern of the plaintext matrix and the group size (this pins the route and what the GPU entry would
receive; a scenario that composes on this twin too has an empty trace).  N = 1024 on {60,40,40,40,60}, and {60,40x5,60} where
the depth needs it.  `python -m tests.test_combine_front_trace_cpu` rewrites the fixture."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import capi
from seal_fyp_logistic_regression_amd import seal as S
from tests import bootstrap_cases as BC
from tests.oracle_backend import OracleBackend
from tests.trace_recording import Recorder, digest

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "combine_front_traces.json")
N, SCALE = 1024, 2.0 ** 40
BITS7, BITS31 = (60, 40, 40, 40, 60), (60, 40, 40, 40, 40, 40, 60)
ENTRIES = ("scalar_combine", "plain_combine", "product_combine", "multiply_plain_sum")


class _StubTwin(OracleBackend):
    """the three entries, and the grouped sum plain_combine may take instead, as stubs: zeros of the result's shape"""

    def _zeros(self, count, size, L):
        return [np.zeros((size, L, self.N), dtype=np.uint64) for _ in range(count)]

    def scalar_combine(self, L, size, ins, in_rows, weights, consts=None):
        return self._zeros(len(weights), size, L)

    def plain_combine(self, L, ins, pts):
        return self._zeros(len(pts), 2, L)

    def product_combine(self, L, As, a_rows, Bs, b_rows, u, lins=None, lin_rows=(), w=None, c=None):
        return self._zeros(len(As), 3, L)

    def multiply_plain_sum(self, L, size, cts, pts, group=None):
        return self._zeros(len(range(0, len(cts), group or len(cts))), size, L)


BACKENDS = {"oracle": OracleBackend, "stubs": _StubTwin}


@functools.lru_cache(maxsize=None)
def _env(backend, bits):
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(S.CoeffModulus.Create(N, list(bits)))
    be = BACKENDS[backend](N, parms.coeff_modulus())
    ctx = S.SEALContext.Create(parms, backend=be)
    kg = S.KeyGenerator(ctx, 3)
    enc, encoder, ev = S.Encryptor(ctx, kg.public_key(), 4), S.CKKSEncoder(ctx, device_encode=False), S.Evaluator(ctx)
    rk, top = kg.relin_keys(), len(bits) - 1
    rng = np.random.default_rng(1)
    values = lambda: rng.uniform(-1.0, 1.0, N // 2)

    def ct(level=top):
        c = enc.encrypt(encoder.encode(values(), SCALE))
        return c if level == top else ev.mod_switch_to_inplace(c, level)

    # every operand is drawn here, in one fixed order, so that a scenario run alone sees the operands of the full run
    x = [ct() for _ in range(5)]                                       # the top level, scale 2^40
    e = dict(ev=ev, be=be, rk=rk, x=x)
    if bits == BITS7:
        e["y"] = [ct(3) for _ in range(2)]                             # one level lower
        e["q"] = [ev.multiply(x[0], x[1]), ev.multiply(x[2], x[3])]    # size 3, scale 2^80
        e["r"] = [ev.relinearize_inplace(ev.multiply(x[i], x[i + 1]), rk) for i in range(2)]   # size 2, scale 2^80
        e["rl"] = [ev.mod_switch_to_inplace(c.copy(), 3) for c in e["r"]]
        e["p"] = [encoder.encode(values(), SCALE) for _ in range(6)]
        e["p_low"] = encoder.encode(values(), SCALE, parms_id=3)
        e["p_30"], e["p_150"] = encoder.encode(values(), 2.0 ** 30), encoder.encode(values(), 2.0 ** 150)
        e["p_zero"] = encoder.encode(np.zeros(N // 2), SCALE)
        sign = lambda shape: rng.uniform(0.1, 1.0, shape) * rng.choice([-1.0, 1.0], shape)
        e["W53"], e["W257"], e["W17"], e["u33"] = sign((3, 5)), sign((2, 257)), sign((17, 2)), sign(33)
    return e


def _chebyshev(d):
    k = np.arange(d + 1)
    nodes = np.cos(np.pi * (k + 0.5) / (d + 1))
    return np.polynomial.chebyshev.chebfit(nodes, 1.0 / (1.0 + np.exp(-6.0 * nodes)), d)


def _evalmod_plan(primes):
    """what eval_mod reads of a bootstrap plan: degree 7 and r = 2 from level 6 end at level 1"""
    target = SCALE
    for i in range(2):
        target = float(np.sqrt(target * float(primes[1 + i])))
    return SimpleNamespace(evalmod_level=6, coeffs=BC.evalmod_interpolant(7, 2), poly_target_scale=target, r=2)


A, B, C = 2.0 ** 20, 2.0 ** 30, 2.0 ** 31
EDGE = 1.0 - 2.0 ** -41   # S = 2^180 is out of bounds at level 4 (180 bits), S * EDGE is close to it and inside


def _scenarios(e):
    """name -> thunk; the operands are those of _env(.., BITS7) unless the name is in ON_BITS31"""
    ev, rk, x = e["ev"], e["rk"], e["x"]
    y, q, r, rl, p = (e.get(k) for k in ("y", "q", "r", "rl", "p"))
    sc, pc, plc = ev.scalar_combine, ev.product_combine, ev.plain_combine
    one = lambda f: lambda: [f()]
    x01 = ([x[0]], [x[1]], 1.0, A)
    mixed = lambda ws: ([([x[0]], [y[0]], 0.75, ws), ([y[1]], [y[1]], 2.0, ws)], [([rl[0]], 1.25, ws), ([r[1]], -0.3, ws)])
    dense = lambda m, G: plc([x[0]] * m, [[p[0]] * m] * G)
    return {
        # ---- scalar_combine
        "sc_m1_G1": lambda: sc([x[0]], [[0.5]], [B]),
        "sc_m5_G3_consts": lambda: sc(x, e["W53"], [B] * 5, [0.25, -0.5, 1.0]),
        "sc_one_input_a_level_higher": lambda: sc([x[0], y[0]], [0.75, -1.25], [B, B]),
        "sc_scale_and_parms_id": lambda: sc([x[0], y[0]], [[0.75, -1.25]], [B, B], [0.5], scale=2.0 ** 70, parms_id=2),
        "sc_size3": lambda: sc(q, [[0.5, -2.0], [1.5, 0.25]], [A, A], [1.0, -1.0]),
        "sc_m257": lambda: sc([x[i % 5] for i in range(257)], e["W257"], [B] * 257, [0.5, -0.5]),
        "sc_G17": lambda: sc(x[:2], e["W17"], [B, B], list(np.linspace(-1.0, 1.0, 17))),
        # ---- product_combine
        "pc_double_angle": lambda: pc([([x[0]], [x[0]], 2.0, 1.0)], (), -1.0),
        "pc_P2_m1_const_n2": lambda: pc([([x[0], x[1]], [x[1], x[2]], 0.75, A), ([x[2], x[3]], [x[2], x[3]], -1.5, A)],
                                        [(r, -0.3, A)], 0.5),
        "pc_mixed_levels": lambda: pc(*mixed(A)),
        "pc_mixed_levels_parms_id": lambda: pc(*mixed(2.0 ** 10), 0.25, parms_id=2),
        "pc_P33": lambda: pc([([x[i % 5]], [x[(i + 1) % 5]], e["u33"][i], A) for i in range(33)], (), 1.0),
        # ---- plain_combine
        "plc_uniform": lambda: plc(x[:3], [p[:3], p[3:]]),
        "plc_non_uniform": lambda: plc(x[:3], [[p[0], None, p[2]], p[3:]]),
        "plc_G65": lambda: plc(x[:2], [p[:2]] * 64 + [[None, p[1]]]),
        "plc_rule_m7": lambda: dense(7, 293), "plc_rule_m8": lambda: dense(8, 256),
        "plc_rule_G3": lambda: dense(683, 3), "plc_rule_G4": lambda: dense(512, 4),
        "plc_rule_words_below": lambda: dense(64, 31), "plc_rule_words_at": lambda: dense(64, 32),
        # ---- the drivers
        "ep_degree7_power": one(lambda: alg.evaluate_polynomial(ev, x[0], alg.SIGMOID_COEFFS[7], rk)),
        "ep_degree15_chebyshev": one(lambda: alg.evaluate_polynomial(ev, x[0], _chebyshev(15), rk, basis="chebyshev")),
        "epm_n2_lazy": lambda: alg.evaluate_polynomial_many(ev, x[:2], _chebyshev(7), rk, basis="chebyshev"),
        "epm_n2_eager": lambda: alg.evaluate_polynomial_many(ev, x[:2], _chebyshev(7), rk, basis="chebyshev", lazy=False),
        "eval_mod_r2": lambda: alg.eval_mod(ev, x[:2], _evalmod_plan(ev.ctx.primes), rk),
        # ---- refusals of scalar_combine: every fault it names ...
        "sc_r_weights_shape": lambda: sc(x[:2], [[1.0]], [B, B]),
        "sc_r_no_ciphertext": lambda: sc([], [[]], []),
        "sc_r_wscales_length": lambda: sc(x[:2], [[1.0, 1.0]], [B]),
        "sc_r_consts_shape": lambda: sc(x[:2], [[1.0, 1.0]], [B, B], [1.0, 2.0]),
        "sc_r_level": lambda: sc([x[0], y[0]], [1.0, 1.0], [B, B], parms_id=4),
        "sc_r_size": lambda: sc([x[0], q[0]], [1.0, 1.0], [B, B]),
        "sc_r_wscale_bounds": lambda: sc([x[0]], [1.0], [2.0 ** 200]),
        "sc_r_wscale_negative": lambda: sc([x[0]], [1.0], [-1.0]),
        "sc_r_term_scale_bounds": lambda: sc([x[0]], [1.0], [2.0 ** 150]),
        "sc_r_scale_mismatch": lambda: sc(x[:2], [1.0, 1.0], [B, C]),
        "sc_r_S_bounds": lambda: sc([x[0]], [1.0], [2.0 ** 140 * EDGE], scale=2.0 ** 180),
        "sc_r_transparent": lambda: sc(x[:2], [0.25, 1e-30], [B, B]),
        # ... and two faults at once
        "sc_rr_level_then_mismatch": lambda: sc([y[0], x[0]], [1.0, 1.0], [B, C], parms_id=4),
        "sc_rr_mismatch_then_level": lambda: sc([x[0], y[0]], [1.0, 1.0], [C, B], scale=2.0 ** 70, parms_id=4),
        "sc_rr_transparent_and_S_bounds": lambda: sc([x[0]], [1e-300], [2.0 ** 150]),
        "sc_rr_transparent_then_size": lambda: sc([x[0], q[0]], [0.0, 1.0], [B, B]),
        "sc_rr_shape_and_level": lambda: sc([x[0], y[0]], [[1.0]], [B, B], parms_id=4),
        "sc_rr_transparent_then_mismatch": lambda: sc(x[:2], [0.0, 1.0], [B, C]),
        # ---- refusals of product_combine
        "pc_r_no_product": lambda: pc([], [(r, 1.0, A)]),
        "pc_r_items": lambda: pc([([x[0], x[1]], [x[1]], 1.0, A)]),
        "pc_r_no_item": lambda: pc([([], [], 1.0, A)]),
        "pc_r_lin_items": lambda: pc([x01], [(r, 1.0, A)]),
        "pc_r_level": lambda: pc([([x[0]], [y[0]], 1.0, A)], parms_id=4),
        "pc_r_size": lambda: pc([([x[0]], [q[0]], 1.0, A)]),
        "pc_r_item_levels": lambda: pc([([x[0], y[0]], [x[1], x[1]], 1.0, A)]),
        "pc_r_product_scale_bounds": lambda: pc([([r[0]], [r[1]], 1.0, 1.0)], parms_id=2),
        "pc_r_wscale_bounds": lambda: pc([([x[0]], [x[1]], 1.0, 2.0 ** 200)]),
        "pc_r_term_scale_bounds": lambda: pc([([x[0]], [x[1]], 1.0, 2.0 ** 120)]),
        "pc_r_scale_mismatch": lambda: pc([x01, ([x[2]], [x[3]], 1.0, 2 * A)]),
        "pc_r_lin_level": lambda: pc([x01], [([rl[0]], 1.0, A)], parms_id=4),
        "pc_r_lin_size": lambda: pc([x01], [([q[0]], 1.0, A)]),
        "pc_r_lin_item_levels": lambda: pc([([x[0], x[1]], [x[1], x[2]], 1.0, A)], [([r[0], rl[0]], 1.0, A)]),
        "pc_r_lin_wscale_bounds": lambda: pc([x01], [([r[0]], 1.0, 2.0 ** 200)]),
        "pc_r_lin_term_scale_bounds": lambda: pc([x01], [([r[0]], 1.0, 2.0 ** 120)]),
        "pc_r_lin_scale_mismatch": lambda: pc([x01], [([r[0]], 1.0, 2 * A)]),
        "pc_r_S_bounds": lambda: pc([([x[0]], [x[1]], 1.0, 2.0 ** 100 * EDGE)], scale=2.0 ** 180),
        "pc_r_transparent_product": lambda: pc([([x[0]], [x[1]], 1e-9, A)]),
        "pc_r_transparent_lin": lambda: pc([x01], [([r[0]], 1e-9, A)]),
        "pc_rr_product_mismatch_and_lin_level": lambda: pc([x01, ([x[2]], [x[3]], 1.0, 2 * A)], [([rl[0]], 1.0, A)], parms_id=4),
        "pc_rr_level_then_mismatch": lambda: pc([([x[0]], [y[0]], 1.0, A), ([x[2]], [x[3]], 1.0, 2 * A)], parms_id=4),
        "pc_rr_transparent_and_S_bounds": lambda: pc([([x[0]], [x[1]], 1e-300, 2.0 ** 120)]),
        "pc_rr_transparent_product_and_lin_size": lambda: pc([([x[0]], [x[1]], 1e-9, A)], [([q[0]], 1.0, A)]),
        "pc_rr_items_and_level": lambda: pc([([x[0], x[1]], [y[0]], 1.0, A)], parms_id=4),
        "pc_rr_size_and_item_levels": lambda: pc([([x[0], y[0]], [x[1], q[0]], 1.0, A)]),
        # ---- refusals of plain_combine
        "plc_r_row_length": lambda: plc(x[:2], [p[:3]]),
        "plc_r_no_row": lambda: plc(x[:2], []),
        "plc_r_no_ciphertext": lambda: plc([], [[]]),
        "plc_r_level": lambda: plc([x[0], y[0]], [p[:2]]),
        "plc_r_size": lambda: plc([q[0], q[1]], [p[:2]]),
        "plc_r_scale": lambda: plc([x[0], r[0]], [p[:2]]),
        "plc_r_no_term": lambda: plc(x[:2], [p[:2], [None, None]]),
        "plc_r_plain_level": lambda: plc(x[:2], [[p[0], e["p_low"]]]),
        "plc_r_plain_scale_bounds": lambda: plc(x[:2], [[p[0], e["p_150"]]]),
        "plc_r_plain_scale_mismatch": lambda: plc(x[:2], [[p[0], e["p_30"]]]),
        "plc_r_plain_zero": lambda: plc(x[:2], [[p[0], e["p_zero"]]]),
        "plc_rr_level_and_scale": lambda: plc([x[0], rl[0]], [p[:2]]),
        "plc_rr_size_and_scale": lambda: plc([x[0], q[0]], [p[:2]]),
        "plc_rr_no_term_and_plain_level": lambda: plc(x[:2], [[p[0], e["p_low"]], [None, None]]),
        "plc_rr_plain_zero_then_level": lambda: plc(x[:2], [[e["p_zero"], e["p_low"]]]),
        "plc_rr_row_length_and_level": lambda: plc([x[0], y[0]], [p[:3]]),
        "plc_rr_plain_mismatch_then_zero": lambda: plc(x[:2], [[p[0], e["p_30"]], [e["p_zero"], p[1]]]),
    }


ON_BITS31 = {"ep_degree15_chebyshev", "eval_mod_r2"}
STUBS_ONLY = {"plc_rule_m7", "plc_rule_m8", "plc_rule_G3", "plc_rule_G4", "plc_rule_words_below", "plc_rule_words_at"}
SCENARIOS = list(_scenarios(dict(ev=SimpleNamespace(scalar_combine=0, product_combine=0, plain_combine=0), rk=0, x=[0] * 5)))
CASES = [(b, s) for b in BACKENDS for s in SCENARIOS if b == "stubs" or s not in STUBS_ONLY]


def _run(backend, scenario):
    e = _env(backend, BITS31 if scenario in ON_BITS31 else BITS7)
    ev = e["ev"]
    rec = Recorder(e["be"], only=ENTRIES)
    ev.be = rec
    got = {}
    try:
        outs = _scenarios(e)[scenario]()
    except (ValueError, RuntimeError) as err:
        got["refused"] = [type(err).__name__, str(err)]
    else:
        if backend == "oracle":
            got["results"] = [[c.size(), c.parms_id(), c.scale, digest(np.asarray(c.data))] for c in outs]
    finally:
        ev.be = e["be"]
    if backend == "stubs":   # the stubs return zeros: only their calls count
        got["trace"] = rec.log
    return json.loads(json.dumps(got))


@pytest.mark.parametrize("backend,scenario", CASES)
def test_results_refusals_and_native_calls_equal_the_recorded_ones(backend, scenario):
    want = json.load(open(FIXTURE))[backend][scenario]
    got = _run(backend, scenario)
    assert got.get("refused") == want.get("refused")
    if scenario.split("_")[1] in ("r", "rr"):
        assert "refused" in got
    assert len(got.get("trace", [])) == len(want.get("trace", [])), [c[0] for c in got["trace"]]
    for i, (g, w) in enumerate(zip(got.get("trace", []), want.get("trace", []))):
        assert g == w, f"call {i}: {g[0]}"
    assert got.get("results") == want.get("results")


def test_the_slot_size_function_is_the_header_formula():
    """2P + m + L (P + m + 1) + n (2P + m + 1) words (include/hefx_bootstrap.h), at the slot's size and one above"""
    header = lambda L, n, P, m: 2 * P + m + L * (P + m + 1) + n * (2 * P + m + 1)
    for shape in [(1, 1, 1, 0), (14, 2, 4, 3), (8, 64, 32, 64), (35, 58, 27, 64), (35, 63, 27, 58)]:
        assert capi.product_combine_words(*shape) == header(*shape)
    assert capi.product_combine_words(35, 58, 27, 64) == capi.PRODUCT_COMBINE_MAX_WORDS == 10240
    assert capi.product_combine_words(35, 63, 27, 58) == capi.PRODUCT_COMBINE_MAX_WORDS + 1


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump({b: {s: _run(b, s) for bb, s in CASES if bb == b} for b in BACKENDS}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
