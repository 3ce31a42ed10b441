"""The Python front end of the linear transforms (algorithms.py, Evaluator, parallel.py) must hand the backend the same
calls with the same operands whatever its own shape: every scenario below is run on three backends behind a recorder,
and the trace -- entry name, integer arguments, Galois elements, parents, which plaintext slots are None, a digest of every
array operand and result -- must equal tests/golden/lt_front_traces.json, recorded before the front end was folded.

Backends: (a) the oracle twin, (b) the twin with the rotation-forest entry, (c) the forest twin plus recorders for the five
native linear-transform entries, which return zeros (this pins WHICH native entry is chosen and with what arguments; its
result bits are not compared).  `python -m tests.test_lt_front_trace_cpu` rewrites the fixture."""
import functools
import json
import os

import numpy as np
import pytest

from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import seal as S
from tests.oracle_backend import OracleBackend, _ForestTwin
from tests.trace_recording import Recorder, digest

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "lt_front_traces.json")
N, BITS, SCALE = 4096, [60, 40, 40, 40, 40, 60], 2.0 ** 40


class _NativeTwin(_ForestTwin):
    """the five native entries as stubs: zeros of the result's shape"""

    def linear_transform_plain(self, L, ct, diag_pts, key_elts, keys, hoisted=False):
        return np.zeros((2, L, self.N), dtype=np.uint64)

    def linear_transform_plain_many(self, L, cts, diag_pts, key_elts, keys):
        return [np.zeros((2, L, self.N), dtype=np.uint64) for _ in cts]

    def linear_transform_cipher(self, L, ct, diag_cts, key_elts, keys):
        return np.zeros((3, L, self.N), dtype=np.uint64)

    def linear_transform_plain_bsgs(self, L, ct, shifted_diag_pts, n1, key_elts, keys, hoisted=True):
        return np.zeros((2, L, self.N), dtype=np.uint64)

    def linear_transform_plain_hoisted2_sparse(self, L, ct, d, steps, diag_pts_keylevel, key_elts, keys):
        return np.zeros((2, L, self.N), dtype=np.uint64)


BACKENDS = {"oracle": OracleBackend, "forest": _ForestTwin, "native": _NativeTwin}


@functools.lru_cache(maxsize=None)
def _env(backend):
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(S.CoeffModulus.Create(N, BITS))
    be = BACKENDS[backend](N, parms.coeff_modulus())
    ctx = S.SEALContext.Create(parms, backend=be)
    kg = S.KeyGenerator(ctx, 4)
    enc, encoder, ev = S.Encryptor(ctx, kg.public_key(), 5), S.CKKSEncoder(ctx), S.Evaluator(ctx)
    rng = np.random.default_rng(1)
    e = dict(ctx=ctx, ev=ev, be=be, gk=kg.galois_keys(), gk5=kg.galois_keys([-5, 1, 2, 3, 4]),
             gk6=kg.galois_keys(alg.bsgs_steps(6)))
    pt = lambda d, **kw: encoder.encode(rng.standard_normal(d), SCALE, **kw)
    e["pts"] = lambda d, n=None, **kw: [pt(d, **kw) for _ in range(d if n is None else n)]
    e["ct"] = lambda d: enc.encrypt(pt(d))
    # every operand is drawn here, in one fixed order, so that a scenario run alone sees the operands of the full run
    key_level = dict(parms_id=ctx.key_parms_id())
    e["in"] = dict(
        ctA=e["ct"](5), ctB=e["ct"](5), D5=e["pts"](5), E5=e["pts"](5), D5k=e["pts"](5, **key_level),
        S5={0: pt(5), 3: pt(5)}, S5k={0: pt(5, **key_level), 3: pt(5, **key_level)},
        ct6=e["ct"](6), D6=[encoder.encode(v, SCALE) for v in alg.bsgs_diagonals(rng.standard_normal((6, 6)))],
        ct4=e["ct"](4), C4=[e["ct"](4) for _ in range(4)],
        mA=e["ct"](4), mB=e["ct"](4), Us=e["pts"](4), Ut=e["pts"](4), V=[e["pts"](4)], W=[e["pts"](4)],
        sUs={l: pt(4) for l in (0, 1, 3)}, sUt={l: pt(4) for l in (0, 2)}, sV=[{l: pt(4) for l in (1, 3)}],
        sW=[{2: pt(4)}], P4=[e["pts"](5, 4), e["pts"](5, 4)], P3=e["pts"](5, 3))
    return e


def _scenarios(e):
    ev, gk, gk5, x = e["ev"], e["gk"], e["gk5"], e["in"]
    one = lambda f: lambda: [f()]
    flat = lambda f: lambda: [c for row in f() for c in row]
    return {
        "plain_d5": one(lambda: alg.linear_transform_plain(ev, x["ctA"], x["D5"], gk)),
        "plain_many_d5": lambda: alg.linear_transforms_plain_many(ev, [x["ctA"], x["ctB"]], [x["D5"], x["E5"]], gk),
        "plain_hoisted_d5": one(lambda: alg.linear_transform_plain(ev, x["ctA"], x["D5"], gk5, hoisted=True)),
        "plain_hoisted2_d5": one(lambda: alg.linear_transform_plain(ev, x["ctA"], x["D5k"], gk5, hoisted=2)),
        "sparse_d5": one(lambda: alg.linear_transform_plain_sparse(ev, x["ctA"], 5, x["S5"], gk)),
        "sparse_hoisted_d5": one(lambda: alg.linear_transform_plain_sparse(ev, x["ctA"], 5, x["S5"], gk5, hoisted=True)),
        "sparse_hoisted2_d5": one(lambda: alg.linear_transform_plain_sparse(ev, x["ctA"], 5, x["S5k"], gk5, hoisted=2)),
        "bsgs_d6_hoisted": one(lambda: alg.linear_transform_plain_bsgs(ev, x["ct6"], x["D6"], e["gk6"])),
        "bsgs_d6": one(lambda: alg.linear_transform_plain_bsgs(ev, x["ct6"], x["D6"], e["gk6"], hoisted=False)),
        "cipher_d4": one(lambda: alg.linear_transform_cipher(ev, x["ct4"], x["C4"], gk)),
        "matmul_n2": one(lambda: alg.cc_matrix_multiplication(ev, x["mA"], x["mB"], 2, x["Us"], x["Ut"], x["V"], x["W"], gk)),
        "matmul_sparse_n2": one(lambda: alg.cc_matrix_multiplication_sparse(ev, x["mA"], x["mB"], 2, x["sUs"], x["sUt"],
                                                                            x["sV"], x["sW"], gk)),
        "rotations_of_many": flat(lambda: alg._rotations_of_many(ev, [x["ctA"], x["ctB"]], (1, 3, -2, 5), gk)),
        "rotations_of_many_fused": flat(lambda: alg._rotations_of_many(ev, [x["ctA"], x["ctB"]], (1, 3, -2, 5), gk, x["P4"])),
        "rotations_batched_fused": lambda: alg._rotations_batched(ev, x["ctA"], (0, 1, 3), gk, x["P3"]),
    }


SCENARIOS = ["plain_d5", "plain_many_d5", "plain_hoisted_d5", "plain_hoisted2_d5", "sparse_d5", "sparse_hoisted_d5",
             "sparse_hoisted2_d5", "bsgs_d6_hoisted", "bsgs_d6", "cipher_d4", "matmul_n2", "matmul_sparse_n2",
             "rotations_of_many", "rotations_of_many_fused", "rotations_batched_fused"]


def _run(backend, scenario):
    e = _env(backend)
    ev = e["ev"]
    rec = Recorder(e["be"])
    ev.be = rec
    try:
        outs = _scenarios(e)[scenario]()
    finally:
        ev.be = e["be"]
    got = {"trace": rec.log}
    if backend != "native":   # the stubs return zeros: only their calls count
        got["results"] = [[c.size(), c.parms_id(), c.scale, digest(np.asarray(c.data))] for c in outs]
    return json.loads(json.dumps(got))


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("backend", list(BACKENDS))
def test_backend_calls_and_results_equal_the_recorded_ones(backend, scenario):
    want = json.load(open(FIXTURE))[backend][scenario]
    got = _run(backend, scenario)
    assert len(got["trace"]) == len(want["trace"]), [c[0] for c in got["trace"]]
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, f"call {i}: {g[0]}"
    assert got.get("results") == want.get("results")


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump({b: {s: _run(b, s) for s in SCENARIOS} for b in BACKENDS}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
