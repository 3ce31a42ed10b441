"""CKKS bootstrapping without a GPU: the lazy plan's relinearisation counts, Evaluator.product_combine's op-by-op composition
against the integer statement of include/hefx_bootstrap.h, the sparse secret key, Evaluator.mod_raise, the float model of
bootstrap.plan, and the whole bootstrap on the oracle-backed twin.

THE ERROR GATE is the project's DFT gate, a cap and not a measurement: the largest slot error is at most 1e-3 of the largest
expected value.  The chain and the inputs (tests/bootstrap_cases.py: N = 2048, {60, 50 x 13, 60}, scale 2^50, Hamming weight
32) are chosen so that plan.apply alone -- float64, no noise -- is at least ten times inside it.  Measured here (rescale
division round; written to profiles/bootstrap.json with BOOTSTRAP_RECORD=1), as error / max|expected|:
    plan.apply 1.2e-08 with every |I| up to 12 and 6.7e-08 on the twin's own raised plaintext (the float model's bound on the
    band is the sine's cubic term, (2 pi 2^-10)^2 / 6 = 6.3e-06); twin bootstrap 1.2e-05, after one more square 2.0e-05; the same
    bootstrap on {50, 40 x 13, 60} at scale 2^40: 1.2e-02, which is why the chain is not that one."""
import json
import os

import numpy as np
import pytest

from tests import bootstrap_cases as BC
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = {}
_ENV = {}


def chain(N, bits):
    from seal_fyp_logistic_regression_amd import seal as S
    return S.CoeffModulus.Create(N, bits)


# ---- the lazy plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis", ["power", "chebyshev"])
def test_lazy_never_relinearises_more_than_eager(basis):
    from seal_fyp_logistic_regression_amd import capi, poly
    primes = chain(2048, [60] + [40] * 8 + [60])[:9]
    rng = np.random.default_rng(3)
    for d in range(1, 64):
        coeffs = rng.uniform(0.1, 1.0, d + 1) * rng.choice([-1.0, 1.0], d + 1)
        p = poly.plan(coeffs, basis, primes, 2.0 ** 40)
        assert p.relinearizations(False) == p.muls
        assert p.relinearizations(True) <= p.muls, (basis, d)
        final = p.steps[-1].dst
        for i, c in p.deferred().items():   # the rule, restated: one reader, a COMBINE, not the result
            mul = p.steps[i]
            reads = [j for j, s in enumerate(p.steps)
                     for src in ([t.src for t in s.terms] if s.op == capi.POLY_COMBINE else [s.a, s.b]) if src == mul.dst]
            assert mul.op == capi.POLY_MUL and reads == [c] and p.steps[c].op == capi.POLY_COMBINE and mul.dst != final and c > i


@pytest.mark.parametrize("degree,r,muls,relins,most", [(31, 3, 19, 12, 4), (63, 2, 36, 21, 5)])
def test_the_counts_on_the_evalmod_interpolant(degree, r, muls, relins, most):
    from seal_fyp_logistic_regression_amd import poly
    primes = chain(2048, [50] + [40] * 13 + [60])[:13]
    p = poly.plan(BC.evalmod_interpolant(degree, r), "chebyshev", primes, 2.0 ** 40)
    assert (p.muls, p.relinearizations(True)) == (muls, relins)
    d = p.deferred()
    assert len(d) == muls   # every MUL result is read exactly once, by a COMBINE
    per_node = [sum(1 for c in d.values() if c == j) for j in range(len(p.steps)) if p.steps[j].op == 1]
    assert min(per_node) == 0 and max(per_node) == most


# ---- Evaluator.product_combine, composed op by op, against the integer statement --------------------------------------------
def twin(N, bits, **kw):
    key = (N, tuple(bits), tuple(sorted(kw.items())))
    if key not in _ENV:
        _ENV[key] = BC.make(N, bits, "oracle", **kw)
    return _ENV[key]


def test_the_composition_equals_the_integer_statement():
    from seal_fyp_logistic_regression_amd import seal as S
    from seal_fyp_logistic_regression_amd.poly import weight_residue
    N = 1024
    e = twin(N, [60, 40, 40, 40, 60], seed=2)
    assert getattr(e["ctx"].backend, "product_combine", None) is None
    ev, primes = e["ev"], e["ctx"].primes
    rng = np.random.default_rng(4)

    def ct(level, scale):
        rows = np.stack([np.stack([rng.integers(0, primes[j], N, dtype=np.uint64) for j in range(level)]) for _ in range(2)])
        return S.Ciphertext()._set(e["ctx"].backend.from_host(rows), 2, level, scale)

    n, L, s = 2, 2, 2.0 ** 30
    x, y, z, l0, l1 = ([ct(lv, sc) for _ in range(n)] for lv, sc in ((3, s), (2, s), (4, s), (2, s * s), (3, s * s)))
    products = [(x, y, 0.75, 2.0 ** 20), (z, z, -1.5, 2.0 ** 20), (y, z, 2.0, 2.0 ** 20)]
    lin = [(l0, -0.3, 2.0 ** 20), (l1, 1.25, 2.0 ** 20)]
    S_out = s * s * 2.0 ** 20
    for const in (None, -1.0):
        outs = ev.product_combine(products, lin, const, parms_id=L)
        ures = [[weight_residue(cf, ws, q) for q in primes[:L]] for _, _, cf, ws in products]
        wres = [[weight_residue(cf, ws, q) for q in primes[:L]] for _, cf, ws in lin]
        cres = None if const is None else [weight_residue(const, S_out, q) for q in primes[:L]]
        for i in range(n):
            assert outs[i].size() == 3 and outs[i].parms_id() == L and outs[i].scale == S_out
            host = lambda c: np.asarray(c.data).reshape(2, c.parms_id(), N)
            want = BC.product_model([host(a[i]) for a, _, _, _ in products], [host(b[i]) for _, b, _, _ in products],
                                    [host(c[i]) for c, _, _ in lin], ures, wres, cres, L, primes)
            assert np.array_equal(BC.words(e, outs[i]), want), (const, i)
    # the checks of the op-by-op sequence
    with pytest.raises(ValueError, match="scale mismatch"):
        ev.product_combine(products, [(l0, 1.0, 2.0 ** 21)], parms_id=L)
    with pytest.raises(ValueError, match="higher level"):
        ev.product_combine(products, lin, parms_id=3)
    with pytest.raises(RuntimeError, match="transparent"):
        ev.product_combine([(x, y, 1e-9, 2.0 ** 20)], parms_id=L)
    with pytest.raises(ValueError, match="scale out of bounds"):
        ev.product_combine([(x, y, 1.0, 2.0 ** 60)], parms_id=1)


def test_lazy_and_eager_decode_alike_on_the_twin_and_eager_is_evaluate_polynomial():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    N, bits_ = 2048, [60, 40, 40, 40, 40, 40, 60]
    e = twin(N, bits_, seed=3)
    coeffs = BC.evalmod_interpolant(31, 3)
    xs = [np.linspace(-1.0, 1.0, N // 2), np.cos(np.arange(N // 2))]
    cts = [e["enc"].encrypt(e["encoder"].encode(x, 2.0 ** 40)) for x in xs]
    lazy = alg.evaluate_polynomial_many(e["ev"], cts, coeffs, e["rk"], basis="chebyshev")
    eager = alg.evaluate_polynomial_many(e["ev"], cts, coeffs, e["rk"], basis="chebyshev", lazy=False)
    for x, c, a, b in zip(xs, cts, lazy, eager):
        one = alg.evaluate_polynomial(e["ev"], c, coeffs, e["rk"], basis="chebyshev")
        assert np.array_equal(BC.words(e, b), BC.words(e, one)) and b.scale == one.scale
        assert a.parms_id() == b.parms_id() == 1 and a.scale == b.scale and not np.array_equal(BC.words(e, a), BC.words(e, b))
        want = np.polynomial.chebyshev.chebval(x, coeffs)
        for name, ct in (("lazy", a), ("eager", b)):
            err = float(np.abs(e["encoder"].decode(e["dec"].decrypt(ct)).real - want).max())
            print(f"[bootstrap cpu] degree 31 {name}: max slot error {err:.3e}")
            assert err < 1e-6


# ---- the sparse secret -----------------------------------------------------------------------------------------------------
def test_the_hamming_weight_key():
    from seal_fyp_logistic_regression_amd import seal as S
    N, bits_ = 1024, [60, 40, 60]
    e = twin(N, bits_, seed=2)
    ctx, be = e["ctx"], e["ctx"].backend

    def coefficients(kg):
        host = kg.secret_key().host
        c = np.asarray(be.ntt_inverse(be.from_host(host), 1, ctx.k, 0)).reshape(ctx.k, N)
        signed = [np.where(c[j] > ctx.primes[j] // 2, c[j].astype(np.int64) - int(ctx.primes[j]), c[j].astype(np.int64)) for j in range(ctx.k)]
        assert all(np.array_equal(signed[0], s) for s in signed)   # the same small integers mod every prime
        return signed[0]

    for h in (1, 32, 64):
        a, b, c = (coefficients(S.KeyGenerator(ctx, seed, hamming_weight=h)) for seed in (7, 7, 8))
        assert np.count_nonzero(a) == h and set(np.unique(a)) <= {-1, 0, 1}
        assert np.array_equal(a, b) and not np.array_equal(a, c)
        assert np.array_equal(a, S.sparse_ternary_secret(S._key32(7), N, h))
    for bad in (0, N + 1):
        with pytest.raises(ValueError, match="hamming_weight"):
            S.KeyGenerator(ctx, 7, hamming_weight=bad)
    # None: the uniform ternary secret of sampler stream 2, and the public key of stream 2 -- word for word what it was
    kg, sparse = S.KeyGenerator(ctx, 7), S.KeyGenerator(ctx, 7, hamming_weight=32)
    was = be.ntt_forward(be.sample("ternary", S._key32(7), 2, 1, ctx.k), 1, ctx.k, 0)
    assert np.array_equal(kg.secret_key().host, np.asarray(was).reshape(ctx.k, N))
    assert np.array_equal(kg.secret_key().host, e["kg"].secret_key().host) == (7 == 2)
    assert np.array_equal(S.KeyGenerator(ctx, 2).secret_key().host, e["kg"].secret_key().host)
    assert np.count_nonzero(coefficients(kg)) > N // 2
    assert kg._stream == sparse._stream == 1   # the other keys keep their sampler streams


# ---- mod_raise ---------------------------------------------------------------------------------------------------------------
def test_mod_raise_equals_lift_coefficients():
    from seal_fyp_logistic_regression_amd import seal as S
    N = 1024
    e = twin(N, [60, 40, 40, 40, 60], seed=2)
    ctx, be, ev = e["ctx"], e["ctx"].backend, e["ev"]
    ct = e["enc"].encrypt(e["encoder"].encode(np.linspace(-1, 1, N // 2), 2.0 ** 30, parms_id=2))
    assert getattr(be, "mod_raise", None) is None
    for target in (3, 4, None):
        up = ev.mod_raise(ct, target)
        L_out = target or ctx.first_parms_id()
        assert up.size() == 2 and up.parms_id() == L_out and up.scale == ct.scale
        got, src = BC.words(e, up), BC.words(e, ct)
        assert np.array_equal(got[:, :2], src)
        for p in range(2):
            coef = np.asarray(be.ntt_inverse(be.from_host(src[p]), 1, 2, 0)).reshape(2, N)
            lifted = S.lift_coefficients(coef, ctx.primes, 2, L_out)
            assert np.array_equal(got[p, 2:], np.asarray(be.ntt_forward(be.from_host(lifted), 1, L_out - 2, 2)).reshape(L_out - 2, N))
        # the raised ciphertext decrypts to the same message plus a multiple of Q_in: dropped again it is the input
        assert np.array_equal(BC.words(e, ev.mod_switch_to_inplace(up.copy(), 2)), src)
    assert np.array_equal(BC.words(e, ev.mod_raise(ct, 2)), BC.words(e, ct))
    with pytest.raises(ValueError, match="target level"):
        ev.mod_raise(ct, 1)
    with pytest.raises(ValueError, match="target level"):
        ev.mod_raise(ct, 5)


def test_mod_raise_refuses_rings_above_16384():
    from types import SimpleNamespace
    from seal_fyp_logistic_regression_amd import seal as S
    ev = S.Evaluator.__new__(S.Evaluator)
    ev.ctx = SimpleNamespace(N=32768, first_parms_id=lambda: 3)
    ev.be = None
    with pytest.raises(ValueError, match="16384"):
        ev.mod_raise(S.Ciphertext()._set(None, 2, 1, 1.0), 3)


# ---- the planner and its float model ---------------------------------------------------------------------------------------
def bootstrap_plan():
    from seal_fyp_logistic_regression_amd import bootstrap as B
    if "plan" not in _ENV:
        _ENV["plan"] = B.plan(BC.N, chain(BC.N, BC.CHAIN_BITS), BC.SCALE)
    return _ENV["plan"]


def test_the_plan_and_its_refusals():
    from seal_fyp_logistic_regression_amd import bootstrap as B
    primes = chain(BC.N, BC.CHAIN_BITS)
    p = bootstrap_plan()
    assert (p.K, p.r, p.degree, p.c2s.levels, p.s2c.levels) == (12, 3, 31, 2, 2)
    assert p.levels() == 12 and p.top_level == 14 and p.evalmod_level == 12 and p.s2c_level == 4 and p.result_level == 2
    assert np.abs(p.coeffs).max() <= 0.64 and p.model_error <= 1e-5
    assert p.galois_steps() == sorted(set(p.c2s.galois_steps()) | set(p.s2c.galois_steps()))
    assert p.key_switches(False) - p.key_switches(True) == 2 * 7   # 7 of 19 relinearisations saved on either chain
    assert p.c2s.primes() == [primes[13], primes[12]] and p.s2c.primes() == [primes[3], primes[2]]
    with pytest.raises(ValueError, match="not enough levels"):
        B.plan(BC.N, primes[:12] + primes[-1:], BC.SCALE)
    with pytest.raises(ValueError, match="misses the precision"):
        B.plan(BC.N, primes, BC.SCALE * 2.0 ** 5)        # q_0 / scale = 2^5: the sine's cubic term alone is 6e-3
    with pytest.raises(ValueError, match="misses the precision"):
        B.plan(BC.N, primes, BC.SCALE, degree=15)        # too low a degree for K = 12, r = 3
    with pytest.raises(ValueError, match="misses the precision"):
        B.plan(BC.N, primes, BC.SCALE, r=2)              # the issue's note: r = 2 needs degree 63 ...
    assert B.plan(BC.N, chain(BC.N, BC.CHAIN_BITS[:1] + [50] * 14 + [60]), BC.SCALE, r=2, degree=63).model_error <= 1e-5


def test_apply_against_plain_mod_reduction():
    p = bootstrap_plan()
    q0 = p.primes[0]
    v = BC.bootstrap_input()
    m = np.round(p.coefficients(v.astype(np.complex128)))   # the encoder's integer polynomial, to rounding
    assert np.abs(m).max() <= BC.SCALE
    rng = np.random.default_rng(6)
    I = rng.integers(-p.K, p.K + 1, BC.N)
    I[:2 * p.K + 1] = np.arange(-p.K, p.K + 1)                # every integer part the plan allows occurs
    t = [int(a) + q0 * int(b) for a, b in zip(m, I)]          # Python integers: q_0 K is above 2^53
    centred = np.array([float((x + q0 // 2) % q0 - q0 // 2) for x in t])
    assert np.array_equal(centred, m)                         # plain mod reduction gives the message back
    out = p.apply(np.array([float(x) for x in t]))            # (float64 of t: 2^-39 of the scale at most)
    err = float(np.abs(p.slots(out) - v).max() / np.abs(v).max())
    RECORD["plan_apply"] = err
    print(f"[bootstrap cpu] plan.apply: max slot error / max|expected| {err:.3e}")
    assert err <= BC.CAP / 10


# ---- the whole bootstrap on the oracle-backed twin ---------------------------------------------------------------------------
def test_bootstrap_on_the_oracle():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    p = bootstrap_plan()
    e = twin(BC.N, BC.CHAIN_BITS, seed=BC.KEY_SEED, hamming_weight=BC.HAMMING_WEIGHT, galois_steps=tuple(p.galois_steps()), conjugate=True)
    v = BC.bootstrap_input()
    ct = e["enc"].encrypt(e["encoder"].encode(v, BC.SCALE, parms_id=1))
    t, I = BC.raised_coefficients(e, ct, p.top_level)
    print(f"[bootstrap cpu] max |I| = {int(np.abs(I).max())} (K = {p.K})")
    assert np.abs(I).max() <= 12                              # a condition on the input (seed 1: 6)
    out = alg.bootstrap(e["ev"], ct, p, e["gk"], e["rk"])
    assert out.size() == 2 and out.parms_id() == p.result_level == 2 and abs(out.scale / BC.SCALE - 1.0) < 1e-12
    err = float(np.abs(e["encoder"].decode(e["dec"].decrypt(out)).real - v).max() / np.abs(v).max())
    sq = e["ev"].rescale_to_next_inplace(e["ev"].relinearize_inplace(e["ev"].square(out), e["rk"]))
    err2 = float(np.abs(e["encoder"].decode(e["dec"].decrypt(sq)).real - v * v).max() / np.abs(v).max())
    model = p.apply(np.array([float(int(x)) for x in t]))
    err_model = float(np.abs(p.slots(model) - v).max() / np.abs(v).max())
    RECORD.update(bootstrap=err, bootstrap_then_square=err2, plan_apply_on_the_same_input=err_model, max_abs_I=int(np.abs(I).max()))
    print(f"[bootstrap cpu] twin bootstrap: error {err:.3e}, after one more square {err2:.3e}, plan.apply alone {err_model:.3e}")
    assert err <= BC.CAP and err2 <= 2 * BC.CAP and err_model <= BC.CAP / 10
    with pytest.raises(ValueError, match="last prime"):
        alg.bootstrap(e["ev"], out, p, e["gk"], e["rk"])


def test_the_library_carries_the_new_surface(tmp_path):
    """built from the new source and header, exported, bound, and the header is plain C like hefx.h"""
    import re
    import subprocess
    from seal_fyp_logistic_regression_amd import _build, capi
    assert "hefx_bootstrap.hip" in _build.SOURCES and "../../include/hefx_bootstrap.h" in _build.HEADERS
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.library_path()], text=True)
    assert set(capi.BOOTSTRAP_SYMBOLS) <= set(re.findall(r" T (hefx_[a-z_0-9]+)", out))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hefx_bootstrap.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(hefx_[a-z_0-9]+)\s*\(", src))) == capi.BOOTSTRAP_SYMBOLS == ["hefx_product_combine"]
    assert not set(capi.BOOTSTRAP_SYMBOLS) & set(capi.EXPORTED_SYMBOLS)   # hefx.h's table stays as it is
    c = tmp_path / "t.c"
    c.write_text('#include "hefx_bootstrap.h"\nint main(void) { return HEFX_PRODUCT_COMBINE_MAX_PRODUCTS + HEFX_PRODUCT_COMBINE_MAX_LIN '
                 '+ HEFX_PRODUCT_COMBINE_MAX_ITEMS; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (capi.PRODUCT_COMBINE_MAX_PRODUCTS, capi.PRODUCT_COMBINE_MAX_LIN, capi.PRODUCT_COMBINE_MAX_ITEMS) == (32, 64, 64)


def test_record_the_measured_errors():
    """BOOTSTRAP_RECORD=1: the figures of this run go into the precision section of profiles/bootstrap.json"""
    if "plan_apply" not in RECORD:
        test_apply_against_plain_mod_reduction()
    if "bootstrap" not in RECORD:
        test_bootstrap_on_the_oracle()
    if os.environ.get("BOOTSTRAP_RECORD"):
        path = os.path.join(ROOT, "profiles", "bootstrap.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["precision_oracle_twin_n2048"] = {"chain_bits": BC.CHAIN_BITS, "scale": "2^50", "hamming_weight": BC.HAMMING_WEIGHT,
                                              "key_seed": BC.KEY_SEED, "cap": BC.CAP, "unit": "max error / max|expected|",
                                              "rescale": "round" if OracleBackend.rescale_rounded else "floor", **RECORD}
        json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
        open(path, "a").write("\n")
