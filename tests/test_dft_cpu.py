"""The planner of the homomorphic DFT (seal_fyp_logistic_regression_amd/dft.py) and algorithms.coeffs_to_slots /
slots_to_coeffs on the oracle-backed twin (no GPU).

FACTORISATION, N = 16 .. 1024, every `levels` from 1 to s = log2(N/2), both directions: the product of the plan's stage matrices,
rebuilt dense from its diagonals, is F_s..F_1 (SlotToCoeff) or (1/N) F_1^H..F_s^H (CoeffToSlot) within 1e-9; the three
identities of dft.py's docstring hold within 1e-9 against the dense U built from the ROOTS zeta^(3^j i), not from the factors;
every stage in its baby/giant form on plain vectors (numpy rolls) is its matrix-vector product; and algorithms' executor, run
on plain vectors behind a counting stand-in for the evaluator, asks for exactly plan.galois_steps() and plan.key_switches()
key switches and returns the same vectors.

END TO END on the oracle twin: N = 1024, primes {60, 40 x 7, 60} through CoeffModulus.Create, scale 2^40, levels = 3, host
encoder, z seeded and uniform in the unit disc.
THE ERROR GATE is a cap, not a measurement: the largest slot error is at most 1e-3 * max|expected|.  A wrong diagonal or split
gives an error of the order of max|expected|; an imprecise plan does not come near the cap.  Measured here (rescale division
round; written to profiles/dft.json with DFT_RECORD=1), as error / max|expected|:
    coeffs_to_slots 2.0e-07, slots_to_coeffs 3.0e-06, round trip 1.6e-07."""
import json
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from seal_fyp_logistic_regression_amd import _build, capi, dft
from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import seal as S
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [16, 32, 64, 128, 256, 512, 1024]
Q = (1 << 40) - 87   # (the planner only carries the primes along; any odd number does for the algebra)
CAP = 1e-3
RECORD = {}


def dense_U(N):
    """the decoding matrix from the roots: U[j][i] = zeta^(3^j i)"""
    n, M = N // 2, 2 * N
    r = np.array([pow(3, j, M) for j in range(n)], dtype=np.int64)
    return np.exp(2j * np.pi * ((r[:, None] * np.arange(N)[None, :]) % M) / M)


def chain_product(plan, which):
    """the dense product of the stage matrices, the chain `which` (0: the a-chain, 1: the chain that meets D)"""
    P = np.eye(plan.n, dtype=np.complex128)
    for st in plan.stages:
        P = dft.dense(st.mats[which if len(st.mats) > 1 else 0]) @ P
    return P


# ---- the algebra ------------------------------------------------------------------------------------------------------------
def test_generator_3_facts():
    """what the derivation rests on, at N = 16 and 64: U1 = D U0 with D = diag(i (-1)^j); U0 = F_s..F_1 R; U0 is NOT a scaled
    unitary (entries of U0^H U0 at distance N/4 from the diagonal); the second twiddle of F_1 is not minus the first"""
    for N in (16, 64):
        n = N // 2
        s = n.bit_length() - 1
        U = dense_U(N)
        U0, U1 = U[:, :n], U[:, n:]
        assert np.abs(U1 - np.diag(dft.d_vector(n)) @ U0).max() < 1e-9
        P = np.eye(n)
        for t in range(1, s + 1):
            P = dft.dense(dft.butterfly_factor(N, t)) @ P
        R = dft.bit_reversal(n)
        assert np.abs(U0 - P[:, np.argsort(R)]).max() < 1e-9 and (np.argsort(R) == R).all()
        gram = U0.conj().T @ U0
        off = np.abs(gram - np.diag(np.diag(gram)))
        i, j = np.unravel_index(np.argmax(off), off.shape)
        assert off.max() > 1.0 and min((i - j) % n, (j - i) % n) == N // 4
        F1 = dft.dense(dft.butterfly_factor(N, 1))
        assert abs(F1[1, 1] + F1[0, 1]) > 0.1
        for t in range(2, s + 1):   # every other stage is a +- butterfly
            F = dft.dense(dft.butterfly_factor(N, t))
            h = 1 << (t - 1)
            assert np.abs(F[h:2 * h, h:2 * h] + F[:h, h:2 * h]).max() < 1e-12


def test_diagonal_counts_of_the_issue():
    """a product of r adjacent factors has at most 2^(r+1) - 1 diagonals: at n = 32, 7 for r = 2 (+-1..3, and +-4, 8, 12), 15
    for r = 3; every entry of such a product has modulus 1 (one path per entry)"""
    N, n = 64, 32
    F = {t: dft.butterfly_factor(N, t) for t in range(1, 6)}
    p12 = dft.matmul(F[2], F[1])
    assert sorted(p12) == [0, 1, 2, 3, 29, 30, 31]
    p34 = dft.matmul(F[4], F[3])
    assert sorted(p34) == [0, 4, 8, 12, 20, 24, 28]
    p123 = dft.matmul(F[3], p12)
    assert len(p123) == 15
    assert sorted(F[5]) == [0, 16] and sorted(F[2]) == [0, 2, 30]
    for M in (p12, p34, p123):
        D = np.abs(dft.dense(M))
        assert np.allclose(D[D > 0], 1.0, atol=1e-12)


class VecBackend:
    """ciphertext payload = the plain slot vector; a Galois key = the rotation step it stands for (or "conj")"""

    def __init__(self):
        self.switches, self.steps = 0, set()

    def apply_galois_batch(self, L, datas, elts, keys):
        self.switches += len(datas)
        self.steps.update(keys)
        return [np.roll(d, -k) for d, k in zip(datas, keys)]

    def apply_galois(self, L, data, elt, key):
        assert key == "conj"
        self.switches += 1
        self.steps.add(key)
        return np.conj(data)


class VecEvaluator:
    """the calls algorithms._dft_stage makes, on plain vectors"""

    def __init__(self, N):
        self.ctx, self.be = SimpleNamespace(N=N), VecBackend()

    def plain_combine(self, cts, rows):
        assert all(any(p is not None for p in r) for r in rows)
        return [S.Ciphertext()._set(sum(p.data * c.data for c, p in zip(cts, r) if p is not None), 2, cts[0].parms_id(), 1.0)
                for r in rows]

    def add_many(self, cts):
        return S.Ciphertext()._set(sum(c.data for c in cts), 2, cts[0].parms_id(), 1.0)

    def add(self, a, b):
        return self.add_many([a, b])

    def complex_conjugate(self, a, gk):
        return S.Ciphertext()._set(self.be.apply_galois(a.parms_id(), a.data, 2 * self.ctx.N - 1, gk.key(2 * self.ctx.N - 1)), 2, a.parms_id(), 1.0)

    def rescale_to_next_many_inplace(self, cts):
        return [c._set(c.data, 2, c.parms_id() - 1, 1.0) for c in cts]


def vec_run(plan, xs):
    N = plan.N
    ev = VecEvaluator(N)
    gk = S.KSwitchKeys()
    for s in plan.galois_steps():
        gk.keys[S.galois_elt_from_step(s, N)] = s
    if plan.direction == dft.C2S:
        gk.keys[2 * N - 1] = "conj"
    table = [[[[None if st.rotated(c, g, b) is None else SimpleNamespace(data=st.rotated(c, g, b)) for b in st.babies]
               for g in st.giants] for c in range(len(st.mats))] for st in plan.stages]
    cts = [S.Ciphertext()._set(np.asarray(x, dtype=np.complex128), 2, plan.levels + 1, 1.0) for x in xs]
    if plan.direction == dft.C2S:
        outs = alg.coeffs_to_slots(ev, cts[0], plan, gk, encoded=table)
    else:
        outs = [alg.slots_to_coeffs(ev, cts[0], cts[1], plan, gk, encoded=table)]
    assert all(o.parms_id() == 1 for o in outs)
    return [o.data for o in outs], ev.be


@pytest.mark.parametrize("N", SIZES)
def test_factorisation_identities_split_and_key_switch_counts(N):
    n = N // 2
    s = n.bit_length() - 1
    U = dense_U(N)
    R = dft.bit_reversal(n)
    F = np.eye(n, dtype=np.complex128)
    for t in range(1, s + 1):
        F = dft.dense(dft.butterfly_factor(N, t)) @ F
    D = np.diag(dft.d_vector(n))
    rng = np.random.default_rng(N)
    m = rng.standard_normal(N)
    a, b = m[:n], m[n:]
    z = U @ m
    tol = 1e-9
    for levels in range(1, s + 1):
        c2s = dft.plan(N, levels, dft.C2S, [Q] * levels)
        s2c = dft.plan(N, levels, dft.S2C, [Q] * levels)
        assert len(c2s.stages) == len(s2c.stages) == levels
        # the product of the stage matrices
        assert np.abs(chain_product(s2c, 0) - F).max() < tol * n and np.abs(chain_product(s2c, 1) - D @ F).max() < tol * n
        assert np.abs(chain_product(c2s, 0) - F.conj().T / N).max() < tol
        assert np.abs(chain_product(c2s, 1) - F.conj().T @ D.conj().T / N).max() < tol
        # the three identities, against U from the roots
        assert np.abs(2 * (chain_product(c2s, 0) @ z).real - a[R]).max() < tol * np.abs(m).max() * 10
        assert np.abs(2 * (chain_product(c2s, 1) @ z).real - b[R]).max() < tol * np.abs(m).max() * 10
        assert np.abs(chain_product(s2c, 0) @ a[R] + chain_product(s2c, 1) @ b[R] - z).max() < tol * np.abs(z).max() * 10
        for plan in (c2s, s2c):
            sizes = sorted(len(st.indices) for st in plan.stages)
            for st in plan.stages:
                # every index is giant + baby exactly once; entries of modulus <= 1
                assert sorted((g + bb) % n for g, bb in st.pairs) == st.indices
                assert {g for g, _ in st.pairs} == set(st.giants) and {bb for _, bb in st.pairs} == set(st.babies)
                assert max(np.abs(v).max() for mat in st.mats for v in mat.values()) <= 1.0 + 1e-12
                # the baby/giant form with numpy rolls is the matrix-vector product
                xs = [rng.standard_normal(n) + 1j * rng.standard_normal(n) for _ in range(st.inputs)]
                got = st.apply(xs)
                if st.mode == "split":
                    want = [dft.dense(mat) @ xs[0] for mat in st.mats]
                elif st.mode == "lockstep":
                    want = [dft.dense(st.mats[0]) @ x for x in xs]
                else:
                    want = [dft.dense(st.mats[0]) @ xs[0] + dft.dense(st.mats[1]) @ xs[1]]
                assert len(got) == len(want) == st.outputs
                for g_, w_ in zip(got, want):
                    assert np.abs(g_ - w_).max() < tol * n
            assert sizes[-1] <= 2 ** (-(-s // levels) + 1) - 1 or levels == 1
        # algorithms' executor on plain vectors: the vectors, the steps and the count
        (ra, rb), be = vec_run(c2s, [z])
        assert np.abs(ra - a[R]).max() < 1e-8 * np.abs(m).max() and np.abs(rb - b[R]).max() < 1e-8 * np.abs(m).max()
        assert be.switches == c2s.key_switches() and be.steps == set(c2s.galois_steps()) | {"conj"}
        (zz,), be = vec_run(s2c, [a[R], b[R]])
        assert np.abs(zz - z).max() < 1e-8 * np.abs(z).max()
        assert be.switches == s2c.key_switches() and be.steps == set(s2c.galois_steps())
        assert 0 not in c2s.galois_steps() and all(0 < st_ < n for st_ in c2s.galois_steps() + s2c.galois_steps())


def test_the_split_needs_fewer_rotations_than_one_per_diagonal():
    """levels = 3 at N = 4096: up to 31 diagonals a stage, well under half as many rotations"""
    plan = dft.plan(4096, 3, dft.C2S, [Q] * 3)
    for st in plan.stages:
        nz = sum(1 for b in st.babies if b) + sum(1 for g in st.giants if g)
        assert nz < len(st.indices) / 2 and len(st.babies) * len(st.giants) >= len(st.indices)
    assert plan.key_switches() == sum(st.key_switches() for st in plan.stages) + 2


def test_factor_is_folded_evenly():
    N, levels = 64, 3
    base = dft.plan(N, levels, dft.S2C, [Q] * levels)
    scaled = dft.plan(N, levels, dft.S2C, [Q] * levels, factor=0.125)
    for a, b in zip(base.stages, scaled.stages):
        for d in a.mats[0]:
            assert np.allclose(b.mats[0][d], a.mats[0][d] * 0.5)
    assert np.abs(chain_product(scaled, 0) - 0.125 * chain_product(base, 0)).max() < 1e-12


def test_refusals_on_the_plan():
    N = 1024   # s = 9
    with pytest.raises(ValueError, match="levels must lie in 1 .. 9"):
        dft.plan(N, 0, dft.C2S, [Q] * 3)
    with pytest.raises(ValueError, match="levels must lie in 1 .. 9"):
        dft.plan(N, 10, dft.S2C, [Q] * 10)
    with pytest.raises(ValueError, match="not enough primes"):
        dft.plan(N, 3, dft.C2S, [Q] * 2)
    with pytest.raises(ValueError, match="direction"):
        dft.plan(N, 3, "sideways", [Q] * 3)
    with pytest.raises(ValueError, match="power of two"):
        dft.plan(1000, 3, dft.C2S, [Q] * 3)
    dft.plan(N, 9, dft.C2S, [Q] * 9)
    dft.plan(N, 3, dft.C2S, [Q] * 5)   # more primes than stages are fine: the first `levels` are used


# ---- end to end on the oracle-backed twin ---------------------------------------------------------------------------------
N_E2E, LEVELS, SCALE = 1024, 3, 2.0 ** 40
BITS = [60] + [40] * 7 + [60]
_ENV = {}


def env():
    if not _ENV:
        parms = S.EncryptionParameters("ckks")
        parms.set_poly_modulus_degree(N_E2E)
        parms.set_coeff_modulus(S.CoeffModulus.Create(N_E2E, BITS))
        ctx = S.SEALContext.Create(parms, backend=OracleBackend(N_E2E, parms.coeff_modulus()))
        kg = S.KeyGenerator(ctx, 3)
        top = ctx.first_parms_id()
        q = ctx.primes
        plans = {"c2s": dft.plan(N_E2E, LEVELS, dft.C2S, [q[top - 1 - i] for i in range(LEVELS)]),
                 "s2c": dft.plan(N_E2E, LEVELS, dft.S2C, [q[top - 1 - i] for i in range(LEVELS)]),
                 "back": dft.plan(N_E2E, LEVELS, dft.S2C, [q[top - LEVELS - 1 - i] for i in range(LEVELS)])}
        steps = sorted(set(plans["c2s"].galois_steps()) | set(plans["s2c"].galois_steps()))
        encoder = S.CKKSEncoder(ctx, device_encode=False)
        _ENV.update(ctx=ctx, kg=kg, enc=S.Encryptor(ctx, kg.public_key(), 4), dec=S.Decryptor(ctx, kg.secret_key()),
                    encoder=encoder, ev=S.Evaluator(ctx), gk=kg.galois_keys(steps, conjugate=True), plans=plans, top=top,
                    tables={"c2s": plans["c2s"].encode(encoder, top), "s2c": plans["s2c"].encode(encoder, top),
                            "back": plans["back"].encode(encoder, top - LEVELS)})
    return _ENV


def inputs():
    """z uniform in the unit disc (seeded); its real coefficients from the DENSE definition, m = (2/N) Re(U^H z); real slot
    vectors of modulus <= 1/n for SlotToCoeff and the z they must give, again through the dense U"""
    n = N_E2E // 2
    rng = np.random.default_rng(2026)
    z = np.sqrt(rng.uniform(0, 1, n)) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
    U = dense_U(N_E2E)
    m = 2.0 / N_E2E * (U.conj().T @ z).real
    R = dft.bit_reversal(n)
    xa, xb = rng.uniform(-1.0 / n, 1.0 / n, n), rng.uniform(-1.0 / n, 1.0 / n, n)
    coeffs = np.empty(N_E2E)
    coeffs[R], coeffs[n + R] = xa, xb      # x_a[i] = m_R(i), x_b[i] = m_(n + R(i))
    return z, m[:n][R], m[n:][R], xa, xb, U @ coeffs


def decoded(e, ct):
    return e["encoder"].decode(e["dec"].decrypt(ct))


def gate(name, got, want):
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"[dft] {name}: max error / max|expected| = {rel:.3e} (max|expected| {np.abs(want).max():.3e})")
    RECORD[name] = rel
    assert rel <= CAP, (name, rel)


def test_coeffs_to_slots_on_the_oracle():
    e = env()
    z, a, b, *_ = inputs()
    ct = e["enc"].encrypt(e["encoder"].encode(z, SCALE))
    be = e["ctx"].backend
    assert not hasattr(be, "plain_combine")    # (this file runs the composition; the fused call is tests/test_gpu_dft.py)
    ca, cb = alg.coeffs_to_slots(e["ev"], ct, e["plans"]["c2s"], e["gk"], encoded=e["tables"]["c2s"])
    for c in (ca, cb):
        assert c.size() == 2 and c.parms_id() == e["top"] - LEVELS
        assert abs(c.scale - SCALE) <= 2.0 ** -40 * SCALE      # tracked through the stages, not set
    da, db = decoded(e, ca), decoded(e, cb)
    assert np.abs(da.imag).max() < 1e-6 and np.abs(db.imag).max() < 1e-6
    gate("coeffs_to_slots", np.concatenate([da, db]), np.concatenate([a, b]).astype(np.complex128))


def test_slots_to_coeffs_on_the_oracle():
    e = env()
    *_, xa, xb, want = inputs()
    ca = e["enc"].encrypt(e["encoder"].encode(xa, SCALE))
    cb = e["enc"].encrypt(e["encoder"].encode(xb, SCALE))
    out = alg.slots_to_coeffs(e["ev"], ca, cb, e["plans"]["s2c"], e["gk"], encoded=e["tables"]["s2c"])
    assert out.size() == 2 and out.parms_id() == e["top"] - LEVELS and abs(out.scale - SCALE) <= 2.0 ** -40 * SCALE
    gate("slots_to_coeffs", decoded(e, out), want)


def test_round_trip_on_the_oracle():
    e = env()
    z = inputs()[0]
    ct = e["enc"].encrypt(e["encoder"].encode(z, SCALE))
    ca, cb = alg.coeffs_to_slots(e["ev"], ct, e["plans"]["c2s"], e["gk"], encoded=e["tables"]["c2s"])
    back = alg.slots_to_coeffs(e["ev"], ca, cb, e["plans"]["back"], e["gk"], encoded=e["tables"]["back"])
    assert back.parms_id() == e["top"] - 2 * LEVELS
    gate("round_trip", decoded(e, back), z)


def test_record_the_measured_errors():
    """DFT_RECORD=1: the figures of this run go into the precision section of profiles/dft.json"""
    for name, f in (("coeffs_to_slots", test_coeffs_to_slots_on_the_oracle), ("slots_to_coeffs", test_slots_to_coeffs_on_the_oracle),
                    ("round_trip", test_round_trip_on_the_oracle)):
        if name not in RECORD:
            f()
    assert all(v <= CAP for v in RECORD.values())
    if os.environ.get("DFT_RECORD"):
        path = os.path.join(ROOT, "profiles", "dft.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["precision_oracle_twin_n1024"] = {"scale": "2^40", "levels": LEVELS, "cap": CAP, "unit": "max error / max|expected|",
                                              "rescale": "round" if OracleBackend.rescale_rounded else "floor", **RECORD}
        json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
        open(path, "a").write("\n")


def test_wrong_plans_are_refused_by_the_executors():
    e = env()
    ct = e["enc"].encrypt(e["encoder"].encode([1.0], SCALE))
    with pytest.raises(ValueError, match="not a CoeffToSlot plan"):
        alg.coeffs_to_slots(e["ev"], ct, e["plans"]["s2c"], e["gk"])
    with pytest.raises(ValueError, match="not a SlotToCoeff plan"):
        alg.slots_to_coeffs(e["ev"], ct, ct, e["plans"]["c2s"], e["gk"])
    with pytest.raises(ValueError, match="does not drop the primes"):
        e["plans"]["c2s"].encode(e["encoder"], e["top"] - 1)
    with pytest.raises(ValueError, match="Galois key not present"):
        alg.coeffs_to_slots(e["ev"], ct, e["plans"]["c2s"], S.KSwitchKeys(), encoded=e["tables"]["c2s"])


# ---- Evaluator.plain_combine, complex_conjugate and the conjugation key on a backend without the fused kernel -------------
def test_plain_combine_is_the_integer_combination_and_makes_the_checks_of_the_sequence():
    e = env()
    ev, q, N = e["ev"], e["ctx"].primes, N_E2E
    L = e["top"]
    rng = np.random.default_rng(8)
    cts = [e["enc"].encrypt(e["encoder"].encode(rng.standard_normal(4), SCALE)) for _ in range(3)]
    pts = [e["encoder"].encode(rng.standard_normal(N // 2), SCALE) for _ in range(4)]
    rows = [[pts[0], None, pts[1]], [None, pts[2], None], [pts[3], pts[3], pts[0]]]
    outs = ev.plain_combine(cts, rows)
    C = [np.asarray(c.data).reshape(2, L, N).astype(object) for c in cts]
    for r, o in zip(rows, outs):
        assert o.parms_id() == L and o.size() == 2 and o.scale == SCALE * SCALE
        got = np.asarray(o.data).reshape(2, L, N)
        for j in range(L):
            for p in range(2):
                want = sum(C[k][p, j] * np.asarray(pt.data).reshape(L, N)[j].astype(object) for k, pt in enumerate(r) if pt is not None) % q[j]
                assert (got[p, j].astype(object) == want).all()
    # ... which is multiply_plain per term and add_many
    seq = ev.add_many([ev.multiply_plain(cts[0], pts[3]), ev.multiply_plain(cts[1], pts[3]), ev.multiply_plain(cts[2], pts[0])])
    assert np.array_equal(np.asarray(seq.data), np.asarray(outs[2].data))
    with pytest.raises(ValueError, match="an output has no term"):
        ev.plain_combine(cts, [[pts[0], None, None], [None, None, None]])
    with pytest.raises(ValueError, match="one plaintext"):
        ev.plain_combine(cts, [[pts[0], None]])
    low = e["encoder"].encode([1.0], SCALE, parms_id=L - 1)
    with pytest.raises(ValueError, match="plain_ntt parameter mismatch"):
        ev.plain_combine(cts, [[pts[0], low, None]])
    with pytest.raises(ValueError, match="scale mismatch"):
        ev.plain_combine(cts, [[pts[0], e["encoder"].encode([1.0], SCALE * 2), None]])
    with pytest.raises(RuntimeError, match="transparent"):
        ev.plain_combine(cts, [[pts[0], e["encoder"].encode([0.0], SCALE), None]])
    other = cts[1].copy()
    other.scale = SCALE * 2
    with pytest.raises(ValueError, match="scale mismatch"):
        ev.plain_combine([cts[0], other, cts[2]], rows)


def test_complex_conjugate_and_its_key():
    e = env()
    z = inputs()[0]
    ct = e["enc"].encrypt(e["encoder"].encode(z, SCALE))
    cc = e["ev"].complex_conjugate(ct, e["gk"])
    assert cc.parms_id() == ct.parms_id() and cc.scale == ct.scale
    assert np.abs(decoded(e, cc) - np.conj(z)).max() < 1e-6
    with pytest.raises(ValueError, match="Galois key not present"):
        e["ev"].complex_conjugate(ct, S.KSwitchKeys())
    # conjugate=False is the key set it always was; conjugate=True adds 2N - 1 behind it, the other keys' streams unchanged
    ctx = e["ctx"]
    plain = S.KeyGenerator(ctx, 11).galois_keys([1, 5])
    both = S.KeyGenerator(ctx, 11).galois_keys([1, 5], conjugate=True)
    assert sorted(both.keys) == sorted(list(plain.keys) + [2 * N_E2E - 1]) and 2 * N_E2E - 1 not in plain.keys
    for elt in plain.keys:
        assert np.array_equal(np.asarray(plain.key(elt)), np.asarray(both.key(elt)))
    assert sorted(S.KeyGenerator(ctx, 11).galois_keys(None, conjugate=True).keys) == sorted(S.KeyGenerator(ctx, 11).galois_keys().keys)


def test_the_library_carries_the_new_surface(tmp_path):
    """built from the new source and header, exported, bound, and the header is plain C like hefx.h"""
    assert "hefx_dft.hip" in _build.SOURCES and "../../include/hefx_dft.h" in _build.HEADERS
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.library_path()], text=True)
    exported = set(re.findall(r" T (hefx_[a-z_0-9]+)", out))
    assert set(capi.DFT_SYMBOLS) <= exported
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hefx_dft.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(hefx_[a-z_0-9]+)\s*\(", src))) == capi.DFT_SYMBOLS == ["hefx_plain_combine"]
    assert not set(capi.DFT_SYMBOLS) & set(capi.EXPORTED_SYMBOLS)   # hefx.h's table stays as it is
    c = tmp_path / "t.c"
    c.write_text('#include "hefx_dft.h"\nint main(void) { return HEFX_PLAIN_COMBINE_MAX_IN + HEFX_PLAIN_COMBINE_MAX_OUT; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (capi.PLAIN_COMBINE_MAX_IN, capi.PLAIN_COMBINE_MAX_OUT) == (256, 64)
