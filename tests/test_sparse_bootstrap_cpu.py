"""Sparse-slot CKKS bootstrapping without a GPU: SubSum, the packed transforms of dft.plan_packed in float64, the planner
surface of bootstrap.plan(..., slots=ns), its float model against plain reduction mod q_0, and algorithms.subsum /
algorithms.bootstrap on the oracle-backed twin.

THE ERROR GATE is tests/bootstrap_cases.CAP = 1e-3 of the largest expected value, a cap and not a measurement; the float
model alone must be ten times inside it.  Chain, scale, key and input are those of the dense tests (tests/bootstrap_cases.py);
the sparse message is the first ns values of the dense input, tiled (tests/sparse_bootstrap_cases.py).  Measured here (rescale
division round; written to profiles/sparse_bootstrap.json with BOOTSTRAP_RECORD=1), as error / max|expected|:
    plan.apply 4.6e-07; twin bootstrap at ns = 16, levels 2 + 2: 1.5e-06, after one more square 1.9e-06, a second bootstrap
    1.7e-06; ns = 512: 1.3e-05; levels 1 + 1 at ns = 16 (recorded, not asserted): 1.4e-03, outside the cap, which is why the
    default stays at 2 + 2."""
import json
import os

import numpy as np
import pytest

from seal_fyp_logistic_regression_amd import dft
from tests import bootstrap_cases as BC
from tests import sparse_bootstrap_cases as SC
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = (1 << 40) - 87   # (the planner only carries the primes along)
RECORD = {}
_ENV = {}


# ---- 1. the linear algebra in float64, no engine ----------------------------------------------------------------------------
def roots(N):
    return np.array([pow(3, j, 2 * N) for j in range(N // 2)], dtype=np.int64)


def slots_of(t):
    """the encoder's N / 2 slots of the real coefficients t: z_j = sum_i t_i zeta^(3^j i)"""
    N = len(t)
    return np.conj(np.fft.fft(t, 2 * N)[roots(N)])


def subsum_numpy(x, ns):
    g = len(x) // ns
    for i in range(g.bit_length() - 1):
        x = x + np.roll(x, -(ns << i))
    return x


def block_of(st, ns):
    """the block matrix dft.plan_packed states for a stage of dft.plan(2 ns, ...), dense and built here"""
    Z = np.zeros((ns, ns), dtype=np.complex128)
    D = [dft.dense(m) for m in st.mats]
    if st.mode == "split":
        return np.block([[D[0], Z], [D[1], Z]])
    if st.mode == "merge":
        return np.block([[D[0], D[1]], [D[0], D[1]]])
    return np.block([[D[0], Z], [Z, D[0]]])


@pytest.mark.parametrize("N,ns,levels", [(64, 4, 1), (64, 16, 2), (256, 8, 3), (1024, 256, 2), (2048, 2, 1), (2048, 16, 2)])
def test_subsum_and_the_packed_transforms_in_float64(N, ns, levels):
    g, n = N // (2 * ns), N // 2
    rng = np.random.default_rng(N + ns + levels)
    t = rng.integers(-6, 7, N).astype(np.float64)            # I: a general polynomial
    t[::g] += rng.uniform(-1.0, 1.0, 2 * ns)                 # mu: on the stride
    on_stride = np.zeros(N)
    on_stride[::g] = g * t[::g]
    x = subsum_numpy(slots_of(t), ns)
    assert np.allclose(x, slots_of(on_stride))
    assert np.allclose(x, np.tile(x[:ns], n // ns))          # ns-periodic
    a, b, R = t[::g][:ns], t[::g][ns:], dft.bit_reversal(ns)
    plans = {d: dft.plan_packed(N, ns, levels, d, [Q] * levels) for d in (dft.C2S, dft.S2C)}
    small = {d: dft.plan(2 * ns, levels, d, [Q] * levels) for d in (dft.C2S, dft.S2C)}
    (y,) = plans[dft.C2S].apply([x])
    assert y.shape == (n,) and np.allclose(y, np.tile(np.concatenate([g * a[R], g * b[R]]), n // (2 * ns)))
    (back,) = plans[dft.S2C].apply([y])
    assert np.allclose(back, x)
    for d in (dft.C2S, dft.S2C):
        p = plans[d]
        assert p.slots == ns and p.levels == levels and p.N == N and p.n == n and p.primes() == [Q] * levels
        assert [st.mode for st in small[d].stages] == (["split"] + ["lockstep"] * (levels - 1) if d == dft.C2S
                                                        else ["lockstep"] * (levels - 1) + ["merge"])
        steps = set()
        for st, sm in zip(p.stages, small[d].stages):
            assert (st.mode, st.inputs, st.outputs, st.n, st.stride, len(st.mats)) == ("single", 1, 1, 2 * ns, sm.stride, 1)
            M = dft.dense(st.mats[0])
            assert M.shape == (2 * ns, 2 * ns) and np.allclose(M, block_of(sm, ns))
            w = rng.normal(size=2 * ns) + 1j * rng.normal(size=2 * ns)
            (got,) = st.apply([np.tile(w, n // (2 * ns))])
            assert np.allclose(got, np.tile(M @ w, n // (2 * ns)))
            assert all(0 <= s < 2 * ns and s % st.stride == 0 for s in st.babies + st.giants)
            assert st.key_switches() == sum(1 for s in st.babies if s) + sum(1 for s in st.giants if s)
            steps |= {s for s in st.babies + st.giants if s}
        assert p.galois_steps() == sorted(steps)
        assert p.key_switches() == sum(st.key_switches() for st in p.stages) + (1 if d == dft.C2S else 0)


def test_plan_packed_refusals_and_the_dense_plan_as_it_was():
    for ns in (1, 3, 32, 12):
        with pytest.raises(ValueError, match="slots"):
            dft.plan_packed(64, ns, 1, dft.C2S, [Q])
    with pytest.raises(ValueError, match="levels"):
        dft.plan_packed(64, 4, 3, dft.C2S, [Q] * 3)
    p = dft.plan(64, 2, dft.C2S, [Q, Q])
    assert p.slots is None and [st.mode for st in p.stages] == ["split", "lockstep"]
    assert p.key_switches() == sum(st.key_switches() for st in p.stages) + 2


def test_encode_tiles_the_diagonals():
    """Plan.encode hands the encoder every pre-rotated diagonal tiled to N / 2 values, at the stage's level and prime"""
    N, ns = 64, 4
    p = dft.plan_packed(N, ns, 2, dft.S2C, [Q, Q - 2])
    seen = []

    class Encoder:
        ctx = type("Ctx", (), {"primes": [5, Q - 2, Q, 7]})()

        def encode_many(self, vs, scale, L):
            seen.append((L, scale, [np.asarray(v) for v in vs]))
            return [("pt", L, i) for i in range(len(vs))]

    tables = p.encode(Encoder(), 3)
    assert [s[:2] for s in seen] == [(3, float(Q)), (2, float(Q - 2))]
    for st, (L, _, vs), table in zip(p.stages, seen, tables):
        want = [st.rotated(0, g, b) for g in st.giants for b in st.babies]
        want = [np.tile(v, (N // 2) // (2 * ns)) for v in want if v is not None]
        assert len(vs) == len(want) and all(v.shape == (N // 2,) and np.array_equal(v, w) for v, w in zip(vs, want))
        assert len(table) == 1 and len(table[0]) == len(st.giants) and all(len(row) == len(st.babies) for row in table[0])
        assert sum(x is not None for row in table[0] for x in row) == len(want)


# ---- 2. the planner surface ---------------------------------------------------------------------------------------------------
def plan_of(ns, **kw):
    key = ("plan", ns, tuple(sorted(kw.items())))
    if key not in _ENV:
        _ENV[key] = SC.sparse_plan(ns, **kw)
    return _ENV[key]


def test_the_sparse_plan():
    from seal_fyp_logistic_regression_amd import bootstrap as B
    from seal_fyp_logistic_regression_amd import poly
    from seal_fyp_logistic_regression_amd import seal as S
    primes = S.CoeffModulus.Create(BC.N, BC.CHAIN_BITS)
    p = plan_of(SC.SPARSE_NS)
    assert p.sparse_slots == 16 and p.c2s.slots == p.s2c.slots == 16
    assert p.subsum_steps() == [16, 32, 64, 128, 256, 512] == [16 << i for i in range(6)]
    assert set(p.subsum_steps()) <= set(p.galois_steps())
    assert set(p.galois_steps()) == set(p.subsum_steps()) | set(p.c2s.galois_steps()) | set(p.s2c.galois_steps())
    assert (p.K, p.r, p.degree, p.c2s.levels, p.s2c.levels) == (12, 3, 31, 2, 2)
    assert p.levels() == 12 and p.top_level == 14 and p.evalmod_level == 12 and p.s2c_level == 4 and p.result_level == 2
    assert p.c2s.primes() == [primes[13], primes[12]] and p.s2c.primes() == [primes[3], primes[2]]
    pp = poly.plan(p.coeffs, "chebyshev", primes[:p.evalmod_level], BC.SCALE, p.poly_target_scale)
    for lazy in (True, False):   # SubSum, both packed transforms, ONE polynomial's relinearisations, r double angles
        assert p.key_switches(lazy) == 6 + p.c2s.key_switches() + p.s2c.key_switches() + pp.relinearizations(lazy) + 3
    assert p.key_switches(False) - p.key_switches(True) == 7
    # the factors: 1 / g sits in CoeffToSlot's diagonals, next to the small plan's 1 / (2 ns)
    assert p.c2s.factor == pytest.approx(BC.SCALE / (primes[0] * 12.25 * 64), rel=1e-15)
    assert p.s2c.factor == pytest.approx(primes[0] / (2.0 * np.pi * BC.SCALE), rel=1e-15)
    # clipping: ns = 2 has one butterfly factor
    c = plan_of(SC.SMALL_NS)
    assert (c.c2s.levels, c.s2c.levels, c.levels(), c.evalmod_level, c.s2c_level, c.result_level) == (1, 1, 10, 13, 5, 4)
    assert c.subsum_steps() == [2 << i for i in range(9)]
    f = plan_of(SC.FULL_NS)
    assert f.subsum_steps() == [512] and f.c2s.stages[0].n == BC.N // 2 and f.levels() == 12
    # fewer levels are allowed
    assert SC.sparse_plan(16, c2s_levels=1, s2c_levels=1).result_level == 4
    for bad in (3, 1, BC.N // 2, 0):
        with pytest.raises(ValueError, match="slots"):
            B.plan(BC.N, primes, BC.SCALE, slots=bad)
    with pytest.raises(ValueError, match="not enough levels"):
        B.plan(BC.N, primes[:12] + primes[-1:], BC.SCALE, slots=16)
    with pytest.raises(ValueError, match="misses the precision"):
        B.plan(BC.N, primes, BC.SCALE, degree=15, slots=16)


# bootstrap.plan(BC.N, chain, BC.SCALE) as it was before `slots` existed
DENSE_GALOIS_STEPS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 24, 32, 64, 96, 128, 256, 384, 512, 640, 768, 896, 993, 1001, 1009, 1017]
DENSE_KEY_SWITCHES = (118, 132)
DENSE_TRANSFORM_KEY_SWITCHES = (47, 41)


def test_the_dense_plan_is_the_one_it_was():
    """without `slots`: the figures of the plan before sparse packing, as literals"""
    from seal_fyp_logistic_regression_amd import bootstrap as B
    from seal_fyp_logistic_regression_amd import seal as S
    p = B.plan(BC.N, S.CoeffModulus.Create(BC.N, BC.CHAIN_BITS), BC.SCALE)
    assert p.sparse_slots is None and p.subsum_steps() == [] and p.c2s.slots is None and p.s2c.slots is None
    assert p.galois_steps() == DENSE_GALOIS_STEPS
    assert (p.key_switches(True), p.key_switches(False)) == DENSE_KEY_SWITCHES
    assert (p.levels(), p.top_level, p.evalmod_level, p.s2c_level, p.result_level, p.depth) == (12, 14, 12, 4, 2, 5)
    assert [st.mode for st in p.c2s.stages] == ["split", "lockstep"] and [st.mode for st in p.s2c.stages] == ["lockstep", "merge"]
    assert (p.c2s.key_switches(), p.s2c.key_switches()) == DENSE_TRANSFORM_KEY_SWITCHES


# ---- 3. plan.apply against plain reduction mod q_0 ----------------------------------------------------------------------------
def test_apply_against_plain_mod_reduction():
    p = plan_of(SC.SPARSE_NS)
    q0, g = p.primes[0], BC.N // (2 * SC.SPARSE_NS)
    v = SC.sparse_input(SC.SPARSE_NS)
    m = np.round(p.coefficients(SC.tiled(v).astype(np.complex128)))
    off = np.ones(BC.N, dtype=bool)
    off[::g] = False
    assert not m[off].any() and np.abs(m).max() <= BC.SCALE      # the message lies in the subring
    rng = np.random.default_rng(6)
    I = rng.integers(-p.K, p.K + 1, BC.N)                        # a general polynomial: off the stride too
    I[:g * (2 * p.K + 1):g] = np.arange(-p.K, p.K + 1)            # every integer part the plan allows occurs on the stride
    assert set(I[::g]) >= set(range(-p.K, p.K + 1)) and I[off].any()
    t = [int(a) + q0 * int(b) for a, b in zip(m, I)]
    centred = np.array([float((x + q0 // 2) % q0 - q0 // 2) for x in t])
    assert np.array_equal(centred, m)
    out = p.apply(np.array([float(x) for x in t]))
    err = float(np.abs(p.slots(out) - SC.tiled(v)).max() / np.abs(v).max())
    stray = float(np.abs(out[off]).max() / BC.SCALE)
    RECORD["plan_apply"] = err
    print(f"[sparse bootstrap cpu] plan.apply: max slot error / max|expected| {err:.3e}, largest coefficient off the stride / scale {stray:.3e}")
    assert err <= BC.CAP / 10 and stray <= BC.CAP / 10


# ---- 4. and 5. on the oracle-backed twin --------------------------------------------------------------------------------------
def twin():
    """one environment for every twin test: the keys of the ns = 16 plan at 2 + 2 and 1 + 1 levels and of the ns = 512 plan"""
    if "twin" not in _ENV:
        steps = set()
        for pl in (plan_of(SC.SPARSE_NS), plan_of(SC.FULL_NS), plan_of(SC.SPARSE_NS, c2s_levels=1, s2c_levels=1)):
            steps |= set(pl.galois_steps())
        _ENV["twin"] = SC.make("oracle", steps)
    return _ENV["twin"]


def rel_error(e, ct, want, count):
    got = e["encoder"].decode(e["dec"].decrypt(ct))
    return float(np.abs(got[:count] - want[:count]).max() / np.abs(want).max()), got


def test_subsum_on_the_twin():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import seal as S
    e = twin()
    n = BC.N // 2
    for ns in (SC.SPARSE_NS, SC.FULL_NS):
        g = BC.N // (2 * ns)
        v = SC.sparse_input(ns)
        ct = e["enc"].encrypt(e["encoder"].encode(SC.tiled(v), BC.SCALE))
        own, _ = rel_error(e, ct, SC.tiled(v), n)                  # the twin's own decode error on this ciphertext
        out = alg.subsum(e["ev"], ct, ns, e["gk"])
        assert out.size() == 2 and out.parms_id() == ct.parms_id() and out.scale == ct.scale
        err, _ = rel_error(e, out, g * SC.tiled(v), n)
        err *= g                                                   # as a fraction of max|v|, like `own`
        print(f"[sparse bootstrap cpu] subsum ns = {ns}: error {err:.3e} of max|v|, g = {g} times the input's own {own:.3e}")
        # g copies of the input's noise (they add incoherently: sqrt(g) of it) and log2(g) key switches: within g times the
        # input's own error.  At g = 2 that leaves the key switch no room (measured 4.1e-11 against 2 x 1.6e-11), so the
        # bound is asserted at ns = 16; ns = 512 is checked on its words (tests/test_gpu_sparse_bootstrap.py)
        # and through the whole bootstrap below.
        if ns == SC.SPARSE_NS:
            assert err <= g * own
    few = e["kg"].galois_keys([16, 32])
    with pytest.raises(ValueError, match="Galois key not present"):
        alg.subsum(e["ev"], ct, 16, few)
    for bad in (3, 1, n):
        with pytest.raises(ValueError, match="slots"):
            alg.subsum(e["ev"], ct, bad, e["gk"])


def test_sparse_bootstrap_on_the_oracle():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    e, ns = twin(), SC.SPARSE_NS
    ev, p = e["ev"], plan_of(ns)
    v = SC.sparse_input(ns)
    ct = SC.encrypt_tiled(e, v)
    _, I = BC.raised_coefficients(e, ct, p.top_level)
    print(f"[sparse bootstrap cpu] max |I| = {int(np.abs(I).max())} (K = {p.K})")
    assert np.abs(I).max() <= 12                                  # a condition on the input
    out = alg.bootstrap(ev, ct, p, e["gk"], e["rk"])
    assert out.size() == 2 and out.parms_id() == p.result_level == 2 and abs(out.scale / BC.SCALE - 1.0) < 1e-12
    err, got = rel_error(e, out, v, ns)
    period = float(np.abs(got[ns:2 * ns] - v).max() / np.abs(v).max())
    everywhere = float(np.abs(got - SC.tiled(v)).max() / np.abs(v).max())
    sq = ev.rescale_to_next_inplace(ev.relinearize_inplace(ev.square(out), e["rk"]))
    err2, _ = rel_error(e, sq, v * v, ns)
    err2 *= float(np.abs(v * v).max() / np.abs(v).max())        # as a fraction of max|v|, like the dense test
    # a second bootstrap: the result is back in the subring
    low = ev.mod_switch_to_inplace(out.copy(), 1)
    _, I2 = BC.raised_coefficients(e, low, p.top_level)
    assert np.abs(I2).max() <= 12
    again = alg.bootstrap(ev, low, p, e["gk"], e["rk"])
    assert again.parms_id() == 2 and abs(again.scale / BC.SCALE - 1.0) < 1e-12
    err3, _ = rel_error(e, again, v, ns)
    RECORD.update(bootstrap=err, slots_ns_to_2ns=period, all_slots=everywhere, bootstrap_then_square=err2, second_bootstrap=err3,
                  max_abs_I=int(np.abs(I).max()), max_abs_I_second=int(np.abs(I2).max()))
    print(f"[sparse bootstrap cpu] twin, ns = {ns}: error {err:.3e}, slots ns .. 2 ns {period:.3e}, all slots {everywhere:.3e}, "
          f"after one more square {err2:.3e}, after a second bootstrap {err3:.3e}")
    assert err <= BC.CAP and period <= BC.CAP and everywhere <= BC.CAP
    assert sq.parms_id() == 1 and err2 <= 2 * BC.CAP and err3 <= 2 * BC.CAP
    with pytest.raises(ValueError, match="last prime"):
        alg.bootstrap(ev, out, p, e["gk"], e["rk"])
    # the packed entries refuse a dense plan and the dense entries a packed one
    dense = dft.plan(BC.N, 2, dft.C2S, p.c2s.primes())
    with pytest.raises(ValueError, match="not a packed plan"):
        alg.coeffs_to_slots_packed(ev, out, dense, e["gk"])
    with pytest.raises(ValueError, match="not a CoeffToSlot plan"):
        alg.coeffs_to_slots(ev, out, p.c2s, e["gk"])
    with pytest.raises(ValueError, match="not a SlotToCoeff plan"):
        alg.slots_to_coeffs(ev, out, out, p.s2c, e["gk"])


def test_sparse_bootstrap_at_a_quarter_of_the_ring():
    """ns = N / 4: no tiling, g = 2, one SubSum step"""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    e, ns = twin(), SC.FULL_NS
    p = plan_of(ns)
    v = SC.sparse_input(ns)
    ct = SC.encrypt_tiled(e, v)
    _, I = BC.raised_coefficients(e, ct, p.top_level)
    assert np.abs(I).max() <= 12
    out = alg.bootstrap(e["ev"], ct, p, e["gk"], e["rk"])
    assert out.size() == 2 and out.parms_id() == p.result_level == 2 and abs(out.scale / BC.SCALE - 1.0) < 1e-12
    err, got = rel_error(e, out, v, ns)
    period = float(np.abs(got[ns:] - v).max() / np.abs(v).max())
    RECORD["bootstrap_ns512"] = err
    print(f"[sparse bootstrap cpu] twin, ns = {ns}: error {err:.3e}, slots ns .. 2 ns {period:.3e}")
    assert err <= BC.CAP and period <= BC.CAP


def test_record_the_measured_errors():
    """BOOTSTRAP_RECORD=1: the figures of this run, and the 1 + 1 levels measurement behind the default of 2 + 2 (no
    assertion: its precision is not claimed), go into profiles/sparse_bootstrap.json"""
    if not os.environ.get("BOOTSTRAP_RECORD"):
        return
    from seal_fyp_logistic_regression_amd import algorithms as alg
    if "plan_apply" not in RECORD:
        test_apply_against_plain_mod_reduction()
    if "bootstrap" not in RECORD:
        test_sparse_bootstrap_on_the_oracle()
    if "bootstrap_ns512" not in RECORD:
        test_sparse_bootstrap_at_a_quarter_of_the_ring()
    e, ns = twin(), SC.SPARSE_NS
    p11 = plan_of(ns, c2s_levels=1, s2c_levels=1)
    v = SC.sparse_input(ns)
    out = alg.bootstrap(e["ev"], SC.encrypt_tiled(e, v), p11, e["gk"], e["rk"])
    RECORD["bootstrap_levels_1_1_not_asserted"], _ = rel_error(e, out, v, ns)
    path = os.path.join(ROOT, "profiles", "sparse_bootstrap.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["precision_oracle_twin_n2048"] = {"chain_bits": BC.CHAIN_BITS, "scale": "2^50", "hamming_weight": BC.HAMMING_WEIGHT,
                                          "key_seed": BC.KEY_SEED, "cap": BC.CAP, "unit": "max error / max|expected|",
                                          "slots": ns, "levels": "2 + 2",
                                          "rescale": "round" if OracleBackend.rescale_rounded else "floor", **RECORD}
    json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
    open(path, "a").write("\n")
