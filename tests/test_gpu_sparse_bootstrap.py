"""Sparse-slot bootstrapping on the GPU: algorithms.subsum, coeffs_to_slots_packed / slots_to_coeffs_packed and
algorithms.bootstrap with a sparse plan give on the engine, word for word, the ciphertexts of the oracle-backed twin.

The twin runs SubSum and the packed transforms OP BY OP -- single rotations, multiply_plain, add, rescale, one conjugation --
where the engine runs the fused sum in the key switch's epilogue, batched rotations and hefx_plain_combine; the whole
bootstrap runs through the same host code on both.  N = 2048 (key switching needs N >= 2048 on the engine), the chain, key
and inputs of tests/bootstrap_cases.py and tests/sparse_bootstrap_cases.py: ns = 16 (six SubSum steps, period 32 tiled 32
times), ns = 512 = N / 4 (one step, the period is the slot count), ns = 2 (one butterfly factor, levels clipped to 1 + 1;
words only, no precision claim)."""
import numpy as np
import pytest

from tests import bootstrap_cases as BC
from tests import sparse_bootstrap_cases as SC

pytestmark = pytest.mark.gpu

_ENV = {}


def plans():
    if "plans" not in _ENV:
        _ENV["plans"] = {ns: SC.sparse_plan(ns) for ns in (SC.SPARSE_NS, SC.FULL_NS, SC.SMALL_NS)}
    return _ENV["plans"]


def envs():
    """engine and twin with the same seeds and the Galois keys of all three plans (the default rescale division)"""
    if "envs" not in _ENV:
        steps = set().union(*[set(p.galois_steps()) for p in plans().values()])
        _ENV["envs"] = {kind: SC.make(kind, steps) for kind in ("gpu", "oracle")}
        eg, eo = _ENV["envs"]["gpu"], _ENV["envs"]["oracle"]
        assert getattr(eg["ctx"].backend, "rotate_add_chain", None) is not None
        assert getattr(eo["ctx"].backend, "rotate_add_chain", None) is None and getattr(eo["ctx"].backend, "plain_combine", None) is None
    return _ENV["envs"]["gpu"], _ENV["envs"]["oracle"]


def subsum_op_by_op(ev, ct, ns, gk):
    x = ct
    for i in range((BC.N // (2 * ns)).bit_length() - 1):
        x = ev.add(x, ev.rotate_vector(x, ns << i, gk))
    return x


def packed_op_by_op(ev, ct, plan, tables, gk):
    """a packed dft.Plan, one evaluator call per operation"""
    from seal_fyp_logistic_regression_amd import dft
    x = ct
    for stage, table in zip(plan.stages, tables):
        assert stage.mode == "single" and len(table) == 1
        rots = [x if b == 0 else ev.rotate_vector(x, b, gk) for b in stage.babies]
        acc = None
        for gi, g in enumerate(stage.giants):
            inner = None
            for bi in range(len(stage.babies)):
                if table[0][gi][bi] is not None:
                    t = ev.multiply_plain(rots[bi], table[0][gi][bi])
                    inner = t if inner is None else ev.add(inner, t)
            moved = inner if g == 0 else ev.rotate_vector(inner, g, gk)
            acc = moved if acc is None else ev.add(acc, moved)
        x = ev.rescale_to_next_inplace(acc)
    return ev.add(x, ev.complex_conjugate(x, gk)) if plan.direction == dft.C2S else x


def same(eg, g, eo, o, level, name):
    assert g.size() == o.size() == 2 and g.parms_id() == o.parms_id() == level and g.scale == o.scale, name
    assert np.array_equal(BC.words(eg, g), BC.words(eo, o)), name


@pytest.mark.parametrize("ns", [SC.SPARSE_NS, SC.FULL_NS])
def test_subsum_same_words_as_the_twin(ns):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    eg, eo = envs()
    v = SC.sparse_input(ns)
    top = eg["ctx"].first_parms_id()
    cg, co = (e["enc"].encrypt(e["encoder"].encode(SC.tiled(v), BC.SCALE)) for e in (eg, eo))
    assert np.array_equal(BC.words(eg, cg), BC.words(eo, co))
    before = BC.words(eg, cg).copy()
    og = alg.subsum(eg["ev"], cg, ns, eg["gk"])
    same(eg, og, eo, subsum_op_by_op(eo["ev"], co, ns, eo["gk"]), top, ("subsum", ns))
    same(eg, og, eo, alg.subsum(eo["ev"], co, ns, eo["gk"]), top, ("subsum through the twin's own path", ns))
    assert np.array_equal(BC.words(eg, cg), before)                # the input is only read
    g = BC.N // (2 * ns)
    got = eg["encoder"].decode(eg["dec"].decrypt(og))
    err = float(np.abs(got - g * SC.tiled(v)).max() / (g * np.abs(v).max()))
    print(f"[gpu sparse bootstrap] subsum ns = {ns}: {g.bit_length() - 1} steps, decode error {err:.3e} of g max|v|")
    assert err <= 1e-6   # (a sanity bound on the decryption, far above the noise: the criterion is the words)
    with pytest.raises(ValueError, match="Galois key not present"):
        alg.subsum(eg["ev"], cg, ns, eg["kg"].galois_keys([1]))


def test_packed_transforms_same_words_as_the_plan_op_by_op_on_the_twin(rescale_mode):
    """on a mod-raised ciphertext: SubSum, CoeffToSlot with the bootstrap's factors, and SlotToCoeff (factor 1) straight
    below it, which takes the result back to ns-periodic slots"""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import dft
    ns = SC.SPARSE_NS
    p = plans()[ns]
    top = p.top_level
    back = dft.plan_packed(BC.N, ns, 2, dft.S2C, [p.primes[top - 3], p.primes[top - 4]])
    steps = set(p.galois_steps()) | set(back.galois_steps())
    v = SC.sparse_input(ns)
    res = {}
    for kind in ("gpu", "oracle"):
        e = SC.make(kind, steps)
        assert (getattr(e["ctx"].backend, "plain_combine", None) is not None) == (kind == "gpu")
        ev, gk = e["ev"], e["gk"]
        t_c2s, t_back = p.c2s.encode(e["encoder"], top), back.encode(e["encoder"], top - 2)
        ct = SC.encrypt_tiled(e, v)
        raised = ev.mod_raise(ct, top)
        if kind == "gpu":
            t, I = BC.raised_coefficients(e, ct, top)
            x = alg.subsum(ev, raised, ns, gk)
            c2s = alg.coeffs_to_slots_packed(ev, x, p.c2s, gk, encoded=t_c2s)
            s2c = alg.slots_to_coeffs_packed(ev, c2s, back, gk, encoded=t_back)
        else:
            x = subsum_op_by_op(ev, raised, ns, gk)
            c2s = packed_op_by_op(ev, x, p.c2s, t_c2s, gk)
            s2c = packed_op_by_op(ev, c2s, back, t_back, gk)
        res[kind] = (e, [x, c2s, s2c])
    (eg, cg), (eo, co) = res["gpu"], res["oracle"]
    for name, g, o, lv in zip(["subsum", "coeffs_to_slots_packed", "slots_to_coeffs_packed"], cg, co, [top, top - 2, top - 4]):
        same(eg, g, eo, o, lv, (name, rescale_mode))
    # the decode gate, against the float model on the raised plaintext the secret key shows
    assert np.abs(I).max() <= 12
    x = p.slots(np.array([float(int(c)) for c in t]))
    for step in p.subsum_steps():
        x = x + np.roll(x, -step)
    (want,) = p.c2s.apply([x])
    (want_back,) = back.apply([want])
    for name, ct, w in (("coeffs_to_slots_packed", cg[1], want), ("slots_to_coeffs_packed", cg[2], want_back)):
        got = eg["encoder"].decode(eg["dec"].decrypt(ct))
        rel = float(np.abs(got - w).max() / np.abs(w).max())
        print(f"[gpu sparse bootstrap] {name} ({rescale_mode}): max error / max|expected| = {rel:.3e}")
        assert rel <= BC.CAP, (name, rel)


def bootstrap_both(ns):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    eg, eo = envs()
    p, v = plans()[ns], SC.sparse_input(ns)
    outs = []
    for e in (eg, eo):
        ct = SC.encrypt_tiled(e, v)
        assert ct.parms_id() == 1
        if e is eg:   # a condition on the input: the key's integer part fits the plan
            _, I = BC.raised_coefficients(e, ct, p.top_level)
            print(f"[gpu sparse bootstrap] ns = {ns}: max |I| = {int(np.abs(I).max())} (K = {p.K})")
            assert np.abs(I).max() <= 12
        outs.append((ct, alg.bootstrap(e["ev"], ct, p, e["gk"], e["rk"], p.encode(e["encoder"]))))
    (cg, og), (co, oo) = outs
    assert np.array_equal(BC.words(eg, cg), BC.words(eo, co))
    same(eg, og, eo, oo, p.result_level, ("bootstrap", ns))
    assert abs(og.scale / BC.SCALE - 1.0) < 1e-12   # ct's scale, as a computed value
    return eg, p, v, og


def test_sparse_bootstrap_same_words_as_the_twin_and_one_more_product():
    ns = SC.SPARSE_NS
    eg, p, v, og = bootstrap_both(ns)
    assert p.result_level == 2
    got = eg["encoder"].decode(eg["dec"].decrypt(og)).real
    err = float(np.abs(got - SC.tiled(v)).max() / np.abs(v).max())   # every slot: the result is ns-periodic
    sq = eg["ev"].rescale_to_next_inplace(eg["ev"].relinearize_inplace(eg["ev"].square(og), eg["rk"]))
    err2 = float(np.abs(eg["encoder"].decode(eg["dec"].decrypt(sq)).real[:ns] - v * v).max() / np.abs(v).max())
    print(f"[gpu sparse bootstrap] ns = {ns}: decode error {err:.3e}, after one more square {err2:.3e} (cap {BC.CAP:g})")
    assert sq.parms_id() == 1 and err <= BC.CAP and err2 <= 2 * BC.CAP


@pytest.mark.parametrize("ns", [SC.SMALL_NS, SC.FULL_NS])
def test_the_edge_sizes_same_words_as_the_twin(ns):
    eg, p, v, og = bootstrap_both(ns)
    assert (p.c2s.levels, p.result_level) == ((1, 4) if ns == SC.SMALL_NS else (2, 2))
    got = eg["encoder"].decode(eg["dec"].decrypt(og)).real
    err = float(np.abs(got[:ns] - v).max() / np.abs(v).max())
    print(f"[gpu sparse bootstrap] ns = {ns}: decode error {err:.3e} (printed, not asserted: the criterion is the words)")
