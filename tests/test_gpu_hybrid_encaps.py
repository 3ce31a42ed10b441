"""Sparse-secret encapsulation on hybrid keys on the GPU, word for word: hefx_hybrid_collapse_key against Python integers,
hefx_hybrid_raise_switch against the independent model of tests/hybrid_encaps_cases.py and against the oracle-backed twin (seal.py's
host statement, held to the same model without a GPU by tests/test_hybrid_encaps_cpu.py) on every row of the cases' table, the
keys of engine and twin, algorithms.bootstrap_hybrid(encaps=) under a dense secret against the twin, both entries on a
caller-owned stream under the decoy protocol of tests/test_gpu_streams_ext.py (its Case machinery, imported), and the aliasing
rule in bytes."""
import numpy as np
import pytest

from tests import bootstrap_cases as BC
from tests import encaps_cases as EC
from tests import hybrid_cases as HC
from tests import hybrid_encaps_cases as HE

pytestmark = pytest.mark.gpu

_CTX = {}


def contexts(name):
    """(engine-backed context, twin context, the two evaluators) of a set, once per process"""
    from seal_fyp_logistic_regression_amd import seal as S
    if name not in _CTX:
        s = HC.sets()[name]
        cg, co = HC.context(s, "gpu"), HC.context(s, "oracle")
        assert all(getattr(cg.backend, n, None) is not None for n in ("hybrid_collapse_key", "hybrid_raise_switch"))
        assert all(getattr(co.backend, n, None) is None for n in ("hybrid_collapse_key", "hybrid_raise_switch"))
        _CTX[name] = (cg, co, S.Evaluator(cg), S.Evaluator(co))
    return _CTX[name]


def as_keys(ctx, alpha, key):
    from seal_fyp_logistic_regression_amd import seal as S
    high = S.HybridKeys(alpha)
    high.keys[1] = ctx.backend.from_host(key)
    return S.HybridEncapsKeys(None, high, HE.HAMMING_WEIGHT)


COLLAPSE_CASES = [(name, L, kind) for name, levels in HE.TABLE.items() for L in levels for kind in ("uniform", "maxkey")
                  if kind in HE.inputs_of(HC.sets()[name])]


@pytest.mark.parametrize("case", COLLAPSE_CASES, ids=HE.case_id)
def test_collapse_key_against_python_integers(case):
    name, L, kind = case
    s = HC.sets()[name]
    e = contexts(name)[0].backend.engine
    _, key = HE.case_input(s, kind)
    dkey = e.to_device(key)
    got = e.hybrid_collapse_key(s.alpha, L, dkey).download()
    assert got.shape == (2, L + s.alpha, s.N) and np.array_equal(got, HE.collapse_model(key, s.primes, s.alpha, L))
    assert np.array_equal(dkey.download(), key)                        # the key is only read


@pytest.mark.parametrize("case", HE.word_cases(), ids=HE.case_id)
def test_raise_switch_equals_the_model_and_the_twin(case):
    name, L, kind = case
    s = HC.sets()[name]
    cg, co, evg, evo = contexts(name)
    e = cg.backend.engine
    ct, key = HE.case_input(s, kind)
    want_ckey, want = HE.case_model(case)
    dct = e.to_device(ct)
    got = e.hybrid_raise_switch(s.alpha, L, dct, e.to_device(want_ckey)).download()
    assert got.shape == (2, L, s.N) and np.array_equal(got, want), "the model"
    assert np.array_equal(dct.download(), ct)                          # the input is only read
    # through the front end, on the engine (collapses and caches the key) and on the twin (the host statement)
    kg_, ko_ = as_keys(cg, s.alpha, key), as_keys(co, s.alpha, key)
    front = evg.raise_switch(EC.as_ciphertext(cg, ct), kg_, L)
    twin = evo.raise_switch(EC.as_ciphertext(co, ct), ko_, L)
    assert front.parms_id() == twin.parms_id() == L and L in kg_._collapsed
    assert np.array_equal(np.asarray(cg.backend.to_host(front.data)).reshape(2, L, s.N), want), "the front end"
    assert np.array_equal(np.asarray(co.backend.to_host(twin.data)).reshape(2, L, s.N), got), "the twin"
    again = evg.raise_switch(EC.as_ciphertext(cg, ct), kg_, L)         # through the cached collapsed key
    assert np.array_equal(np.asarray(cg.backend.to_host(again.data)).reshape(2, L, s.N), want)
    if s.alpha == 1:                                                   # also the words of the one-special-prime entries
        dkey = e.to_device(key)
        ck1 = e.collapse_key(L, dkey)
        assert np.array_equal(ck1.download(), e.hybrid_collapse_key(1, L, dkey).download())
        assert np.array_equal(e.raise_switch(L, dct, ck1).download(), got), "hefx_raise_switch"


@pytest.mark.parametrize("name", ["k7a2-p50_60", "k4a1-p50_60", "k8a3-d40_s60"])
def test_the_keys_of_engine_and_twin_are_equal_word_for_word(name):
    from seal_fyp_logistic_regression_amd import seal as S
    s = HC.sets()[name]
    cg, co, _, _ = contexts(name)
    keys = [S.KeyGenerator(c, BC.KEY_SEED).hybrid_encapsulation_keys(s.alpha, HE.HAMMING_WEIGHT, seed=HE.AUX_SEED) for c in (cg, co)]
    for get in (lambda k: k.low, lambda k: k.high.hybrid_key(1)):
        a, b = (np.asarray(c.backend.to_host(get(k))).reshape(-1) for c, k in zip((cg, co), keys))
        assert a.size and np.array_equal(a, b)
    if s.alpha == 1:
        plain = S.KeyGenerator(cg, BC.KEY_SEED).encapsulation_keys(HE.HAMMING_WEIGHT, seed=HE.AUX_SEED)
        assert np.array_equal(np.asarray(cg.backend.to_host(keys[0].high.hybrid_key(1))).reshape(-1), np.asarray(cg.backend.to_host(plain.high)).reshape(-1))


def test_bootstrap_hybrid_under_a_dense_secret_same_words_as_the_twin():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from tests.test_encaps_cpu import raised_integer_part
    outs = []
    for kind in ("gpu", "oracle"):
        e = HE.boot_env(kind)
        assert HE.dense(e)
        v, ct = HE.boot_input(e)
        plan, ev, keys = e["plan"], e["ev"], e["keys"]
        if kind == "gpu":   # a condition on the input: the SPARSE secret's integer part fits the plan
            I = raised_integer_part(e, ev.raise_switch(ev.switch_key(ct, keys.low), keys, plan.top_level))
            print(f"[gpu hybrid encaps] max |I| = {I} (K = {plan.K})")
            assert I <= plan.K
        outs.append((e, ct, alg.bootstrap_hybrid(ev, ct, plan, e["hgk"], e["hrk"], e["encoded"], encaps=keys), v))
    (eg, cg, og, v), (eo, co, oo, _) = outs
    assert np.array_equal(BC.words(eg, cg), BC.words(eo, co))
    assert og.size() == oo.size() == 2 and og.parms_id() == oo.parms_id() == eg["plan"].result_level and og.scale == oo.scale
    assert np.array_equal(BC.words(eg, og), BC.words(eo, oo))
    err = float(np.abs(eg["encoder"].decode(eg["dec"].decrypt(og))[:len(v)] - v).max() / np.abs(v).max())
    print(f"[gpu hybrid encaps] bootstrap_hybrid under a dense secret: words equal; decode error {err:.3e} (cap {BC.CAP:g})")
    assert err <= BC.CAP


# ---- stream order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HE.STREAM_CASES, ids=HE.case_id)
def test_both_entries_on_a_caller_owned_stream_behind_a_gate(case):
    """the protocol of tests/test_gpu_streams_ext.py: operands staged on the stream behind the gate, decoys in place until it
    opens, outputs snapshotted behind the call, decoys restored behind the snapshot; neither entry may have waited for the
    stream.  hefx_hybrid_raise_switch reads the collapsed key the collapse case writes on the same stream just before."""
    from tests.test_gpu_streams_ext import ExtWorld, gated, op
    s = HC.sets()[case[0]]
    collapse_case, rs = HE.stream_cases(case)
    assert all(collapse_case.differs()) and all(rs.differs())
    world = ExtWorld(s.N, s.primes)
    try:
        collapse = op(world, collapse_case)
        ckey = collapse.outs[0]
        gated(world, [collapse, op(world, rs, lambda i, t, st: rs.call(world.e, i, t, st, ckey))])
    finally:
        world.close()


# ---- the aliasing rule ----------------------------------------------------------------------------------------------------
def test_every_byte_overlap_is_refused_with_nothing_submitted():
    """an output one row into an input or key, an input or key one row into the output, d_ct_out == d_ct_in: ValueError
    (HEFX_ERR_INVALID), the slab's words unchanged, no key switch counted; the adjacent layout runs and writes its output alone"""
    name = "k7a2-p50_60"
    s = HC.sets()[name]
    e = contexts(name)[0].backend.engine
    N, k, A, L = s.N, s.k, s.alpha, s.k - s.alpha
    dn = (L + A - 1) // A
    rng = np.random.default_rng(3)
    words = {"key": dn * 2 * k * N, "ckey": 2 * (L + A) * N, "in1": 2 * N, "out": 2 * (L + A) * N, "pad": dn * 2 * k * N}
    at, pos = {}, 0
    for nm, w in words.items():
        at[nm], pos = pos, pos + w
    host = rng.integers(0, int(min(s.primes)), pos, dtype=np.uint64)
    slab = e.to_device(host)
    view = lambda off, shape: slab.view(off, shape)
    last_row = lambda y, used=None: at[y] + (words[y] if used is None else used) - N   # where y's last row starts
    stats = e.ks_stats()

    def refused(call, match="overlap|independent"):
        with pytest.raises(ValueError, match=match):
            call()
        e.sync()
        assert np.array_equal(slab.download(), host) and e.ks_stats() == stats

    in1, key, ckey = view(at["in1"], (2, 1, N)), view(at["key"], (dn, 2, k, N)), view(at["ckey"], (2, L + A, N))
    outc, out2 = view(at["out"], (2, L + A, N)), view(at["out"], (2, L, N))
    # hefx_hybrid_collapse_key
    refused(lambda: e.hybrid_collapse_key(A, L, key, out=view(last_row("key"), (2, L + A, N))))
    refused(lambda: e.hybrid_collapse_key(A, L, key, out=view(at["key"], (2, L + A, N))))
    refused(lambda: e.hybrid_collapse_key(A, L, view(last_row("out"), (dn, 2, k, N)), out=outc))
    # hefx_hybrid_raise_switch
    refused(lambda: e.hybrid_raise_switch(A, L, in1, ckey, out=view(at["in1"], (2, L, N))))            # d_ct_out == d_ct_in
    refused(lambda: e.hybrid_raise_switch(A, L, in1, ckey, out=view(last_row("in1"), (2, L, N))))
    refused(lambda: e.hybrid_raise_switch(A, L, view(last_row("out", 2 * L * N), (2, 1, N)), ckey, out=out2))
    refused(lambda: e.hybrid_raise_switch(A, L, in1, ckey, out=view(last_row("ckey"), (2, L, N))))
    refused(lambda: e.hybrid_raise_switch(A, L, in1, view(last_row("out", 2 * L * N), (2, L + A, N)), out=out2))
    # the levels and alpha out of range
    refused(lambda: e.hybrid_raise_switch(A, 1, in1, ckey, out=out2), match="at least 2")
    refused(lambda: e.hybrid_raise_switch(A, k - A + 1, in1, ckey, out=out2), match="level")
    refused(lambda: e.hybrid_collapse_key(A, k - A + 1, key, out=outc), match="level")
    refused(lambda: e.hybrid_collapse_key(A, 0, key, out=outc), match="level")
    for alpha in (0, k, 9):
        refused(lambda: e.hybrid_raise_switch(alpha, 2, in1, ckey, out=out2), match="alpha")
        refused(lambda: e.hybrid_collapse_key(alpha, 2, key, out=outc), match="alpha")
    # the adjacent layout runs, and writes its output alone
    e.hybrid_raise_switch(A, L, in1, ckey, out=out2)
    e.sync()
    got = slab.download()
    lo, hi = at["out"], at["out"] + 2 * L * N
    assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[hi:], host[hi:]) and not np.array_equal(got[lo:hi], host[lo:hi])
    want = HE.raise_switch_model(HC.twin(s), s.primes, A, L, host[at["in1"]:at["in1"] + 2 * N].reshape(2, 1, N),
                                 host[at["ckey"]:at["ckey"] + 2 * (L + A) * N].reshape(2, L + A, N))
    assert np.array_equal(got[lo:hi].reshape(2, L, N), want)
