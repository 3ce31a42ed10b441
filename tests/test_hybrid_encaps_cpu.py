"""Sparse-secret encapsulation on hybrid keys on the oracle-backed twin (no GPU): seal.py's host statement
(hybrid_collapse_key_host, hybrid_raise_switch_host -- what Evaluator.raise_switch runs with HybridEncapsKeys where the backend has
no native entry) against the independent model of tests/hybrid_encaps_cases.py on every row of its table; alpha = 1 against the
one-special-prime path; KeyGenerator.hybrid_encapsulation_keys; the noise under real keys against the header's bound; the whole
bootstrap_hybrid under a DENSE main secret; the refusals and the C surface."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bootstrap_cases as BC
from tests import encaps_cases as EC
from tests import hybrid_cases as HC
from tests import hybrid_encaps_cases as HE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def twin_evaluator(s):
    from seal_fyp_logistic_regression_amd import seal as S
    ctx = HC.context(s, "oracle")
    assert getattr(ctx.backend, "hybrid_raise_switch", None) is None and getattr(ctx.backend, "hybrid_collapse_key", None) is None
    return ctx, S.Evaluator(ctx)


def as_keys(ctx, alpha, key):
    from seal_fyp_logistic_regression_amd import seal as S
    high = S.HybridKeys(alpha)
    high.keys[1] = ctx.backend.from_host(key)
    return S.HybridEncapsKeys(None, high, HE.HAMMING_WEIGHT)


@pytest.mark.parametrize("case", HE.word_cases(), ids=HE.case_id)
def test_the_host_statement_equals_the_model(case):
    from seal_fyp_logistic_regression_amd import seal as S
    name, L, kind = case
    s = HC.sets()[name]
    ct, key = HE.case_input(s, kind)
    want_ckey, want = HE.case_model(case)
    assert np.array_equal(S.hybrid_collapse_key_host(key, s.primes, s.alpha, L), want_ckey)
    assert np.array_equal(S.hybrid_raise_switch_host(HC.twin(s), s.primes, s.alpha, L, ct, want_ckey), want)
    # ... and through the front end, which collapses the key itself and caches it per level
    ctx, ev = twin_evaluator(s)
    keys = as_keys(ctx, s.alpha, key)
    got = ev.raise_switch(EC.as_ciphertext(ctx, ct, 2.0 ** 30), keys, L)
    assert got.size() == 2 and got.parms_id() == L and got.scale == 2.0 ** 30 and L in keys._collapsed
    assert np.array_equal(np.asarray(ctx.backend.to_host(got.data)).reshape(2, L, s.N), want)


@pytest.mark.parametrize("name", HE.ALPHA_ONE)
def test_alpha_one_gives_the_words_of_the_one_special_prime_path(name):
    from seal_fyp_logistic_regression_amd import seal as S
    s = HC.sets()[name]
    assert s.alpha == 1
    ctx, ev = twin_evaluator(s)
    for L in HE.TABLE[name]:
        for kind in HE.INPUTS:
            ct, key = HE.case_input(s, kind)
            ckey, want = HE.case_model((name, L, kind))
            assert np.array_equal(S.collapse_key_host(key, s.primes, L)[:, list(range(L)) + [s.k - 1]], ckey)
            composed = ev._raise_switch_composed(EC.as_ciphertext(ctx, ct), EC.as_keys(ctx, key), L)
            assert np.array_equal(np.asarray(ctx.backend.to_host(composed)).reshape(2, L, s.N), want), (L, kind)


def test_the_default_level_is_k_minus_alpha_and_the_range_is_checked():
    s = HC.sets()["k7a2-p50_60"]
    ctx, ev = twin_evaluator(s)
    ct, key = HE.case_input(s, "uniform")
    keys = as_keys(ctx, s.alpha, key)
    got = ev.raise_switch(EC.as_ciphertext(ctx, ct), keys)
    assert got.parms_id() == s.k - s.alpha == 5
    assert np.array_equal(np.asarray(ctx.backend.to_host(got.data)).reshape(2, 5, s.N), HE.case_model(("k7a2-p50_60", 5, "uniform"))[1])
    for L in (1, s.k - s.alpha + 1):
        with pytest.raises(ValueError, match="target level"):
            ev.raise_switch(EC.as_ciphertext(ctx, ct), keys, L)
    with pytest.raises(ValueError, match="last prime"):
        ev.raise_switch(got, keys, 5)


# ---- the keys -------------------------------------------------------------------------------------------------------------
def generator(s, seed=BC.KEY_SEED):
    from seal_fyp_logistic_regression_amd import seal as S
    ctx = HC.context(s, "oracle")
    return ctx, S.KeyGenerator(ctx, seed)


def test_low_is_the_ordinary_low_key_and_high_at_alpha_one_the_ordinary_high_key():
    from seal_fyp_logistic_regression_amd import seal as S
    s = HC.sets()["k4a1-p50_60"]
    ctx, kg = generator(s)
    be, k, N = ctx.backend, s.k, s.N
    plain = kg.encapsulation_keys(HE.HAMMING_WEIGHT, seed=HE.AUX_SEED)
    keys = kg.hybrid_encapsulation_keys(1, HE.HAMMING_WEIGHT, seed=HE.AUX_SEED)
    assert isinstance(keys, S.HybridEncapsKeys) and isinstance(keys.high, S.HybridKeys) and keys.high.alpha == 1
    assert not any(isinstance(v, S.SecretKey) for v in vars(keys).values()) and keys.hamming_weight == HE.HAMMING_WEIGHT
    low = np.asarray(be.to_host(keys.low)).reshape(k - 1, 2, k, N)
    assert np.array_equal(low, np.asarray(be.to_host(plain.low)).reshape(k - 1, 2, k, N))
    mask = np.zeros(low.shape, dtype=bool)
    mask[0][:, [0, k - 1]] = True
    assert not low[~mask].any() and low[mask].all()
    assert np.array_equal(np.asarray(be.to_host(keys.high.hybrid_key(1))).reshape(-1), np.asarray(be.to_host(plain.high)).reshape(-1))
    with pytest.raises(ValueError, match="alpha"):
        kg.hybrid_encapsulation_keys(s.k, HE.HAMMING_WEIGHT, seed=HE.AUX_SEED)
    with pytest.raises(ValueError, match="hamming_weight"):
        kg.hybrid_encapsulation_keys(1, 0, seed=HE.AUX_SEED)


def test_low_is_the_same_at_alpha_two_and_the_generators_later_keys_keep_their_stream_ids():
    s = HC.sets()["k7a2-p50_60"]
    ctx, kg = generator(s)
    _, other = generator(s)
    be, k, N = ctx.backend, s.k, s.N
    before = kg._stream
    keys = kg.hybrid_encapsulation_keys(s.alpha, HE.HAMMING_WEIGHT, seed=HE.AUX_SEED)
    assert kg._stream == before
    low = np.asarray(be.to_host(keys.low)).reshape(k - 1, 2, k, N)
    assert np.array_equal(low, np.asarray(be.to_host(other.encapsulation_keys(HE.HAMMING_WEIGHT, seed=HE.AUX_SEED).low)).reshape(low.shape))
    assert not low[1:].any() and not low[0][:, 1:k - 1].any() and low[0][:, [0, k - 1]].all()
    assert np.asarray(be.to_host(keys.high.hybrid_key(1))).size == s.dnum * 2 * k * N
    # the keys drawn AFTER the encapsulation keys are the ones a generator that never made them draws
    assert np.array_equal(be.to_host(kg.hybrid_relin_keys(s.alpha).hybrid_key(0)), be.to_host(other.hybrid_relin_keys(s.alpha).hybrid_key(0)))
    assert np.array_equal(kg.public_key(), other.public_key())


# ---- the noise under real keys --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HE.NOISE_SETS)
def test_the_noise_under_real_keys_stays_within_the_derived_bound(name):
    """a DENSE main secret; s' redrawn from its seed; dec_s(out) - (y + x s') centred mod Q_L, in exact integers, against B"""
    s = HC.sets()[name]
    L = s.k - s.alpha
    B, Q = HE.noise_bound(s, L)
    assert 4 * B < Q                                                    # a condition on the input
    ctx, kg = generator(s)
    be = ctx.backend
    e = dict(ctx=ctx, kg=kg)
    assert HE.dense(e)
    keys = kg.hybrid_encapsulation_keys(s.alpha, HE.HAMMING_WEIGHT, seed=HE.AUX_SEED)
    aux = EC.sparse_secret(ctx, HE.AUX_SEED, HE.HAMMING_WEIGHT)
    from seal_fyp_logistic_regression_amd import seal as S
    ct, _ = HE.case_input(s, "uniform")
    out = np.asarray(be.to_host(S.Evaluator(ctx).raise_switch(EC.as_ciphertext(ctx, ct), keys, L).data)).reshape(2, L, s.N)
    tw, q = HC.twin(s), s.primes
    y, x = HE.centred_lift(tw, q[0], ct[0, 0]), HE.centred_lift(tw, q[0], ct[1, 0])
    assert int(np.abs(x).max()) <= q[0] // 2
    want = [(HC._fwd(tw, j, y, q[j]) + HC._fwd(tw, j, x, q[j]) * aux.host[j].astype(object)) % q[j] for j in range(L)]
    got = HC.decrypt_rows(out, kg.secret_key().host, q)
    diff, Q_ = HC.centred_integers(tw, [(g - w) % q[j] for j, (g, w) in enumerate(zip(got, want))], q)
    noise = int(np.abs(diff).max())
    print(f"[hybrid encaps cpu] {name} L = {L}: max noise {noise}, bound B = {B} (Q_L has {Q.bit_length()} bits)")
    assert Q_ == Q and noise <= B


# ---- the bootstrap under a dense secret, on the twin ----------------------------------------------------------------------
def test_bootstrap_hybrid_under_a_dense_secret_on_the_twin():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from tests import hybrid_bsgs_cases as HB
    from tests.test_encaps_cpu import raised_integer_part
    e = HE.boot_env("oracle")
    plan, ev, keys = e["plan"], e["ev"], e["keys"]
    assert HE.dense(e) and plan.special == HB.BOOT_ALPHA == keys.high.alpha
    v, ct = HE.boot_input(e)
    raised = ev.raise_switch(ev.switch_key(ct, keys.low), keys, plan.top_level)
    assert raised.parms_id() == plan.top_level == e["ctx"].k - HB.BOOT_ALPHA
    I = raised_integer_part(e, raised)
    print(f"[hybrid encaps cpu] bootstrap chain, auxiliary seed {HE.AUX_SEED}: max |I| = {I} (K = {plan.K})")
    assert I <= plan.K == 12 and I == HE.AUX_MAX_I                      # a condition on the input
    out = alg.bootstrap_hybrid(ev, ct, plan, e["hgk"], e["hrk"], e["encoded"], encaps=keys)
    assert out.size() == 2 and out.parms_id() == plan.result_level and abs(out.scale / BC.SCALE - 1.0) < 1e-12
    got = e["encoder"].decode(e["dec"].decrypt(out))
    err = float(np.abs(got[:len(v)] - v).max() / np.abs(v).max())
    # beside it: the same chain with a SPARSE main secret and no encapsulation (tests/hybrid_bsgs_cases.boot_env)
    es = HB.boot_env("oracle", True)
    _, cts = HE.boot_input(es)
    outs = alg.bootstrap_hybrid(es["ev"], cts, es["plan"], es["hgk"], es["hrk"], es["encoded"])
    errs = float(np.abs(es["encoder"].decode(es["dec"].decrypt(outs))[:len(v)] - v).max() / np.abs(v).max())
    print(f"[hybrid encaps cpu] twin bootstrap_hybrid under a dense secret, ns = {HB.BOOT_NS}: decode error {err:.3e}; under a sparse main "
          f"secret without encapsulation {errs:.3e} (cap {BC.CAP:g})")
    assert 0 < err <= BC.CAP


def test_the_refusals():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import bootstrap as B
    from seal_fyp_logistic_regression_amd import seal as S
    from tests import hybrid_bsgs_cases as HB
    e = HE.boot_env("oracle")
    plan, ev, kg = e["plan"], e["ev"], e["kg"]
    _, ct = HE.boot_input(e)
    plain = S.EncapsKeys(None, None, HE.HAMMING_WEIGHT)                 # (refused by its type, before anything is read)
    with pytest.raises(TypeError, match="hybrid_encapsulation_keys"):
        alg.bootstrap_hybrid(ev, ct, plan, e["hgk"], e["hrk"], e["encoded"], encaps=plain)
    other = S.HybridEncapsKeys(None, S.HybridKeys(1), HE.HAMMING_WEIGHT)
    with pytest.raises(ValueError, match="special"):
        alg.bootstrap_hybrid(ev, ct, plan, e["hgk"], e["hrk"], e["encoded"], encaps=other)
    # a HybridEncapsKeys passed to bootstrap: a TypeError that names the right constructor
    ref = BC.make(BC.N, BC.CHAIN_BITS, "oracle", galois_steps=(1,))
    p1 = B.plan(BC.N, ref["ctx"].primes, BC.SCALE, slots=HB.BOOT_NS)
    c1 = ref["enc"].encrypt(ref["encoder"].encode(np.ones(4), BC.SCALE, parms_id=1))
    with pytest.raises(TypeError, match="encapsulation_keys"):
        alg.bootstrap(ref["ev"], c1, p1, ref["gk"], ref["rk"], None, S.HybridEncapsKeys(None, None, HE.HAMMING_WEIGHT))
    # encaps=None is a keyword behind hoist_giants and changes nothing
    import inspect
    params = list(inspect.signature(alg.bootstrap_hybrid).parameters)
    assert params[-2:] == ["hoist_giants", "encaps"] and inspect.signature(alg.bootstrap_hybrid).parameters["encaps"].default is None
    assert {"sk", "key32", "sid"} <= set(inspect.signature(kg._hybrid_key).parameters)


# ---- the C surface --------------------------------------------------------------------------------------------------------
def test_the_library_carries_the_new_surface(tmp_path):
    from seal_fyp_logistic_regression_amd import _build, capi
    from seal_fyp_logistic_regression_amd.engine import Engine
    assert "hefx_hybrid_encaps.hip" in _build.SOURCES and "../../include/ext/hefx_hybrid_encaps.h" in _build.HEADERS
    assert all(os.path.exists(os.path.join(_build.CSRC, d)) for d in _build.DEPS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.library_path()], text=True)
    assert set(capi.HYBRID_ENCAPS_SYMBOLS) <= set(re.findall(r" T (hefx_[a-z_0-9]+)", out))
    header = os.path.join(ROOT, "include", "ext", "hefx_hybrid_encaps.h")
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(hefx_[a-z_0-9]+)\s*\(", src))) == capi.HYBRID_ENCAPS_SYMBOLS \
        == ["hefx_hybrid_collapse_key", "hefx_hybrid_raise_switch"]
    others = (capi.EXPORTED_SYMBOLS, capi.HYBRID_SYMBOLS, capi.HYBRID_HOIST_SYMBOLS, capi.HYBRID_BSGS_SYMBOLS, capi.ENCAPS_SYMBOLS)
    assert all(not set(capi.HYBRID_ENCAPS_SYMBOLS) & set(t) for t in others)
    assert all(callable(getattr(Engine, n, None)) for n in ("hybrid_collapse_key", "hybrid_raise_switch"))
    c = tmp_path / "t.c"
    c.write_text('#include "ext/hefx_hybrid_encaps.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_header_sits_outside_the_stream_coverage_table():
    """include/ext/ is not enumerated by tests/stream_ext_cases.extension_headers(): the reason the header gives for its place
    stays true, and its two stream entries are held to stream order by tests/test_gpu_hybrid_encaps.py instead"""
    from tests import stream_ext_cases as SX
    header = os.path.join(ROOT, "include", "ext", "hefx_hybrid_encaps.h")
    assert os.path.exists(header) and header not in SX.extension_headers()
    assert not any(os.path.basename(h) == "hefx_hybrid_encaps.h" for h in SX.extension_headers())
    assert sorted(SX.stream_entries(header)) == ["hefx_hybrid_collapse_key", "hefx_hybrid_raise_switch"]
    assert not set(SX.stream_entries(header)) & set(SX.COVERAGE)
    text = open(header).read()
    assert "include/ext/" in text and "tests/test_gpu_hybrid_encaps.py" in text


def test_the_decoys_of_the_stream_cases_give_other_words():
    for case in HE.STREAM_CASES:
        for c in HE.stream_cases(case):
            assert c.differs() and all(c.differs()), c.name
