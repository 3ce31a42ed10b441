"""Hybrid key switching without a GPU: the model of tests/hybrid_cases.py -- the integer statement of include/hefx_hybrid.h --
is pinned to what is already pinned (at alpha = 1 it is the oracle's key switch, word for word), held to the derived noise bound
at alpha > 1 under real keys, and the Python front end (keys, routing, refusals) runs on the oracle-backed twin."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import hybrid_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_SEED = 3

_ENV = {}


def env(name):
    """the twin of a set with real keys: Galois keys of the elements 3 and 2N - 1, the relinearisation key, one seed"""
    from seal_fyp_logistic_regression_amd import seal as S
    if name not in _ENV:
        s = HC.sets()[name]
        ctx = HC.context(s, "oracle")
        kg = S.KeyGenerator(ctx, KEY_SEED)
        _ENV[name] = dict(s=s, ctx=ctx, kg=kg, ev=S.Evaluator(ctx), gk=kg.hybrid_galois_keys(s.alpha, [1], conjugate=True),
                          rk=kg.hybrid_relin_keys(s.alpha))
    return _ENV[name]


def host(e, h):
    return np.asarray(e["ctx"].backend.to_host(h), dtype=np.uint64)


def centred_row(be, m, row, q):
    v = HC._inv(be, m, np.asarray(row % q).astype(np.uint64))
    return np.where((v > q // 2).astype(bool), v - q, v)


@pytest.mark.parametrize("name", HC.SMALL_SET_NAMES)
def test_a_generated_key_satisfies_the_key_equation_with_clipped_noise(name):
    """key[j][0] + key[j][1] s = F_j (.) s' - e_j in every row, e_j ONE integer polynomial with |e_j| <= 19"""
    e = env(name)
    s, be, q, N = e["s"], e["ctx"].backend, e["s"].primes, e["s"].N
    sk = e["kg"].secret_key().host.astype(object)
    P = int(np.prod(q[s.k - s.alpha:], dtype=object))
    targets = {3: HC.gather(N, 3, e["kg"].secret_key().host), 0: None}
    for index, keys in ((3, e["gk"]), (0, e["rk"])):
        key = host(e, keys.hybrid_key(index)).reshape(s.dnum, 2, s.k, N)
        new = targets[index].astype(object) if index else np.stack([sk[m] * sk[m] % q[m] for m in range(s.k)])
        for j in range(s.dnum):
            G = range(j * s.alpha, min((j + 1) * s.alpha, s.k - s.alpha))
            noise = None
            for m in range(s.k):
                F = P % q[m] if m in G else 0
                minus_e = (key[j, 0, m].astype(object) + key[j, 1, m].astype(object) * sk[m] - F * new[m]) % q[m]
                em = -centred_row(be, m, minus_e, q[m])
                assert np.abs(em).max() <= 19, (name, index, j, m)
                assert noise is None or np.array_equal(em, noise), (name, index, j, m)
                noise = em
            assert np.abs(noise).max() > 0


@pytest.mark.parametrize("mix", HC.MIXES)
def test_at_alpha_one_the_key_is_the_key_of_the_existing_generator(mix):
    from seal_fyp_logistic_regression_amd import seal as S
    s = HC.sets()[f"k4a1-{mix}"]
    ctx = HC.context(s, "oracle")
    old, new = S.KeyGenerator(ctx, KEY_SEED), S.KeyGenerator(ctx, KEY_SEED)
    gk, hk = old.galois_keys([1], conjugate=True), new.hybrid_galois_keys(1, [1], conjugate=True)
    assert sorted(gk.keys) == sorted(hk.keys) == [3, 2 * s.N - 1] and isinstance(hk, S.HybridKeys) and hk.alpha == 1
    for g in gk.keys:
        assert np.array_equal(np.asarray(gk.key(g)).reshape(-1), np.asarray(hk.hybrid_key(g)).reshape(-1)), g
    assert np.array_equal(np.asarray(old.relin_keys().key(0)).reshape(-1), np.asarray(new.hybrid_relin_keys(1).hybrid_key(0)).reshape(-1))


@pytest.mark.parametrize("name", HC.ALPHA_ONE_SET_NAMES, ids=HC.ALPHA_ONE_IDS)
def test_at_alpha_one_the_model_is_the_oracles_key_switch(name):
    """word for word: apply_galois (the element 1 is switch_key) and relinearize of the oracle, every word case of the set -- at
    k10a1 with nine digits (L = 9) and on the max key too"""
    s = HC.sets()[name]
    be = HC.twin(s)
    assert s.alpha == 1 and (name.startswith("k4a1") or max(s.levels) == 9)
    for case in HC.word_cases(s):
        L, form, kind, elt, key_kind = case
        ct, key = HC.case_input(s, case), HC.case_key(s, key_kind)
        assert key.shape == (s.k - 1, 2, s.k, s.N)
        want = be.apply_galois(L, ct.copy(), elt, key) if form == "galois" else be.relinearize(L, ct.copy(), key)
        assert np.array_equal(HC.case_model(s, case), np.asarray(want).reshape(2, L, s.N)), (name, case)


def noise_cases():
    out = []
    for name in HC.SMALL_SET_NAMES:
        s = HC.sets()[name]
        if s.alpha == 1:
            continue
        for L in s.levels:
            B, Q = HC.noise_bound(s, L)
            if 4 * B < Q:
                out.append((name, L))
            else:
                assert "s40" in name, (name, L)   # every set with 60-bit special primes qualifies at every level
    return out + [("n16384", 5), ("big7", 5)]             # the model at the large rings: one level each (the keys cost seconds there)


@pytest.mark.parametrize("name,L", noise_cases())
def test_the_model_keeps_the_noise_bound_under_real_keys(name, L):
    """dec(out) - pi_g(dec(in)) centred mod Q_L, in exact integers, against B = ceil(L/alpha) alpha N 19 Dmax / P + alpha (1 + N)
    (tests/hybrid_cases.py derives it); the operands are uniform or all q - 1: the identity holds for any words"""
    e = env(name)
    s, be, q, N = e["s"], e["ctx"].backend, e["s"].primes, e["s"].N
    sk = e["kg"].secret_key().host
    B, Q = HC.noise_bound(s, L)
    worst = 0
    for form, kind, elt in (("galois", "uniform", 3), ("galois", "max", 2 * N - 1), ("relin", "uniform", 0)):
        ct = HC.operand(s, kind, L, 2 if form == "galois" else 3, seed=41 + L)
        if form == "galois":
            out = HC.apply_galois_model(be, q, s.alpha, L, ct, elt, host(e, e["gk"].hybrid_key(elt)))
        else:
            out = HC.relinearize_model(be, q, s.alpha, L, ct, host(e, e["rk"].hybrid_key(0)))
        noise, Q_ = HC.switch_noise(s, L, form, elt, ct, out, sk)
        assert Q_ == Q
        worst = max(worst, noise)
    print(f"[hybrid cpu] {name} L = {L}: noise {worst} (bound {B}, Q_L / 4 = 2^{(Q // 4).bit_length() - 1})")
    assert worst <= B


def test_the_restated_launch_rules_at_hand_computed_points():
    """HC.split_of, item_rows and chunk_of (hy_split, hybrid_item_rows, hybrid_run's chunk lines) at points worked out by hand:
    N = 2048 has 4 workgroups a row group (1024 records / 256), N = 32768 has 64"""
    # a chunk: N = 2048, alpha = 2, L = 1: 3 + 1 * 3 + 2 + 4 + 2 = 14 rows, 2^30 / (14 * 2048 * 8) = 4681, the slot (10240 - 16) / 4 = 2556,
    # the cap 1024
    assert HC.item_rows(2048, 2, 1) == 14 and HC.table_words(2, 1) == 16 and HC.chunk_of(2048, 2, 1) == 1024
    # N = 32768, k = 7, alpha = 2, L = 5, dn = 3: 15 + 2 * 3 * 7 + 10 + 2 * 4 + 2 * 10 = 95 rows of 256 KiB: 2^30 / 24903680 = 43.1
    assert HC.item_rows(32768, 2, 5) == 95 and HC.chunk_of(32768, 2, 5) == 43
    assert HC.item_rows(16384, 2, 5) == 15 + 21 + 10 + 4 + 10              # every block once below N = 32768
    assert HC.table_words(1, 61) == 4151 and HC.RING_SLOT_PTRS == 10240     # the largest table the ABI allows fits a slot
    # the splits of the batch sweep, k7a2 at L = 5: convert has dn n = 3 n groups and 7 targets, spread 2 n groups and 5 targets
    for n, convert, spread in ((1, 4, 4), (43, 2, 4), (64, 2, 2), (86, 1, 2), (128, 1, 1)):
        assert (HC.convert_split(2048, 2, 5, n), HC.spread_split(2048, 5, n)) == (convert, spread), n
    assert HC.split_of(2048, 85 * 3, 7) == 2 and HC.split_of(2048, 86 * 3, 7) == 1     # 1020 < 1024 <= 1032 workgroups
    assert HC.split_of(2048, 127 * 2, 5) == 2 and HC.split_of(2048, 128 * 2, 5) == 1   # 1016 < 1024 <= 1024
    assert HC.split_of(2048, 1, 1) == 1 and HC.split_of(2048, 1, 2) == 2 and HC.split_of(2048, 1, 3) == 2   # at most targets / 2
    assert HC.split_of(32768, 1, 7) == 4 and HC.split_of(32768, 8, 7) == 2 and HC.split_of(32768, 16, 7) == 1   # 64, 512, 1024
    assert HC.convert_split(2048, 5, 7, 128) == 1 and HC.spread_split(2048, 7, 128) == 1    # k12a5 at L = 7, dn = 2


@pytest.mark.parametrize("name", ["k7a2-p50_60", "k8a3-d40_s60"])
def test_the_evaluator_on_the_twin_runs_the_statement(name):
    """rotate_vector, apply_galois, complex_conjugate, relinearize and switch_key with HybridKeys on a backend without the native
    entries: the words of the model"""
    from seal_fyp_logistic_regression_amd import seal as S
    e = env(name)
    s, be, ev, q, N = e["s"], e["ctx"].backend, e["ev"], e["s"].primes, e["s"].N
    L = max(s.levels)
    as_ct = lambda w, size: S.Ciphertext()._set(be.from_host(w), size, L, 1.0)
    ct2, ct3 = HC.operand(s, "uniform", L, 2, seed=9), HC.operand(s, "uniform", L, 3, seed=10)
    k3, kc, kr = (host(e, e["gk"].hybrid_key(3)), host(e, e["gk"].hybrid_key(2 * N - 1)), host(e, e["rk"].hybrid_key(0)))
    words = lambda c: np.asarray(be.to_host(c.data)).reshape(c.size(), L, N)
    want3 = HC.apply_galois_model(be, q, s.alpha, L, ct2, 3, k3)
    assert np.array_equal(words(ev.rotate_vector(as_ct(ct2, 2), 1, e["gk"])), want3)
    assert np.array_equal(words(ev.apply_galois(as_ct(ct2, 2), 3, e["gk"])), want3)
    assert np.array_equal(words(ev.complex_conjugate(as_ct(ct2, 2), e["gk"])), HC.apply_galois_model(be, q, s.alpha, L, ct2, 2 * N - 1, kc))
    assert np.array_equal(words(ev.relinearize_inplace(as_ct(ct3, 3), e["rk"])), HC.relinearize_model(be, q, s.alpha, L, ct3, kr))
    sw = e["kg"].hybrid_switching_key(s.alpha, e["kg"].secret_key())
    assert np.array_equal(words(ev.switch_key(as_ct(ct2, 2), sw)), HC.apply_galois_model(be, q, s.alpha, L, ct2, 1, host(e, sw.hybrid_key(1))))
    assert np.array_equal(words(as_ct(ct2, 2)), ct2)


def test_kswitch_keys_run_what_they_ran():
    """with KSwitchKeys the evaluator's methods call the backend's apply_galois / relinearize as before"""
    from seal_fyp_logistic_regression_amd import seal as S
    s = HC.sets()["k4a1-p50_60"]
    ctx = HC.context(s, "oracle")
    kg, ev, be, L = S.KeyGenerator(ctx, KEY_SEED), S.Evaluator(ctx), ctx.backend, 3
    gk, rk = kg.galois_keys([1], conjugate=True), kg.relin_keys()
    ct2, ct3 = HC.operand(s, "uniform", L, 2, seed=9), HC.operand(s, "uniform", L, 3, seed=10)
    as_ct = lambda w, size: S.Ciphertext()._set(be.from_host(w), size, L, 1.0)
    want = np.asarray(be.apply_galois(L, ct2.copy(), 3, gk.key(3)))
    assert np.array_equal(np.asarray(ev.rotate_vector(as_ct(ct2, 2), 1, gk).data), want)
    assert np.array_equal(np.asarray(ev.apply_galois(as_ct(ct2, 2), 3, gk).data), want)
    assert np.array_equal(np.asarray(ev.relinearize_inplace(as_ct(ct3, 3), rk).data), np.asarray(be.relinearize(L, ct3.copy(), rk.key(0))))
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.apply_galois(as_ct(ct2, 2), 5, gk)


def test_the_front_end_refuses_levels_alphas_and_fused_composites():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import seal as S
    e = env("k7a2-p50_60")
    s, be, ev, kg = e["s"], e["ctx"].backend, e["ev"], e["kg"]
    top = s.k - s.alpha
    at = lambda L, size: S.Ciphertext()._set(be.from_host(HC.operand(s, "uniform", L, size, seed=2) if L <= top else
                                                        np.zeros((size, L, s.N), dtype=np.uint64)), size, L, 1.0)
    for call in (lambda: ev.rotate_vector(at(top + 1, 2), 1, e["gk"]), lambda: ev.apply_galois(at(top + 1, 2), 3, e["gk"]),
                 lambda: ev.complex_conjugate(at(top + 1, 2), e["gk"]), lambda: ev.relinearize_inplace(at(top + 1, 3), e["rk"])):
        with pytest.raises(ValueError, match=r"level <= k - alpha = 5"):
            call()
    for alpha in (0, -1, s.k, S.HYBRID_ALPHA_MAX + 1):
        with pytest.raises(ValueError, match="alpha must lie in"):
            kg.hybrid_galois_keys(alpha, [1])
        with pytest.raises(ValueError, match="alpha must lie in"):
            kg.hybrid_relin_keys(alpha)
    ct = at(top, 2)
    for call in (lambda: alg.linear_transform_plain(ev, ct, [None, None], e["gk"]),
                 lambda: alg.linear_transform_plain_bsgs(ev, ct, [None, None], e["gk"]),
                 lambda: alg.linear_transform_cipher(ev, ct, [ct, ct], e["gk"]),
                 lambda: alg.coeffs_to_slots(ev, ct, None, e["gk"]),
                 lambda: alg.subsum(ev, ct, 4, e["gk"]),
                 lambda: alg.eval_mod(ev, [ct], None, e["rk"]),
                 lambda: alg.bootstrap(ev, ct, None, e["gk"], kg.relin_keys()),
                 lambda: alg.bootstrap(ev, ct, None, None, e["rk"])):
        with pytest.raises(TypeError, match=r"with HybridKeys \(alpha = 2\) is not supported"):
            call()
    with pytest.raises(TypeError, match="HybridKeys"):       # a composite that reads its keys itself
        e["gk"].key(3)
    with pytest.raises(TypeError, match="HybridKeys"):       # sizes above 3 need the keys of higher powers
        ev.relinearize_inplace(at(top, 4), e["rk"])


def test_capi_declares_the_four_symbols_and_the_build_lists_the_sources(tmp_path):
    from seal_fyp_logistic_regression_amd import _build, capi
    assert capi.HYBRID_SYMBOLS == ["hefx_hybrid_apply_galois_batch", "hefx_hybrid_digits", "hefx_hybrid_keygen",
                                   "hefx_hybrid_relinearize_batch"]
    assert "hefx_hybrid.hip" in _build.SOURCES and "../../include/hefx_hybrid.h" in _build.HEADERS
    text = open(os.path.join(ROOT, "include", "hefx_hybrid.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(hefx_[a-z_0-9]+)\s*\(", src))) == capi.HYBRID_SYMBOLS, "header and capi.py disagree"
    assert not set(capi.HYBRID_SYMBOLS) & set(capi.EXPORTED_SYMBOLS)   # hefx.h's table stays as it is
    assert int(re.search(r"#define HEFX_HYBRID_ALPHA_MAX (\d+)", text).group(1)) == capi.HYBRID_ALPHA_MAX
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.library_path()], text=True)
    assert set(capi.HYBRID_SYMBOLS) <= set(re.findall(r" T (hefx_[a-z_0-9]+)", out))
    c = tmp_path / "t.c"
    c.write_text('#include "hefx_hybrid.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_end_to_end_on_the_twin_and_the_allowance_of_the_gpu_test():
    """the program of tests/test_gpu_hybrid.py's end-to-end test on the oracle twin: its decode error, times HC.E2E_FACTOR, is the
    engine's allowance there -- held here to a thousandth of the largest expected value, so that a wrong rotation, a missing
    term or a wrong key cannot hide in it"""
    s = HC.sets()[HC.E2E_SET]
    assert (s.k, s.alpha) == (7, 2)
    e = HC.make_env(s, "oracle")
    ct, err = HC.end_to_end(e)
    v, w = HC.e2e_values(s.N)
    largest = float(np.abs(np.roll(v, -1) * w).max())
    print(f"[hybrid cpu] end to end at {s.name}: decode error {err:.3e}, allowance {HC.E2E_FACTOR * err:.3e}, largest value {largest:.3f}")
    assert ct.size() == 2 and ct.parms_id() == s.k - s.alpha - 1
    assert 0 < HC.E2E_FACTOR * err <= 1e-3 * largest
    assert float(np.abs(np.roll(v, -2) * w - np.roll(v, -1) * w).max()) > 0.1   # another rotation is far outside it
