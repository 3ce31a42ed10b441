"""Sparse-secret encapsulation on the oracle-backed twin (no GPU): KeyGenerator.encapsulation_keys, Evaluator.switch_key /
raise_switch and algorithms.bootstrap(..., encaps=).

The twin has no hefx_raise_switch: Evaluator.raise_switch takes its fall-back there -- the REFERENCE, the oracle's ordinary key
switch on a synthetic two-digit operand -- and this file holds it, word for word, to the statement of include/hefx_encaps.h
written directly in Python integers over the twin's transforms (tests/encaps_cases.py).  Then the noise against the prediction,
and the whole bootstrap under a DENSE main secret."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bootstrap_cases as BC
from tests import encaps_cases as EC
from tests import sparse_bootstrap_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENV = {}


def env(chain):
    if chain not in _ENV:
        _ENV[chain] = EC.make("oracle", bits=EC.CHAINS[chain])
    return _ENV[chain]


def switched_input(e, chain):
    """(the ciphertext under the dense secret at the last prime, the same switched to the sparse one)"""
    ct = e["enc"].encrypt(e["encoder"].encode(EC.input_values(), EC.SCALES[chain], parms_id=1))
    return ct, e["ev"].switch_key(ct, e["keys"].low)


def test_the_main_secret_is_dense_and_the_keys_keep_no_secret():
    from seal_fyp_logistic_regression_amd import seal as S
    e = env("wide0")
    ctx, be = e["ctx"], e["ctx"].backend
    coef = np.asarray(be.to_host(be.ntt_inverse(be.from_host(e["kg"].secret_key().host[:1].copy()), 1, 1, 0))).reshape(-1)
    assert np.count_nonzero(coef) > EC.N // 2
    keys = e["keys"]
    assert not any(isinstance(v, S.SecretKey) for v in vars(keys).values()) and keys.hamming_weight == EC.HAMMING_WEIGHT
    # the auxiliary secret is what the cases rebuild from its seed: exactly 32 entries of +-1
    sp = np.asarray(be.to_host(be.ntt_inverse(be.from_host(e["dec_sparse"].sk.host[:1].copy()), 1, 1, 0))).reshape(-1)
    assert np.count_nonzero(sp) == EC.HAMMING_WEIGHT and set(np.unique(sp)) <= {0, 1, int(ctx.primes[0]) - 1}
    with pytest.raises(ValueError, match="hamming_weight"):
        e["kg"].encapsulation_keys(0, seed=3)


def test_the_generators_other_keys_keep_their_stream_ids():
    a = BC.make(EC.N, EC.CHAINS["narrow0"], "oracle", seed=EC.DENSE_SEED, galois_steps=(1,))
    from seal_fyp_logistic_regression_amd import seal as S
    parms_ctx = a["ctx"]
    kg = S.KeyGenerator(parms_ctx, EC.DENSE_SEED)
    before = kg._stream
    kg.encapsulation_keys(EC.HAMMING_WEIGHT, seed=EC.SPARSE_SEED)
    assert kg._stream == before
    # (the order BC.make draws them in: Galois keys, public key, relinearisation key)
    assert np.array_equal(parms_ctx.backend.to_host(kg.galois_keys([1]).key(3)), parms_ctx.backend.to_host(a["gk"].key(3)))
    assert np.array_equal(kg.public_key(), a["kg"].public_key())
    assert np.array_equal(parms_ctx.backend.to_host(kg.relin_keys().key(0)), parms_ctx.backend.to_host(a["rk"].key(0)))


@pytest.mark.parametrize("chain", sorted(EC.CHAINS))
def test_low_is_zero_outside_what_one_prime_reads_and_switches_like_the_full_key(chain):
    from seal_fyp_logistic_regression_amd import seal as S
    e = env(chain)
    ctx, be, kg = e["ctx"], e["ctx"].backend, e["kg"]
    k, N = ctx.k, ctx.N
    low = np.asarray(be.to_host(e["keys"].low)).reshape(k - 1, 2, k, N)
    mask = np.zeros(low.shape, dtype=bool)
    mask[0][:, [0, k - 1]] = True
    assert not low[~mask].any() and low[mask].all()
    aux = EC.sparse_secret(ctx, EC.SPARSE_SEED, EC.HAMMING_WEIGHT)
    full = kg._kswitch_key(kg.secret_key().host, kg.secret_key().data, sk=aux, key32=S._key32(EC.SPARSE_SEED), sid=1)
    fullh = np.asarray(be.to_host(full)).reshape(k - 1, 2, k, N)
    assert np.array_equal(fullh[mask], low[mask]) and fullh[~mask].any()
    ct, sw = switched_input(e, chain)
    assert np.array_equal(BC.words(e, sw), np.asarray(be.apply_galois(1, ct.data, 1, full)).reshape(2, 1, N))
    # ... and the switched ciphertext decrypts under the SPARSE secret to what the input held
    got = e["encoder"].decode(e["dec_sparse"].decrypt(sw)).real
    err = float(np.abs(got - EC.input_values()).max())
    print(f"[encaps cpu] {chain}: dense -> sparse at one prime, decode error {err:.3e} at scale 2^{int(np.log2(EC.SCALES[chain]))}")
    # a sanity bound, not the criterion: a fresh encryption's coefficient noise is about 3.2 sqrt(4 N / 3) = 170, a slot sums N of
    # them with unit weights (7.6e3), and 2^17 is about 17 of those deviations; the key switch at one prime adds little to it
    assert err <= 2.0 ** 17 / EC.SCALES[chain]


@pytest.mark.parametrize("chain", sorted(EC.CHAINS))
@pytest.mark.parametrize("level", ["two", "top"])
def test_collapse_and_the_fall_back_equal_the_statement(chain, level):
    from seal_fyp_logistic_regression_amd import seal as S
    e = env(chain)
    ctx, be = e["ctx"], e["ctx"].backend
    L = 2 if level == "two" else ctx.first_parms_id()
    assert getattr(be, "raise_switch", None) is None
    high = np.asarray(be.to_host(e["keys"].high))
    want_kc = EC.collapse_model(high, ctx.primes, L)
    assert np.array_equal(S.collapse_key_host(high, ctx.primes, L)[:, list(range(L)) + [ctx.k - 1]], want_kc)
    _, sw = switched_input(e, chain)
    got = e["ev"].raise_switch(sw, e["keys"], L)
    assert got.size() == 2 and got.parms_id() == L and got.scale == sw.scale
    assert np.array_equal(BC.words(e, got), EC.raise_switch_model(be, ctx.primes, L, BC.words(e, sw), high))


@pytest.mark.parametrize("chain", sorted(EC.CHAINS))
def test_the_noise_stays_within_eight_predicted_deviations(chain):
    e = env(chain)
    ctx, ev = e["ctx"], e["ev"]
    L, q0 = ctx.first_parms_id(), int(ctx.primes[0])
    _, sw = switched_input(e, chain)
    want = EC.centred_q0(e, e["dec_sparse"].decrypt(ev.mod_raise(sw, L)))
    collapsed = EC.centred_q0(e, e["dec"].decrypt(ev.raise_switch(sw, e["keys"], L)))
    ordinary = EC.centred_q0(e, e["dec"].decrypt(ev.switch_key(ev.mod_raise(sw, L), e["keys"].high)))
    sigma = EC.predicted_deviation(ctx.primes, L, ctx.N)
    n_col = int(np.abs(EC.centred_difference(collapsed, want, q0)).max())
    n_ord = int(np.abs(EC.centred_difference(ordinary, want, q0)).max())
    print(f"[encaps cpu] {chain} L = {L}: predicted deviation {sigma:.1f}, bound {EC.NOISE_FACTOR * sigma:.0f}; "
          f"max noise collapsed {n_col}, ordinary {n_ord}")
    assert n_col <= EC.NOISE_FACTOR * sigma and n_ord <= EC.NOISE_FACTOR * sigma
    if chain == "wide0":
        assert round(sigma) == 94


def raised_integer_part(e, raised):
    """max |I| of the plaintext m + q_0 I of a raised ciphertext under the main secret (BC.raised_coefficients' arithmetic)"""
    be, ctx = e["ctx"].backend, e["ctx"]
    pt = e["dec"].decrypt(raised)
    rows = np.array(be.to_host(pt.data), dtype=np.uint64).reshape(raised.parms_id(), ctx.N)[:2].copy()
    coef = np.asarray(be.to_host(be.ntt_inverse(be.from_host(rows), 1, 2, 0))).reshape(2, ctx.N)
    q0, q1 = int(ctx.primes[0]), int(ctx.primes[1])
    a0, a1 = coef[0].astype(object), coef[1].astype(object)
    t = a0 + q0 * (((a1 - a0) * pow(q0, -1, q1)) % q1)
    t = np.where((t > q0 * q1 // 2).astype(bool), t - q0 * q1, t)
    return int(max(abs((int(x) + q0 // 2) // q0) for x in t))


def test_bootstrap_under_a_dense_secret():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    ns = SC.SPARSE_NS
    p = SC.sparse_plan(ns)
    e = EC.make("oracle", BC.N, BC.CHAIN_BITS, galois_steps=tuple(sorted(set(p.galois_steps()))), conjugate=True)
    be = e["ctx"].backend
    coef = np.asarray(be.to_host(be.ntt_inverse(be.from_host(e["kg"].secret_key().host[:1].copy()), 1, 1, 0))).reshape(-1)
    assert np.count_nonzero(coef) > BC.N // 2                      # the main secret is DENSE
    v = SC.sparse_input(ns)
    ct = SC.encrypt_tiled(e, v)
    raised = e["ev"].raise_switch(e["ev"].switch_key(ct, e["keys"].low), e["keys"], p.top_level)
    I = raised_integer_part(e, raised)
    print(f"[encaps cpu] bootstrap chain, sparse seed {EC.SPARSE_SEED}: max |I| = {I} (K = {p.K})")
    assert I <= p.K == 12                                           # a condition on the input
    out = alg.bootstrap(e["ev"], ct, p, e["gk"], e["rk"], p.encode(e["encoder"]), encaps=e["keys"])
    assert out.size() == 2 and out.parms_id() == p.result_level and abs(out.scale / BC.SCALE - 1.0) < 1e-12
    err = float(np.abs(e["encoder"].decode(e["dec"].decrypt(out)).real - SC.tiled(v)).max() / np.abs(v).max())
    print(f"[encaps cpu] twin bootstrap under a dense secret, ns = {ns}: decode error {err:.3e} (cap {BC.CAP:g})")
    assert err <= BC.CAP
    # the refusals
    ev = e["ev"]
    sw = ev.switch_key(ct, e["keys"].low)
    with pytest.raises(ValueError, match="size must be 2"):
        ev.raise_switch(ev.square(ev.mod_raise(sw, 2)), e["keys"], 2)
    with pytest.raises(ValueError, match="size must be 2"):
        ev.switch_key(ev.square(ev.mod_raise(sw, 2)), e["keys"].low)
    with pytest.raises(ValueError, match="last prime"):
        ev.raise_switch(ev.mod_raise(sw, 2), e["keys"], 3)
    with pytest.raises(ValueError, match="target level"):
        ev.raise_switch(sw, e["keys"], 1)
    with pytest.raises(ValueError, match="target level"):
        ev.raise_switch(sw, e["keys"], e["ctx"].first_parms_id() + 1)
    from seal_fyp_logistic_regression_amd import bootstrap as B
    from seal_fyp_logistic_regression_amd import seal as S
    shorter = B.plan(BC.N, S.CoeffModulus.Create(BC.N, BC.CHAIN_BITS[:-2] + [60]), BC.SCALE, slots=ns)   # a plan for another chain
    with pytest.raises(ValueError, match="another ring or chain"):
        alg.bootstrap(ev, ct, shorter, e["gk"], e["rk"], encaps=e["keys"])


def test_the_library_carries_the_new_surface(tmp_path):
    from seal_fyp_logistic_regression_amd import _build, capi
    assert "hefx_encaps.hip" in _build.SOURCES and "../../include/hefx_encaps.h" in _build.HEADERS
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.library_path()], text=True)
    assert set(capi.ENCAPS_SYMBOLS) <= set(re.findall(r" T (hefx_[a-z_0-9]+)", out))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hefx_encaps.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(hefx_[a-z_0-9]+)\s*\(", src))) == capi.ENCAPS_SYMBOLS \
        == ["hefx_collapse_key", "hefx_raise_switch", "hefx_switch_key"]
    assert not set(capi.ENCAPS_SYMBOLS) & set(capi.EXPORTED_SYMBOLS)   # hefx.h's table stays as it is
    c = tmp_path / "t.c"
    c.write_text('#include "hefx_encaps.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
