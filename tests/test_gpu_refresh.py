"""Mod-raise and refresh on the GPU (include/hefx_refresh.h): the lift against an exact model, the refresh against the
oracle twin, refusals, caller-owned streams, and the training step that ends.

The lift.  hefx_mod_raise against tests/refresh_cases.lift (plain CRT in Python integers), word for word, on polynomials
that carry 0, 1, Q - 1, Q // 2, Q // 2 + 1 and values whose mixed-radix digits above digit 0 are those of Q // 2, at
coefficient 0, at N - 1 and at random positions among random fill.  N = 1024 (four workgroups of the lift kernel per item,
the smallest degree the engine serves); L_in -> L_out in {1 -> 2, 1 -> 8, 2 -> 3, 7 -> 8, 3 -> 8}: one digit (no Garner
step), two digits, the longest digit array of the LR chain, one new row and many.  Prime sets: the LR chain {60, 40 x 7,
60}; `mixed` of tests/policy_sets.py (a 60-bit prime, a tiny one and 40-bit primes among the old rows, a data prime just
above 2^60 in row 7 among the new rows); `straddle60` (60-bit old rows, new rows above 2^60; four data primes, so the shapes
are cut to those that fit).  count 1 runs the lift where its rows belong, count 3 through the group's workspace.

The refresh.  The same host code (seal.Decryptor.refresh) on the engine -- one hefx_refresh call -- and on the oracle twin,
which has no such entry and composes decrypt, transforms, seal.lift_coefficients and encrypt: same seeds, same words.

Training.  algorithms.update_weights_refreshed / train_cipher on engine and twin, word for word in both rescale
divisions, and the decoded weights within refresh_cases.train_allowance (8 x the twin's own error against the plain
recurrence, tests/test_refresh_cpu.py) of w - (lr / n) g(w)."""
import os
import subprocess

import numpy as np
import pytest

from tests import lr_gradient_cases as G
from tests import refresh_cases as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 2), (1, 8), (2, 3), (7, 8), (3, 8)]
_engines = {}
_sets = {}


def prime_set(name, N=1024):
    if (name, N) not in _sets:
        from seal_fyp_logistic_regression_amd import seal as S
        from tests import policy_sets
        if name == "lr":
            _sets[(name, N)] = S.CoeffModulus.Create(N, G.LR_BITS)
        else:
            _sets[(name, N)] = policy_sets.toy_sets(N)[{"mixed": "mixed2048", "straddle60": "straddle60"}[name]].primes
    return _sets[(name, N)]


def engine(name, N=1024):
    from seal_fyp_logistic_regression_amd import Engine
    if (name, N) not in _engines:
        _engines[(name, N)] = Engine(N, prime_set(name, N))
    return _engines[(name, N)]


def test_the_policy_sets_put_the_primes_where_the_docstring_says():
    mixed, straddle = prime_set("mixed"), prime_set("straddle60")
    assert len(mixed) == 10 and 1 << 59 < mixed[0] < 1 << 60 and 1 << 60 < mixed[7] < 1 << 61 and mixed[1] < 1 << 20
    assert len(straddle) == 5 and all(1 << 59 < q < 1 << 60 for q in straddle[:2]) and all(q > 1 << 60 for q in straddle[2:])


# ---- the lift against the exact model
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["lr", "mixed", "straddle60"])
def test_mod_raise_equals_the_exact_model(name, shape, count):
    primes, e = prime_set(name), engine(name)
    data = len(primes) - 1
    L_in, L_out = min(shape[0], data - 1), min(shape[1], data)
    words = R.crafted_words(primes, L_in, 1024, count, seed=100 * L_in + L_out)
    want = R.lift(words, primes, L_in, L_out)
    d_in = e.to_device(words)
    out = e.mod_raise(L_in, L_out, d_in, count=count)
    got = out.download().reshape(count, L_out, 1024)
    assert np.array_equal(got[:, :L_in], words), "rows below L_in are the input's words"
    assert np.array_equal(got, want)
    assert d_in.download().tobytes() == words.tobytes(), "the input is left as it is"


def test_mod_raise_at_n4096():
    primes, e = prime_set("lr", 4096), engine("lr", 4096)
    words = R.crafted_words(primes, 2, 4096, 2, seed=7)
    d_in = e.to_device(words)
    got = e.mod_raise(2, 8, d_in, count=2).download().reshape(2, 8, 4096)
    assert np.array_equal(got, R.lift(words, primes, 2, 8))
    assert d_in.download().tobytes() == words.tobytes()


# ---- refresh against the twin
_envs = {}


def both_envs(mode="round", galois_steps=None):
    """engine and twin environments on the LR chain at N = 4096 from the same seeds, made once per rescale division and
    key set.  Encryptions advance their stream counters: every test draws the same calls from both."""
    from tests.test_gpu_composites import make
    key = (mode, tuple(galois_steps) if galois_steps else None)
    if key not in _envs:
        _envs[key] = tuple(make(4096, G.LR_BITS, kind, seed=G.KEY_SEED, galois_steps=galois_steps) for kind in ("gpu", "oracle"))
    return _envs[key]


def _low_level_ct(e, size, level):
    v = np.linspace(-1.5, 1.5, 16)
    ct = e["enc"].encrypt(e["encoder"].encode(v, G.SCALE))
    if size == 3:
        ct = e["ev"].multiply(ct, e["enc"].encrypt(e["encoder"].encode(np.ones(16), G.SCALE)))
        e["ev"].rescale_to_next_inplace(ct)
    e["ev"].mod_switch_to_inplace(ct, level)
    assert ct.size() == size and ct.parms_id() == level
    return ct


@pytest.mark.parametrize("size,L_in,target", [(2, 1, None), (3, 1, None), (2, 3, 5), (3, 2, 2), (2, 8, None)])
def test_refresh_same_words_as_the_twin(size, L_in, target):
    """sizes 2 and 3 to the first level, a lift between two inner levels, and L_in == L_out (the lift is skipped) below
    and at the first level"""
    eg, eo = both_envs()
    assert hasattr(eg["ctx"].backend, "refresh") and not hasattr(eo["ctx"].backend, "refresh")
    eg["enc"]._stream = eo["enc"]._stream = 1000 + 10 * size + L_in
    rs = []
    for e in (eg, eo):
        ct = _low_level_ct(e, size, L_in)
        rs.append((ct, e["dec"].refresh(ct, e["enc"], parms_id=target)))
    (cg, rg), (co, ro) = rs
    assert G.compare(eg, cg, eo, co) == []
    L_out = target if target is not None else eg["ctx"].first_parms_id()
    assert (rg.size(), rg.parms_id(), rg.scale) == (2, L_out, cg.scale)
    assert G.compare(eg, rg, eo, ro) == []
    assert eg["enc"]._stream == eo["enc"]._stream
    a = eg["encoder"].decode(eg["dec"].decrypt(cg))[:16].real
    b = eg["encoder"].decode(eg["dec"].decrypt(rg))[:16].real
    assert np.abs(a - b).max() < 1e-6  # fresh noise of at most 19 (2N + 1) per coefficient at scale 2^40


def test_refresh_many_same_words_as_the_twin():
    eg, eo = both_envs()
    eg["enc"]._stream = eo["enc"]._stream = 2000
    outs = []
    for e in (eg, eo):
        cts = [_low_level_ct(e, 2, 1) for _ in range(3)]
        outs.append(e["dec"].refresh_many(cts, e["enc"]))
    for a, b in zip(*outs):
        assert (a.size(), a.parms_id()) == (2, eg["ctx"].first_parms_id())
        assert G.compare(eg, a, eo, b) == []
    assert eg["enc"]._stream == eo["enc"]._stream


def test_a_wrong_word_of_a_refresh_is_caught():
    """the comparison is not vacuous: one word of the twin's result flipped, on a copy"""
    from seal_fyp_logistic_regression_amd import seal as S
    eg, eo = both_envs()
    eg["enc"]._stream = eo["enc"]._stream = 3000
    rg, ro = (e["dec"].refresh(_low_level_ct(e, 2, 1), e["enc"]) for e in (eg, eo))
    assert G.compare(eg, rg, eo, ro) == []
    for p, j, i in ((0, 0, 0), (1, 7, 4095), (0, 3, 17)):  # an old row, the last new row, one in between
        flipped = G.words(eo, ro).copy()
        flipped[p, j, i] ^= 1
        assert G.compare(eg, rg, eo, S.Ciphertext()._set(flipped, 2, ro.parms_id(), ro.scale)) == ["words"]
    assert G.compare(eg, rg, eo, ro) == []  # the twin's own result was not touched


# ---- the batch against the single call
def _random_rows(rng, primes, shape_front, rows, N):
    out = np.empty(tuple(shape_front) + (len(rows), N), dtype=np.uint64)
    for r, j in enumerate(rows):
        out[..., r, :] = rng.integers(0, int(primes[j]), tuple(shape_front) + (N,), dtype=np.uint64)
    return out


def _raw_operands(e, primes, L_in, size, n, seed=3):
    """canonical random words: any words are a ciphertext, a secret key and a public key to the arithmetic"""
    N, k = e.N, len(primes)
    rng = np.random.default_rng(seed)
    cts = [e.to_device(_random_rows(rng, primes, (size,), range(L_in), N)) for _ in range(n)]
    sk = e.to_device(_random_rows(rng, primes, (), range(k), N))
    pk = e.to_device(_random_rows(rng, primes, (2,), range(k), N))
    return cts, sk, pk


KEY32 = bytes(range(32))


def test_refresh_batch_equals_the_single_calls():
    from seal_fyp_logistic_regression_amd import capi
    primes, e = prime_set("lr"), engine("lr")
    group = capi.REFRESH_GROUP
    for n in (1, 3, group + 1):
        cts, sk, pk = _raw_operands(e, primes, 1, 2, n, seed=n)
        outs = e.refresh_batch(1, 2, 2, cts, sk, pk, KEY32, 50)
        assert len(outs) == n
        for i in range(n):
            one = e.refresh(1, 2, 2, cts[i], sk, pk, KEY32, 50 + i).download()
            assert np.array_equal(outs[i].download(), one), (n, i)
    # three polynomials, two old rows, and no lift at all
    for L_in, size, L_out in ((2, 3, 5), (3, 2, 3)):
        cts, sk, pk = _raw_operands(e, primes, L_in, size, 3, seed=9)
        outs = e.refresh_batch(L_in, size, L_out, cts, sk, pk, KEY32, 7)
        for i in range(3):
            assert np.array_equal(outs[i].download(), e.refresh(L_in, size, L_out, cts[i], sk, pk, KEY32, 7 + i).download())


def test_refresh_is_decrypt_mod_raise_encrypt():
    """the words the header promises: hefx_decrypt, hefx_mod_raise, hefx_encrypt with the same key32 / stream id"""
    primes, e = prime_set("mixed"), engine("mixed")
    for L_in, size, L_out in ((1, 2, 9), (3, 3, 8), (4, 2, 4)):
        cts, sk, pk = _raw_operands(e, primes, L_in, size, 1, seed=L_out)
        pt = e.decrypt(L_in, size, cts[0], sk)
        if L_in < L_out:
            pt = e.mod_raise(L_in, L_out, pt)
        want = e.encrypt(L_out, pk, pt, KEY32, 11).download()
        assert np.array_equal(e.refresh(L_in, size, L_out, cts[0], sk, pk, KEY32, 11).download(), want)


# ---- refusals: HEFX_ERR_INVALID before a word is written
PATTERN = np.uint64(0xA5A5A5A5A5A5A5A5)


def test_refusals_write_nothing():
    from seal_fyp_logistic_regression_amd import Engine, capi
    from tests import policy_sets
    N = 1024
    primes = policy_sets.primes_below(1 << 41, N, 19)  # 18 data primes: room for an L_in above the digit array
    e = Engine(N, primes)
    lib, h = capi.lib(), e._h
    k = len(primes)
    rng = np.random.default_rng(1)
    slab_words = 64 * N
    host = rng.integers(0, 1 << 40, slab_words, dtype=np.uint64)
    host[: 40 * N] = PATTERN  # the outputs' region
    slab = e.to_device(host)  # every operand is a window of one slab: overlaps are plain offsets
    out, out2 = slab.ptr, slab.ptr + 20 * N * 8  # room for [2][8][N] each
    src = slab.ptr + 40 * N * 8                  # [3][2][N] ciphertexts / plaintext rows
    src2 = src + 6 * N * 8
    keys = e.to_device(rng.integers(0, 1 << 40, 3 * k * N, dtype=np.uint64))
    sk, pk = keys.ptr, keys.ptr + k * N * 8
    keys_host = keys.download()
    arr = lambda *p: capi.ptr_array(list(p))

    def refused(rc, what):
        assert rc == capi.HEFX_ERR_INVALID, (what, rc, lib.hefx_last_error())
        e.sync()
        assert slab.download().tobytes() == host.tobytes(), what
        assert keys.download().tobytes() == keys_host.tobytes(), what

    raise_ = lambda L_in, L_out, count, i, o: lib.hefx_mod_raise(h, L_in, L_out, count, i, o, None)
    refused(raise_(2, 2, 1, src, out), "mod_raise L_in == L_out")
    refused(raise_(3, 2, 1, src, out), "mod_raise L_in > L_out")
    refused(raise_(0, 2, 1, src, out), "mod_raise L_in < 1")
    refused(raise_(1, k, 1, src, out), "mod_raise L_out above the data primes")
    refused(raise_(17, 18, 1, src, out), "mod_raise L_in above the digit array")
    refused(raise_(1, 2, 0, src, out), "mod_raise count < 1")
    refused(raise_(1, 2, 1, None, out), "mod_raise null input")
    refused(raise_(1, 2, 1, src, None), "mod_raise null output")
    refused(raise_(1, 2, 1, src, src), "mod_raise in place")
    refused(raise_(2, 3, 1, src, src + N * 8), "mod_raise output inside the input")
    refused(raise_(1, 2, 2, src, src - 3 * N * 8), "mod_raise output's tail over the input")

    one = lambda L_in, size, L_out, ct, s, p, key, o, sid=5: lib.hefx_refresh(h, L_in, size, L_out, ct, s, p, key, sid, o, None)
    refused(one(3, 2, 2, src, sk, pk, KEY32, out), "refresh L_in > L_out")
    refused(one(0, 2, 2, src, sk, pk, KEY32, out), "refresh L_in < 1")
    refused(one(1, 2, k, src, sk, pk, KEY32, out), "refresh L_out above the data primes")
    refused(one(17, 2, 18, src, sk, pk, KEY32, out), "refresh L_in above the digit array")
    refused(one(1, 1, 2, src, sk, pk, KEY32, out), "refresh size < 2")
    refused(one(1, 2, 2, src, sk, pk, KEY32, out, sid=1 << 62), "refresh stream id")
    for i, what in enumerate(("ct", "sk", "pk", "key32", "out")):
        a = [src, sk, pk, KEY32, out]
        a[i] = None
        refused(one(1, 2, 2, *a), "refresh null " + what)
    refused(one(1, 2, 2, src, sk, pk, KEY32, src), "refresh in place")
    refused(one(1, 2, 2, src, sk, pk, KEY32, src + N * 8), "refresh output over the ciphertext's second polynomial")
    refused(one(2, 2, 2, src, sk, pk, KEY32, src - 3 * N * 8), "refresh output's tail over the ciphertext")
    refused(one(2, 2, 2, src, sk, pk, KEY32, sk + N * 8), "refresh output over the secret key's rows")
    refused(one(1, 2, 2, src, sk, pk, KEY32, pk + (2 * k - 4) * N * 8), "refresh output over the public key's last rows")
    refused(one(1, 2, 2, src, sk, pk, KEY32, pk), "refresh output over the public key")

    batch = lambda L_in, size, L_out, n, cts, s, p, key, outs, sid=5: lib.hefx_refresh_batch(
        h, L_in, size, L_out, n, cts, s, p, key, sid, outs, None)
    good_c, good_o = arr(src, src2), arr(out, out2)
    refused(batch(3, 2, 2, 2, good_c, sk, pk, KEY32, good_o), "batch L_in > L_out")
    refused(batch(1, 2, k, 2, good_c, sk, pk, KEY32, good_o), "batch L_out above the data primes")
    refused(batch(17, 2, 18, 2, good_c, sk, pk, KEY32, good_o), "batch L_in above the digit array")
    refused(batch(1, 1, 2, 2, good_c, sk, pk, KEY32, good_o), "batch size < 2")
    refused(batch(1, 2, 2, 0, good_c, sk, pk, KEY32, good_o), "batch n < 1")
    refused(batch(1, 2, 2, 2, None, sk, pk, KEY32, good_o), "batch null ciphertext list")
    refused(batch(1, 2, 2, 2, good_c, None, pk, KEY32, good_o), "batch null sk")
    refused(batch(1, 2, 2, 2, good_c, sk, None, KEY32, good_o), "batch null pk")
    refused(batch(1, 2, 2, 2, good_c, sk, pk, None, good_o), "batch null key32")
    refused(batch(1, 2, 2, 2, good_c, sk, pk, KEY32, None), "batch null output list")
    refused(batch(1, 2, 2, 2, arr(src, None), sk, pk, KEY32, good_o), "batch null ciphertext")
    refused(batch(1, 2, 2, 2, good_c, sk, pk, KEY32, arr(out, None)), "batch null output")
    refused(batch(1, 2, 2, 2, good_c, sk, pk, KEY32, arr(out, src)), "batch output 1 is item 0's ciphertext")
    refused(batch(1, 2, 2, 2, good_c, sk, pk, KEY32, arr(src2 + N * 8, out)), "batch output 0 inside item 1's ciphertext")
    refused(batch(1, 2, 2, 2, good_c, sk, pk, KEY32, arr(out, out)), "batch two outputs the same")
    refused(batch(1, 2, 2, 2, good_c, sk, pk, KEY32, arr(out, out + 3 * N * 8)), "batch two outputs overlap")
    refused(batch(1, 2, 2, 2, good_c, sk, pk, KEY32, arr(out, sk)), "batch output over the secret key")
    refused(batch(1, 2, 2, 2, good_c, sk, pk, KEY32, arr(pk + k * N * 8, out)), "batch output over the public key")
    refused(batch(1, 2, 2, 2, good_c, sk, pk, KEY32, good_o, sid=(1 << 62) - 1), "batch stream ids")
    # ... and the same calls with nothing wrong go through and write only their outputs
    assert batch(1, 2, 2, 2, good_c, sk, pk, KEY32, good_o) == capi.HEFX_OK
    assert one(2, 3, 8, src, sk, pk, KEY32, out) == capi.HEFX_OK
    assert raise_(1, 2, 2, src, out2) == capi.HEFX_OK
    e.sync()
    after = slab.download()
    assert after[40 * N:].tobytes() == host[40 * N:].tobytes() and keys.download().tobytes() == keys_host.tobytes()
    assert (after[: 16 * N] != PATTERN).all() and (after[20 * N: 24 * N] != PATTERN).all()
    assert (after[16 * N: 20 * N] == PATTERN).all() and (after[24 * N: 40 * N] == PATTERN).all()


# ---- caller-owned streams
def test_the_three_entries_return_while_their_stream_is_held_shut():
    from tests.hip_stream_gate import Stream
    primes, e = prime_set("lr"), engine("lr")
    N = 1024
    cts, sk, pk = _raw_operands(e, primes, 2, 2, 3, seed=21)
    pts = e.to_device(R.crafted_words(primes, 2, N, 3, seed=5))
    want_raise = e.mod_raise(2, 8, pts, count=3).download()
    want_one = e.refresh(2, 2, 8, cts[0], sk, pk, KEY32, 9).download()
    want_many = [o.download() for o in e.refresh_batch(2, 2, 8, cts, sk, pk, KEY32, 9)]
    o_raise, o_one, o_many = e.zeros(3, 8, N), e.zeros(2, 8, N), [e.zeros(2, 8, N) for _ in range(3)]
    e.sync()
    with Stream() as S:
        gate = S.gate()
        e.mod_raise(2, 8, pts, count=3, out=o_raise, stream=S.handle)
        assert not gate.opened, "hefx_mod_raise waited on the host"
        e.refresh(2, 2, 8, cts[0], sk, pk, KEY32, 9, out=o_one, stream=S.handle)
        assert not gate.opened, "hefx_refresh waited on the host"
        e.refresh_batch(2, 2, 8, cts, sk, pk, KEY32, 9, outs=o_many, stream=S.handle)
        assert not gate.opened, "hefx_refresh_batch waited on the host"
        e.sync(S.handle)
        assert gate.opened
    assert np.array_equal(o_raise.download(), want_raise)
    assert np.array_equal(o_one.download(), want_one)
    for got, want in zip(o_many, want_many):
        assert np.array_equal(got.download(), want)


# ---- training
_twin_steps = {}


def _keys(shape):
    return [1, -8] if shape == (8, 8) else None


def _steps(e, shape, iters):
    """the weights after each of `iters` steps of update_weights_refreshed, from freshly encrypted inputs"""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    e["enc"]._stream = 0  # the environments are shared: every run draws the same stream ids
    feats, featsT, cy, cw = G.encrypt_inputs(e, *G.inputs(*shape))
    out = []
    for _ in range(iters):
        cw = alg.update_weights_refreshed(e["ev"], e["encoder"], e["enc"], e["dec"], feats, featsT, cy, cw,
                                          R.LEARNING_RATE[shape], e["gk"], e["rk"], G.SCALE)
        out.append(cw)
    return out, (feats, featsT, cy)


def twin_steps(shape, mode):
    """computed once per (shape, division), read by the tests, never changed"""
    if (shape, mode) not in _twin_steps:
        _twin_steps[(shape, mode)] = _steps(both_envs(mode, _keys(shape))[1], shape, R.ITERS if shape == (3, 4) else 1)[0]
    return _twin_steps[(shape, mode)]


@pytest.mark.parametrize("shape", [(3, 4), (8, 8)])
def test_update_weights_refreshed_same_words_as_the_twin(shape, rescale_mode):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    eg, eo = both_envs(rescale_mode, _keys(shape))
    assert hasattr(eg["ctx"].backend, "refresh") and not hasattr(eo["ctx"].backend, "refresh")
    want = twin_steps(shape, rescale_mode)[0]
    (got,), _ = _steps(eg, shape, 1)
    top = eg["ctx"].first_parms_id()
    assert (got.size(), got.parms_id(), got.scale) == (2, top, 2.0 ** 40)
    assert G.compare(eg, got, eo, want) == []
    X, w, y = G.inputs(*shape)
    ws, _ = R.plain_training(X, w, y, alg.SIGMOID_COEFFS[3], R.LEARNING_RATE[shape], 1)
    err_g, err_o = G.decode_error(eg, got, ws[0]), G.decode_error(eo, want, ws[0])
    print(f"update_weights_refreshed {shape} {rescale_mode}: max |decoded - w| engine {err_g:.3e}, twin {err_o:.3e}, "
          f"allowance {R.train_allowance(shape):.3e}")
    assert err_g <= R.train_allowance(shape) and err_o <= R.train_allowance(shape)


def test_two_iterations_of_train_cipher_same_words_as_the_twin(rescale_mode):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    shape = (3, 4)
    eg, eo = both_envs(rescale_mode, _keys(shape))
    want = twin_steps(shape, rescale_mode)
    assert len(want) == R.ITERS == 2
    eg["enc"]._stream = 0
    X, w, y = G.inputs(*shape)
    feats, featsT, cy, cw = G.encrypt_inputs(eg, X, w, y)
    got = alg.train_cipher(eg["ev"], eg["encoder"], eg["enc"], eg["dec"], feats, featsT, cy, cw, R.LEARNING_RATE[shape],
                           R.ITERS, eg["gk"], eg["rk"], G.SCALE)
    assert (got.size(), got.parms_id(), got.scale) == (2, eg["ctx"].first_parms_id(), 2.0 ** 40)
    assert G.compare(eg, got, eo, want[-1]) == []
    ws, _ = R.plain_training(X, w, y, alg.SIGMOID_COEFFS[3], R.LEARNING_RATE[shape], R.ITERS)
    err = G.decode_error(eg, got, ws[-1])
    print(f"train_cipher {shape} {rescale_mode}: max |decoded - w| after {R.ITERS} iterations {err:.3e}, "
          f"allowance {R.train_allowance(shape):.3e}")
    assert err <= R.train_allowance(shape)
    # update_weights on the same inputs still stops where SEAL stops
    with pytest.raises(ValueError, match="scale out of bounds"):
        alg.update_weights(eg["ev"], eg["encoder"], eg["enc"], feats, featsT, cy, cw, 0.1, eg["gk"], eg["rk"], G.SCALE)


# ---- the C++ shim
def test_refresh_selftest_driver():
    """drivers/refresh_selftest.cpp through include/seal/seal.h and include/seal/shim_refresh.h: a ciphertext taken down to
    one prime, refreshed, multiplied by a plaintext (refused before the refresh), decoded"""
    exe = os.path.join(ROOT, "drivers", "_ref", "refresh_selftest")
    if not os.path.exists(exe):  # our own source: build it where it is missing
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "drivers"), "_ref/refresh_selftest"], check=False)
    assert os.path.exists(exe), "drivers/_ref/refresh_selftest could not be built (make -C drivers _ref/refresh_selftest)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SELFTEST PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout
