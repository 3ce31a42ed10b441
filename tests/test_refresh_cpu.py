"""Refresh without a GPU: the host lift against the exact model, the oracle twin's refresh and training step, and the
surface of include/hefx_refresh.h.

The twin.  seal.Decryptor.refresh on the oracle-backed backend (tests/oracle_backend.py, which has no `refresh`) composes
decrypt, inverse transform, seal.lift_coefficients, forward transform and encrypt: the words the engine's hefx_refresh must
give (tests/test_gpu_refresh.py).  Here it is held to what a refresh is: decrypt(refresh(ct)) differs from the exact lift
of decrypt(ct) by fresh encryption noise alone, e0 + e1 s - u e_pk, whose centred coefficients are at most
19 + 19 N + 19 N = 19 (2 N + 1) -- the sampler clips the noise at 19.2 (integers up to 19), u and s are ternary.  Derived,
not measured."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import lr_gradient_cases as G
from tests import refresh_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_env = {}


def env(galois_steps=None):
    """the oracle twin on the LR chain at N = 4096, made once per key set; the tests share its keys and only advance its
    encryptor's stream counter"""
    from tests.test_gpu_composites import make
    key = tuple(galois_steps) if galois_steps else None
    if key not in _env:
        _env[key] = make(4096, G.LR_BITS, "oracle", seed=G.KEY_SEED, galois_steps=galois_steps)
    return _env[key]


def _keys(shape):
    return [1, -8] if shape == (8, 8) else None


# ---- the host lift
@pytest.mark.parametrize("L_in,L_out", [(1, 2), (1, 8), (2, 3), (7, 8), (3, 8)])
def test_host_lift_equals_the_exact_model_on_the_crafted_sets(L_in, L_out):
    from seal_fyp_logistic_regression_amd import seal as S
    N = 1024
    primes = S.CoeffModulus.Create(N, G.LR_BITS)
    coef = R.crafted_coefficients(primes, L_in, N, 2, seed=L_in * 16 + L_out)
    vals = R.crafted_values(primes, L_in)
    Q = R.modulus(primes, L_in)
    assert {0, 1, Q - 1, Q // 2, Q // 2 + 1} <= set(vals)
    for c in range(2):
        want = R.lift_coefficients(coef[c], primes, L_in, L_out)
        assert np.array_equal(want[:L_in], coef[c])
        got = S.lift_coefficients(coef[c], primes, L_in, L_out)
        assert got.shape == (L_out - L_in, N) and got.dtype == np.uint64
        assert np.array_equal(got, want[L_in:])
    # the sign rule itself, on the two boundary values: Q // 2 is positive, Q // 2 + 1 is Q // 2 + 1 - Q = -(Q // 2)
    two = np.array([[(Q // 2) % q, (Q // 2 + 1) % q] for q in primes[:L_in]], dtype=np.uint64)
    got = S.lift_coefficients(two, primes, L_in, L_out)
    for j in range(L_in, L_out):
        assert [int(v) for v in got[j - L_in]] == [(Q // 2) % primes[j], (-(Q // 2)) % primes[j]]


# ---- refresh on the twin
def _centred_difference(e, a_rows, b_rows, L):
    """centred coefficients of a - b, both [L][N] NTT form"""
    o = R.oracle_for(e["ctx"].N, e["ctx"].primes)
    q = e["ctx"].primes
    diff = np.stack([o.ntt_inv(j, (a_rows[j].astype(object) - b_rows[j].astype(object)) % q[j]) for j in range(L)])
    x, Q = R.compose(diff, q, L)
    return [int(v) - Q if v > Q // 2 else int(v) for v in x]


@pytest.mark.parametrize("size", [2, 3])
def test_refresh_on_the_twin_is_the_exact_lift_plus_fresh_noise(size):
    e = env()
    assert not hasattr(e["ctx"].backend, "refresh")
    ctx, N = e["ctx"], e["ctx"].N
    top = ctx.first_parms_id()
    v = np.linspace(-1.5, 1.5, 16)
    ct = e["enc"].encrypt(e["encoder"].encode(v, G.SCALE))
    if size == 3:
        ct = e["ev"].multiply(ct, e["enc"].encrypt(e["encoder"].encode(np.ones(16), G.SCALE)))
        e["ev"].rescale_to_next_inplace(ct)
    e["ev"].mod_switch_to_inplace(ct, 1)
    assert ct.size() == size and ct.parms_id() == 1
    before = e["enc"]._stream
    r = e["dec"].refresh(ct, e["enc"])
    assert e["enc"]._stream == before + 1
    assert (r.size(), r.parms_id(), r.scale) == (2, top, ct.scale)
    plain = np.asarray(e["dec"].decrypt(ct).data).reshape(1, 1, N)
    want = R.lift(plain, ctx.primes, 1, top)[0]
    got = np.asarray(e["dec"].decrypt(r).data).reshape(top, N)
    noise = _centred_difference(e, got, want, top)
    bound = 19 * (2 * N + 1)
    print(f"refresh size {size}: largest |noise coefficient| {max(abs(x) for x in noise)}, bound {bound}")
    assert max(abs(x) for x in noise) <= bound
    assert any(noise)  # a fresh encryption, not a copy
    # the values survive: slots of the refreshed ciphertext against the original's
    a = e["encoder"].decode(e["dec"].decrypt(ct))[:16].real
    b = e["encoder"].decode(e["dec"].decrypt(r))[:16].real
    assert np.abs(a - b).max() < 1e-6  # noise 19 (2N + 1) / 2^40 spread over the slots
    # same level: no lift, a plain re-encryption
    same = e["dec"].refresh(ct, e["enc"], parms_id=1)
    assert (same.size(), same.parms_id()) == (2, 1)
    with pytest.raises(ValueError):
        e["dec"].refresh(r, e["enc"], parms_id=1)


def test_refresh_many_on_the_twin_is_refresh_item_by_item():
    e = env()
    cts = [e["enc"].encrypt(e["encoder"].encode(np.arange(4) * (i + 1) / 8.0, G.SCALE)) for i in range(3)]
    for c in cts:
        e["ev"].mod_switch_to_inplace(c, 2)
    first = e["enc"]._stream
    many = e["dec"].refresh_many(cts, e["enc"])
    assert e["enc"]._stream == first + 3
    e["enc"]._stream = first
    one = [e["dec"].refresh(c, e["enc"]) for c in cts]
    for a, b in zip(many, one):
        assert G.compare(e, a, e, b) == []


# ---- the training step
@pytest.mark.parametrize("shape", [(3, 4), (8, 8)])
def test_the_allowance_cannot_hide_a_missed_update(shape):
    """per shape and per iteration: 8 x the twin's recorded error is at most a tenth of the smallest |lr / n * g_j|"""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    X, w, y = G.inputs(*shape)
    lr = R.LEARNING_RATE[shape]
    _, gs = R.plain_training(X, w, y, alg.SIGMOID_COEFFS[3], lr, R.ITERS)
    for it, g in enumerate(gs):
        smallest = float(np.abs(lr / shape[0] * g).min())
        print(f"train {shape} iteration {it + 1}: smallest |lr/n g_j| {smallest:.3e}, allowance {R.train_allowance(shape):.3e}")
        assert R.train_allowance(shape) <= 0.1 * smallest


@pytest.mark.parametrize("shape", [(3, 4), (8, 8)])
def test_two_iterations_of_train_cipher_on_the_twin(shape):
    """level, scale and size of every step's result; decoded weights against the plain recurrence; update_weights still
    stops at :336.  Prints the figure recorded in refresh_cases.TRAIN_TWIN_ERROR."""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    e = env(_keys(shape))
    X, w, y = G.inputs(*shape)
    feats, featsT, cy, cw = G.encrypt_inputs(e, X, w, y)
    with pytest.raises(ValueError, match="scale out of bounds"):
        alg.update_weights(e["ev"], e["encoder"], e["enc"], feats, featsT, cy, cw, 0.1, e["gk"], e["rk"], G.SCALE)
    lr = R.LEARNING_RATE[shape]
    one = alg.update_weights_refreshed(e["ev"], e["encoder"], e["enc"], e["dec"], feats, featsT, cy, cw, lr, e["gk"],
                                       e["rk"], G.SCALE)
    top = e["ctx"].first_parms_id()
    assert (one.size(), one.parms_id(), one.scale) == (2, top, 2.0 ** 40)
    assert cw.parms_id() == top  # the caller's weights are not touched
    final = alg.train_cipher(e["ev"], e["encoder"], e["enc"], e["dec"], feats, featsT, cy, cw, lr, R.ITERS, e["gk"],
                             e["rk"], G.SCALE)
    assert (final.size(), final.parms_id(), final.scale) == (2, top, 2.0 ** 40)
    ws, _ = R.plain_training(X, w, y, alg.SIGMOID_COEFFS[3], lr, R.ITERS)
    err1, err2 = G.decode_error(e, one, ws[0]), G.decode_error(e, final, ws[-1])
    print(f"train_cipher {shape} on the twin: max |decoded - w| after 1 iteration {err1:.3e}, after {R.ITERS} {err2:.3e}")
    assert max(err1, err2) <= R.train_allowance(shape)
    assert np.abs(ws[-1] - w).min() > 100 * R.train_allowance(shape)  # the weights did move


# ---- the surface of include/hefx_refresh.h
def _header():
    return open(os.path.join(ROOT, "include", "hefx_refresh.h")).read()


def _header_symbols():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(hefx_[a-z_0-9]+)\s*\(", src)))


def test_refresh_header_is_plain_c():
    src = '#include "hefx_refresh.h"\nint main(void) { return hefx_mod_raise(0, 1, 2, 1, 0, 0, 0) == HEFX_OK; }\n'
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(src)
        path = f.name
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), path], capture_output=True, text=True)
    os.unlink(path)
    assert r.returncode == 0, r.stderr


def test_refresh_symbols_are_exported_and_bound():
    from seal_fyp_logistic_regression_amd import _build, capi
    _build.build()
    syms = _header_symbols()
    assert syms == ["hefx_mod_raise", "hefx_refresh", "hefx_refresh_batch"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.library_path()], text=True)
    exported = set(re.findall(r" T (hefx_[a-z_0-9]+)", out))
    assert not [s for s in syms if s not in exported]
    assert sorted(capi.REFRESH_SYMBOLS) == syms
    assert not set(capi.REFRESH_SYMBOLS) & set(capi.EXPORTED_SYMBOLS)
    lib = capi.lib()
    for s in syms:
        assert getattr(lib, s).argtypes is not None
    # the constants the binding mirrors
    assert int(re.search(r"#define HEFX_REFRESH_GROUP (\d+)", _header()).group(1)) == capi.REFRESH_GROUP
    assert int(re.search(r"#define HEFX_LIFT_MAX_LIN (\d+)", _header()).group(1)) == capi.LIFT_MAX_LIN
    assert "../../include/hefx_refresh.h" in _build.HEADERS


def test_refresh_header_states_the_aliasing_rule_in_front_of_each_entry():
    src = _header()
    for name in _header_symbols():
        at = src.index("int " + name + "(")
        comment = " ".join(src[src.rindex("/*", 0, at):at].replace("\n *", " ").split())
        assert "overlap" in comment and "HEFX_ERR_INVALID before anything is submitted" in comment, name
