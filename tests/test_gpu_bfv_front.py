"""The BFV entries beyond multiply and decrypt_round on the GPU (include/hefx_bfv.h: scale_plain_add, lift_plain,
noise_budget, batching, batch_encode, batch_decode) against the exact models of tests/bfv_front_cases.py, word for word:
every prime set x plain modulus, the values on both sides of the lift's threshold, the wrap of c0, odd coefficient counts,
the in-place form, one noise spike at the lane, wave and workgroup edges of the reduction for every bit length, a
caller-owned stream, refusals that write nothing, one pipeline through BfvPlan + Engine, and the C++ shim's self-test.

Every entry is exact, so there is no tolerance anywhere in this file: np.array_equal or nothing."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import bfv_cases as B
from tests import bfv_front_cases as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.uint64(0x5EA15EA15EA15EA1)
N = F.N
SETS = sorted(B.prime_sets())
KEY32 = bytes(range(32))

_engines = {}
_plans = {}


def engine(name):
    from seal_fyp_logistic_regression_amd import Engine
    if name not in _engines:
        n, primes, _ = B.prime_sets()[name]
        _engines[name] = Engine(n, primes)
    return _engines[name]


def plan(name, t, L=None):
    from seal_fyp_logistic_regression_amd import BfvPlan
    L = L or B.prime_sets()[name][2]
    if (name, t, L) not in _plans:
        _plans[(name, t, L)] = BfvPlan(engine(name), L, t)
    return _plans[(name, t, L)]


def _streams():
    """one caller-owned stream, as a context manager (imported late: it loads the library)"""
    from tests.hip_stream_gate import Stream
    return Stream()


@pytest.mark.parametrize("t", B.PLAIN_MODULI)
@pytest.mark.parametrize("name", SETS)
def test_scale_plain_add_equals_the_model(name, t):
    _, primes, L = B.prime_sets()[name]
    p, e = plan(name, t), engine(name)
    m = F.message_values(t, N, seed=1)
    c0s = {"null": None, "uniform": B.uniform(primes, L, 1, N, 2)[0],
           "wrap": np.array([[int(primes[j]) - 1] * N for j in range(L)], dtype=np.uint64)}
    with _streams() as S:
        for ncoeff in (1, N - 1, N):
            dm = e.to_device(m[:ncoeff])
            for kind, c0 in c0s.items():
                want = F.scale_plain_add_model(m, ncoeff, c0, primes, L, t)
                if c0 is not None:
                    assert np.array_equal(want[:, ncoeff:], c0[:, ncoeff:])  # the tail is c0_in
                for stream in (None, S.handle) if ncoeff == N - 1 else (None,):
                    dc = e.to_device(c0) if c0 is not None else None
                    got = p.scale_plain_add(dm, dc, stream=stream)
                    e.sync(stream)
                    bad = np.argwhere(got.download() != want)
                    assert bad.size == 0, f"{kind}, ncoeff = {ncoeff}: {len(bad)} wrong words, first at [row, coefficient] = {bad[0].tolist()}"
                    assert np.array_equal(dm.download(), m[:ncoeff])
                    if dc is not None:
                        assert np.array_equal(dc.download(), c0)
                        p.scale_plain_add(dm, dc, out=dc, stream=stream)  # d_out == d_c0_in
                        e.sync(stream)
                        assert np.array_equal(dc.download(), want), f"in place, {kind}, ncoeff = {ncoeff}"
        # a message word above t is still reduced modulo q_j as a whole
        big = np.array([(1 << 64) - 1, t, t + 1], dtype=np.uint64)
        got = p.scale_plain_add(e.to_device(big), None)
        e.sync()
        assert np.array_equal(got.download(), F.scale_plain_add_model(big, 3, None, primes, L, t))


@pytest.mark.parametrize("t", B.PLAIN_MODULI)
@pytest.mark.parametrize("name", SETS)
def test_lift_plain_equals_the_model(name, t):
    _, primes, L = B.prime_sets()[name]
    p, e = plan(name, t), engine(name)
    m = F.message_values(t, N, seed=3)
    with _streams() as S:
        for ncoeff in (1, N - 1, N):
            dm = e.to_device(m[:ncoeff])
            want = F.lift_plain_model(m, ncoeff, primes, L, t)
            dw = e.to_device(want)
            e.ntt_forward(dw, 1, L)
            e.sync()
            want_ntt = dw.download()
            for stream in (None, S.handle) if ncoeff == N - 1 else (None,):
                for ntt_form, ref in ((False, want), (True, want_ntt)):
                    got = p.lift_plain(dm, ntt_form=ntt_form, stream=stream)
                    e.sync(stream)
                    bad = np.argwhere(got.download() != ref)
                    assert bad.size == 0, f"ntt_form = {ntt_form}, ncoeff = {ncoeff}: {len(bad)} wrong words, first at {bad[0].tolist()}"
                    assert np.array_equal(dm.download(), m[:ncoeff])


POSITIONS = (0, 63, 64, 255, 256, N - 1)


def _budget(p, e, dx, stream=None, out=None):
    """out: a zeroed word to reuse (the entry writes its low 32 bits)"""
    out = p.noise_budget(dx, out=out, stream=stream)
    e.sync(stream)
    return int(out.download()[0])


@pytest.mark.parametrize("t", B.PLAIN_MODULI)
@pytest.mark.parametrize("name", SETS)
def test_noise_budget_equals_the_model(name, t):
    """one spike per polynomial: every magnitude 1, 2^k - 1, 2^k (k < bits(Q) - 1) and (Q-1)/2 with both signs, the
    positions taken in turn so that every position meets both signs (the closed form is the model's value for a spike:
    tests/test_bfv_front_cpu.py); then zero, uniform, and two spikes in different workgroups"""
    _, primes, L = B.prime_sets()[name]
    p, e = plan(name, t), engine(name)
    Q = B.modulus(primes, L)
    ti = pow(t, -1, Q)
    x = np.zeros((L, N), dtype=np.uint64)
    dx, word = e.to_device(x), e.to_device(np.zeros(1, dtype=np.uint64))
    assert _budget(p, e, dx) == Q.bit_length() - 1  # the all-zero polynomial
    vals = F.noise_values(primes, L)
    seen = set()
    for i, v in enumerate(vals):
        pos = POSITIONS[(i // 2 + i % 2) % len(POSITIONS)]
        seen.add((pos, v > 0))
        x[:, pos] = B.residues([(v * ti) % Q], primes, L)[:, 0]
        dx.upload(x)
        got = _budget(p, e, dx, out=word)
        assert got == F.budget_of(v, primes, L), f"v = {v} at n = {pos}: budget {got}"
        assert np.array_equal(dx.download(), x)
        x[:, pos] = 0
    assert len(seen) == 2 * len(POSITIONS)
    with _streams() as S:
        # every position once more with the largest and the smallest magnitude, on a caller-owned stream
        for pos in POSITIONS:
            for v in (-1, (Q - 1) // 2):
                x[:, pos] = B.residues([(v * ti) % Q], primes, L)[:, 0]
                dx.upload(x)
                assert _budget(p, e, dx, stream=S.handle, out=word) == F.budget_of(v, primes, L), (pos, v)
                x[:, pos] = 0
        u = B.uniform(primes, L, 1, N, 5)[0]
        du = e.to_device(u)
        want = F.noise_budget_model(u, primes, L, t)
        assert want <= 1
        for stream in (None, S.handle):
            assert _budget(p, e, du, stream=stream) == want
        assert np.array_equal(du.download(), u)
    # two spikes in different workgroups, the larger one second
    small, large = 1 << (Q.bit_length() // 3), -(1 << (Q.bit_length() // 2))
    poly = [0] * N
    poly[100], poly[700] = small, large
    x2 = F.x_for_noise(poly, primes, L, t)
    assert F.noise_budget_model(x2, primes, L, t) == F.budget_of(large, primes, L) != F.budget_of(small, primes, L)
    assert _budget(p, e, e.to_device(x2)) == F.budget_of(large, primes, L)


@functools.lru_cache(maxsize=None)
def _slot_case(t, nvalues):
    rng = np.random.default_rng(nvalues)
    v = [int(x) for x in rng.integers(0, t, nvalues, dtype=np.uint64)]
    v[0] = t - 1
    if nvalues > 1:
        v[1], v[-1] = 0, t - 1
    return v, F.batch_encode_model(v, t)


@pytest.mark.parametrize("t", F.batching_moduli())
def test_batching_equals_the_model(t):
    name = SETS[t % len(SETS)]
    p, e = plan(name, t), engine(name)
    assert p.batching()
    with _streams() as S:
        for nvalues in (1, N // 2, N // 2 + 1, N):
            v, want = _slot_case(t, nvalues)
            hv = np.array(v, dtype=np.uint64)
            dv = e.to_device(hv)
            for stream in (None, S.handle) if nvalues == N // 2 + 1 else (None,):
                dm = p.batch_encode(dv, stream=stream)
                e.sync(stream)
                bad = np.argwhere(dm.download() != want)
                assert bad.size == 0, f"encode of {nvalues} values: {len(bad)} wrong words, first at {bad[0].tolist()}"
                assert np.array_equal(dv.download(), hv)
                back = p.batch_decode(dm, stream=stream)
                e.sync(stream)
                assert np.array_equal(back.download(), np.array(v + [0] * (N - nvalues), dtype=np.uint64))
                assert np.array_equal(dm.download(), want)
        # decode of a polynomial that no encode made: against evaluation at psi^(e_i)
        m = np.random.default_rng(9).integers(0, t, N, dtype=np.uint64)
        m[0], m[1] = t - 1, 0
        want = F.batch_decode_model(m, t)
        for stream in (None, S.handle):
            got = p.batch_decode(e.to_device(m), stream=stream)
            e.sync(stream)
            assert np.array_equal(got.download(), want)


@pytest.mark.parametrize("t", (2, 1024))
def test_no_batching_is_unsupported_and_writes_nothing(t):
    from seal_fyp_logistic_regression_amd import capi
    name = "bfv4096_bits"
    p, e = plan(name, t), engine(name)
    lib = capi.lib()
    assert not p.batching() and lib.hefx_bfv_batching(p._h) == 0 and lib.hefx_bfv_batching(None) == 0
    host = np.full(2 * N, SENTINEL, dtype=np.uint64)
    slab = e.to_device(host)
    for rc in (lib.hefx_bfv_batch_encode(p._h, slab.ptr, N, slab.ptr + N * 8, None),
               lib.hefx_bfv_batch_decode(p._h, slab.ptr, slab.ptr + N * 8, None)):
        assert rc == capi.HEFX_ERR_UNSUPPORTED, lib.hefx_last_error()
    e.sync()
    assert np.array_equal(slab.download(), host)


def test_refusals_write_nothing():
    """by return code, with nothing submitted: the slab that holds every operand is unchanged after a sync"""
    from seal_fyp_logistic_regression_amd import capi
    name, t = "bfv4096_bits", 65537
    _, primes, L = B.prime_sets()[name]
    e, p = engine(name), plan(name, t)
    lib = capi.lib()
    poly = L * N
    host = np.full(8 * poly, SENTINEL, dtype=np.uint64)
    host[4 * poly:5 * poly] = B.uniform(primes, L, 1, N, 31).reshape(-1)
    host[5 * poly:5 * poly + N] = F.message_values(t, N, seed=2)
    slab = e.to_device(host)
    W = 8
    out, c0, m = slab.ptr, slab.ptr + 4 * poly * W, slab.ptr + 5 * poly * W

    def refused(rc, what, code=capi.HEFX_ERR_INVALID):
        assert rc == code, (what, rc, lib.hefx_last_error())
        e.sync()
        assert slab.download().tobytes() == host.tobytes(), what

    sc = lambda h, m_, n_, c_, o_: lib.hefx_bfv_scale_plain_add(h, m_, n_, c_, o_, None)
    refused(sc(None, m, N, c0, out), "scale_plain_add: null object")
    refused(sc(p._h, m, 0, c0, out), "scale_plain_add: ncoeff = 0")
    refused(sc(p._h, m, N + 1, c0, out), "scale_plain_add: ncoeff = N + 1")
    refused(sc(p._h, m, -1, c0, out), "scale_plain_add: ncoeff = -1")
    refused(sc(p._h, None, N, c0, out), "scale_plain_add: null d_m")
    refused(sc(p._h, m, N, c0, None), "scale_plain_add: null d_out")
    refused(sc(p._h, m, N, c0, c0 + W), "scale_plain_add: d_out one word into d_c0_in")
    refused(sc(p._h, m, N, c0, c0 - W), "scale_plain_add: d_out's last word is d_c0_in's first")
    refused(sc(p._h, m, N, None, m), "scale_plain_add: d_out == d_m")
    refused(sc(p._h, m, N, None, m - poly * W + W), "scale_plain_add: d_out's last word is d_m's first")
    refused(sc(p._h, m, N, None, m + (N - 1) * W), "scale_plain_add: d_out starts at d_m's last word")
    li = lambda h, m_, n_, o_, f=0: lib.hefx_bfv_lift_plain(h, m_, n_, f, o_, None)
    refused(li(None, m, N, out), "lift_plain: null object")
    refused(li(p._h, m, 0, out), "lift_plain: ncoeff = 0")
    refused(li(p._h, m, N + 1, out), "lift_plain: ncoeff = N + 1")
    refused(li(p._h, None, N, out), "lift_plain: null d_m")
    refused(li(p._h, m, N, m, 1), "lift_plain: d_out == d_m")
    refused(li(p._h, m, N, m - poly * W + W), "lift_plain: d_out's last word is d_m's first")
    refused(li(p._h, m, 1, m), "lift_plain: one coefficient, in place")
    nb = lambda h, x_, b_: lib.hefx_bfv_noise_budget(h, x_, b_, None)
    refused(nb(None, c0, out), "noise_budget: null object")
    refused(nb(p._h, None, out), "noise_budget: null d_x")
    refused(nb(p._h, c0, None), "noise_budget: null d_budget")
    refused(nb(p._h, c0, c0), "noise_budget: d_budget is d_x's first word")
    refused(nb(p._h, c0, c0 + poly * W - 4), "noise_budget: d_budget is the last four bytes of d_x")
    en = lambda h, v_, n_, m_: lib.hefx_bfv_batch_encode(h, v_, n_, m_, None)
    refused(en(None, m, N, out), "batch_encode: null object")
    refused(en(p._h, m, 0, out), "batch_encode: nvalues = 0")
    refused(en(p._h, m, N + 1, out), "batch_encode: nvalues = N + 1")
    refused(en(p._h, m, N, m), "batch_encode: in place")
    refused(en(p._h, m, 1, m - (N - 1) * W), "batch_encode: d_m's last word is the one value")
    refused(en(p._h, None, N, out), "batch_encode: null d_values")
    de = lambda h, m_, v_: lib.hefx_bfv_batch_decode(h, m_, v_, None)
    refused(de(None, m, out), "batch_decode: null object")
    refused(de(p._h, m, m), "batch_decode: in place")
    refused(de(p._h, m, m + (N - 1) * W), "batch_decode: d_values starts at d_m's last word")
    refused(de(p._h, m, None), "batch_decode: null d_values")
    # the accepted neighbours do run: the budget's four bytes right in front of d_x, then d_out right in front of d_m
    assert nb(p._h, c0, c0 - 4) == capi.HEFX_OK
    assert sc(p._h, m, N, None, m - poly * W) == capi.HEFX_OK
    e.sync()
    got = slab.download()
    msg, x = host[5 * poly:5 * poly + N], host[4 * poly:5 * poly].reshape(L, N)
    assert np.array_equal(got[4 * poly:5 * poly].reshape(L, N), F.scale_plain_add_model(msg, N, None, primes, L, t))
    # four bytes written, no more: the upper half of the word in front of d_x, its lower half still the sentinel
    assert int(got[4 * poly - 1]) == (F.noise_budget_model(x, primes, L, t) << 32) | (int(SENTINEL) & 0xFFFFFFFF)
    assert np.array_equal(got[:4 * poly - 1], host[:4 * poly - 1]) and np.array_equal(got[5 * poly:], host[5 * poly:])


def test_one_pipeline_through_the_plan_and_the_engine():
    """encode, Delta x onto an encryption of zero brought to coefficient form, + Delta y (add_plain), times the lifted z
    (multiply_plain), decrypt, round, decode: (x + y) z in every slot, and every intermediate the models can state"""
    name, t = "bfv4096_bits", 65537
    _, primes, L = B.prime_sets()[name]
    k = len(primes)
    e, p = engine(name), plan(name, t)
    rng = np.random.default_rng(77)
    x, y, z = ([int(v) for v in rng.integers(0, t, N, dtype=np.uint64)] for _ in range(3))
    mx, my, mz = (p.batch_encode(e.to_device(np.array(v, dtype=np.uint64))) for v in (x, y, z))
    e.sync()
    assert np.array_equal(mx.download(), F.batch_encode_model(x, t))
    # a key pair without key noise: s ternary, pk = (-a s, a), NTT form over all k primes
    s = e.sample("ternary", KEY32, 1, 1, k)
    e.ntt_forward(s, 1, k)
    a = e.sample("uniform", KEY32, 2, 1, k)
    e.sync()
    hs, ha = s.download()[0], a.download()[0]
    pk0 = np.array([[(-int(ha[j][i]) * int(hs[j][i])) % int(primes[j]) for i in range(N)] for j in range(k)], dtype=np.uint64)
    pk, sk = e.to_device(np.stack([pk0, ha])), e.to_device(hs)
    ct = e.encrypt(L, pk, None, KEY32, 3)
    e.ntt_inverse(ct, 2, L)
    e.sync()
    zero = ct.download()
    c0 = ct.view(0, (L, N))
    p.scale_plain_add(mx, c0, out=c0)
    p.scale_plain_add(my, c0, out=c0)
    e.sync()
    after = ct.download()
    want = F.scale_plain_add_model(my.download(), N, F.scale_plain_add_model(mx.download(), N, zero[0], primes, L, t), primes, L, t)
    assert np.array_equal(after[0], want) and np.array_equal(after[1], zero[1])
    pt = p.lift_plain(mz, ntt_form=True)
    e.ntt_forward(ct, 2, L)
    prod = e.multiply_plain(L, 2, ct, pt)
    dec = e.decrypt(L, 2, prod, sk)
    e.ntt_inverse(dec, 1, L)
    m = p.decrypt_round(dec)
    budget = p.noise_budget(dec)
    vals = p.batch_decode(m)
    e.sync()
    hx = dec.download()
    assert np.array_equal(m.download(), B.decrypt_round_model(hx, primes, L, t))
    assert int(budget.download()[0]) == F.noise_budget_model(hx, primes, L, t) > 0
    assert [int(v) for v in vals.download()] == [(x[i] + y[i]) * z[i] % t for i in range(N)]


# ---- the C++ shim
def _driver(name, args=(), timeout=300):
    exe = os.path.join(ROOT, "drivers", "_ref", name)
    if not os.path.exists(exe):  # our own source: build it where it is missing
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "drivers"), "_ref/" + name], check=False)
    assert os.path.exists(exe), f"drivers/_ref/{name} could not be built (make -C drivers _ref/{name})"
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def test_bfv_front_selftest_driver():
    """drivers/bfv_front_selftest.cpp through include/seal/seal.h: the device words against bfv_scaled_plain,
    bfv_lifted_plain, decrypt_round_host's worst and PlainNtt; encode -> encrypt -> add_plain -> multiply_plain -> decrypt
    -> decode in the slots; one level below the top"""
    r = _driver("bfv_front_selftest")
    assert r.returncode == 0 and "SELFTEST PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout
    assert "host fall-back" not in r.stdout  # both parameter sets, and the level below each, are served by the device path
