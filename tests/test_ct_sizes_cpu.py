"""Host logic of ciphertexts of any size -- Evaluator.multiply / square / relinearize_inplace beyond size 2 x 2 and 3,
KeyGenerator.relin_keys(count), add / sub of unequal sizes -- on the oracle-backed twins: no GPU.  The twin with the
general routes (tests/ct_sizes_backend.py) is what the engine must equal word for word (tests/test_gpu_ct_sizes.py); the
plain OracleBackend has no such routes and keeps the messages it always gave."""
import os
import re

import numpy as np
import pytest

from seal_fyp_logistic_regression_amd import seal as S
from tests import exact_ckks as X
from tests import policy_sets as ps
from tests.ct_sizes_backend import VALUES, SizesOracleBackend, make, xyz
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = [50, 30, 30, 30, 50]


@pytest.fixture(scope="module")
def env():
    return make(4096, BITS, "oracle", seed=5)


def _host(e, c):
    return np.asarray(e["ctx"].backend.to_host(c.data)).reshape(c.size(), c.parms_id(), e["ctx"].N)


def test_xyz_with_one_relinearisation_at_the_end(rescale_mode):
    """x * y * z as a size-4 ciphertext, one relinearize_inplace with relin_keys(2), two rescales: sizes, levels, scales,
    and both the size-4 ciphertext and the relinearised one decrypt to x * y * z within atol 1e-2 at scale 2^30 (the
    tolerance of tests/test_multiply_sum_cpu.py for decrypted products; inputs in [-1, 1])"""
    e = make(4096, BITS, "oracle", seed=5)
    s = xyz(e)
    scale, L = 2.0 ** 30, e["ctx"].first_parms_id()
    assert s["size4"].size() == 4 and s["size4"].parms_id() == L and s["size4"].scale == scale ** 3
    assert s["relin"].size() == 2 and s["relin"].parms_id() == L and s["relin"].scale == scale ** 3
    q = e["ctx"].primes
    assert s["rescaled"].size() == 2 and s["rescaled"].parms_id() == L - 2
    assert s["rescaled"].scale == scale ** 3 / float(q[L - 1]) / float(q[L - 2])
    want = VALUES[0] * VALUES[1] * VALUES[2]
    assert np.abs(VALUES).max() <= 1.0
    for tag in ("size4", "relin", "rescaled"):
        got = e["encoder"].decode(e["dec"].decrypt(s[tag]))[:len(want)].real
        assert np.allclose(got, want, atol=1e-2), (tag, np.abs(got - want).max())
    # the relinearised words are the loop of SEAL's relinearize_internal: power 3 first, then power 2
    o, c = e["ctx"].backend.o, _host(e, s["size4"])
    head = o.switch_key(np.ascontiguousarray(c[:2]), c[3], e["rk"].power_key(3))
    head = o.switch_key(head, c[2], e["rk"].power_key(2))
    assert (_host(e, s["relin"]) == head).all()
    # and deferring is not the op-by-op sequence: relinearising after every product gives other words, the same value
    ev = e["ev"]
    x, y, z = (e["enc"].encrypt(e["encoder"].encode(v, scale)) for v in VALUES)
    xy = ev.multiply(x, y)
    ev.relinearize_inplace(xy, e["rk"])
    step = ev.multiply(xy, z)
    ev.relinearize_inplace(step, e["rk"])
    assert np.allclose(e["encoder"].decode(e["dec"].decrypt(step))[:len(want)].real, want, atol=1e-2)


def test_products_of_every_size_and_the_square(env):
    e, ev, scale = env, env["ev"], 2.0 ** 20
    x, y = (e["enc"].encrypt(e["encoder"].encode(v, scale)) for v in VALUES[:2])
    o = e["ctx"].backend.o
    x2 = ev.multiply(x, y)
    x3 = ev.multiply(x2, x)
    for a, b in ((x2, x), (x, x2), (x2, x2), (x3, x), (x3, x2)):
        got = ev.multiply(a, b)
        assert got.size() == a.size() + b.size() - 1 and got.scale == a.scale * b.scale and got.parms_id() == a.parms_id()
        assert (_host(e, got) == o.multiply(_host(e, a), _host(e, b))).all()
    sq = ev.square(x2)
    assert sq.size() == 5 and (_host(e, sq) == o.multiply(_host(e, x2), _host(e, x2))).all()
    c = x2.copy()
    ev.square_inplace(c)
    assert c.size() == 5 and (_host(e, c) == _host(e, sq)).all()
    c = x2.copy()
    ev.multiply_inplace(c, x)
    assert c.size() == 4 and (_host(e, c) == _host(e, ev.multiply(x2, x))).all()
    # size 2 x size 2 still takes the dedicated backend calls
    calls = []

    class Spy(SizesOracleBackend):
        def multiply(self, *a):
            calls.append("multiply")
            return super().multiply(*a)

        def square(self, *a):
            calls.append("square")
            return super().square(*a)

        def multiply_sizes(self, *a):
            calls.append("multiply_sizes")
            return super().multiply_sizes(*a)

    spy = S.Evaluator(e["ctx"])
    spy.be = Spy(e["ctx"].N, e["ctx"].primes)
    assert (_host(e, spy.multiply(x, y)) == _host(e, x2)).all()
    spy.square(x)
    spy.multiply(x2, x)
    assert calls == ["multiply", "square", "multiply_sizes"]


def test_seal_messages(env):
    e, ev, scale = env, env["ev"], 2.0 ** 20
    x, y = (e["enc"].encrypt(e["encoder"].encode(v, scale)) for v in VALUES[:2])
    x3 = ev.multiply(x, y)
    x4 = ev.multiply(x3, x)
    with pytest.raises(ValueError, match="not enough relinearization keys"):
        ev.relinearize_inplace(ev.multiply(x4, x), e["rk"])                 # size 5 needs s^4: relin_keys(2) has s^2, s^3
    with pytest.raises(ValueError, match="not enough relinearization keys"):
        ev.relinearize_inplace(x4.copy(), e["kg"].relin_keys())             # size 4 needs s^3
    with pytest.raises(ValueError, match="not enough relinearization keys"):
        ev.relinearize_inplace(x3.copy(), S.RelinKeys())
    assert x4.size() == 4                                                    # a refused call leaves its operand alone
    huge = x3.copy()
    huge.scale = 2.0 ** 120
    with pytest.raises(ValueError, match="scale out of bounds"):
        ev.multiply(huge, x3)
    low = x3.copy()
    ev.mod_switch_to_next_inplace(low)
    with pytest.raises(ValueError, match="encrypted1 and encrypted2 parameter mismatch"):
        ev.multiply(x3, low)
    # a result beyond the engine's limit of 16 polynomials
    chain = [x]
    for _ in range(7):
        nxt = ev.multiply(chain[-1], y)
        nxt.scale = scale                                                    # (keep the scale check out of the way)
        chain.append(nxt)
    eight, nine = chain[6], chain[7]
    assert (eight.size(), nine.size()) == (8, 9)
    with pytest.raises(ValueError, match="invalid size"):
        ev.multiply(nine, nine)                                              # 17 polynomials
    assert ev.multiply(nine, eight).size() == S.CT_SIZE_MAX                  # 16 is fine
    for bad in (0, -1, 15):
        with pytest.raises(ValueError, match="invalid count"):
            e["kg"].relin_keys(bad)


def test_the_plain_twin_keeps_its_messages():
    """a backend without the general routes: the ValueErrors the evaluator always raised, text for text"""
    e = make(4096, BITS, "plain_oracle", seed=5, relin_count=1)
    assert type(e["ctx"].backend) is OracleBackend and not hasattr(e["ctx"].backend, "multiply_sizes")
    ev, scale = e["ev"], 2.0 ** 20
    x, y = (e["enc"].encrypt(e["encoder"].encode(v, scale)) for v in VALUES[:2])
    x3 = ev.multiply(x, y)
    for a, b in ((x3, x), (x, x3), (x3, x3)):
        with pytest.raises(ValueError) as err:
            ev.multiply(a, b)
        assert str(err.value) == "multiply: only size-2 operands are supported (all reference call sites)"
    with pytest.raises(ValueError) as err:
        ev.square(x3)
    assert str(err.value) == "multiply: only size-2 operands are supported (all reference call sites)"
    four = S.Ciphertext()._set(np.concatenate([_host(e, x3), _host(e, x)[:1]]), 4, x.parms_id(), x3.scale)
    with pytest.raises(ValueError) as err:
        ev.relinearize_inplace(four, e["rk"])
    assert str(err.value) == "relinearize: encrypted size must be 2 or 3"
    # and what it always could: 3 -> 2, a no-op at size 2, sums of unequal sizes
    ev.relinearize_inplace(x3, e["rk"])
    assert x3.size() == 2 and ev.relinearize_inplace(x, e["rk"]) is x


def test_relin_keys_count(env):
    """relin_keys(1) is relin_keys() word for word; relin_keys(3) holds s^2, s^3, s^4 under index power - 2, each the
    key-switching key of its power: c0 + c1 s - P s^p on digit i's own row is one small polynomial in every row"""
    e = env
    one, none = make(4096, BITS, "oracle", seed=5, relin_count=1), S.KeyGenerator(e["ctx"], 5)
    assert sorted(one["rk"].keys) == [0]
    none.public_key()                                   # (the stream id make() spends before its relin_keys)
    assert (np.asarray(one["rk"].key(0)) == np.asarray(none.relin_keys().key(0))).all()
    assert (np.asarray(one["rk"].key(0)) == np.asarray(e["rk"].key(0))).all()       # the first key of relin_keys(2) too
    s = ps.sets()["mixed2048"]
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(s.N)
    parms.set_coeff_modulus(s.primes)
    ctx = S.SEALContext.Create(parms, backend=SizesOracleBackend(s.N, s.primes))
    kg = S.KeyGenerator(ctx, 11)
    rk = kg.relin_keys(3)
    assert sorted(rk.keys) == [0, 1, 2] and [rk.get_index(p) for p in (2, 3, 4)] == [0, 1, 2]
    assert all(rk.has_power(p) for p in (2, 3, 4)) and not rk.has_power(5) and not rk.has_power(1)
    o, sk = ctx.backend.o, kg.secret_key().host
    sko = [X._obj(sk[m]) for m in range(s.k)]
    power = sko
    for p in (2, 3, 4):
        power = [(power[m] * sko[m]) % q for m, q in enumerate(s.primes)]
        sp = np.asarray([[int(t) for t in power[m]] for m in range(s.k)], dtype=np.uint64)
        errs = X.kswitch_key_errors(o, s.primes, sk, sp, np.asarray(rk.power_key(p)))
        assert any(int(abs(err).max()) > 0 for err in errs), p
        with pytest.raises(AssertionError):                                          # ... of THAT power
            X.kswitch_key_errors(o, s.primes, sk, sk, np.asarray(rk.power_key(p)))


def test_add_and_sub_of_unequal_sizes(env):
    """the words of the operation on the shorter operand padded with zero polynomials, through whichever route the backend
    has: the twins pad through the host; a backend with addsub_unequal is asked once and its payload handed back"""
    e, ev, scale = env, env["ev"], 2.0 ** 20
    o = e["ctx"].backend.o
    x, y = (e["enc"].encrypt(e["encoder"].encode(v, scale)) for v in VALUES[:2])
    p = ev.multiply(ev.multiply(x, y), x)                                            # size 4
    t = ev.multiply(x, y)                                                            # size 3
    t.scale = p.scale
    hp, ht = _host(e, p), _host(e, t)
    pad = np.concatenate([ht, np.zeros_like(hp[:1])])
    for a, b, f, want in ((p, t, ev.add, o.add(hp, pad)), (t, p, ev.add, o.add(pad, hp)),
                          (p, t, ev.sub, o.sub(hp, pad)), (t, p, ev.sub, o.sub(pad, hp))):
        got = f(a, b)
        assert got.size() == 4 and got.scale == p.scale and (_host(e, got) == want).all()
    # a backend that offers the device route is used, with the operands as they are
    seen = []

    class Native(SizesOracleBackend):
        def addsub_unequal(self, L, size_a, a, size_b, b, sub):
            seen.append((L, size_a, size_b, sub, a is p.data or a is t.data))
            big, small = (a, b) if size_a > size_b else (b, a)
            z = np.concatenate([self._ct(small, min(size_a, size_b), L), np.zeros_like(self._ct(big, 4, L)[:1])])
            lhs, rhs = (self._ct(big, 4, L), z) if size_a > size_b else (z, self._ct(big, 4, L))
            return (self.o.sub if sub else self.o.add)(lhs, rhs)

    nat = S.Evaluator(e["ctx"])
    nat.be = Native(e["ctx"].N, e["ctx"].primes)
    assert (_host(e, nat.sub(t, p)) == o.sub(pad, hp)).all() and (_host(e, nat.add(p, t)) == o.add(hp, pad)).all()
    assert seen == [(p.parms_id(), 3, 4, True, True), (p.parms_id(), 4, 3, False, True)]
    nat.add(p, p)
    assert len(seen) == 2                                                            # equal sizes never go there


def test_abi_has_the_new_entries():
    from seal_fyp_logistic_regression_amd import capi
    new = ["hefx_multiply_sizes", "hefx_multiply_sizes_batch", "hefx_relinearize_sizes", "hefx_relinearize_sizes_batch"]
    assert all(n in capi.EXPORTED_SYMBOLS for n in new)
    header = open(os.path.join(ROOT, "include", "hefx.h")).read()
    for n in new:
        assert re.search(r"\bint " + n + r"\(hefx_context \*ctx, int L,", header), n
    assert re.search(r"#define HEFX_CT_SIZE_MAX 16\b", header) and S.CT_SIZE_MAX == 16
    # none of them joins the entries that wait on the host
    block = header[header.index("The entries that DO wait on the host"):header.index("Besides these")]
    assert not any(n in block for n in new)
    from seal_fyp_logistic_regression_amd.engine import Engine
    from seal_fyp_logistic_regression_amd.seal import GpuBackend
    for m in ("multiply_sizes", "multiply_sizes_batch", "relinearize_sizes"):
        assert callable(getattr(Engine, m)) and callable(getattr(GpuBackend, m))
