"""The oracle against the big-int model at every arithmetic-policy boundary of the engine (tests/policy_sets.py), and
the coverage of those boundaries by the named sets.

tests/test_gpu_policy_edges.py compares the engine with the oracle on these sets; here the oracle itself is pinned
against tests/pymodel.py (independent big-int restatement) on the same sets re-derived at toy ring size -- same bounds,
same prime counts -- for every level of the sets, every operand pattern and both key patterns."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import policy_sets as ps
from tests import pymodel as pm

TOY = ps.toy_sets(16)


def _ctx(s):
    o = O.Oracle(s.N, s.primes)
    return o, [o.psi(j) for j in range(s.k)]


def _levels(s):
    return ps.LSWEEP if s.name == "lsweep" else s.levels


@pytest.mark.parametrize("name", sorted(TOY))
def test_switch_key_matches_the_model_at_every_level_operand_and_key(name):
    s = TOY[name]
    o, psis = _ctx(s)
    keys = {kk: ps.key(o, kk, seed=31) for kk in ps.KEYS}
    for L in _levels(s):
        for kind in ps.OPERANDS:
            ct = ps.operand(o, kind, L, seed=100 + L)
            for kk, key in keys.items():
                got = o.switch_key(ct, ct[1], key)
                want = pm.switch_key(ct.tolist(), ct[1].tolist(), key.tolist(), s.primes, psis, L)
                assert got.tolist() == want, (L, kind, kk)


@pytest.mark.parametrize("name", sorted(TOY))
def test_apply_galois_matches_the_model(name):
    """the regular rotation and the exactly hoisted statement the engine's hoisted path follows (same words, whichever
    path it reports) against the model's coefficient-domain automorphism + key switch"""
    s = TOY[name]
    o, psis = _ctx(s)
    n = s.N
    elts = (3, 2 * n - 1, O.galois_elt_from_step(n, -5))
    for L in _levels(s)[:2]:
        for kind in ("uniform", "ntt_max", "coef_max", "coef_max_z"):
            ct = ps.operand(o, kind, L, seed=200 + L)
            for kk in ps.KEYS:
                key = ps.key(o, kk, seed=32)
                for elt in elts:
                    want = pm.apply_galois(ct.tolist(), elt, key.tolist(), s.primes, psis, L)
                    assert o.apply_galois(ct, elt, key).tolist() == want, (L, kind, kk, elt)
                    hoisted, _ = o.apply_galois_hoisted_exact(ct, elt, key)
                    assert hoisted.tolist() == want, (L, kind, kk, elt, "hoisted")


@pytest.mark.parametrize("name", sorted(TOY))
def test_rescale_floor_and_round_match_the_model(name):
    s = TOY[name]
    o, psis = _ctx(s)
    for L in sorted({max(2, L) for L in _levels(s)} | {s.k - 1}):
        for kind in ps.OPERANDS:
            for size in (2, 3):
                ct = ps.operand(o, kind, L, npoly=size, seed=300 + L)
                assert o.rescale(ct, rounded=False).tolist() == pm.rescale_floor(ct.tolist(), s.primes, psis, L), (L, kind)
                assert o.rescale(ct, rounded=True).tolist() == pm.rescale_round(ct.tolist(), s.primes, psis, L), (L, kind)


def test_rescale_round_is_the_nearest_integer_quotient():
    """the model's rounded division, checked against its meaning: CRT-compose the rows, divide by q_l rounding half up,
    reduce again -- at the toy `mixed` set, where the dropped prime lies above, below and between the other rows"""
    s = TOY["mixed2048"]
    o, psis = _ctx(s)
    for L in (9, 5, 2):
        ct = ps.operand(o, "uniform", L, npoly=1, seed=7)
        coef = [pm.intt_def(ct[0][j], psis[j], s.primes[j]) for j in range(L)]
        Q = 1
        for q in s.primes[:L]:
            Q *= q
        ql = s.primes[L - 1]
        want = []
        for j in range(L - 1):
            q = s.primes[j]
            row = []
            for a in range(s.N):
                x = 0
                for i in range(L):  # CRT: the coefficient as an integer in [0, Q)
                    Qi = Q // s.primes[i]
                    x += coef[i][a] * Qi * pow(Qi % s.primes[i], -1, s.primes[i])
                x %= Q
                row.append(((x + ql // 2) // ql) % q)
            want.append(pm.ntt_def(row, psis[j], q))
        assert pm.rescale_round(ct.tolist(), s.primes, psis, L)[0] == want
        assert o.rescale(ct, rounded=True)[0].tolist() == want


@pytest.mark.parametrize("name", sorted(TOY))
def test_ntt_forward_and_inverse_match_the_definition(name):
    s = TOY[name]
    o, psis = _ctx(s)
    rng = np.random.default_rng(5)
    for j, q in enumerate(s.primes):
        for a in (rng.integers(0, q, s.N, dtype=np.uint64), np.full(s.N, q - 1, dtype=np.uint64),
                  np.zeros(s.N, dtype=np.uint64)):
            assert o.ntt_fwd(j, a).tolist() == pm.ntt_def(a, psis[j], q), j
            assert o.ntt_inv(j, a).tolist() == pm.intt_def(a, psis[j], q), j


# ---------------------------------------------------------------------------------------------------------------------
# coverage: a later edit of the sets must not drop a class
# ---------------------------------------------------------------------------------------------------------------------
def _reached(sets_):
    fwd, mac, flags, sides = set(), set(), {"digit": set(), "lt2q": set(), "rescale": set()}, set()
    for s in sets_.values():
        for q in s.primes:
            fwd.add(ps.fwd_policy(q))
            for b, name in ((ps.C40_LO, "c40"), (1 << 41, "2^41"), (1 << 60, "2^60")):
                sides.add((name, q > b))
        for L in _levels(s):
            for m in list(range(L)) + [s.k - 1]:
                pol, slack = ps.mac_policy(s.primes[m], L)
                mac.add(f"{pol}{slack}" if pol == "MacL" else (f"MacW{'>' if s.primes[m] >> 60 else '<'}2^60" if pol == "MacW" else pol))
            for f, v in ps.inmode_flags(s.primes, L).items():
                flags[f] |= v
    return fwd, mac, flags, sides


@pytest.mark.parametrize("which", ["gpu", "toy"])
def test_named_sets_reach_every_policy_class(which):
    fwd, mac, flags, sides = _reached(ps.sets() if which == "gpu" else TOY)
    assert fwd == {"F64-c40", "F64-generic", "U64L", "U64"}
    assert mac == {"MacF", "MacL2", "MacL1", "MacL0", "MacW<2^60", "MacW>2^60"}
    assert all(v == {False, True} for v in flags.values()), flags
    assert sides == {(b, v) for b in ("c40", "2^41", "2^60") for v in (False, True)}


def test_toy_sets_keep_every_prime_in_its_class():
    """the toy re-derivation has the GPU sets' shape: same prime count and levels, and prime for prime the same forward
    and MAC policy at every level, so pinning the oracle on them pins it on the classes the GPU module runs (the input
    flags compare primes a few steps of 2N apart, which need not keep their order at toy size: the toy sets' own
    coverage of both values is asserted above)"""
    for name, s in ps.sets().items():
        t = TOY[name]
        assert (t.k, t.levels) == (s.k, s.levels), name
        for L in _levels(s):
            assert [ps.policy_of(q, L) for q in t.primes] == [ps.policy_of(q, L) for q in s.primes], (name, L)


def test_named_sets_hit_the_bounds_they_are_named_for():
    S = ps.sets()
    assert [ps.fwd_policy(q) for q in S["f41"].primes[1:4]] == ["F64-generic"] * 3
    assert all(q.bit_length() == 41 for q in S["f41"].primes[1:4])
    assert S["f41_wide"].k == 62 and all(q >> 41 == 0 for q in S["f41_wide"].primes[:61])
    assert 61 * 0.52 * S["f41_wide"].primes[60] > 2 ** 45   # past the bound the MacF comment once stated
    c40 = S["c40_edge"].primes[1:5]
    assert [ps.fwd_policy(q) for q in c40] == ["F64-generic"] * 2 + ["F64-c40"] * 2
    assert all(q >> 39 == 1 for q in c40)
    i42 = S["i42"]
    assert all(ps.fwd_policy(q) == "U64L" and q.bit_length() == 42 for q in i42.primes[1:4])
    assert ps.inmode_flags(i42.primes, 4)["lt2q"] == {False, True}     # off on the 42-bit rows, on on the 60-bit one
    st = S["straddle60"].primes
    assert [q >> 60 for q in st] == [0, 0, 1, 1, 1]
    assert [ps.mac_policy(q, 4)[0] for q in st] == ["MacL", "MacL", "MacW", "MacW", "MacW"]
    assert all(q < 1 << 18 for q in S["small_p"].primes[:3]) and S["small_p"].primes[3] >> 60 == 1
    for name, bits in (("p_min", 50), ("p_min40", 40)):
        p = S[name].primes
        assert p[2].bit_length() == bits and p[2] < min(p[:2])
        assert ps.inmode_flags(p, 2)["digit"] == {False, True}
    assert [ps.mac_policy(S["lsweep"].primes[0], L) for L in ps.LSWEEP] == [
        ("MacL", 2), ("MacL", 2), ("MacL", 2), ("MacL", 1), ("MacL", 1), ("MacL", 0), ("MacL", 0), ("MacW", 0),
        ("MacW", 0), ("MacW", 0)]
    for N in (2048, 16384):
        m = S[f"mixed{N}"].primes
        assert {ps.fwd_policy(q) for q in m} == {"F64-c40", "F64-generic", "U64L", "U64"}
        # a 40-bit prime where the one-FMA form would be inexact: (x >> 40) * (2^40 mod q) >= 2^53 for a 60-bit digit
        assert any(q >> 39 == 1 and ((1 << 20) - 1) * ((1 << 40) % q) >= 1 << 53 for q in m)
    p61 = S["p_min61"].primes
    assert all(q >> 60 == 1 for q in p61[:8]) and p61[8].bit_length() == 42
    assert [ps.mac_policy(p61[8], L) for L in (8, 5, 3)] == [("MacL", 0), ("MacL", 1), ("MacL", 2)]
    deep = S["seal_deep"].primes
    assert deep == O.coeff_modulus_create(32768, [60] + [40] * 19 + [60])
    assert sum(ps.fwd_policy(q) == "F64-generic" for q in deep[1:20]) == 13   # 13 of the 19 40-bit primes: no c40


def test_operand_patterns():
    s = TOY["mixed2048"]
    o, _ = _ctx(s)
    L = 9
    q = np.asarray(s.primes[:L], dtype=np.uint64)[:, None]
    assert (ps.operand(o, "ntt_max", L) == q - 1).all()
    assert (ps.operand(o, "zero", L) == 0).all()
    for kind, zeros in (("coef_max", 0), ("coef_max_z", 1)):
        x = ps.operand(o, kind, L, seed=3)
        for p in range(2):
            for j in range(L):
                coef = o.ntt_inv(j, x[p, j])
                assert (coef == 0).sum() == zeros and ((coef == 0) | (coef == q[j] - 1)).all()
    k = ps.key(o, "max")
    assert k.shape == (s.k - 1, 2, s.k, s.N) and (k == np.asarray(s.primes, dtype=np.uint64)[:, None] - 1).all()
    assert (ps.plain(o, "max", L) == q - 1).all()
