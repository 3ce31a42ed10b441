"""Key switch, NTT, rescale and the element-wise ops at every arithmetic-policy boundary of the engine, word for word
against the CPU oracle (which tests/test_policy_edges_cpu.py pins against the big-int model on the same sets).

The sets (tests/policy_sets.py) put primes on both sides of every bound a policy choice rests on: the FP64 policy's top
(2^41), the one-FMA reduction's window (2^40 - 2^23, 2^40), the [0,16q) forward transform's top (2^60), the limb MAC's
level cut (L = 8) and its lazy-operand levels (3, 5), and the input-reduction flags (q_i > m, P < 2 q_j, q_l > q_j) on
both of their values.  The operands are the ones that load the lazy ranges: all-(q-1) NTT words (sparse digits),
all-(q-1) coefficients (every digit coefficient q_i - 1), the same with one zero, and all-(q-1) keys, plaintexts and
diagonals (the MAC columns at their maximum)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import policy_sets as ps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ps.sets()
PATTERNS = ("uniform", "ntt_max", "coef_max")          # every op
HOISTED_PATTERNS = PATTERNS + ("coef_max_z", "zero")   # the exactly hoisted rotation: also the inputs of its fallback
BATCH_NAMES = [n for n in SETS if n != "seal_deep"]
# lsweep's first nine primes: the limb MAC (MacL, canonical operands) at the double-hoisted transform's only level, L = k - 1 = 8
EXTRA = {"lsweep9": ps.PSet("lsweep9", SETS["lsweep"].N, SETS["lsweep"].primes[:9], (8,), "MacL at L = 8")}


class Ctx:
    """one parameter set on the engine and the oracle; keys: all (q-1) and two uniform ones, host and device"""

    def __init__(self, name):
        from oracle import oracle as O
        from seal_fyp_logistic_regression_amd import Engine
        self.s = s = SETS[name] if name in SETS else EXTRA[name]
        self.O = O
        self.o, self.e = O.Oracle(s.N, s.primes), Engine(s.N, s.primes)
        self.keys = [ps.key(self.o, "max"), ps.key(self.o, "uniform", seed=71)]
        self.dkeys = [self.e.to_device(k) for k in self.keys]
        self.elts = (3, 2 * s.N - 1, O.galois_elt_from_step(s.N, -5))
        self._gal = {}

    def levels(self):
        return ps.LSWEEP if self.s.name == "lsweep" else self.s.levels

    def operand(self, kind, L, npoly=2, seed=1):
        return ps.operand(self.o, kind, L, npoly=npoly, seed=seed)

    def galois(self, tag, ct, elt, ki):
        """the oracle's rotation, cached by (tag, elt, key): the batches below repeat their few distinct items"""
        k = (tag, ct.shape[1], elt, ki)
        if k not in self._gal:
            self._gal[k] = self.o.apply_galois(ct, elt, self.keys[ki])
        return self._gal[k]


@pytest.fixture(scope="module")
def ctxs():
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()  # one set at a time on the device (f41_wide and seal_deep keys are a quarter GB each)
            cache[name] = Ctx(name)
        return cache[name]

    yield get
    cache.clear()


# ---------------------------------------------------------------------------------------------------------------------
# transforms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_ntt_forward_and_inverse_over_every_row(name, ctxs):
    """all k rows (the special prime's included), two polynomials, from row 0 and from a nonzero mod_first: uniform and
    all-(q-1) coefficients forward, uniform and all-(q-1) NTT words inverse"""
    c = ctxs(name)
    o, e, s = c.o, c.e, c.s
    rng = np.random.default_rng(3)
    qs = np.asarray(s.primes, dtype=np.uint64)[:, None]
    uni = np.stack([rng.integers(0, q, s.N, dtype=np.uint64) for q in s.primes])
    for mod_first in (0, 1, s.k - 2):
        rows = s.k - mod_first
        for a in (np.stack([uni, np.broadcast_to(qs - 1, uni.shape)]), np.stack([np.broadcast_to(qs - 1, uni.shape), uni])):
            a = np.ascontiguousarray(a[:, mod_first:])
            fwd = np.stack([[o.ntt_fwd(mod_first + j, a[p, j]) for j in range(rows)] for p in range(2)])
            inv = np.stack([[o.ntt_inv(mod_first + j, a[p, j]) for j in range(rows)] for p in range(2)])
            d = e.to_device(a)
            e.ntt_forward(d, 2, rows, mod_first)
            assert (d.download() == fwd).all(), ("forward", mod_first)
            e.ntt_inverse(d, 2, rows, mod_first)
            assert (d.download() == a).all(), ("round trip", mod_first)
            d = e.to_device(a)
            e.ntt_inverse(d, 2, rows, mod_first)
            assert (d.download() == inv).all(), ("inverse", mod_first)


# ---------------------------------------------------------------------------------------------------------------------
# key switching: batches through the pair path, quarter rows and the chunked path
# ---------------------------------------------------------------------------------------------------------------------
def _batch_items(c, kind, L, n):
    """n items over two sources (one for the constant patterns), the three elements and both keys"""
    srcs = [c.operand(kind, L, seed=10 + i) for i in range(2 if kind == "uniform" else 1)]
    return [(i % len(srcs), c.elts[i % 3], (i // 3) % 2) for i in range(n)], srcs


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_key_switch_batches_bit_exact(name, ctxs):
    """apply_galois_batch, rotate_multiply_plain_batch (all-(q-1) plaintexts), apply_galois_add_batch (all-(q-1)
    accumulators) and relinearize_batch (all-(q-1) key) with n = 1, 8, 40 at every level of the set, on uniform,
    all-(q-1) NTT words and all-(q-1) coefficients"""
    c = ctxs(name)
    o, e = c.o, c.e
    for L in (c.levels() if name != "f41_wide" else (61,)):
        pt = ps.plain(o, "max", L)
        dpt = e.to_device(pt)
        acc = c.operand("ntt_max", L)
        dacc = e.to_device(acc)
        for kind in PATTERNS:
            items, srcs = _batch_items(c, kind, L, 40)
            dsrcs = [e.to_device(x) for x in srcs]
            ct3 = c.operand(kind, L, npoly=3, seed=20)
            relin = o.relinearize(ct3, c.keys[0])
            dct3 = e.to_device(ct3)
            for n in (1, 8, 40):
                it = items[:n]
                want = [c.galois((kind, si), srcs[si], elt, ki) for si, elt, ki in it]
                cts, elts, keys = [dsrcs[si] for si, _, _ in it], [x[1] for x in it], [c.dkeys[x[2]] for x in it]
                got = e.apply_galois_batch(L, cts, elts, keys)
                for i in range(n):
                    assert (got[i].download() == want[i]).all(), ("apply_galois", L, kind, n, i)
                got = e.rotate_multiply_plain_batch(L, cts, elts, keys, [dpt] * n)
                for i in range(n):
                    assert (got[i].download() == o.multiply_plain(want[i], pt)).all(), ("rotate*plain", L, kind, n, i)
                outs, accs = e.apply_galois_add_batch(L, cts, elts, keys, [dacc] * n)
                for i in range(n):
                    assert (outs[i].download() == want[i]).all(), ("galois_add out", L, kind, n, i)
                    assert (accs[i].download() == o.add(acc, want[i])).all(), ("galois_add acc", L, kind, n, i)
                got = e.relinearize_batch(L, [dct3] * n, c.dkeys[0])
                for i in range(n):
                    assert (got[i].download() == relin).all(), ("relinearize", L, kind, n, i)


@pytest.mark.parametrize("name", ["f41_wide"])
def test_key_switch_at_level_31_of_the_widest_fp64_set(name, ctxs):
    """f41_wide at L = 31 (past the bound the MacF comment used to state), one item and a batch"""
    c = ctxs(name)
    o, e = c.o, c.e
    L = 31
    for kind in PATTERNS:
        ct = c.operand(kind, L, seed=5)
        d = e.to_device(ct)
        for n in (1, 3):
            got = e.apply_galois_batch(L, [d] * n, list(c.elts[:n]), [c.dkeys[0]] * n)
            for i in range(n):
                assert (got[i].download() == c.galois(kind, ct, c.elts[i], 0)).all(), (kind, n, i)


@pytest.mark.parametrize("name", list(SETS))
def test_exactly_hoisted_rotations_bit_exact_and_fallback_as_the_oracle_says(name, ctxs):
    """rotate_hoisted_batch gives the regular rotation's words on every pattern; where the oracle's hoisted statement
    reports the regular path (a zero digit coefficient) the engine's fallback counter grows, where it reports the
    hoisted path it does not -- so the flip-mask term ran at each policy edge.  40 items: the engine hoists batches of
    more than 32 (below that the latency path runs, with nothing to fall back from)"""
    c = ctxs(name)
    o, e = c.o, c.e
    pairs = [(c.elts[i % 3], (i // 3) % 2) for i in range(6)]   # three elements x two keys, repeated to 40 items
    items = [pairs[i % 6] for i in range(40)]
    elts, keys = [x[0] for x in items], [c.dkeys[x[1]] for x in items]
    # (the two widest sets at their top level only: the oracle's rotation costs a quarter second there)
    for L in (c.levels()[:1] if c.s.k > 20 else c.levels()[:2]):
        pt = ps.plain(o, "max", L)
        dpt = e.to_device(pt)
        for kind in HOISTED_PATTERNS:
            ct = c.operand(kind, L, seed=40 + L)
            d = e.to_device(ct)
            words, regular = {}, set()
            for elt, ki in pairs:
                words[elt, ki], r = o.apply_galois_hoisted_exact(ct, elt, c.keys[ki])   # (== apply_galois: the CPU suite)
                regular.add(r)
            want = [words[x] for x in items]
            assert len(regular) == 1, "the fallback is decided by the source alone"
            regular = regular.pop()
            before = e.ks_fallback_count()
            got = e.rotate_hoisted_batch(L, d, elts, keys)
            mid = e.ks_fallback_count()
            fused = e.rotate_hoisted_batch(L, d, elts, keys, pts=[dpt] * len(elts))
            after = e.ks_fallback_count()
            for i in range(len(elts)):
                assert (got[i].download() == want[i]).all(), ("hoisted", L, kind, i)
                assert (fused[i].download() == o.multiply_plain(want[i], pt)).all(), ("hoisted*plain", L, kind, i)
            if regular:
                assert mid > before and after > mid, ("the oracle took the regular path: the engine must fall back", L, kind)
            else:
                assert after == before, ("the oracle's hoisted identity applies: no fallback", L, kind)


# ---------------------------------------------------------------------------------------------------------------------
# double-hoisted linear transform: full LT2_CHUNK columns with all-(q-1) diagonals
# ---------------------------------------------------------------------------------------------------------------------
def _lt2(c, d, kind):
    o, e, s = c.o, c.e, c.s
    L = s.k - 1
    O = c.O
    steps = list(range(d))
    diags = [ps.plain(o, "max", s.k)] * d
    elts = [O.galois_elt_from_step(s.N, l) for l in steps[1:]]
    e_d = O.galois_elt_from_step(s.N, -d)
    ct = c.operand(kind, L, seed=60)
    ct_new = o.add(ct, o.apply_galois(ct, e_d, c.keys[0]))
    want = o.lt_double_hoisted_core(ct_new, diags, elts, [c.keys[0]] * len(elts))
    key_elts = sorted(set(elts + [e_d]))
    got = e.linear_transform_plain_hoisted2_sparse(L, e.to_device(ct), d, steps, [e.to_device(x) for x in diags], key_elts,
                                                   [c.dkeys[0]] * len(key_elts))
    return got.download(), want


@pytest.mark.parametrize("name,d", [("lsweep9", 9), ("lsweep9", 12), ("lsweep", 12), ("mixed2048", 12), ("i42", 9),
                                    ("straddle60", 9), ("f41", 9), ("c40_edge", 9)])
def test_double_hoisted_transform_with_full_mac_columns(name, d, ctxs):
    """linear_transform_plain_hoisted2_sparse with all-(q-1) key-level diagonals and keys, d - 1 >= 8 rotations (one full
    LT2_CHUNK: sixteen terms per 64-bit column of the limb MAC): MacL at L = 8 (the first nine primes of lsweep), MacW
    at L = 16, and the mixed / integer / FP64 sets"""
    c = ctxs(name)
    L = c.s.k - 1
    if name == "lsweep9":
        assert ps.mac_policy(c.s.primes[0], L) == ("MacL", 0)
    elif name == "lsweep":
        assert ps.mac_policy(c.s.primes[0], L) == ("MacW", 0)
    for kind in PATTERNS:
        got, want = _lt2(c, d, kind)
        assert (got == want).all(), (kind, d)


# ---------------------------------------------------------------------------------------------------------------------
# rescale, mod drop, products, sums
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_rescale_mod_drop_products_and_sums(name, ctxs):
    """rescale_to_next in both divisions (sizes 2 and 3), mod_drop, multiply, square, multiply_plain with an all-(q-1)
    plaintext and add_many of 64 all-(q-1) ciphertexts (plus the patterns), at every level of the set"""
    c = ctxs(name)
    o, e = c.o, c.e
    for L in sorted(set(c.levels()) | {2}):
        rs = L >= 2
        pmax = ps.plain(o, "max", L)
        dpmax = e.to_device(pmax)
        for kind in PATTERNS:
            a = c.operand(kind, L, seed=80 + L)
            b = c.operand("uniform" if kind != "uniform" else "coef_max", L, seed=90 + L)
            da, db = e.to_device(a), e.to_device(b)
            a3 = c.operand(kind, L, npoly=3, seed=85 + L)
            da3 = e.to_device(a3)
            for rounded in ((False, True) if rs else ()):
                assert (e.rescale_to_next(L, 2, da, rounded=rounded).download() == o.rescale(a, rounded=rounded)).all(), \
                    ("rescale", L, kind, rounded)
                assert (e.rescale_to_next(L, 3, da3, rounded=rounded).download() == o.rescale(a3, rounded=rounded)).all(), \
                    ("rescale size 3", L, kind, rounded)
            for L_out in (sorted({1, L - 1}) if rs else ()):
                assert (e.mod_drop(L, L_out, 2, da).download() == a[:, :L_out]).all(), ("mod_drop", L, L_out)
            assert (e.multiply(L, da, db).download() == o.multiply(a, b)).all(), ("multiply", L, kind)
            assert (e.square(L, da).download() == o.multiply(a, a)).all(), ("square", L, kind)
            assert (e.multiply_plain(L, 2, da, dpmax).download() == o.multiply_plain(a, pmax)).all(), ("multiply_plain", L, kind)
            terms = [c.operand("ntt_max", L)] * 64 + [a, b]
            want = terms[0]
            for t in terms[1:]:
                want = o.add(want, t)
            dmax = e.to_device(terms[0])
            assert (e.add_many(L, 2, [dmax] * 64 + [da, db]).download() == want).all(), ("add_many", L, kind)


# ---------------------------------------------------------------------------------------------------------------------
# knobs: the mixed sets under every path the engine can be forced onto
# ---------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from oracle import oracle as O
from seal_fyp_logistic_regression_amd import Engine
from tests import policy_sets as ps
ok = True
for name in ("mixed2048", "mixed16384"):
    s = ps.sets()[name]
    o, e = O.Oracle(s.N, s.primes), Engine(s.N, s.primes)
    keys = [ps.key(o, "max"), ps.key(o, "uniform", seed=71)]
    dkeys = [e.to_device(k) for k in keys]
    elts = (3, 2 * s.N - 1, O.galois_elt_from_step(s.N, -5))
    a = ps.operand(o, "coef_max", s.k, npoly=1)[0]
    d = e.to_device(a[None])
    e.ntt_inverse(d, 1, s.k, 0)
    ok &= bool((d.download()[0] == np.stack([o.ntt_inv(j, a[j]) for j in range(s.k)])).all())
    for L in s.levels:
        pt = ps.plain(o, "max", L)
        dpt = e.to_device(pt)
        for kind in ("uniform", "ntt_max", "coef_max"):
            ct = ps.operand(o, kind, L, seed=L)
            dct = e.to_device(ct)
            want = {(elt, ki): o.apply_galois(ct, elt, keys[ki]) for elt in elts for ki in (0, 1)}
            for n in (1, 8, 40):
                it = [(elts[i %% 3], (i // 3) %% 2) for i in range(n)]
                outs = e.apply_galois_batch(L, [dct] * n, [x[0] for x in it], [dkeys[x[1]] for x in it])
                ok &= all((outs[i].download() == want[it[i]]).all() for i in range(n))
                outs = e.rotate_multiply_plain_batch(L, [dct] * n, [x[0] for x in it], [dkeys[x[1]] for x in it], [dpt] * n)
                ok &= all((outs[i].download() == o.multiply_plain(want[it[i]], pt)).all() for i in range(n))
            ct3 = ps.operand(o, kind, L, npoly=3, seed=L)
            outs = e.relinearize_batch(L, [e.to_device(ct3)] * 3, dkeys[0])
            r = o.relinearize(ct3, keys[0])
            ok &= all((x.download() == r).all() for x in outs)
            for rounded in (False, True):
                ok &= bool((e.rescale_to_next(L, 2, dct, rounded=rounded).download() == o.rescale(ct, rounded=rounded)).all())
    print(name, "ok" if ok else "MISMATCH", flush=True)
print("PARITY", ok)
"""


@pytest.mark.parametrize("knob", ["HEFX_PAIR=0", "HEFX_PAIR=1", "HEFX_QUARTER=0", "HEFX_QUARTER=1", "HEFX_NO_FP64=1"])
def test_mixed_sets_under_every_path_knob(knob):
    """both mixed sets (every prime class interleaved in one launch) with the pair path and quarter rows forced on / off,
    and with the FP64 policy off (every row on the integer policy): batches of 1, 8, 40
    rotations, fused products, relinearisations and both rescales against the oracle, in a child process per knob"""
    env = {k: v for k, v in os.environ.items() if k not in ("HEFX_QUARTER", "HEFX_QMASK", "HEFX_PAIR", "HEFX_NO_FP64")}
    k, v = knob.split("=")
    env[k] = v
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PARITY True" in r.stdout, (r.returncode, r.stdout[-800:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------------
# a SEAL-valid deep chain through the SEAL-shaped API
# ---------------------------------------------------------------------------------------------------------------------
def test_seal_deep_chain_matches_its_oracle_twin_and_numpy(rescale_mode):
    """CoeffModulus.Create(32768, [60] + [40] * 19 + [60]) -- 13 of its 19 40-bit primes outside the one-FMA window --
    through seal.py: encode, encrypt, rotate, then three rounds of multiply + relinearize + rescale; the engine's words
    equal the oracle twin's at every step in both divisions, and the decoded values equal numpy's"""
    from tests.test_gpu_composites import make, bits, decode
    N, chain = 32768, [60] + [40] * 19 + [60]
    rng = np.random.default_rng(11)
    v, w = rng.uniform(-1, 1, 64), rng.uniform(-1, 1, 64)
    res = {}
    for kind in ("gpu", "oracle"):
        e = make(N, chain, kind, seed=5, galois_steps=[1])
        ev, enc, encoder = e["ev"], e["enc"], e["encoder"]
        scale = 2.0 ** 40
        x = ev.rotate_vector(enc.encrypt(encoder.encode(v, scale)), 1, e["gk"])
        y = enc.encrypt(encoder.encode(w, scale))
        trace = [bits(e, x)]
        for _ in range(3):
            ev.mod_switch_to_inplace(y, x.parms_id())
            x = ev.multiply(x, y)
            trace.append(bits(e, x))
            ev.relinearize_inplace(x, e["rk"])
            trace.append(bits(e, x))
            ev.rescale_to_next_inplace(x)
            trace.append(bits(e, x))
        assert x.parms_id() == 17
        res[kind] = (e, x, trace)
    (eg, xg, tg), (eo, xo, to) = res["gpu"], res["oracle"]
    for i, (a, b) in enumerate(zip(tg, to)):
        assert (a == b).all(), ("step", i, rescale_mode)
    want = np.roll(np.concatenate([v, np.zeros(N // 2 - 64)]), -1)[:64] * w ** 3
    assert np.abs(decode(eg, xg, 64) - want).max() < 1e-3
