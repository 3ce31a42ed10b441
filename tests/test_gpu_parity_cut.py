"""The digit transforms cut by coefficient parity, with their last stage inside the regular key MAC, word for word
against the CPU oracle.

An ordinary key-switch chunk now hands scratch `x` over as the two parity classes [E | O] of every digit row BEFORE the
last forward stage (hefx_ntt.cuh parity_fwd_raw); the regular key MAC fetches (E[w], O[w]) with one 16-byte load per lane
pair and a lane exchange, runs the last butterfly in the target prime's forward policy and reduces to what its
accumulation takes (hefx_keyswitch.hip mac_items, xin_cut).  Hoisted chunks, quarter rows, the pair path and the
double-hoisted transform keep finished rows.

What the cases below reach:
  ring sizes        2048, 4096, 8192 (the R == 0 trip through LDS), 16384, 32768
  producer policy   FP64 (generic and c40 windows), U64L below 2^60, U64 at 61 bits, and HEFX_NO_FP64=1
  consumer policy   MacF; MacL at slack 2 (L = 2, 3), 1 (L = 4, 5), 0 (L = 6, 8); MacW (L >= 9, 61-bit primes)
  operands          all-(q-1) NTT words, all-(q-1) coefficients, uniform, against all-(q-1) and uniform keys: the inputs
                    that load the lazy ranges the last stage and its reductions rest on
  shapes            batches above 32 items over DISTINCT sources (so that the regular path runs and not exact hoisting:
                    asserted through ks_stats), odd item counts (the MAC's one-item tail), neighbours with different
                    keys (the MAC's one-item path), a chunk that streams x and one that does not, relinearisations,
                    rotate-and-add, fused plaintext products, and one batch whose two chunks are one ordinary and one
                    hoisted chunk over the same scratch.
Not here: L = 61 of f41_wide (a 124 MB `x` block per item, 4.3 GB for a batch of 35 and a quarter-gigabyte key per
oracle rotation) -- this file takes the set at L = 31, the same MacF consumer behind the same FP64 producer with 31 terms
per sum.  Every other level the sets name runs, L = 1 included (one digit into the special prime's row)."""
import json
import os

import numpy as np
import pytest

from tests import policy_sets as ps

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "appendix_b.json")))
BENCH_SETS = {s["name"]: s for s in GOLD["sets"]}
SETS = ps.sets()
KINDS = ("ntt_max", "coef_max", "uniform")
# levels per set: every level the set names (lsweep: LSWEEP), except f41_wide (the docstring says why)
LEVELS = {"f41_wide": (31,), "lsweep": ps.LSWEEP}
# N = 32768 with a limb-MAC consumer at every slack: two 60-bit and three 40-bit data primes under a 60-bit special prime
# (the policy sets have this ring size only in seal_deep, whose levels are all above 8, i.e. MacW)
DEEP_INT = ps.PSet("deep_int", 32768, ps.primes_below(1 << 60, 32768, 3)[:2] + ps.primes_below(1 << 40, 32768, 3)
                   + ps.primes_below(1 << 60, 32768, 3)[2:], (5, 3, 2), "MacL at N = 32768, slack 1 and 2")
NAMES = ["f41", "f41_wide", "c40_edge", "i42", "straddle60", "small_p", "p_min", "p_min40", "p_min61", "lsweep",
         "mixed2048", "mixed16384", "seal_deep"]


class _Env:
    """context-creation levers (HEFX_CHUNK, HEFX_STREAMS, HEFX_NO_FP64 are read once, at hefx_context_create)"""

    def __init__(self, env):
        self.env, self.old = env or {}, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _make(N, primes, env=None):
    from oracle import oracle as O
    from seal_fyp_logistic_regression_amd import Engine
    with _Env(env):
        e = Engine(N, primes)
    return O, O.Oracle(N, primes), e


def _regular(e, fn, items, chunks=None):
    """run fn() and assert that its `items` key switches all took the regular path (none exactly hoisted)"""
    s0 = e.ks_stats()
    out = fn()
    s1 = e.ks_stats()
    assert s1["key_switches"] - s0["key_switches"] == items
    assert s1["hoisted"] == s0["hoisted"], "the case is meant for the regular path"
    if chunks is not None:
        assert s1["chunks"] - s0["chunks"] == chunks
    return out


def _distinct(e, host, n):
    """n device copies of one host ciphertext: distinct sources for the engine, one oracle result for the checker"""
    return [e.to_device(host) for _ in range(n)]


def _policy_case(name, env=None, levels=None, kinds=KINDS):
    s = SETS[name] if isinstance(name, str) else name
    name = s.name
    O, o, e = _make(s.N, s.primes, env)
    keys = [ps.key(o, "max"), ps.key(o, "uniform", seed=71)]
    dkeys = [e.to_device(k) for k in keys]
    elts = (3, 2 * s.N - 1, O.galois_elt_from_step(s.N, -5))
    for L in (levels or LEVELS.get(name, s.levels)):
        pt = ps.plain(o, "max", L)
        dpt = e.to_device(pt)
        for kind in kinds:
            ct = ps.operand(o, kind, L, seed=30 + L)
            want = {(elt, ki): o.apply_galois(ct, elt, keys[ki]) for elt in elts for ki in (0, 1)}
            # 34 items, 17 per key: whichever key group comes first is odd, so one MAC unit straddles two keys
            # 35 items: the last MAC unit has one item
            for n in (34, 35):
                it = [(elts[i % 3], i % 2) for i in range(n)]
                srcs = _distinct(e, ct, n)
                ev, kv = [x[0] for x in it], [dkeys[x[1]] for x in it]
                got = _regular(e, lambda: e.apply_galois_batch(L, srcs, ev, kv), n)
                for i in range(n):
                    assert (got[i].download() == want[it[i]]).all(), ("apply_galois", name, L, kind, n, i)
            got = _regular(e, lambda: e.rotate_multiply_plain_batch(L, srcs, ev, kv, [dpt] * n), n)
            for i in range(n):
                assert (got[i].download() == o.multiply_plain(want[it[i]], pt)).all(), ("rotate*plain", name, L, kind, i)
    return e


@pytest.mark.parametrize("name", NAMES)
def test_regular_chunks_at_every_policy_edge(name):
    """34 and 35 rotations of distinct sources (the regular path, asserted), all-(q-1) and uniform operands and keys, at
    the levels of every policy set: MacF / MacL slack 2, 1, 0 / MacW consumers behind FP64 / U64L / U64 producers"""
    _policy_case(name)


def test_the_sets_reach_every_consumer_policy_and_slack():
    """the table in the docstring, checked against policy_sets' statement of the engine's rules"""
    seen = set()
    for name in NAMES:
        s = SETS[name]
        for L in LEVELS.get(name, s.levels):
            for q in s.primes[:L] + s.primes[-1:]:
                seen.add((ps.fwd_policy(q).split("-")[0], ps.mac_policy(q, L)))
    for want in (("F64", ("MacF", 0)), ("U64L", ("MacL", 2)), ("U64L", ("MacL", 1)), ("U64L", ("MacL", 0)),
                 ("U64L", ("MacW", 0)), ("U64", ("MacW", 0))):
        assert want in seen, want
    assert {SETS[n].N for n in NAMES} >= {8192, 16384, 32768}


@pytest.mark.parametrize("name", ["mixed16384", "f41", "mixed2048"])
def test_integer_policy_everywhere(name):
    """HEFX_NO_FP64=1: every row on the integer policies, the 40-bit primes included (MacL / MacW on tiny primes)"""
    _policy_case(name, env={"HEFX_NO_FP64": "1"})


@pytest.mark.parametrize("env", [None, {"HEFX_NO_FP64": "1"}])
def test_ring_32768_limb_mac_with_adversarial_operands(env):
    """N = 32768 (one digit workgroup per CU), MacL consumers at slack 1 and 2 -- with HEFX_NO_FP64=1 on every row, the
    40-bit ones included -- on all-(q-1) NTT words, all-(q-1) coefficients and uniform inputs, all-(q-1) and uniform keys"""
    for L in DEEP_INT.levels:
        assert ps.mac_policy(DEEP_INT.primes[0], L)[0] == "MacL" and ps.mac_policy(DEEP_INT.primes[-1], L)[0] == "MacL"
    _policy_case(DEEP_INT, env=env)


@pytest.mark.parametrize("setname", ["C2", "C3", "C4", "C5"])
def test_bench_sets_every_entry_point(setname):
    """the bench's parameter sets (N = 8192, 16384, 16384 at L = 8, 32768): rotations, fused products, rotate-and-add and
    relinearisations in batches of 33 and 40 distinct items on uniform inputs"""
    s = BENCH_SETS[setname]
    N, primes = s["N"], [int(p, 16) for p in s["primes"]]
    O, o, e = _make(N, primes)
    L = len(primes) - 1
    keys = [o.uniform(o.k, 2 * (o.k - 1), 70 + i).reshape(o.k - 1, 2, o.k, N) for i in range(2)]
    dkeys = [e.to_device(k) for k in keys]
    elts = (3, 9, O.galois_elt_from_step(N, -1))
    cts = [o.uniform(L, 2, 100 + i) for i in range(3)]
    pt = o.uniform(L, 1, 5)[0]
    acc = o.uniform(L, 2, 6)
    dpt, dacc = e.to_device(pt), e.to_device(acc)
    want = {(c, el, k): o.apply_galois(cts[c], elts[el], keys[k]) for c in range(3) for el in range(3) for k in range(2)}
    for n in (33, 40):
        it = [(i % 3, (i // 3) % 3, (i // 9) % 2) for i in range(n)]
        srcs = [e.to_device(cts[x[0]]) for x in it]
        ev, kv = [elts[x[1]] for x in it], [dkeys[x[2]] for x in it]
        got = _regular(e, lambda: e.rotate_multiply_plain_batch(L, srcs, ev, kv, [dpt] * n), n)
        for i in range(n):
            assert (got[i].download() == o.multiply_plain(want[it[i]], pt)).all(), ("rotate*plain", setname, n, i)
        outs, accs = _regular(e, lambda: e.apply_galois_add_batch(L, srcs, ev, kv, [dacc] * n), n)
        for i in range(n):
            assert (outs[i].download() == want[it[i]]).all(), ("galois_add out", setname, n, i)
            assert (accs[i].download() == o.add(acc, want[it[i]])).all(), ("galois_add acc", setname, n, i)
    ct3 = o.uniform(L, 3, 200)
    relin = o.relinearize(ct3, keys[0])
    d3 = [e.to_device(ct3) for _ in range(35)]
    got = _regular(e, lambda: e.relinearize_batch(L, d3, dkeys[0]), 35)
    for i in range(35):
        assert (got[i].download() == relin).all(), ("relinearize", setname, i)


def test_streamed_and_cached_chunks_at_c3():
    """N = 16384, L = 5: a digit x modulus block is 3.9 MB per item, so one chunk of 80 items (315 MB) streams `x` past
    the 256 MB Infinity Cache and one of 40 does not; serial chunks of 40 + 40 + 1 (HEFX_STREAMS=0, HEFX_CHUNK=40) end in a
    one-item chunk on the small-batch launches"""
    s = BENCH_SETS["C3"]
    N, primes = s["N"], [int(p, 16) for p in s["primes"]]
    L = len(primes) - 1
    assert 80 * L * (L + 1) * N * 8 > 256 << 20 >= 40 * L * (L + 1) * N * 8
    for env, n, chunks in (({"HEFX_CHUNK": "80"}, 80, 1), ({"HEFX_CHUNK": "40"}, 40, 1),
                           ({"HEFX_CHUNK": "40", "HEFX_STREAMS": "0"}, 81, 3)):
        O, o, e = _make(N, primes, env)
        key = o.uniform(o.k, 2 * (o.k - 1), 77).reshape(o.k - 1, 2, o.k, N)
        dkey = e.to_device(key)
        cts = [o.uniform(L, 2, 300 + i) for i in range(4)]
        pts = [o.uniform(L, 1, 350 + i)[0] for i in range(4)]
        want = [o.rotate_mulplain(cts[i], 3, key, pts[i]) for i in range(4)]
        dpts = [e.to_device(p) for p in pts]
        srcs = [e.to_device(cts[i % 4]) for i in range(n)]
        got = _regular(e, lambda: e.rotate_multiply_plain_batch(L, srcs, [3] * n, [dkey] * n, [dpts[i % 4] for i in range(n)]),
                       n, chunks)
        for i in range(n):
            assert (got[i].download() == want[i % 4]).all(), (env, i)


def test_an_ordinary_and_a_hoisted_chunk_in_one_batch():
    """80 rotations in chunks of 40 on ONE stream (the two chunks then use the same scratch block): the first 40 rotate one
    source -- exactly hoisted, finished rows in `x` -- the other 40 rotate 20 sources twice each -- an ordinary chunk,
    parity classes in `x`.  Both orders, so that each layout is written over the other one."""
    s = BENCH_SETS["C3"]
    N, primes = s["N"], [int(p, 16) for p in s["primes"]]
    L = len(primes) - 1
    O, o, e = _make(N, primes, {"HEFX_CHUNK": "40", "HEFX_STREAMS": "0"})
    key = o.uniform(o.k, 2 * (o.k - 1), 78).reshape(o.k - 1, 2, o.k, N)
    dkey = e.to_device(key)
    elts = [O.galois_elt_from_step(N, st) for st in (1, 2, 3, -1)]
    shared = o.uniform(L, 2, 400)
    other = o.uniform(L, 2, 401)
    want_s = [o.apply_galois(shared, el, key) for el in elts]
    want_o = [o.apply_galois(other, el, key) for el in elts]
    dshared = e.to_device(shared)
    dothers = [e.to_device(other) for _ in range(20)]
    hoisted = [(dshared, i % 4, want_s) for i in range(40)]
    ordinary = [(dothers[i // 2], i % 4, want_o) for i in range(40)]
    for items in (hoisted + ordinary, ordinary + hoisted):
        s0 = e.ks_stats()
        got = e.apply_galois_batch(L, [x[0] for x in items], [elts[x[1]] for x in items], [dkey] * 80)
        s1 = e.ks_stats()
        assert s1["chunks"] - s0["chunks"] == 2 and s1["hoisted"] - s0["hoisted"] == 40, (s0, s1)
        for i, (_, el, want) in enumerate(items):
            assert (got[i].download() == want[el]).all(), i
    assert e.ks_fallback_count() == 0
