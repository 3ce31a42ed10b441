"""Hoisted hybrid key switching on the GPU, word for word (include/hefx_hybrid_hoist.h): hefx_hybrid_rotate_hoisted_batch and
hefx_hybrid_plain_combine_hoisted against the integer statement in Python integers (tests/hybrid_hoist_cases.py, which
tests/test_hybrid_hoist_cpu.py pins to seal.py's host statement, to the unhoisted model at the element 1 and to the noise
bound), the consistency of the two entries with each other and with hefx_hybrid_apply_galois_batch, refusals, a caller-owned
stream, and the hybrid DFT against the oracle twin."""
import numpy as np
import pytest

from tests import hybrid_cases as HC
from tests import hybrid_hoist_cases as HH

pytestmark = pytest.mark.gpu

_GPU = {}


def gpu(name):
    """(set, context, engine) on the HIP engine, once per set"""
    if name not in _GPU:
        s = HC.sets()[name]
        ctx = HC.context(s, "gpu")
        _GPU[name] = (s, ctx, ctx.backend.engine)
    return _GPU[name]


def up(e, x):
    return None if x is None else e.to_device(x)


WORD_CASES = [("k7a2-p50_60", 5), ("k7a2-p50_60", 4), ("k7a2-p50_60", 3), ("k7a2-p50_60", 1), ("k8a3-above60", 5), ("k8a3-above60", 2),
              ("k7a4-d40_s60", 3), ("k4a1-p50_60", 3), ("k4a1-p50_60", 1), ("k12a5-p50_60", 7), ("k12a5-p50_60", 3), ("k18a8-d40_s60", 10),
              ("k14a2-above60", 11), ("big7", 5)]


@pytest.mark.parametrize("name,L", WORD_CASES)
def test_both_entries_give_the_words_of_the_statement(name, L):
    """n = 2 sources, the elements {1 with a NULL key, 3, 2N - 1}, G = 2 outputs with one structural zero each; big7 is
    N = 32768, where every block a transform reads is laid out twice.  The inputs are only read."""
    s, ctx, e = gpu(name)
    assert L in s.levels
    cts, elts, keys, pts = HH.case(s, L)
    want_rot, want_comb = HH.case_models(s, L)
    d_cts, d_keys = [e.to_device(c) for c in cts], [up(e, k) for k in keys]
    d_pts = [[up(e, p) for p in row] for row in pts]
    rot = e.hybrid_rotate_hoisted_batch(s.alpha, L, d_cts, elts, d_keys)
    comb = e.hybrid_plain_combine_hoisted(s.alpha, L, d_cts, elts, d_keys, d_pts)
    assert len(rot) == 6 and len(comb) == 2
    for t in range(6):
        assert np.array_equal(rot[t].download(), want_rot[t]), (name, L, "rotation", t)
    for o in range(2):
        assert np.array_equal(comb[o].download(), want_comb[o]), (name, L, "output", o)
    for d, h in zip(d_cts, cts):
        assert np.array_equal(d.download(), h), "the inputs are only read"
    for d, h in zip(d_keys[1:], keys[1:]):
        assert np.array_equal(d.download().reshape(-1), h.reshape(-1)), "the keys are only read"
    assert all(np.array_equal(d.download(), h) for dr, hr in zip(d_pts, pts) for d, h in zip(dr, hr) if h is not None)


@pytest.mark.parametrize("L", [20, 17])
def test_sixty_four_terms_at_the_largest_words_give_the_words_of_the_statement(L):
    """k24a4-top61: the 24 largest primes below 2^61, the max operand, the max key, plaintexts of q_m - 1 and 64 terms in ONE
    output: the combine's 128-bit sum holds HEFX_HYBRID_HOIST_MAX_TERMS products of the largest factors there are; L = 20 has
    five full digits, L = 17 a last digit of one prime"""
    from seal_fyp_logistic_regression_amd import capi
    s, ctx, e = gpu("k24a4-top61")
    cts, elts, keys, pts, want = HH.full_case(s, L)
    assert len(cts) * len(elts) == 64 == capi.HYBRID_HOIST_MAX_TERMS and min(s.primes) >> 60 == 1
    ct, key, pt = e.to_device(cts[0]), e.to_device(keys[0]), e.to_device(pts[0][0])
    (out,) = e.hybrid_plain_combine_hoisted(s.alpha, L, [ct] * 8, elts, [key] * 8, [[pt] * 64])
    assert np.array_equal(out.download(), want), L


def test_the_entries_agree_with_each_other_and_with_the_unhoisted_entry():
    """the element 1 with a real key: hefx_hybrid_apply_galois_batch's words; a combine of one term with the plaintext 1: the
    rotate entry's words; n = 2 sources: two calls with n = 1"""
    s, ctx, e = gpu("k8a3-above60")
    L, N = 5, s.N
    cts, elts, keys, pts = HH.case(s, L)
    d_cts, d_keys = [e.to_device(c) for c in cts], [up(e, k) for k in keys]
    (one,) = e.hybrid_rotate_hoisted_batch(s.alpha, L, d_cts[:1], [1], [d_keys[1]])
    (want,) = e.hybrid_apply_galois_batch(s.alpha, L, d_cts[:1], [1], [d_keys[1]])
    assert np.array_equal(one.download(), want.download())
    rot = e.hybrid_rotate_hoisted_batch(s.alpha, L, d_cts, elts, d_keys)
    unit = e.to_device(HH.plaintext(s, "one", 0))
    rows = [[unit if t == o else None for t in range(6)] for o in range(6)]
    for o, got in enumerate(e.hybrid_plain_combine_hoisted(s.alpha, L, d_cts, elts, d_keys, rows)):
        assert np.array_equal(got.download(), rot[o].download()), o
    singles = [e.hybrid_rotate_hoisted_batch(s.alpha, L, [c], elts, d_keys) for c in d_cts]
    for i in range(2):
        for k in range(3):
            assert np.array_equal(singles[i][k].download(), rot[i * 3 + k].download()), (i, k)
    d_pts = [[up(e, p) for p in row] for row in pts]
    both = e.hybrid_plain_combine_hoisted(s.alpha, L, d_cts, elts, d_keys, [d_pts[0][:3] + [None] * 3, [None] * 3 + d_pts[1][3:]])
    (first,) = e.hybrid_plain_combine_hoisted(s.alpha, L, d_cts[:1], elts, d_keys, [d_pts[0][:3]])
    (second,) = e.hybrid_plain_combine_hoisted(s.alpha, L, d_cts[1:], elts, d_keys, [d_pts[1][3:]])
    assert np.array_equal(both[0].download(), first.download()) and np.array_equal(both[1].download(), second.download())


def test_bad_arguments_and_the_limits_are_refused():
    from seal_fyp_logistic_regression_amd import capi
    s, ctx, e = gpu("k7a2-p50_60")
    N, top = s.N, s.k - s.alpha
    key, pt = e.to_device(HC.random_key(s, 11)), e.zeros(s.k, N)
    ct = lambda L: e.zeros(2, L, N)
    rot = lambda alpha, L, cts, elts, keys: e.hybrid_rotate_hoisted_batch(alpha, L, cts, elts, keys)
    comb = lambda alpha, L, cts, elts, keys, pts: e.hybrid_plain_combine_hoisted(alpha, L, cts, elts, keys, pts)
    for alpha in (0, -1, s.k, 9):
        with pytest.raises(ValueError, match="alpha must be in"):
            rot(alpha, 1, [ct(1)], [3], [key])
        with pytest.raises(ValueError, match="alpha must be in"):
            comb(alpha, 1, [ct(1)], [3], [key], [[pt]])
    for L in (0, top + 1):
        with pytest.raises(ValueError, match=r"level L must be in \[1, k - alpha\]"):
            rot(s.alpha, L, [ct(max(L, 1))], [3], [key])
        with pytest.raises(ValueError, match=r"level L must be in \[1, k - alpha\]"):
            comb(s.alpha, L, [ct(max(L, 1))], [3], [key], [[pt]])
    for elt in (2, 2 * N + 1):
        with pytest.raises(ValueError, match="odd and < 2N"):
            rot(s.alpha, 2, [ct(2)], [elt], [key])
        with pytest.raises(ValueError, match="odd and < 2N"):
            comb(s.alpha, 2, [ct(2)], [elt], [key], [[pt]])
    with pytest.raises(ValueError, match="its element must be 1"):       # a NULL key is the identity term
        rot(s.alpha, 2, [ct(2)], [3], [None])
    with pytest.raises(ValueError, match="its element must be 1"):
        comb(s.alpha, 2, [ct(2)], [1, 2 * N - 1], [None, None], [[pt, pt]])
    with pytest.raises(ValueError, match="n < 1 or m < 1"):
        rot(s.alpha, 2, [], [3], [key])
    with pytest.raises(ValueError, match="n < 1 or m < 1"):
        comb(s.alpha, 2, [ct(2)], [], [], [[]])

    class Null:
        ptr = None
    with pytest.raises(ValueError, match="null pointer"):
        rot(s.alpha, 2, [Null()], [3], [key])
    with pytest.raises(ValueError, match="null pointer"):
        e.hybrid_rotate_hoisted_batch(s.alpha, 2, [ct(2)], [3], [key], outs=[Null()])
    with pytest.raises(ValueError, match="an output has no term"):
        comb(s.alpha, 2, [ct(2)], [1, 3], [None, key], [[pt, None], [None, None]])
    # the limits: 64 terms run, 65 do not; 64 outputs run, 65 do not (L = 1: the smallest workspace)
    c1 = ct(1)
    assert capi.HYBRID_HOIST_MAX_TERMS == 64 == capi.HYBRID_HOIST_MAX_OUT
    assert len(rot(s.alpha, 1, [c1] * 8, [3] * 8, [key] * 8)) == 64
    with pytest.raises(ValueError, match="HEFX_HYBRID_HOIST_MAX_TERMS"):
        rot(s.alpha, 1, [c1] * 13, [3] * 5, [key] * 5)
    with pytest.raises(ValueError, match="HEFX_HYBRID_HOIST_MAX_TERMS"):
        comb(s.alpha, 1, [c1] * 5, [3] * 13, [key] * 13, [[pt] * 65])
    assert len(comb(s.alpha, 1, [c1], [3], [key], [[pt]] * 64)) == 64
    with pytest.raises(ValueError, match="HEFX_HYBRID_HOIST_MAX_OUT"):
        comb(s.alpha, 1, [c1], [3], [key], [[pt]] * 65)
    e.sync()


def test_every_byte_overlap_is_refused_and_leaves_the_outputs_untouched():
    """the strict rule: an output may overlap no input, no plaintext (k N words), not the read digits of a key and no other
    output -- ValueError with nothing submitted; an output on the key's digits that level L does not read runs"""
    s, ctx, e = gpu("k7a2-p50_60")
    N, k, L, alpha = s.N, s.k, 3, s.alpha
    dn = (L + alpha - 1) // alpha
    keyw, readw, ctw, ptw = s.dnum * 2 * k * N, dn * 2 * k * N, 2 * L * N, k * N
    rng = np.random.default_rng(3)
    words = {"key": keyw, "a": ctw, "b": ctw, "pt": ptw, "o1": ctw, "o2": ctw, "pad": keyw}
    at, pos = {}, 0
    for name, w in words.items():
        at[name], pos = pos, pos + w
    host = rng.integers(0, min(s.primes), pos, dtype=np.uint64)
    slab = e.to_device(host)
    view = lambda off, shape=(2, L, N): slab.view(off, shape)
    key, a, b, pt = view(at["key"], (s.dnum, 2, k, N)), view(at["a"]), view(at["b"]), view(at["pt"], (k, N))
    o1, o2 = view(at["o1"]), view(at["o2"])

    def refused(call):
        with pytest.raises(ValueError, match="overlap"):
            call()
        e.sync()
        assert np.array_equal(slab.download(), host)

    rot = lambda ins, keys, outs: e.hybrid_rotate_hoisted_batch(alpha, L, ins, [3] * len(keys), keys, outs=outs)
    comb = lambda ins, keys, pts, outs: e.hybrid_plain_combine_hoisted(alpha, L, ins, [3] * len(keys), keys, pts, outs=outs)
    for run in (lambda ins, keys, outs: rot(ins, keys, outs), lambda ins, keys, outs: comb(ins, keys, [[pt] * len(ins)] * len(outs), outs)):
        refused(lambda: run([a], [key], [a]))                                             # in place: not allowed here
        refused(lambda: run([a], [key], [view(at["a"] + ctw - N)]))                       # the last row of its input
        refused(lambda: run([a, b], [key], [o1, view(at["b"] - N)]))                      # one row into another source
        refused(lambda: run([a, b], [key], [o1, view(at["o1"] + ctw - N)]))               # two outputs share a row
        refused(lambda: run([a], [key], [view(at["key"] + readw - N)]))                   # the last read row of the key
        refused(lambda: run([a], [view(at["o1"] + ctw - readw, (s.dnum, 2, k, N))], [o1]))  # a key whose read digits end in the output
    refused(lambda: comb([a], [key], [[pt]], [view(at["pt"] + ptw - N)]))                 # the last row of a plaintext
    refused(lambda: comb([a], [key], [[view(at["o1"] - ptw + N, (k, N))]], [o1]))         # a plaintext that ends in the output
    refused(lambda: comb([a], [key], [[pt], [pt]], [o1, view(at["o1"] + N)]))
    # an output on the key's digits that level L does not read runs (dn = 2 of dnum = 3 digits), and writes its output alone
    rot([a], [key], [view(at["key"] + readw)])
    comb([b], [key], [[pt]], [o1])
    e.sync()
    got = slab.download()
    changed = np.zeros(pos, dtype=bool)
    changed[at["key"] + readw: at["key"] + readw + ctw] = changed[at["o1"]: at["o1"] + ctw] = True
    assert np.array_equal(got[~changed], host[~changed]) and not np.array_equal(got[changed], host[changed])
    seg = lambda name, w: host[at[name]: at[name] + w]
    want = HH.combine_model(HC.twin(s), s.primes, alpha, L, [seg("b", ctw)], [3], [seg("key", keyw)], [[seg("pt", ptw).reshape(k, N)]])[0]
    assert np.array_equal(got[at["o1"]: at["o1"] + ctw].reshape(2, L, N), want)


def test_both_entries_return_while_their_stream_is_held_shut():
    """no entry of the header waits on first use: on a fresh context, with (alpha, L) pairs and Galois elements never used before,
    both calls return before the gate opens; after it the words are the model's"""
    from tests.hip_stream_gate import Stream
    s = HC.sets()["k8a3-above60"]
    ctx = HC.context(s, "gpu")                                      # fresh: no constants cached, no scratch yet
    e, N = ctx.backend.engine, s.N
    cts5, elts, keys, pts5 = HH.case(s, 5)
    cts2, _, _, pts2 = HH.case(s, 2)
    d_keys = [up(e, k) for k in keys]
    d5, d2 = [e.to_device(c) for c in cts5], [e.to_device(c) for c in cts2]
    p2 = [[up(e, p) for p in row] for row in pts2]
    o_r, o_c = [e.zeros(2, 5, N) for _ in range(6)], [e.zeros(2, 2, N) for _ in range(2)]
    e.sync()
    with Stream() as st:
        gate = st.gate()
        e.hybrid_rotate_hoisted_batch(s.alpha, 5, d5, elts, d_keys, outs=o_r, stream=st.handle)       # the pair (3, 5), elements 3 and 2N - 1
        assert not gate.opened, "hefx_hybrid_rotate_hoisted_batch waited on the host"
        e.hybrid_plain_combine_hoisted(s.alpha, 2, d2, elts, d_keys, p2, outs=o_c, stream=st.handle)  # a new pair: (3, 2)
        assert not gate.opened, "hefx_hybrid_plain_combine_hoisted waited on the host"
        e.sync(st.handle)
        assert gate.opened
    want_r, want_c = HH.case_models(s, 5)[0], HH.case_models(s, 2)[1]
    assert all(np.array_equal(o.download(), w) for o, w in zip(o_r, want_r))
    assert all(np.array_equal(o.download(), w) for o, w in zip(o_c, want_c))


@pytest.mark.parametrize("which", ["dense", "packed"])
def test_the_hybrid_dft_gives_the_words_of_the_oracle_twin(which):
    """coeffs_to_slots_hybrid and slots_to_coeffs_hybrid (the packed pair: their packed forms) with the plans of the CPU test, on
    the engine and on the twin under the same seeds: every ciphertext word for word, level and scale included"""
    g, o = HH.dft_env("gpu"), HH.dft_env("oracle")
    assert getattr(g["ctx"].backend, "hybrid_plain_combine_hoisted", None) is not None
    assert getattr(o["ctx"].backend, "hybrid_plain_combine_hoisted", None) is None
    results = []
    for e in (g, o):
        hybrid, c2s, s2c, z, want = HH.dft_program(e, which)
        ct = e["enc"].encrypt(e["encoder"].encode(z, HH.DFT_SCALE, parms_id=e["top"]))
        mids, out = hybrid(ct)
        results.append([(c.parms_id(), c.scale, np.asarray(e["ctx"].backend.to_host(c.data)).reshape(2, c.parms_id(), -1)) for c in (*mids, out)])
    assert len(results[0]) == len(results[1]) == (3 if which == "dense" else 2)
    for (Lg, sg, wg), (Lo, so, wo) in zip(*results):
        assert Lg == Lo and sg == so and np.array_equal(wg, wo)
    assert results[0][-1][0] == g["top"] - 2 * HH.DFT_LEVELS


def test_the_front_end_on_the_engine_gives_the_words_of_the_twin():
    """Evaluator.rotate_hoisted and plain_combine_hoisted run the native entries on the engine and the host statement on the twin:
    the same ciphertexts under the same seeds, word for word, level and scale included; a step of zero is a copy"""
    g, o = HH.dft_env("gpu"), HH.dft_env("oracle")
    assert getattr(g["ctx"].backend, "hybrid_rotate_hoisted_batch", None) is not None
    assert getattr(o["ctx"].backend, "hybrid_rotate_hoisted_batch", None) is None
    steps = [0] + g["plans"]["pc2s"].galois_steps()[:2]
    rng = np.random.default_rng(5)
    vals, weights = rng.uniform(-1, 1, (2, g["s"].N // 2)), rng.uniform(-1, 1, (2 * len(steps), g["s"].N // 2))
    words = lambda e, c: (c.parms_id(), c.scale, np.asarray(e["ctx"].backend.to_host(c.data)).reshape(2, c.parms_id(), -1))
    got = []
    for e in (g, o):
        cts = [e["enc"].encrypt(e["encoder"].encode(v, HH.DFT_SCALE, parms_id=e["top"] - 1)) for v in vals]
        rots = e["ev"].rotate_hoisted(cts, steps, e["gk"])
        assert [len(r) for r in rots] == [len(steps)] * 2
        assert np.array_equal(words(e, rots[1][0])[2], words(e, cts[1])[2])
        pts = e["encoder"].encode_many(list(weights), HH.DFT_SCALE, e["s"].k)
        rows = [pts, [None] + pts[1:]]
        outs = e["ev"].plain_combine_hoisted(cts, steps, rows, e["gk"])
        got.append([words(e, c) for r in rots for c in r] + [words(e, c) for c in outs])
    assert len(got[0]) == len(got[1]) == 2 * len(steps) + 2
    for (Lg, sg, wg), (Lo, so, wo) in zip(*got):
        assert Lg == Lo == g["top"] - 1 and sg == so and np.array_equal(wg, wo)


def test_a_call_whose_workspace_passes_one_gib_is_refused_before_anything_is_submitted():
    """N = 32768, k = 12, alpha = 2, L = 10, 8 sources x 8 elements: by the header's row count 80 + 2 * 8 * 5 * 12 + 2 * 64 * 10 +
    2 * 2 * 64 * 2 + 2 * 2 * 64 * 10 = 5392 rows of 256 KiB, 1348 MiB -- HEFX_ERR_UNSUPPORTED, no chunking; one source x 8 elements
    (10 + 120 + 160 + 64 + 320 rows, 169 MiB) runs"""
    from seal_fyp_logistic_regression_amd.capi import HefxError
    s = HC.HSet("k12a2-n32768", 32768, 12, 2, (10,), HC.mix_primes("p50_60", 32768, 12, 2))
    e = HC.context(s, "gpu").backend.engine
    L, N = 10, s.N
    rows = lambda n, m: n * L + 2 * n * 5 * (L + 2) + 2 * n * m * L + 2 * 2 * n * m * 2 + 2 * 2 * n * m * L
    assert rows(8, 8) * N * 8 > 1 << 30 > rows(1, 8) * N * 8
    ct, key = e.to_device(HC.operand(s, "uniform", L, 2, seed=1)), e.to_device(HC.random_key(s, 2))
    outs = [e.zeros(2, L, N) for _ in range(64)]
    elts = [pow(3, i + 1, 2 * N) for i in range(8)]
    with pytest.raises(HefxError, match="passes 1 GiB"):
        e.hybrid_rotate_hoisted_batch(s.alpha, L, [ct] * 8, elts, [key] * 8, outs=outs)
    e.sync()
    assert not outs[0].download().any() and not outs[63].download().any()
    e.hybrid_rotate_hoisted_batch(s.alpha, L, [ct], elts, [key] * 8, outs=outs[:8])
    e.sync()
    assert outs[0].download().any() and outs[7].download().any() and not outs[8].download().any()
