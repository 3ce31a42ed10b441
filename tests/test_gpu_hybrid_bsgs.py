"""The hoisted giant steps on the GPU, word for word (include/hefx_hybrid_bsgs.h): hefx_hybrid_bsgs_hoisted against the integer
statement in Python integers (tests/hybrid_bsgs_cases.py, which tests/test_hybrid_bsgs_cpu.py pins to seal.py's host statement,
to the combine and to the noise bound), the accumulator at its bound, the identities with the combine entry, refusals,
chunking, a caller-owned stream, and the hybrid DFT, EvalMod and bootstrap_hybrid against the oracle twin."""
import numpy as np
import pytest

from tests import bootstrap_cases as BC
from tests import hybrid_bsgs_cases as HB
from tests import hybrid_cases as HC
from tests import hybrid_hoist_cases as HH
from tests import sparse_bootstrap_cases as SC

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


@pytest.mark.parametrize("kind", HB.KINDS)
@pytest.mark.parametrize("name,L", HB.WORD_CASES)
def test_the_entry_gives_the_words_of_the_statement(name, L, kind):
    """2 sources, the baby elements {1 with a NULL key, 3, 2N - 1}, G = 4 inner sums with one structural zero each, O = 2 outputs
    of one unrotated and one giant-rotated inner sum each (giant elements 3 and 2N - 1); big is N = 32768, where every block a
    transform reads is laid out twice; k12a5 runs the unsplit lane loops.  The inputs are only read."""
    s, ctx, e = gpu(name)
    assert L in s.levels
    cts, elts, keys, pts, gelts, gkeys, dest = HB.case(s, L, kind)
    want = HB.case_model(s, L, kind)
    d_cts, d_keys, d_gkeys = [e.to_device(c) for c in cts], [up(e, k) for k in keys], [up(e, k) for k in gkeys]
    d_pts = [[up(e, p) for p in row] for row in pts]
    got = e.hybrid_bsgs_hoisted(s.alpha, L, d_cts, elts, d_keys, d_pts, gelts, d_gkeys, dest)
    assert len(got) == 2
    for q in range(2):
        assert np.array_equal(got[q].download(), want[q]), (name, L, kind, "output", q)
    for d, h in zip(d_cts, cts):
        assert np.array_equal(d.download(), h), "the inputs are only read"
    for d, h in zip(d_gkeys, gkeys):
        assert h is None or np.array_equal(d.download().reshape(-1), h.reshape(-1)), "the giant keys are only read"


def test_sixty_four_rotated_inner_sums_into_one_output_at_the_largest_words():
    """k7a2-p50_60, L = 5: G = 64 inner sums into ONE output, every one giant-rotated with the max key (dn + 1 = 4 steps of the
    lazy range each, 256 in all: the kernel folds on the way), the max operand, plaintexts of q_m - 1"""
    from seal_fyp_logistic_regression_amd import capi
    s, ctx, e = gpu("k7a2-p50_60")
    cts, elts, keys, pts, gelts, gkeys, dest, want = HB.full_case(s, 5)
    assert len(pts) == 64 == capi.HYBRID_HOIST_MAX_OUT and dest == [0] * 64
    ct, key, pt = e.to_device(cts[0]), e.to_device(keys[0]), e.to_device(pts[0][0])
    (out,) = e.hybrid_bsgs_hoisted(s.alpha, 5, [ct], elts, [key, key], [[pt, pt]] * 64, gelts, [key] * 64, dest)
    assert np.array_equal(out.download(), want)


def test_without_giant_keys_the_entry_gives_the_words_of_the_combine_entry():
    """all giant keys NULL: dest the identity is hefx_hybrid_plain_combine_hoisted; all dest 0 is that entry with G = 1 and the
    plaintexts summed mod q_m"""
    s, ctx, e = gpu("k8a3-above60")
    L = 5
    cts, elts, keys, pts, _, _, _ = HB.case(s, L)
    d_cts, d_keys = [e.to_device(c) for c in cts], [up(e, k) for k in keys]
    d_pts = [[up(e, p) for p in row] for row in pts]
    comb = e.hybrid_plain_combine_hoisted(s.alpha, L, d_cts, elts, d_keys, d_pts)
    got = e.hybrid_bsgs_hoisted(s.alpha, L, d_cts, elts, d_keys, d_pts, [1] * 4, [None] * 4, [0, 1, 2, 3])
    assert len(got) == 4 and all(np.array_equal(g.download(), w.download()) for g, w in zip(got, comb))
    summed = []
    for t in range(6):
        live = [row[t] for row in pts if row[t] is not None]
        summed.append(e.to_device(np.stack([(sum(p[m].astype(object) for p in live) % int(s.primes[m])).astype(np.uint64) for m in range(s.k)])))
    (one,) = e.hybrid_plain_combine_hoisted(s.alpha, L, d_cts, elts, d_keys, [summed])
    (got,) = e.hybrid_bsgs_hoisted(s.alpha, L, d_cts, elts, d_keys, d_pts, [1] * 4, [None] * 4, [0] * 4)
    assert np.array_equal(got.download(), one.download())


def test_bad_arguments_and_the_limits_are_refused():
    from seal_fyp_logistic_regression_amd import capi
    s, ctx, e = gpu("k7a2-p50_60")
    N, top = s.N, s.k - s.alpha
    key, pt = e.to_device(HC.random_key(s, 11)), e.zeros(s.k, N)
    ct = lambda L: e.zeros(2, L, N)

    def call(alpha=s.alpha, L=2, cts=None, elts=(3,), keys=None, pts=None, gelts=(3,), gkeys=None, dest=(0,), outs=None):
        cts = [ct(max(L, 1))] if cts is None else cts
        keys = [key] * len(elts) if keys is None else keys
        pts = [[pt] * (len(cts) * len(elts))] * len(gelts) if pts is None else pts
        gkeys = [key] * len(gelts) if gkeys is None else gkeys
        return e.hybrid_bsgs_hoisted(alpha, L, cts, list(elts), keys, pts, list(gelts), gkeys, list(dest), outs=outs)

    for alpha in (0, -1, s.k, 9):
        with pytest.raises(ValueError, match="alpha must be in"):
            call(alpha=alpha, L=1)
    for L in (0, top + 1):
        with pytest.raises(ValueError, match=r"level L must be in \[1, k - alpha\]"):
            call(L=L)
    for elt in (2, 2 * N + 1):
        with pytest.raises(ValueError, match="odd and < 2N"):
            call(elts=(elt,))
        with pytest.raises(ValueError, match="odd and < 2N"):
            call(gelts=(elt,))
    with pytest.raises(ValueError, match="its element must be 1"):        # a NULL key is the identity term
        call(keys=[None])
    with pytest.raises(ValueError, match="NULL giant key"):                # a NULL giant key with an element other than 1
        call(gkeys=[None])
    with pytest.raises(ValueError, match="NULL giant key"):                # and the reverse: a giant key with the element 1
        call(gelts=(1,))
    with pytest.raises(ValueError, match="n < 1 or m < 1"):
        call(cts=[], pts=[[]])
    with pytest.raises(ValueError, match="n < 1 or m < 1"):
        call(elts=(), pts=[[]])

    class Null:
        ptr = None
    with pytest.raises(ValueError, match="null pointer"):
        call(cts=[Null()])
    with pytest.raises(ValueError, match="null pointer"):
        call(outs=[Null()])
    with pytest.raises(ValueError, match="an inner sum has no term"):
        call(gelts=(3, 3), dest=(0, 0), pts=[[pt], [None]])
    with pytest.raises(ValueError, match="dest out of range"):
        call(gelts=(3, 3), dest=(0, 2), outs=[ct(2), ct(2)])
    with pytest.raises(ValueError, match="an output has no inner sum"):
        call(gelts=(3, 3), dest=(1, 1), outs=[ct(2), ct(2)])
    with pytest.raises(ValueError, match="1 <= O <= G"):                    # more outputs than inner sums
        call(outs=[ct(2), ct(2)])
    with pytest.raises(ValueError, match="1 <= O <= G"):
        call(dest=(5,))
    # the limits: 64 terms and 64 inner sums run, 65 do not (L = 1: the smallest workspace)
    c1 = ct(1)
    assert capi.HYBRID_HOIST_MAX_TERMS == 64 == capi.HYBRID_HOIST_MAX_OUT
    assert len(call(L=1, cts=[c1] * 8, elts=(3,) * 8)) == 1
    with pytest.raises(ValueError, match="HEFX_HYBRID_HOIST_MAX_TERMS"):
        call(L=1, cts=[c1] * 5, elts=(3,) * 13)
    assert len(call(L=1, cts=[c1], gelts=(3,) * 64, dest=tuple(range(64)))) == 64
    with pytest.raises(ValueError, match="HEFX_HYBRID_HOIST_MAX_OUT"):
        call(L=1, cts=[c1], gelts=(3,) * 65, dest=(0,) * 65)
    e.sync()


def test_every_byte_overlap_is_refused_and_leaves_the_outputs_untouched():
    """the strict rule of the hoist header, extended to the giant keys' read digits: ValueError with nothing submitted; an
    output on the giant key's digits that level L does not read runs"""
    s, ctx, e = gpu("k7a2-p50_60")
    N, k, L, alpha = s.N, s.k, 3, s.alpha
    dn = (L + alpha - 1) // alpha
    keyw, readw, ctw, ptw = s.dnum * 2 * k * N, dn * 2 * k * N, 2 * L * N, k * N
    rng = np.random.default_rng(3)
    words = {"key": keyw, "gkey": keyw, "a": ctw, "b": ctw, "pt": ptw, "o1": ctw, "o2": ctw, "pad": keyw}
    at, pos = {}, 0
    for name, w in words.items():
        at[name], pos = pos, pos + w
    host = rng.integers(0, min(s.primes), pos, dtype=np.uint64)
    slab = e.to_device(host)
    view = lambda off, shape=(2, L, N): slab.view(off, shape)
    key, gkey = view(at["key"], (s.dnum, 2, k, N)), view(at["gkey"], (s.dnum, 2, k, N))
    a, b, pt = view(at["a"]), view(at["b"]), view(at["pt"], (k, N))
    o1, o2 = view(at["o1"]), view(at["o2"])

    def refused(call):
        with pytest.raises(ValueError, match="overlap"):
            call()
        e.sync()
        assert np.array_equal(slab.download(), host)

    def run(ins, keys, outs, pts=None, gkeys=None):
        G = len(outs)
        pts = [[pt] * len(ins)] * G if pts is None else pts
        return e.hybrid_bsgs_hoisted(alpha, L, ins, [3] * len(keys), keys, pts, [3] * G, [gkey] * G if gkeys is None else gkeys,
                                     list(range(G)), outs=outs)

    refused(lambda: run([a], [key], [a]))                                             # in place: not allowed here
    refused(lambda: run([a], [key], [view(at["a"] + ctw - N)]))                       # the last row of its input
    refused(lambda: run([a, b], [key], [o1, view(at["b"] - N)]))                      # one row into another source
    refused(lambda: run([a, b], [key], [o1, view(at["o1"] + ctw - N)]))               # two outputs share a row
    refused(lambda: run([a], [key], [view(at["key"] + readw - N)]))                   # the last read row of the key
    refused(lambda: run([a], [view(at["o1"] + ctw - readw, (s.dnum, 2, k, N))], [o1]))  # a key whose read digits end in the output
    refused(lambda: run([a], [key], [view(at["gkey"] + readw - N)]))                  # the last read row of the giant key
    refused(lambda: run([a], [key], [o1], gkeys=[view(at["o1"] + ctw - readw, (s.dnum, 2, k, N))]))  # a giant key that ends in the output
    refused(lambda: run([a], [key], [o1, o2], gkeys=[gkey, view(at["o2"] + ctw - readw, (s.dnum, 2, k, N))]))  # the second giant key
    refused(lambda: run([a], [key], [view(at["pt"] + ptw - N)]))                      # the last row of a plaintext
    refused(lambda: run([a], [key], [o1], pts=[[view(at["o1"] - ptw + N, (k, N))]]))  # a plaintext that ends in the output
    # an output on the giant key's digits that level L does not read runs (dn = 2 of dnum = 3 digits), and writes its output alone
    run([a], [key], [view(at["gkey"] + readw)])
    run([b], [key], [o1])
    e.sync()
    got = slab.download()
    changed = np.zeros(pos, dtype=bool)
    changed[at["gkey"] + readw: at["gkey"] + readw + ctw] = changed[at["o1"]: at["o1"] + ctw] = True
    assert np.array_equal(got[~changed], host[~changed]) and not np.array_equal(got[changed], host[changed])
    seg = lambda name, w: host[at[name]: at[name] + w]
    want = HB.bsgs_model(HC.twin(s), s.primes, alpha, L, [seg("b", ctw)], [3], [seg("key", keyw)], [[seg("pt", ptw).reshape(k, N)]],
                         [3], [seg("gkey", keyw)], [0])[0]
    assert np.array_equal(got[at["o1"]: at["o1"] + ctw].reshape(2, L, N), want)


def chunk_set():
    return HC.HSet("k12a2-n32768-l6", 32768, 12, 2, (6, 10), HC.mix_primes("p50_60", 32768, 12, 2))


def test_a_call_that_fits_only_when_chunked_gives_the_words_of_the_statement():
    """N = 32768 (x = 2), alpha = 2, L = 6, dn = 3, one source and one baby element, G = 64 giant-rotated inner sums into O = 2
    outputs.  By the header's row count the fixed blocks take 6 + 2 * 3 * 8 + 2 * 8 + 2 * 64 * 8 + 2 * 2 * 6 + 2 * 2 * 2 * 2 +
    2 * 2 * 2 * 6 = 1182 rows and 64 inner sums in one chunk 64 * (2 + 12 + 12 + 48) = 4736: 5918 rows of 256 KiB, past the 4096
    of 1 GiB; 39 per chunk fit (1182 + 14 * 40 + 60 * 39 = 4082), so the call runs as chunks of 39 and 25.  Two distinct inner
    sums and two giant elements in a pattern of period 3 against 4: the model computes the 4 distinct W and weighs them."""
    s = chunk_set()
    e = HC.context(s, "gpu").backend.engine
    be, L, N, G = HC.twin(s), 6, s.N, 64
    fixed = 6 + 2 * 3 * 8 + 2 * 8 + 2 * G * 8 + 2 * 2 * 6 + 2 * 2 * 2 * 2 + 2 * 2 * 2 * 6
    per = lambda C: (C + C % 2) * 2 + 2 * (C + C % 2) * 6 + 2 * C * 6 + 2 * C * 3 * 8
    assert fixed + per(64) > 4096 >= fixed + per(39) and fixed + per(40) > 4096
    ct, key = HC.operand(s, "uniform", L, 2, seed=1), HC.random_key(s, 2)
    gkeys = [HC.random_key(s, 3), HC.random_key(s, 4)]
    gelts = [3, 2 * N - 1]
    pts = [HH.plaintext(s, "uniform", 5), HH.plaintext(s, "uniform", 6)]
    which = [(o % 2, (o // 2) % 2 if o % 3 else 1 - (o // 2) % 2, o % 3 == 0) for o in range(G)]   # (plaintext, giant, output 0?)
    dest = [0 if z else 1 for _, _, z in which]
    sums = HB.sums_model(s.primes, s.alpha, L, HH.terms_model(be, s.primes, s.alpha, L, [ct], [3], [key]), [[pts[0]], [pts[1]]])
    W = {(p, g): HB.giant_model(be, s.primes, s.alpha, L, sums[p], gelts[g], gkeys[g]) for p in range(2) for g in range(2)}
    kinds = sorted(W)
    weights = lambda out: [sum(1 for (p, g, z), d in zip(which, dest) if (p, g) == kd and d == out) for kd in kinds]
    want = [HB.outputs_model(be, s.primes, s.alpha, L, [W[kd] for kd in kinds], [0] * 4, weights(out))[0] for out in range(2)]
    d_ct, d_key, d_g, d_p = e.to_device(ct), e.to_device(key), [e.to_device(x) for x in gkeys], [e.to_device(x) for x in pts]
    got = e.hybrid_bsgs_hoisted(s.alpha, L, [d_ct], [3], [d_key], [[d_p[p]] for p, _, _ in which], [gelts[g] for _, g, _ in which],
                                [d_g[g] for _, g, _ in which], dest)
    for out in range(2):
        assert np.array_equal(got[out].download(), want[out]), out


def test_a_call_past_one_gib_with_one_inner_sum_per_chunk_is_refused_before_anything_is_submitted():
    """the same ring at L = 10, dn = 5, 8 sources x 8 baby elements, G = 64: the fixed blocks alone take 80 + 2 * 8 * 5 * 12 +
    2 * 64 * 12 + 2 * 64 * 12 + 20 + 8 + 40 = 4180 rows of 256 KiB, past 1 GiB: HEFX_ERR_UNSUPPORTED, nothing written"""
    from seal_fyp_logistic_regression_amd.capi import HefxError
    s = chunk_set()
    e = HC.context(s, "gpu").backend.engine
    L, N = 10, s.N
    assert 80 + 2 * 8 * 5 * 12 + 2 * 64 * 12 + 2 * 64 * 12 + 20 + 8 + 40 > 4096
    ct, key, pt = e.to_device(HC.operand(s, "uniform", L, 2, seed=1)), e.to_device(HC.random_key(s, 2)), e.zeros(s.k, N)
    out = e.zeros(2, L, N)
    elts = [pow(3, i + 1, 2 * N) for i in range(8)]
    with pytest.raises(HefxError, match="passes 1 GiB"):
        e.hybrid_bsgs_hoisted(s.alpha, L, [ct] * 8, elts, [key] * 8, [[pt] * 64] * 64, [3] * 64, [key] * 64, [0] * 64, outs=[out])
    e.sync()
    assert not out.download().any()


def test_the_entry_returns_while_its_stream_is_held_shut():
    """the entry does not wait on first use: on a fresh context, with an (alpha, L) pair and Galois elements never used before,
    the call returns before the gate opens; after it the words are the model's"""
    from tests.hip_stream_gate import Stream
    s = HC.sets()["k8a3-above60"]
    ctx = HC.context(s, "gpu")                                      # fresh: no constants cached, no scratch yet
    e, N = ctx.backend.engine, s.N
    cts, elts, keys, pts, gelts, gkeys, dest = HB.case(s, 5)
    d_cts, d_keys, d_gkeys = [e.to_device(c) for c in cts], [up(e, k) for k in keys], [up(e, k) for k in gkeys]
    d_pts = [[up(e, p) for p in row] for row in pts]
    outs = [e.zeros(2, 5, N) for _ in range(2)]
    e.sync()
    with Stream() as st:
        gate = st.gate()
        e.hybrid_bsgs_hoisted(s.alpha, 5, d_cts, elts, d_keys, d_pts, gelts, d_gkeys, dest, outs=outs, stream=st.handle)
        assert not gate.opened, "hefx_hybrid_bsgs_hoisted waited on the host"
        e.sync(st.handle)
        assert gate.opened
    assert all(np.array_equal(o.download(), w) for o, w in zip(outs, HB.case_model(s, 5)))


# ---- the front end, the DFT, EvalMod and the bootstrap: the engine against the oracle twin ---------------------------------
def words(e, c):
    return c.parms_id(), c.scale, np.asarray(e["ctx"].backend.to_host(c.data)).reshape(c.size(), c.parms_id(), -1)


def fresh_enc(e, seed=77):
    """an encryptor of its own per test and backend: the i-th ciphertext of a seeded Encryptor depends on how many it has made,
    and the shared environments are used by other tests"""
    from seal_fyp_logistic_regression_amd import seal as S
    return S.Encryptor(e["ctx"], e["kg"].public_key(), seed)


def same(got, want):
    assert len(got) == len(want)
    for (Lg, sg, wg), (Lo, so, wo) in zip(got, want):
        assert Lg == Lo and sg == so and np.array_equal(wg, wo)


@pytest.mark.parametrize("which", ["dense", "packed"])
def test_the_hybrid_dft_with_hoisted_giants_gives_the_words_of_the_oracle_twin(which):
    from tests.test_hybrid_bsgs_cpu import dft_hoisted
    g, o = HH.dft_env("gpu"), HH.dft_env("oracle")
    assert getattr(g["ctx"].backend, "hybrid_bsgs_hoisted", None) is not None
    assert getattr(o["ctx"].backend, "hybrid_bsgs_hoisted", None) is None
    results = []
    for e in (g, o):
        _, _, _, z, _ = HH.dft_program(e, which)
        ct = fresh_enc(e).encrypt(e["encoder"].encode(z, HH.DFT_SCALE, parms_id=e["top"]))
        mids, out = dft_hoisted(e, which, True)(ct)
        results.append([words(e, c) for c in (*mids, out)])
        if e is g:      # hoist_giants=False: the words of a call that omits the keyword
            omitted, _, _, _, _ = HH.dft_program(e, which)
            same([words(e, dft_hoisted(e, which, False)(ct)[1])], [words(e, omitted(ct)[1])])
    same(*results)
    assert results[0][-1][0] == g["top"] - 2 * HH.DFT_LEVELS


def test_relinearize_many_on_hybrid_keys_is_one_engine_call_with_the_words_of_the_loop():
    from seal_fyp_logistic_regression_amd import seal as S
    e = HB.boot_env("gpu")
    ctx, rk, L = e["ctx"], e["hrk"], 6
    s = HC.HSet("boot", BC.N, ctx.k, HB.BOOT_ALPHA, (L,), ctx.primes)
    make = lambda: [S.Ciphertext()._set(ctx.backend.from_host(HC.operand(s, "uniform", L, 3, seed=60 + i)), 3, L, BC.SCALE) for i in range(3)]
    loop = [e["ev"].relinearize_inplace(c, rk) for c in make()]
    calls, real = [], ctx.backend.hybrid_relinearize_batch

    class Counting:
        def __getattr__(self, name):
            return getattr(ctx.backend, name)

        def hybrid_relinearize_batch(self, alpha, L_, ct3s, key):
            calls.append(len(ct3s))
            return real(alpha, L_, ct3s, key)
    ev = S.Evaluator(ctx)
    ev.be = Counting()
    batch = ev.relinearize_many_inplace(make(), rk)
    assert calls == [3]
    same([words(e, c) for c in batch], [words(e, c) for c in loop])


@pytest.mark.parametrize("lazy", [True, False], ids=["lazy", "eager"])
def test_eval_mod_hybrid_gives_the_words_of_the_oracle_twin(lazy):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    got = []
    for kind in ("gpu", "oracle"):
        e = HB.boot_env(kind)
        plan = e["plan"]
        u = np.random.default_rng(9).uniform(-0.4, 0.4, BC.N // 2)
        ct = fresh_enc(e).encrypt(e["encoder"].encode(u, BC.SCALE, parms_id=plan.evalmod_level))
        ys = alg.eval_mod_hybrid(e["ev"], [ct, ct.copy()], plan, e["hrk"], lazy=lazy)
        assert len(ys) == 2 and ys[0].parms_id() == plan.s2c_level
        got.append([words(e, y) for y in ys])
    same(*got)


@pytest.mark.parametrize("hoist", [True, False], ids=["hoisted", "unhoisted"])
def test_the_sparse_bootstrap_hybrid_gives_the_words_of_the_oracle_twin(hoist):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    got = []
    for kind in ("gpu", "oracle"):
        e = HB.boot_env(kind)
        plan = e["plan"]
        v = SC.sparse_input(HB.BOOT_NS)
        ct = fresh_enc(e).encrypt(e["encoder"].encode(SC.tiled(v), BC.SCALE, parms_id=1))
        if kind == "oracle":
            _, I = BC.raised_coefficients(e, ct, plan.top_level)
            assert np.abs(I).max() <= plan.K                                # a condition on the input
        out = alg.bootstrap_hybrid(e["ev"], ct, plan, e["hgk"], e["hrk"], e["encoded"], hoist_giants=hoist)
        assert out.size() == 2 and out.parms_id() == plan.result_level
        got.append([words(e, out)])
        if kind == "gpu":
            dec = e["encoder"].decode(e["dec"].decrypt(out))
            err = float(np.abs(dec[:HB.BOOT_NS] - v).max() / np.abs(v).max())
            print(f"[hybrid bsgs gpu] sparse bootstrap_hybrid, giants {'hoisted' if hoist else 'not hoisted'}: error {err:.3e}")
            assert err <= BC.CAP
    same(*got)
