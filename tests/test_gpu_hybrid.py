"""Hybrid key switching on the GPU, word for word (include/hefx_hybrid.h): hefx_hybrid_keygen against the key composed on the
oracle twin, hefx_hybrid_apply_galois_batch / hefx_hybrid_relinearize_batch against the integer statement in Python integers
(tests/hybrid_cases.py, which tests/test_hybrid_cpu.py pins to the oracle at alpha = 1 and holds to the noise bound above it),
at alpha = 1 also against the engine's own hefx_apply_galois_batch / hefx_relinearize_batch; batches, chunks, aliasing,
a caller-owned stream, and seal.py end to end.  N = 2048 for every set but "big" (N = 32768: the split transforms) and the wide
sets of tests/hybrid_cases.py: alpha up to 8, up to nine digits and the chain of 61, every ring size up to 32768.  The batch tests
assert through HC.split_of and HC.chunk_of -- the launch rules restated -- that they run every split and cross a chunk."""
import numpy as np
import pytest

from tests import hybrid_cases as HC

pytestmark = pytest.mark.gpu

_GPU = {}


def gpu(name):
    """(set, context, engine) on the HIP engine, once per set"""
    if name not in _GPU:
        s = HC.sets()[name]
        ctx = HC.context(s, "gpu")
        _GPU[name] = (s, ctx, ctx.backend.engine)
    return _GPU[name]


_KEYS = {}


def dev_key(name, kind="uniform"):
    """the key of a set's word cases on the device, once per set and key kind"""
    if (name, kind) not in _KEYS:
        s, ctx, e = gpu(name)
        _KEYS[name, kind] = e.to_device(HC.case_key(s, kind))
    return _KEYS[name, kind]


def run_case(e, s, case, key_dev):
    L, form, kind, elt, _ = case
    ct = e.to_device(HC.case_input(s, case))
    if form == "galois":
        (out,) = e.hybrid_apply_galois_batch(s.alpha, L, [ct], [elt], [key_dev])
    else:
        (out,) = e.hybrid_relinearize_batch(s.alpha, L, [ct], key_dev)
    assert np.array_equal(ct.download(), HC.case_input(s, case)), "the input is only read"
    return out.download()


@pytest.mark.parametrize("name", HC.SET_NAMES)
def test_keygen_gives_the_words_of_the_key_composed_on_the_twin(name):
    from seal_fyp_logistic_regression_amd import seal as S
    s, ctx, e = gpu(name)
    assert e.hybrid_digits(s.alpha) == s.dnum
    kg, ko = S.KeyGenerator(ctx, 3), S.KeyGenerator(HC.context(s, "oracle"), 3)
    assert getattr(ctx.backend, "hybrid_keygen", None) is not None and getattr(ko.ctx.backend, "hybrid_keygen", None) is None
    for make in (lambda g: g.hybrid_relin_keys(s.alpha).hybrid_key(0), lambda g: g.hybrid_galois_keys(s.alpha, [1]).hybrid_key(3)):
        got, want = make(kg), make(ko)
        assert got.shape == (s.dnum, 2, s.k, s.N)
        assert np.array_equal(got.download().reshape(-1), np.asarray(want).reshape(-1)), name


@pytest.mark.parametrize("name", HC.SET_NAMES)
def test_the_entries_give_the_words_of_the_statement(name):
    s, ctx, e = gpu(name)
    for case in HC.word_cases(s):
        assert np.array_equal(run_case(e, s, case, dev_key(name, case[4])), HC.case_model(s, case)), (name, case)


@pytest.mark.parametrize("name", HC.LONG_SET_NAMES)
def test_the_longest_chain_gives_the_words_of_the_statement(name):
    """k = 62, alpha = 1, L = 61 on the largest primes the context takes, operand and key at q - 1: the MAC sums 61 products, the
    count its bound "below 2^128" is written for, each the largest a word pair gives"""
    s, ctx, e = gpu(name)
    (case,) = HC.word_cases(s)
    assert case[0] == 61 == s.dnum and case[2] == case[4] == "max" and min(s.primes) >> 60 == 1
    key = e.to_device(HC.case_key(s, "max"))      # 118 MiB: not kept
    assert np.array_equal(run_case(e, s, case, key), HC.case_model(s, case)), (name, case)


@pytest.mark.parametrize("name", HC.ALPHA_ONE_SET_NAMES, ids=HC.ALPHA_ONE_IDS)
def test_at_alpha_one_the_entries_give_the_words_of_the_existing_key_switch(name):
    s, ctx, e = gpu(name)
    assert s.alpha == 1
    for case in HC.word_cases(s):
        L, form, kind, elt, key_kind = case
        ct, key = e.to_device(HC.case_input(s, case)), dev_key(name, key_kind)
        if form == "galois":
            (want,) = e.apply_galois_batch(L, [ct], [elt], [key])
        else:
            (want,) = e.relinearize_batch(L, [ct], key)
        assert np.array_equal(run_case(e, s, case, key), want.download()), (name, case)


def test_a_batch_with_a_shared_key_an_in_place_item_and_mixed_elements_equals_single_calls():
    s, ctx, e = gpu("k7a2-p50_60")
    L, N = 4, s.N
    k3, kc = e.to_device(HC.random_key(s, 11)), e.to_device(HC.random_key(s, 12))
    ins = [HC.operand(s, "uniform", L, 2, seed=20 + i) for i in range(3)]
    elts, keys = [3, 2 * N - 1, 3], [k3, kc, k3]
    singles = [e.hybrid_apply_galois_batch(s.alpha, L, [e.to_device(x)], [g], [k])[0].download() for x, g, k in zip(ins, elts, keys)]
    for x, g, k, w in zip(ins, elts, keys, singles):
        assert np.array_equal(w, HC.apply_galois_model(HC.twin(s), s.primes, s.alpha, L, x, g, HC.random_key(s, 11 if g == 3 else 12)))
    devs = [e.to_device(x) for x in ins]
    outs = [e.zeros(2, L, N), devs[1], e.zeros(2, L, N)]            # item 1 in place
    got = e.hybrid_apply_galois_batch(s.alpha, L, devs, elts, keys, outs=outs)
    for i in range(3):
        assert np.array_equal(got[i].download(), singles[i]), i
    assert np.array_equal(devs[0].download(), ins[0]) and np.array_equal(devs[2].download(), ins[2])
    r3 = [HC.operand(s, "uniform", L, 3, seed=30 + i) for i in range(3)]
    rs = [e.hybrid_relinearize_batch(s.alpha, L, [e.to_device(x)], k3)[0].download() for x in r3]
    rb = e.hybrid_relinearize_batch(s.alpha, L, [e.to_device(x) for x in r3], k3)
    for i in range(3):
        assert np.array_equal(rb[i].download(), rs[i]), i


def test_a_batch_longer_than_a_chunk_equals_single_calls():
    """at L = 1 a chunk takes 1024 items (the descriptor slot): 1030 items run as two chunks through the same scratch"""
    s, ctx, e = gpu("k7a2-p50_60")
    L, N, n = 1, s.N, 1030
    key = e.to_device(HC.random_key(s, 11))
    ins = [e.to_device(HC.operand(s, "uniform", L, 2, seed=40 + i)) for i in range(3)]
    want = [e.hybrid_apply_galois_batch(s.alpha, L, [x], [3], [key])[0].download() for x in ins]
    slab = e.zeros(n, 2, L, N)
    outs = [slab.view(i * 2 * L * N, (2, L, N)) for i in range(n)]
    e.hybrid_apply_galois_batch(s.alpha, L, [ins[i % 3] for i in range(n)], [3] * n, [key] * n, outs=outs)
    got = slab.download()
    for i in (0, 1, 2, 511, 1023, 1024, 1025, 1029):
        assert np.array_equal(got[i], want[i % 3]), i
    assert all(np.array_equal(got[i], want[i % 3]) for i in range(n))


def test_bad_arguments_are_refused():
    s, ctx, e = gpu("k7a2-p50_60")
    N, top = s.N, s.k - s.alpha
    key = e.to_device(HC.random_key(s, 11))
    ct = lambda L, size=2: e.zeros(size, L, N)
    for alpha in (0, -1, s.k, 9):
        with pytest.raises(ValueError, match="alpha must be in"):
            e.hybrid_apply_galois_batch(alpha, 1, [ct(1)], [3], [key])
        with pytest.raises(ValueError, match="alpha must be in"):
            e.hybrid_digits(alpha)
        with pytest.raises(ValueError, match="alpha must be in"):
            e.hybrid_keygen(alpha, ct(s.k, 1), ct(s.k, 1), bytes(32), 1, out=e.zeros(1, 2, s.k, N))
    for L in (0, top + 1):
        with pytest.raises(ValueError, match=r"level L must be in \[1, k - alpha\]"):
            e.hybrid_apply_galois_batch(s.alpha, L, [ct(max(L, 1))], [3], [key])
        with pytest.raises(ValueError, match=r"level L must be in \[1, k - alpha\]"):
            e.hybrid_relinearize_batch(s.alpha, L, [ct(max(L, 1), 3)], key)
    for elt in (2, 2 * N + 1):
        with pytest.raises(ValueError, match="odd and < 2N"):
            e.hybrid_apply_galois_batch(s.alpha, 2, [ct(2)], [elt], [key])

    class Null:
        ptr = None
    with pytest.raises(ValueError, match="null pointer"):
        e.hybrid_apply_galois_batch(s.alpha, 2, [ct(2)], [3], [Null()])
    with pytest.raises(ValueError, match="null pointer"):
        e.hybrid_relinearize_batch(s.alpha, 2, [Null()], key, outs=[ct(2)])


def test_every_other_byte_overlap_is_refused_and_leaves_the_outputs_untouched():
    """the aliasing rule of hefx_apply_galois_batch / hefx_relinearize: the exact in-place Galois item runs (tested above), any
    other overlap of an output with an output, an input or the read digits of a key is ValueError with nothing submitted"""
    s, ctx, e = gpu("k7a2-p50_60")
    N, k, L, alpha = s.N, s.k, 3, s.alpha
    dn = (L + alpha - 1) // alpha
    keyw, readw, ctw = s.dnum * 2 * k * N, dn * 2 * k * N, 2 * L * N
    rng = np.random.default_rng(3)
    words = {"key": keyw, "a": 3 * L * N, "b": 3 * L * N, "o1": ctw, "o2": ctw, "pad": keyw}
    at, pos = {}, 0
    for name, w in words.items():
        at[name], pos = pos, pos + w
    host = rng.integers(0, min(s.primes), pos, dtype=np.uint64)
    slab = e.to_device(host)
    view = lambda off, shape: slab.view(off, shape)
    key = view(at["key"], (s.dnum, 2, k, N))
    a2, b2, a3 = view(at["a"], (2, L, N)), view(at["b"], (2, L, N)), view(at["a"], (3, L, N))
    o1, o2 = view(at["o1"], (2, L, N)), view(at["o2"], (2, L, N))

    def refused(call):
        with pytest.raises(ValueError, match="overlap|independent"):
            call()
        e.sync()
        assert np.array_equal(slab.download(), host)

    gal = lambda ins, keys, outs: e.hybrid_apply_galois_batch(alpha, L, ins, [3] * len(ins), keys, outs=outs)
    rel = lambda ins, kk, outs: e.hybrid_relinearize_batch(alpha, L, ins, kk, outs=outs)
    refused(lambda: gal([a2], [key], [view(at["a"] + N, (2, L, N))]))                       # one row into its own input
    refused(lambda: gal([a2, b2], [key, key], [o1, view(at["a"], (2, L, N))]))              # another item's input, exactly
    refused(lambda: gal([a2, b2], [key, key], [o1, view(at["o1"] + ctw - N, (2, L, N))]))   # two outputs share a row
    refused(lambda: gal([a2], [key], [view(at["key"] + readw - N, (2, L, N))]))             # the last read row of the key
    refused(lambda: gal([a2], [key], [view(at["key"], (2, L, N))]))
    refused(lambda: gal([a2], [view(at["o1"] + ctw - readw, (s.dnum, 2, k, N))], [o1]))     # a key whose read digits end in the output
    refused(lambda: rel([a3], key, [view(at["a"], (2, L, N))]))                             # relinearisation: no in-place form
    refused(lambda: rel([a3], key, [view(at["a"] + 2 * L * N, (2, L, N))]))                 # on c2
    refused(lambda: rel([a3], key, [view(at["key"] + readw - N, (2, L, N))]))
    # an output on the key's digits that level L does not read runs (dn = 2 of dnum = 3 digits), and writes its output alone
    beyond = view(at["key"] + readw, (2, L, N))
    gal([a2], [key], [beyond])
    gal([b2], [key], [o1])
    e.sync()
    got = slab.download()
    changed = np.zeros(pos, dtype=bool)
    changed[at["key"] + readw: at["key"] + readw + ctw] = changed[at["o1"]: at["o1"] + ctw] = True
    assert np.array_equal(got[~changed], host[~changed]) and not np.array_equal(got[changed], host[changed])
    want = HC.apply_galois_model(HC.twin(s), s.primes, alpha, L, host[at["b"]: at["b"] + ctw], 3, host[at["key"]: at["key"] + keyw])
    assert np.array_equal(got[at["o1"]: at["o1"] + ctw].reshape(2, L, N), want)


def test_the_entries_return_while_their_stream_is_held_shut():
    """the header lists no entry as waiting on first use: on a fresh context, with (alpha, L) pairs and a Galois element never used
    before, every call returns before the gate opens; after it the words are the model's"""
    from tests.hip_stream_gate import Stream
    from seal_fyp_logistic_regression_amd import seal as S
    s = HC.sets()["k8a3-p50_60"]
    ctx = HC.context(s, "gpu")                                      # fresh: no constants cached, no scratch yet
    e, N = ctx.backend.engine, s.N
    kg = S.KeyGenerator(ctx, 3)
    sk = kg.secret_key().data
    key_host = HC.random_key(s, HC.SEED)
    key, L = e.to_device(key_host), 5
    c2, c3 = HC.operand(s, "uniform", L, 2, seed=1), HC.operand(s, "uniform", L, 3, seed=2)
    d2, d3 = e.to_device(c2), e.to_device(c3)
    o_g, o_r, o_k = e.zeros(2, L, N), e.zeros(2, L, N), e.zeros(s.dnum, 2, s.k, N)
    e.sync()
    with Stream() as st:
        gate = st.gate()
        e.hybrid_apply_galois_batch(s.alpha, L, [d2], [2 * N - 1], [key], outs=[o_g], stream=st.handle)
        assert not gate.opened, "hefx_hybrid_apply_galois_batch waited on the host"
        e.hybrid_relinearize_batch(s.alpha, L, [d3], key, outs=[o_r], stream=st.handle)
        assert not gate.opened, "hefx_hybrid_relinearize_batch waited on the host"
        e.hybrid_keygen(s.alpha, sk, sk, bytes(range(32)), 7, out=o_k, stream=st.handle)
        assert not gate.opened, "hefx_hybrid_keygen waited on the host"
        e.sync(st.handle)
        assert gate.opened
    be = HC.twin(s)
    assert np.array_equal(o_g.download(), HC.apply_galois_model(be, s.primes, s.alpha, L, c2, 2 * N - 1, key_host))
    assert np.array_equal(o_r.download(), HC.relinearize_model(be, s.primes, s.alpha, L, c3, key_host))
    assert np.array_equal(o_k.download(), e.hybrid_keygen(s.alpha, sk, sk, bytes(range(32)), 7).download())


def test_end_to_end_through_seal_with_hybrid_keys():
    """encrypt, rotate_vector, multiply, relinearize with HybridKeys at k = 7, alpha = 2, rescale, decode: the twin's words, and
    a decode error within HC.E2E_FACTOR times the twin's own (the derivation HC.end_to_end names)"""
    s = HC.sets()[HC.E2E_SET]
    eg, eo = HC.make_env(s, "gpu"), HC.make_env(s, "oracle")
    for name in ("gk", "rk"):
        for idx in eg[name].keys:
            assert np.array_equal(eg[name].hybrid_key(idx).download().reshape(-1), np.asarray(eo[name].hybrid_key(idx)).reshape(-1))
    cg, err_g = HC.end_to_end(eg)
    co, err_o = HC.end_to_end(eo)
    assert cg.size() == co.size() == 2 and cg.parms_id() == co.parms_id() == s.k - s.alpha - 1 and cg.scale == co.scale
    assert np.array_equal(cg.data.download().reshape(-1), np.asarray(co.data).reshape(-1))
    print(f"[gpu hybrid] end to end at {s.name}: words equal; decode error engine {err_g:.3e}, twin {err_o:.3e}, "
          f"allowance {HC.E2E_FACTOR * err_o:.3e}")
    assert err_g <= HC.E2E_FACTOR * err_o
    # a level above k - alpha is refused by the front end, KSwitchKeys still run the existing entries
    top = eg["enc"].encrypt(eg["encoder"].encode(HC.e2e_values(s.N)[0], HC.E2E_SCALE))
    with pytest.raises(ValueError, match="level <= k - alpha"):
        eg["ev"].rotate_vector(top, 1, eg["gk"])


# ---------------------------------------------------------------------------------------------------------------------
# batches at the launch shapes: three items of a set -- the elements 3, 2N - 1 and 1, the second on a key of its own -- and three
# relinearisations, their single-item results computed once per (set, level) and shared
# ---------------------------------------------------------------------------------------------------------------------
_TRIOS = {}


def trio(name, L):
    if (name, L) not in _TRIOS:
        s, ctx, e = gpu(name)
        host_keys = [HC.random_key(s, 11), HC.random_key(s, 12)]
        dev_keys, which = [e.to_device(h) for h in host_keys], (0, 1, 0)
        t = dict(elts=[3, 2 * s.N - 1, 1], keys=[dev_keys[w] for w in which], host_keys=[host_keys[w] for w in which],
                 ins=[HC.operand(s, "uniform", L, 2, seed=50 + i) for i in range(3)],
                 ins3=[HC.operand(s, "uniform", L, 3, seed=60 + i) for i in range(3)])
        t["devs"], t["devs3"] = [e.to_device(x) for x in t["ins"]], [e.to_device(x) for x in t["ins3"]]
        t["singles"] = [e.hybrid_apply_galois_batch(s.alpha, L, [d], [g], [k])[0].download() for d, g, k in zip(t["devs"], t["elts"], t["keys"])]
        t["singles3"] = [e.hybrid_relinearize_batch(s.alpha, L, [d], t["keys"][0])[0].download() for d in t["devs3"]]
        _TRIOS[name, L] = t
    return _TRIOS[name, L]


def check_galois_batch(name, L, n):
    """n items that cycle through the trio's inputs, elements and keys; the outputs are views of one slab, item min(1, n - 1) runs
    in place on its view; one download, every item against its single-item call"""
    s, ctx, e = gpu(name)
    t, words, shape = trio(name, L), 2 * L * s.N, (2, L, s.N)
    slab = e.zeros(n, *shape)
    outs = [slab.view(i * words, shape) for i in range(n)]
    cts, in_place = [t["devs"][i % 3] for i in range(n)], min(1, n - 1)
    cts[in_place] = outs[in_place].upload(t["ins"][in_place % 3])
    e.hybrid_apply_galois_batch(s.alpha, L, cts, [t["elts"][i % 3] for i in range(n)], [t["keys"][i % 3] for i in range(n)], outs=outs)
    got = slab.download()
    for i in range(n):
        assert np.array_equal(got[i], t["singles"][i % 3]), (name, L, n, i)
    for d, x in zip(t["devs"], t["ins"]):
        assert np.array_equal(d.download(), x), "the shared inputs are only read"


def check_relin_batch(name, L, n):
    s, ctx, e = gpu(name)
    t, words, shape = trio(name, L), 2 * L * s.N, (2, L, s.N)
    slab = e.zeros(n, *shape)
    e.hybrid_relinearize_batch(s.alpha, L, [t["devs3"][i % 3] for i in range(n)], t["keys"][0], outs=[slab.view(i * words, shape) for i in range(n)])
    got = slab.download()
    for i in range(n):
        assert np.array_equal(got[i], t["singles3"][i % 3]), (name, L, n, i)


def check_singles_against_the_model(name, L):
    s, t = HC.sets()[name], trio(name, L)
    for x, g, k, w in zip(t["ins"], t["elts"], t["host_keys"], t["singles"]):
        assert np.array_equal(w, HC.apply_galois_model(HC.twin(s), s.primes, s.alpha, L, x, g, k)), (name, L, g)
    for x, w in zip(t["ins3"], t["singles3"]):
        assert np.array_equal(w, HC.relinearize_model(HC.twin(s), s.primes, s.alpha, L, x, t["host_keys"][0])), (name, L)


SWEEP = (1, 43, 64, 86, 128)


def test_batches_at_every_split_of_the_lane_loops_equal_single_calls():
    """k7a2 at L = 5: three digits, the last of one prime; convert walks R = 7 targets, spread L = 5 -- neither a multiple of 2 or 4,
    so the split parts are uneven (2, 2, 2, 1 and 2, 2, 1, 0 rows).  The batch sizes are chosen so that BOTH passes run split 4, 2
    and 1 -- asserted from the restated rule, not assumed: at 128 items both run the production form, one lane walking every
    target of several digits"""
    name, L = "k7a2-p50_60", 5
    s, ctx, e = gpu(name)
    splits = [(HC.convert_split(s.N, s.alpha, L, n), HC.spread_split(s.N, L, n)) for n in SWEEP]
    assert {c for c, _ in splits} == {1, 2, 4} and {p for _, p in splits} == {1, 2, 4}, splits
    assert splits[0] == (4, 4) and splits[-1] == (1, 1) and (L + s.alpha) % 2 == L % 2 == 1, splits
    assert max(SWEEP) <= HC.chunk_of(s.N, s.alpha, L), "every batch is one chunk"
    check_singles_against_the_model(name, L)
    for n in SWEEP:
        check_galois_batch(name, L, n)
    assert HC.spread_split(s.N, L, 128) == 1
    check_relin_batch(name, L, 128)


def test_a_batch_at_alpha_five_with_unsplit_lane_loops_equals_single_calls():
    """k12a5 at L = 7 (digits of 5 and 2 rows), 128 items: hy_convert_kernel<5> and hy_spread_kernel<5> with split = 1"""
    name, L, n = "k12a5-p50_60", 7, 128
    s, ctx, e = gpu(name)
    assert s.alpha == 5 and (HC.convert_split(s.N, s.alpha, L, n), HC.spread_split(s.N, L, n)) == (1, 1) and n <= HC.chunk_of(s.N, s.alpha, L)
    check_singles_against_the_model(name, L)
    check_galois_batch(name, L, n)
    check_relin_batch(name, L, n)


def test_at_n_32768_a_mixed_batch_equals_single_calls():
    """big7 at L = 5: three items and three digits, the last partial -- every block a transform reads is laid out twice (xf_raw)
    for cnt = 3 items, and the split transforms run over cnt * dn = 9 polynomials; two keys, three elements, one item in place"""
    name, L = "big7", 5
    s, ctx, e = gpu(name)
    assert s.N == 32768 and HC.item_rows(s.N, s.alpha, L) == 95
    check_galois_batch(name, L, 3)
    check_relin_batch(name, L, 3)


def test_at_n_32768_a_batch_past_the_scratch_rule_equals_single_calls():
    """50 items where a chunk's scratch (95 rows of 256 KiB an item) stays below 1 GiB up to 43: the batch runs as 43 + 7 through
    the same scratch -- the byte rule of hybrid_run, not the descriptor cap"""
    name, L, n = "big7", 5, 50
    s, ctx, e = gpu(name)
    assert HC.chunk_of(s.N, s.alpha, L) == 43 < n < HC.KS_MAX_CHUNK
    check_galois_batch(name, L, n)


@pytest.mark.parametrize("name", ["k7a2-p50_60", "n8192"])
def test_the_elements_of_rotations_and_elements_with_the_n_bit_set(name):
    """hy_gather computes the automorphism's index in the kernel and swaps the halves of a record by the parity of the source
    index: powers of 5 (small, the last one of the cycle, the one of order two), elements with the N bit set and without, next
    to 2N; one batch on one key, two of the items in place"""
    s, ctx, e = gpu(name)
    L, N = 2, s.N
    elts = [5, 25, pow(5, N // 2 - 1, 2 * N), pow(5, N // 4, 2 * N), N + 1, N - 1, 2 * N - 3]
    assert all(g % 2 == 1 and 1 < g < 2 * N for g in elts) and elts[2] * 5 % (2 * N) == 1 and sum(1 for g in elts if g & N) >= 3
    ins = [HC.operand(s, "uniform", L, 2, seed=70 + i) for i in range(len(elts))]
    devs = [e.to_device(x) for x in ins]
    outs = [devs[i] if i in (2, 4) else e.zeros(2, L, N) for i in range(len(elts))]
    got = e.hybrid_apply_galois_batch(s.alpha, L, devs, elts, [dev_key(name)] * len(elts), outs=outs)
    for i, g in enumerate(elts):
        want = HC.apply_galois_model(HC.twin(s), s.primes, s.alpha, L, ins[i], g, HC.case_key(s, "uniform"))
        assert np.array_equal(got[i].download(), want), (name, g)
        assert i in (2, 4) or np.array_equal(devs[i].download(), ins[i]), (name, g)


# ---------------------------------------------------------------------------------------------------------------------
# the front end and the engine's own keys
# ---------------------------------------------------------------------------------------------------------------------
def front_end_run(s, kind):
    """the Evaluator's methods that route on HybridKeys, on a ciphertext of seeded words at the top hybrid level: name ->
    (words, parms_id, scale), and the words of the out-of-place calls' input afterwards"""
    from seal_fyp_logistic_regression_amd import seal as S
    ctx = gpu(s.name)[1] if kind == "gpu" else HC.context(s, kind)
    be, L, scale = ctx.backend, s.k - s.alpha, 2.0 ** 40
    kg, ev = S.KeyGenerator(ctx, 3), S.Evaluator(ctx)
    gk = kg.hybrid_galois_keys(s.alpha, [1, -1, 4], conjugate=True)
    sw = kg.hybrid_switching_key(s.alpha, S.KeyGenerator(ctx, 4).secret_key())
    hops = ev.rotation_plan(3, gk)
    assert not gk.has_key(S.galois_elt_from_step(3, s.N)) and len(hops) == 2 and all(gk.has_key(g) for g in hops)
    host = HC.operand(s, "uniform", L, 2, seed=80)
    fresh = lambda: S.Ciphertext()._set(be.from_host(host), 2, L, scale)
    words = lambda c: np.asarray(be.to_host(c.data), dtype=np.uint64).reshape(c.size(), L, s.N)
    ct, out = fresh(), {}
    out["apply_galois"] = ev.apply_galois(ct, 3, gk)
    out["complex_conjugate"] = ev.complex_conjugate(ct, gk)
    out["switch_key"] = ev.switch_key(ct, sw)
    out["rotate_vector"] = ev.rotate_vector(ct, 3, gk)
    assert np.array_equal(words(ct), host) and ct.parms_id() == L and ct.scale == scale, "the out-of-place calls only read their input"
    inplace = fresh()
    assert ev.rotate_vector_inplace(inplace, 3, gk) is inplace
    out["rotate_vector_inplace"] = inplace
    return {name: (words(c), c.parms_id(), c.scale) for name, c in out.items()}, L, scale


def test_the_front_end_routes_on_hybrid_keys_as_the_twin_does():
    """apply_galois, complex_conjugate, switch_key (a key between two secrets), a rotation of two hops and its in-place form with
    HybridKeys on the engine: the words, parms_id and scale of the same calls on the oracle twin under the same seeds"""
    s = HC.sets()[HC.E2E_SET]
    got, L, scale = front_end_run(s, "gpu")
    want, _, _ = front_end_run(s, "oracle")
    assert sorted(got) == sorted(want) and len(got) == 5
    for name in want:
        assert got[name][1:] == want[name][1:] == (L, scale), name
        assert np.array_equal(got[name][0], want[name][0]), name
    assert np.array_equal(got["rotate_vector_inplace"][0], got["rotate_vector"][0])
    assert not np.array_equal(got["rotate_vector"][0], got["apply_galois"][0])


@pytest.mark.parametrize("name,L", [("k18a8-p50_60", 10), ("k14a2-above60", 11)])
def test_the_engine_keeps_the_noise_bound_under_its_own_keys(name, L):
    """keys from hefx_hybrid_keygen, the switch on the engine, the decryption in exact integers (HC.switch_noise): the noise of
    tests/test_hybrid_cpu.py's model test, at alpha = 8 with a partial digit and at six digits"""
    from seal_fyp_logistic_regression_amd import seal as S
    s, ctx, e = gpu(name)
    assert getattr(ctx.backend, "hybrid_keygen", None) is not None
    kg = S.KeyGenerator(ctx, 3)
    gk, rk, sk = kg.hybrid_galois_keys(s.alpha, [1], conjugate=True), kg.hybrid_relin_keys(s.alpha), kg.secret_key().host
    B, Q = HC.noise_bound(s, L)
    worst = 0
    for form, kind, elt in (("galois", "uniform", 3), ("galois", "max", 2 * s.N - 1), ("relin", "uniform", 0)):
        ct = HC.operand(s, kind, L, 2 if form == "galois" else 3, seed=41 + L)
        if form == "galois":
            (out,) = e.hybrid_apply_galois_batch(s.alpha, L, [e.to_device(ct)], [elt], [gk.hybrid_key(elt)])
        else:
            (out,) = e.hybrid_relinearize_batch(s.alpha, L, [e.to_device(ct)], rk.hybrid_key(0))
        noise, Q_ = HC.switch_noise(s, L, form, elt, ct, out.download(), sk)
        assert Q_ == Q
        worst = max(worst, noise)
    print(f"[gpu hybrid] {name} L = {L}: noise {worst} under the engine's own keys (bound {B}, Q_L / 4 = 2^{(Q // 4).bit_length() - 1})")
    assert worst <= B
