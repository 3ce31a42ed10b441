"""Hybrid key switching on the GPU, word for word (include/hefx_hybrid.h): hefx_hybrid_keygen against the key composed on the
oracle twin, hefx_hybrid_apply_galois_batch / hefx_hybrid_relinearize_batch against the integer statement in Python integers
(tests/hybrid_cases.py, which tests/test_hybrid_cpu.py pins to the oracle at alpha = 1 and holds to the noise bound above it),
at alpha = 1 also against the engine's own hefx_apply_galois_batch / hefx_relinearize_batch; batches, chunks, aliasing,
a caller-owned stream, and seal.py end to end.  N = 2048 for every set but "big" (N = 32768: the split transforms)."""
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


def run_case(e, s, case, key_dev):
    L, form, kind, elt = case
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
    key = e.to_device(HC.random_key(s, HC.SEED))
    for case in HC.word_cases(s):
        assert np.array_equal(run_case(e, s, case, key), HC.case_model(s, case)), (name, case)


@pytest.mark.parametrize("mix", HC.MIXES)
def test_at_alpha_one_the_entries_give_the_words_of_the_existing_key_switch(mix):
    s, ctx, e = gpu(f"k4a1-{mix}")
    key = e.to_device(HC.random_key(s, HC.SEED))
    for case in HC.word_cases(s):
        L, form, kind, elt = case
        ct = e.to_device(HC.case_input(s, case))
        if form == "galois":
            (want,) = e.apply_galois_batch(L, [ct], [elt], [key])
        else:
            (want,) = e.relinearize_batch(L, [ct], key)
        assert np.array_equal(run_case(e, s, case, key), want.download()), (mix, case)


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
