"""Sparse-secret encapsulation on the GPU, word for word: hefx_collapse_key against Python integers, hefx_switch_key against the
twin's key switch, hefx_raise_switch against its fall-back -- the ordinary key switch on a synthetic two-digit operand -- run on
the ENGINE and on the oracle-backed TWIN, and algorithms.bootstrap / update_weights_bootstrapped with encaps= against the twin.

The fall-back is the reference: tests/test_encaps_cpu.py holds it to the integer statement of include/hefx_encaps.h.  Shapes:
the two chains of tests/encaps_cases.py at N = 2048 and L_out in {2, top} (real keys), then random canonical operands -- any
words are an input of the statement -- at N = 4096, at N = 16384, on every set of tests/policy_sets.py with two data primes or
more (every arithmetic policy of the engine's transforms and key switch on the reference side), and one case at N = 32768,
where the transforms are the out-of-place split ones and no side calls hefx_mod_raise."""
import numpy as np
import pytest

from tests import bootstrap_cases as BC
from tests import encaps_cases as EC
from tests import lr_bootstrap_cases as LB
from tests import policy_sets as PS
from tests import sparse_bootstrap_cases as SC

pytestmark = pytest.mark.gpu

_ENV = {}


def envs(chain):
    """engine and twin on one of the two chains, same seeds: dense main secret, encapsulation keys"""
    if chain not in _ENV:
        _ENV[chain] = tuple(EC.make(kind, bits=EC.CHAINS[chain]) for kind in ("gpu", "oracle"))
        eg, eo = _ENV[chain]
        assert all(getattr(eg["ctx"].backend, n, None) is not None for n in ("switch_key", "collapse_key", "raise_switch"))
        assert all(getattr(eo["ctx"].backend, n, None) is None for n in ("switch_key", "collapse_key", "raise_switch", "mod_raise"))
        for name in ("low", "high"):
            assert np.array_equal(eg["ctx"].backend.to_host(getattr(eg["keys"], name)).reshape(-1),
                                  eo["ctx"].backend.to_host(getattr(eo["keys"], name)).reshape(-1)), name
    return _ENV[chain]


def encrypted(e, chain, level):
    return e["enc"].encrypt(e["encoder"].encode(EC.input_values(), EC.SCALES[chain], parms_id=level))


def levels(ctx):
    return {"two": 2, "top": ctx.first_parms_id()}


def same(eg, g, eo, o, level, name):
    assert g.size() == o.size() == 2 and g.parms_id() == o.parms_id() == level and g.scale == o.scale, name
    assert np.array_equal(BC.words(eg, g), BC.words(eo, o)), name


@pytest.mark.parametrize("chain", sorted(EC.CHAINS))
@pytest.mark.parametrize("level", ["two", "top"])
def test_collapse_key_against_python_integers(chain, level):
    eg, _ = envs(chain)
    ctx, e = eg["ctx"], eg["ctx"].backend.engine
    L = levels(ctx)[level]
    high = eg["keys"].high
    before = high.download()
    got = e.collapse_key(L, high).download()
    assert got.shape == (2, L + 1, ctx.N) and np.array_equal(got, EC.collapse_model(before, ctx.primes, L))
    assert np.array_equal(high.download(), before)


@pytest.mark.parametrize("chain", sorted(EC.CHAINS))
def test_switch_key_same_words_as_the_twin_also_in_place(chain):
    eg, eo = envs(chain)
    e, top = eg["ctx"].backend.engine, eg["ctx"].first_parms_id()
    for L, which in ((1, "low"), (top, "high")):
        cg, co = encrypted(eg, chain, L), encrypted(eo, chain, L)
        assert np.array_equal(BC.words(eg, cg), BC.words(eo, co))
        before = BC.words(eg, cg).copy()
        want = np.asarray(eo["ctx"].backend.apply_galois(L, co.data, 1, getattr(eo["keys"], which))).reshape(2, L, EC.N)
        same(eg, eg["ev"].switch_key(cg, getattr(eg["keys"], which)), eo, eo["ev"].switch_key(co, getattr(eo["keys"], which)), L, (chain, L))
        assert np.array_equal(BC.words(eg, eg["ev"].switch_key(cg, getattr(eg["keys"], which))), want)
        assert np.array_equal(BC.words(eg, cg), before)                # out of place: the input is only read
        buf = e.copy(cg.data)
        assert e.switch_key(L, buf, getattr(eg["keys"], which), out=buf) is buf   # the exact in-place form
        assert np.array_equal(buf.download(), want), (chain, L, "in place")


@pytest.mark.parametrize("chain", sorted(EC.CHAINS))
@pytest.mark.parametrize("level", ["two", "top"])
def test_raise_switch_equals_the_fall_back_on_the_engine_and_on_the_twin(chain, level):
    eg, eo = envs(chain)
    L = levels(eg["ctx"])[level]
    sg, so = (e["ev"].switch_key(encrypted(e, chain, 1), e["keys"].low) for e in (eg, eo))
    assert np.array_equal(BC.words(eg, sg), BC.words(eo, so))
    before = BC.words(eg, sg).copy()
    got = eg["ev"].raise_switch(sg, eg["keys"], L)
    assert L in eg["keys"]._collapsed and np.array_equal(BC.words(eg, sg), before)
    same(eg, got, eo, eo["ev"].raise_switch(so, eo["keys"], L), L, (chain, L, "twin"))
    composed = np.asarray(eg["ev"]._raise_switch_composed(sg, eg["keys"], L).download())
    assert np.array_equal(BC.words(eg, got), composed), (chain, L, "the fall-back on the engine")
    again = eg["ev"].raise_switch(sg, eg["keys"], L)                   # through the cached collapsed key
    assert np.array_equal(BC.words(eg, again), composed)
    # decrypted under the DENSE secret it is the message (mod q_0: row 0 alone)
    pt = eg["dec"].decrypt(eg["ev"].mod_switch_to_inplace(got.copy(), 1))
    err = float(np.abs(eg["encoder"].decode(pt).real - EC.input_values()).max())
    print(f"[gpu encaps] {chain} L_out = {L}: words equal; decode error {err:.3e} at scale 2^{int(np.log2(EC.SCALES[chain]))}")
    assert err <= 2.0 ** 17 / EC.SCALES[chain]   # (a sanity bound on the decryption: the criterion is the words)


def random_case(N, primes, L, seed):
    """hefx_raise_switch on random canonical operands against the fall-back on the engine and on the twin"""
    ct, key = EC.random_operands(N, primes, seed)
    outs = {}
    for kind in ("gpu", "oracle"):
        ctx = EC.context(kind, N, primes)
        ev_ct, keys = EC.as_ciphertext(ctx, ct), EC.as_keys(ctx, key)
        from seal_fyp_logistic_regression_amd import seal as S
        ev = S.Evaluator(ctx)
        if kind == "gpu":
            outs["native"] = np.asarray(ctx.backend.to_host(ev.raise_switch(ev_ct, keys, L).data)).reshape(2, L, N)
            assert np.array_equal(ctx.backend.to_host(ev_ct.data).reshape(2, 1, N), ct)
        outs[kind] = np.asarray(ctx.backend.to_host(ev._raise_switch_composed(ev_ct, keys, L))).reshape(2, L, N)
    assert np.array_equal(outs["native"], outs["gpu"]), "the fall-back on the engine"
    assert np.array_equal(outs["native"], outs["oracle"]), "the fall-back on the twin"


SETS = sorted(name for name, s in PS.sets().items() if s.k - 1 >= 2)


@pytest.mark.parametrize("name", SETS)
def test_raise_switch_on_every_policy_set(name):
    s = PS.sets()[name]
    for L in sorted({2, max(s.levels)}):
        random_case(s.N, s.primes, L, seed=31 + L)


@pytest.mark.parametrize("N,bits,L", [(4096, [60, 50, 50, 50, 60], 2), (4096, [60, 50, 50, 50, 60], 4), (4096, [40, 50, 50, 60], 3),
                                      (16384, [60, 50, 50, 60], 2), (16384, [60, 50, 50, 60], 3),
                                      (32768, [60, 50, 60], 2)])
def test_raise_switch_at_larger_rings(N, bits, L):
    from seal_fyp_logistic_regression_amd import seal as S
    random_case(N, S.CoeffModulus.Create(N, bits), L, seed=N + L)


def test_the_entries_return_while_their_stream_is_held_shut():
    from tests.hip_stream_gate import Stream
    eg, _ = envs("wide0")
    ctx, e = eg["ctx"], eg["ctx"].backend.engine
    top, N, keys = ctx.first_parms_id(), ctx.N, eg["keys"]
    ct1, cttop = encrypted(eg, "wide0", 1), encrypted(eg, "wide0", top)
    want_sw = e.switch_key(top, cttop.data, keys.high).download()
    want_kc = e.collapse_key(top, keys.high)
    want_rs = e.raise_switch(top, ct1.data, want_kc).download()
    o_sw, o_kc, o_rs = e.zeros(2, top, N), e.zeros(2, top + 1, N), e.zeros(2, top, N)
    e.sync()
    with Stream() as S:
        gate = S.gate()
        e.switch_key(top, cttop.data, keys.high, out=o_sw, stream=S.handle)
        assert not gate.opened, "hefx_switch_key waited on the host"
        e.collapse_key(top, keys.high, out=o_kc, stream=S.handle)
        assert not gate.opened, "hefx_collapse_key waited on the host"
        e.raise_switch(top, ct1.data, o_kc, out=o_rs, stream=S.handle)   # (reads the collapsed key the same stream makes)
        assert not gate.opened, "hefx_raise_switch waited on the host"
        e.sync(S.handle)
        assert gate.opened
    assert np.array_equal(o_sw.download(), want_sw)
    assert np.array_equal(o_kc.download(), want_kc.download())
    assert np.array_equal(o_rs.download(), want_rs)


def test_every_byte_overlap_is_refused_with_nothing_submitted():
    """an output one row into an input or key, an input or key one row into the output, and the exact in-place forms the entries
    do not serve: ValueError (HEFX_ERR_INVALID), the slab's words unchanged, no key switch counted"""
    eg, _ = envs("narrow0")
    ctx, e = eg["ctx"], eg["ctx"].backend.engine
    N, k, L = ctx.N, ctx.k, ctx.first_parms_id()
    rng = np.random.default_rng(3)
    words = {"key": (k - 1) * 2 * k * N, "ckey": 2 * (L + 1) * N, "in1": 2 * N, "inL": 2 * L * N, "out": 2 * (L + 1) * N,
             "pad": (k - 1) * 2 * k * N}   # pad: whatever is moved onto the output's last row still ends inside the slab
    at, pos = {}, 0
    for name, w in words.items():
        at[name], pos = pos, pos + w
    host = rng.integers(0, int(min(ctx.primes)), pos, dtype=np.uint64)
    slab = e.to_device(host)
    view = lambda off, shape: slab.view(off, shape)
    last_row = lambda y, used=None: at[y] + (words[y] if used is None else used) - N   # where y's last row starts
    stats = e.ks_stats()

    def refused(call):
        with pytest.raises(ValueError, match="overlap|independent"):
            call()
        e.sync()
        assert np.array_equal(slab.download(), host) and e.ks_stats() == stats

    inL, in1 = view(at["inL"], (2, L, N)), view(at["in1"], (2, 1, N))
    key, ckey = view(at["key"], (k - 1, 2, k, N)), view(at["ckey"], (2, L + 1, N))
    out2, out3 = view(at["out"], (2, L, N)), view(at["out"], (2, L + 1, N))
    # hefx_switch_key: partial overlaps with the input, any overlap with the key (the exact in-place form runs: tested above)
    refused(lambda: e.switch_key(L, inL, key, out=view(last_row("inL"), (2, L, N))))
    refused(lambda: e.switch_key(L, view(last_row("out", 2 * L * N), (2, L, N)), key, out=out2))
    refused(lambda: e.switch_key(L, inL, key, out=view(last_row("key", L * 2 * k * N), (2, L, N))))
    refused(lambda: e.switch_key(L, inL, key, out=view(at["key"], (2, L, N))))
    refused(lambda: e.switch_key(L, inL, view(last_row("out", 2 * L * N), (k - 1, 2, k, N)), out=out2))
    # hefx_collapse_key
    refused(lambda: e.collapse_key(L, key, out=view(last_row("key", L * 2 * k * N), (2, L + 1, N))))
    refused(lambda: e.collapse_key(L, key, out=view(at["key"], (2, L + 1, N))))
    refused(lambda: e.collapse_key(L, view(last_row("out"), (k - 1, 2, k, N)), out=out3))
    # hefx_raise_switch
    refused(lambda: e.raise_switch(L, in1, ckey, out=view(at["in1"], (2, L, N))))               # d_ct_out == d_ct_in
    refused(lambda: e.raise_switch(L, in1, ckey, out=view(last_row("in1"), (2, L, N))))
    refused(lambda: e.raise_switch(L, view(last_row("out", 2 * L * N), (2, 1, N)), ckey, out=out2))
    refused(lambda: e.raise_switch(L, in1, ckey, out=view(last_row("ckey"), (2, L, N))))
    refused(lambda: e.raise_switch(L, in1, view(last_row("out", 2 * L * N), (2, L + 1, N)), out=out2))
    with pytest.raises(ValueError, match="at least 2"):
        e.raise_switch(1, in1, ckey, out=view(at["out"], (2, 1, N)))
    # the adjacent layout runs, and writes its output alone
    e.raise_switch(L, in1, ckey, out=out2)
    e.sync()
    got = slab.download()
    lo, hi = at["out"], at["out"] + 2 * L * N
    assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[hi:], host[hi:]) and not np.array_equal(got[lo:hi], host[lo:hi])


def dense(e):
    be = e["ctx"].backend
    coef = np.asarray(be.to_host(be.ntt_inverse(be.from_host(e["kg"].secret_key().host[:1].copy()), 1, 1, 0))).reshape(-1)
    return np.count_nonzero(coef) > e["ctx"].N // 2


def test_bootstrap_under_a_dense_secret_same_words_as_the_twin():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from tests.test_encaps_cpu import raised_integer_part
    ns = SC.SPARSE_NS
    p, v = SC.sparse_plan(ns), SC.sparse_input(ns)
    steps = tuple(sorted(set(p.galois_steps())))
    outs = []
    for kind in ("gpu", "oracle"):
        e = EC.make(kind, BC.N, BC.CHAIN_BITS, galois_steps=steps, conjugate=True)
        assert dense(e)
        ct = SC.encrypt_tiled(e, v)
        if kind == "gpu":   # a condition on the input: the SPARSE secret's integer part fits the plan
            I = raised_integer_part(e, e["ev"].raise_switch(e["ev"].switch_key(ct, e["keys"].low), e["keys"], p.top_level))
            print(f"[gpu encaps] ns = {ns}: max |I| = {I} (K = {p.K})")
            assert I <= p.K
        outs.append((e, ct, alg.bootstrap(e["ev"], ct, p, e["gk"], e["rk"], p.encode(e["encoder"]), encaps=e["keys"])))
    (eg, cg, og), (eo, co, oo) = outs
    assert np.array_equal(BC.words(eg, cg), BC.words(eo, co))
    same(eg, og, eo, oo, p.result_level, ("bootstrap", ns))
    err = float(np.abs(eg["encoder"].decode(eg["dec"].decrypt(og)).real - SC.tiled(v)).max() / np.abs(v).max())
    print(f"[gpu encaps] bootstrap under a dense secret, ns = {ns}: words equal; decode error {err:.3e} (cap {BC.CAP:g})")
    assert err <= BC.CAP


def test_one_training_step_under_a_dense_secret_same_words_as_the_twin():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    shape = "A"                                                     # the smallest: 3 rows, 4 weights, ns = 4
    rows, weights, ns, _ = LB.SHAPES[shape]
    p = LB.plan(ns)
    steps = tuple(alg.lr_bootstrap_galois_steps(p, rows, weights))
    outs = []
    for kind in ("gpu", "oracle"):
        e = LB.fresh(EC.make(kind, LB.N, LB.CHAIN_BITS, galois_steps=steps, conjugate=True))
        assert dense(e)
        feats, featsT, cy, cw = LB.encrypt_inputs(e, shape, level=LB.START_LEVEL)
        outs.append((e, alg.update_weights_bootstrapped(e["ev"], e["encoder"], e["enc"], feats, featsT, cy, cw, LB.LEARNING_RATE, e["gk"],
                                                        e["rk"], LB.SCALE, p, LB.DEGREE, LB.POLY, p.encode(e["encoder"]), encaps=e["keys"])))
    (eg, og), (eo, oo) = outs
    same(eg, og, eo, oo, LB.START_LEVEL, ("update_weights_bootstrapped", shape))
    first, everywhere = LB.errors(eg, og, LB.model(shape)[0])
    print(f"[gpu encaps] one step of shape {shape} under a dense secret: words equal; decode error {first:.3e} in the first {ns} "
          f"slots, {everywhere:.3e} in all (cap {BC.CAP * LB.MAX_VALUE:g})")
    assert first <= BC.CAP * LB.MAX_VALUE and everywhere <= BC.CAP * LB.MAX_VALUE
