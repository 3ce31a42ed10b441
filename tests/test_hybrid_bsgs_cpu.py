"""The hoisted giant steps without a GPU (include/hefx_hybrid_bsgs.h): seal.py's host statement against the independent model
of tests/hybrid_bsgs_cases.py, the identities that tie the statement to the combine of hefx_hybrid_hoist.h, the noise bound
under real keys, the hybrid DFT with hoisted giants, bootstrap.plan's special primes, eval_mod_hybrid / bootstrap_hybrid on the
oracle twin against the one-special-prime bootstrap, the front end and the C surface.  (The accumulator's bound is a matter
of the kernel's 128-bit sums: tests/test_gpu_hybrid_bsgs.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bootstrap_cases as BC
from tests import hybrid_bsgs_cases as HB
from tests import hybrid_cases as HC
from tests import hybrid_hoist_cases as HH
from tests import sparse_bootstrap_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_SEED = 3
CAP = 1e-3          # the project's cap on a decode error, relative to the largest expected value

_ENV = {}


def env(name):
    """the twin of a set with real hybrid keys of the steps 1 and 2 and of the conjugation"""
    from seal_fyp_logistic_regression_amd import seal as S
    if name not in _ENV:
        s = HC.sets()[name]
        ctx = HC.context(s, "oracle")
        kg = S.KeyGenerator(ctx, KEY_SEED)
        _ENV[name] = dict(s=s, ctx=ctx, kg=kg, ev=S.Evaluator(ctx), gk=kg.hybrid_galois_keys(s.alpha, [1, 2], conjugate=True),
                          enc=S.Encryptor(ctx, kg.public_key(), KEY_SEED + 1), dec=S.Decryptor(ctx, kg.secret_key()),
                          encoder=S.CKKSEncoder(ctx, device_encode=False))
    return _ENV[name]


def host(e, h):
    return np.asarray(e["ctx"].backend.to_host(h), dtype=np.uint64)


@pytest.mark.parametrize("kind", HB.KINDS)
@pytest.mark.parametrize("name,L", HB.WORD_CASES)
def test_the_host_statement_is_the_model_word_for_word(name, L, kind):
    from seal_fyp_logistic_regression_amd import seal as S
    s = HC.sets()[name]
    assert L in s.levels
    want = HB.case_model(s, L, kind)
    got = S.hybrid_bsgs_host(HC.twin(s), s.primes, s.alpha, L, *HB.case(s, L, kind))
    assert len(got) == len(want) == 2
    for q, (g, w) in enumerate(zip(got, want)):
        assert g.shape == (2, L, s.N) and np.array_equal(g, w), (name, L, kind, "output", q)


@pytest.mark.parametrize("name", ["k7a2-p50_60", "k8a3-above60"])
def test_without_giant_keys_the_statement_is_the_combine(name):
    """all giant keys NULL and dest the identity: the words of the combine; all dest 0: the combine with G = 1 and the
    plaintexts summed mod q_m (the model and the host statement both)"""
    from seal_fyp_logistic_regression_amd import seal as S
    s = HC.sets()[name]
    be, L = HC.twin(s), max(s.levels)
    cts, elts, keys, pts, _, _, _ = HB.case(s, L)
    comb = HH.combine_model(be, s.primes, s.alpha, L, cts, elts, keys, pts)
    summed = [None] * 6
    for t in range(6):
        live = [row[t] for row in pts if row[t] is not None]
        summed[t] = np.stack([(sum(p[m].astype(object) for p in live) % int(s.primes[m])).astype(np.uint64) for m in range(s.k)])
    (one,) = HH.combine_model(be, s.primes, s.alpha, L, cts, elts, keys, [summed])
    for run in (HB.bsgs_model, S.hybrid_bsgs_host):
        got = run(be, s.primes, s.alpha, L, cts, elts, keys, pts, [1] * 4, [None] * 4, [0, 1, 2, 3])
        assert len(got) == 4 and all(np.array_equal(g, w) for g, w in zip(got, comb)), (name, run.__name__)
        (got,) = run(be, s.primes, s.alpha, L, cts, elts, keys, pts, [1] * 4, [None] * 4, [0] * 4)
        assert np.array_equal(got, one), (name, run.__name__)


def noise_bound(s, L, r):
    """include/hefx_hybrid_bsgs.h, NOISE: r (B + (alpha + 1) N) + alpha (1 + N), B the hybrid switch's own bound"""
    B, Q = HC.noise_bound(s, L)
    return r * (B + (s.alpha + 1) * s.N) + s.alpha * (1 + s.N), Q


def noise_cases():
    out = []
    for name in ("k7a2-p50_60", "k8a3-above60", "k7a4-d40_s60"):
        s = HC.sets()[name]
        for L in s.levels:
            bound, Q = noise_bound(s, L, 3)
            if 4 * bound < Q:
                out.append((name, L))
    return out


def giant_noise(s, L, ct, out, elts, sk):
    """max |dec(out) - sum_g pi_g(dec(ct))| centred mod Q_L in exact integers (HC.switch_noise's method)"""
    q = s.primes
    plain = HC.decrypt_rows(ct, sk, q)
    want = [sum(HC.gather(s.N, g, r) for g in elts) for r in plain]
    got = HC.decrypt_rows(out, sk, q)
    diff, Q = HC.centred_integers(HC.twin(s), [(g - w) % int(q[j]) for j, (g, w) in enumerate(zip(got, want))], q)
    return int(np.abs(diff).max()), Q


@pytest.mark.parametrize("name,L", noise_cases())
def test_the_giant_steps_keep_the_stated_noise_bound_under_real_keys(name, L):
    """one source, the identity baby term, the plaintext 1, r in {1, 3} giant terms into one output"""
    e = env(name)
    s, be, N = e["s"], e["ctx"].backend, e["s"].N
    sk = e["kg"].secret_key().host
    gelts = [3, 9, 2 * N - 1]
    gkeys = [host(e, e["gk"].hybrid_key(g)) for g in gelts]
    one = HH.plaintext(s, "one", 0)
    for r in (1, 3):
        bound, Q = noise_bound(s, L, r)
        worst = 0
        for kind in ("uniform", "max"):
            ct = HC.operand(s, kind, L, 2, seed=43 + L)
            (out,) = HB.bsgs_model(be, s.primes, s.alpha, L, [ct], [1], [None], [[one]] * r, gelts[:r], gkeys[:r], [0] * r)
            noise, Q_ = giant_noise(s, L, ct, out, gelts[:r], sk)
            assert Q_ == Q
            worst = max(worst, noise)
        print(f"[hybrid bsgs cpu] {name} L = {L}, {r} giant terms: noise {worst} (bound {bound})")
        assert 0 < worst <= bound


def test_the_front_end_refuses():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import seal as S
    e = env("k7a2-p50_60")
    s, be, ev, gk, encoder = e["s"], e["ctx"].backend, e["ev"], e["gk"], e["encoder"]
    top = s.k - s.alpha
    at = lambda L: S.Ciphertext()._set(be.from_host(HC.operand(s, "uniform", L, 2, seed=2) if L <= top else
                                                    np.zeros((2, L, s.N), dtype=np.uint64)), 2, L, 2.0 ** 40)
    ct = at(top)
    pt = encoder.encode(np.ones(4), 2.0 ** 40, parms_id=s.k)
    with pytest.raises(ValueError, match=r"level <= k - alpha = 5"):
        ev.bsgs_hoisted([at(top + 1)], [1], [[pt]], [0], [0], gk)
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.bsgs_hoisted([ct], [0, 3], [[pt, pt]], [0], [0], gk)             # a baby step without its key
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.bsgs_hoisted([ct], [0, 1], [[pt, pt]], [3], [0], gk)             # a giant step without its key
    with pytest.raises(ValueError, match="key-level plaintexts"):
        ev.bsgs_hoisted([ct], [0, 1], [[pt, encoder.encode(np.ones(4), 2.0 ** 40, parms_id=top)]], [1], [0], gk)
    with pytest.raises(ValueError, match="an inner sum has no term"):
        ev.bsgs_hoisted([ct], [0, 1], [[pt, None], [None, None]], [0, 1], [0, 0], gk)
    with pytest.raises(ValueError, match="one plaintext"):
        ev.bsgs_hoisted([ct], [0, 1], [[pt]], [0], [0], gk)
    with pytest.raises(ValueError, match="one giant step and one dest"):
        ev.bsgs_hoisted([ct], [0, 1], [[pt, pt]], [0, 1], [0], gk)
    for bad in ([0, 2], [-1, 0], [1, 5]):
        with pytest.raises(ValueError, match="dest out of range|an output has no inner sum"):
            ev.bsgs_hoisted([ct], [0, 1], [[pt, pt], [pt, None]], [0, 1], bad, gk)
    with pytest.raises(ValueError, match="an output has no inner sum"):
        ev.bsgs_hoisted([ct], [0, 1], [[pt, pt]] * 3, [0, 1, 2], [0, 2, 2], gk)
    with pytest.raises(TypeError, match="HybridKeys"):
        ev.bsgs_hoisted([ct], [1], [[pt]], [0], [0], e["kg"].galois_keys([1]))
    # a giant step of 0 everywhere and dest the identity: plain_combine_hoisted's ciphertexts, level and scale included
    rows = [[pt, pt], [None, pt]]
    got, want = ev.bsgs_hoisted([ct], [0, 1], rows, [0, 0], [0, 1], gk), ev.plain_combine_hoisted([ct], [0, 1], rows, gk)
    for g, w in zip(got, want):
        assert g.parms_id() == w.parms_id() == top and g.scale == w.scale and np.array_equal(host(e, g.data), host(e, w.data))
    # the old composites still refuse hybrid keys, the new ones the other kind
    rk = e["kg"].hybrid_relin_keys(s.alpha)
    for call in (lambda: alg.bootstrap(ev, ct, None, gk, rk), lambda: alg.eval_mod(ev, [ct], None, rk), lambda: alg.subsum(ev, ct, 16, gk),
                 lambda: alg.coeffs_to_slots(ev, ct, None, gk), lambda: alg.slots_to_coeffs_packed(ev, ct, None, gk)):
        with pytest.raises(TypeError, match=r"with HybridKeys \(alpha = 2\) is not supported"):
            call()
    with pytest.raises(TypeError, match="HybridKeys"):
        alg.bootstrap_hybrid(ev, ct, None, e["kg"].galois_keys([1]), rk)
    with pytest.raises(TypeError, match="HybridKeys"):
        alg.bootstrap_hybrid(ev, ct, None, gk, e["kg"].relin_keys())
    with pytest.raises(TypeError, match="HybridKeys"):
        alg.eval_mod_hybrid(ev, [ct], None, e["kg"].relin_keys())
    with pytest.raises(TypeError, match="HybridKeys"):
        alg.subsum_hybrid(ev, ct, 16, e["kg"].galois_keys([1]))


# ---- the hybrid DFT with hoisted giant steps ---------------------------------------------------------------------------
def dft_hoisted(e, which, hoist_giants):
    """HH.dft_program's round trip with the keyword given: ct -> ((CoeffToSlot's results), the final ciphertext)"""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    ev, gk, plans = e["ev"], e["gk"], e["plans"]
    if which == "dense":
        def run(ct):
            a, b = alg.coeffs_to_slots_hybrid(ev, ct, plans["c2s"], gk, hoist_giants=hoist_giants)
            return (a, b), alg.slots_to_coeffs_hybrid(ev, a, b, plans["s2c"], gk, hoist_giants=hoist_giants)
    else:
        def run(ct):
            mid = alg.coeffs_to_slots_packed_hybrid(ev, ct, plans["pc2s"], gk, hoist_giants=hoist_giants)
            return (mid,), alg.slots_to_coeffs_packed_hybrid(ev, mid, plans["ps2c"], gk, hoist_giants=hoist_giants)
    return run


def decode_err(e, ct, want):
    return float(np.abs(e["encoder"].decode(e["dec"].decrypt(ct)) - want).max())


@pytest.mark.parametrize("which", ["dense", "packed"])
def test_decode_of_the_hybrid_dft_with_hoisted_giants_against_the_op_by_op_run(which):
    """the criterion of tests/test_hybrid_hoist_cpu.py's round trip test: at most twice the op-by-op run's error and within CAP
    of the largest value; with hoist_giants=False the words are those of a call that omits the keyword"""
    from tests.test_hybrid_hoist_cpu import dft_programs
    e = HH.dft_env("oracle")
    omitted, op_by_op, z, want = dft_programs(e, which)
    ct = e["enc"].encrypt(e["encoder"].encode(z, HH.DFT_SCALE, parms_id=e["top"]))
    _, got_h = dft_hoisted(e, which, True)(ct)
    got_o = op_by_op(ct)
    assert got_h.size() == 2 and got_h.parms_id() == got_o.parms_id() == e["top"] - 2 * HH.DFT_LEVELS
    assert abs(got_h.scale - got_o.scale) <= 2.0 ** -40 * got_o.scale
    err_h, err_o, largest = decode_err(e, got_h, want), decode_err(e, got_o, want), float(np.abs(want).max())
    print(f"[hybrid bsgs cpu] {which} DFT round trip: decode error with hoisted giants {err_h:.3e}, op by op {err_o:.3e}, largest value {largest:.3e}")
    assert 0 < err_h <= 2 * err_o and err_h <= CAP * largest
    _, got_f = dft_hoisted(e, which, False)(ct)
    got_d = omitted(ct)
    assert got_f.parms_id() == got_d.parms_id() and got_f.scale == got_d.scale
    assert np.array_equal(host(e, got_f.data), host(e, got_d.data))
    assert not np.array_equal(host(e, got_h.data), host(e, got_d.data))        # one rounding per output: other words


# ---- bootstrap.plan(..., special) ---------------------------------------------------------------------------------------
def test_the_plan_with_special_primes():
    from seal_fyp_logistic_regression_amd import bootstrap as B
    from seal_fyp_logistic_regression_amd import seal as S
    primes = HB.boot_primes()
    for slots in (None, 16):
        p0, p1, p2 = (B.plan(BC.N, primes, BC.SCALE, slots=slots, **kw) for kw in ({}, {"special": 1}, {"special": 2}))
        assert p0.special == p1.special == 1 and p2.special == 2
        for f in ("N", "primes", "scale", "K", "r", "degree", "Kp", "sparse_slots", "poly_target_scale", "max_value", "model_error",
                  "top_level", "depth", "evalmod_level", "s2c_level", "result_level"):
            assert getattr(p0, f) == getattr(p1, f), f
        assert np.array_equal(p0.coeffs, p1.coeffs) and p0.galois_steps() == p1.galois_steps()
        for a, b in ((p0.c2s, p1.c2s), (p0.s2c, p1.s2c)):
            assert a.primes() == b.primes() and a.levels == b.levels and a.galois_steps() == b.galois_steps()
        for f in ("top_level", "evalmod_level", "s2c_level", "result_level"):
            assert getattr(p2, f) == getattr(p0, f) - 1, f
        assert p2.top_level == len(primes) - 2
        assert p2.c2s.primes() == [int(primes[p2.top_level - 1 - i]) for i in range(p2.c2s.levels)]
        assert p2.s2c.primes() == [int(primes[p2.s2c_level - 1 - i]) for i in range(p2.s2c.levels)]
    for bad in (0, -1, S.HYBRID_ALPHA_MAX + 1):
        with pytest.raises(ValueError, match="special"):
            B.plan(BC.N, primes, BC.SCALE, special=bad)
    with pytest.raises(ValueError, match="not enough levels|data primes"):
        B.plan(BC.N, primes, BC.SCALE, special=5)
    with pytest.raises(ValueError, match="data primes"):
        B.plan(BC.N, primes[:3], BC.SCALE, special=3)


def test_plan_encode_extended_has_the_words_of_the_default_in_the_stage_rows():
    e = HB.boot_env("oracle")
    plan, encoder, be, k = e["plan"], e["encoder"], e["ctx"].backend, e["ctx"].k
    default, extended = plan.encode(encoder), e["encoded"]
    seen = 0
    for tables_d, tables_x, top in zip(default, extended, (plan.top_level, plan.s2c_level)):
        for i, (stage_d, stage_x) in enumerate(zip(tables_d, tables_x)):
            L = top - i
            for mat_d, mat_x in zip(stage_d, stage_x):
                for row_d, row_x in zip(mat_d, mat_x):
                    for a, x in zip(row_d, row_x):
                        assert (a is None) == (x is None)
                        if a is None:
                            continue
                        assert a.parms_id() == L and x.parms_id() == k and a.scale == x.scale
                        assert np.array_equal(np.asarray(be.to_host(a.data)).reshape(L, -1), np.asarray(be.to_host(x.data)).reshape(k, -1)[:L])
                        seen += 1
    assert seen > 0


# ---- EvalMod and the bootstrap on hybrid keys, on the twin --------------------------------------------------------------
class Recording:
    """a backend that passes everything on and serves hybrid_relinearize_batch from the host statement, counting its calls"""

    def __init__(self, be, primes):
        self._be, self._primes, self.calls = be, primes, []

    def __getattr__(self, name):
        return getattr(self._be, name)

    def hybrid_relinearize_batch(self, alpha, L, ct3s, key):
        from seal_fyp_logistic_regression_amd import seal as S
        self.calls.append(len(ct3s))
        be, q = self._be, self._primes
        outs = []
        for d in ct3s:
            ct = np.asarray(be.to_host(d), dtype=np.uint64).reshape(3, L, -1)
            outs.append(be.from_host(S._hybrid_rows_add_host(q, S.hybrid_switch_host(be, q, alpha, L, ct[2], be.to_host(key)), ct[:2])))
        return outs


def test_relinearize_many_on_hybrid_keys_is_one_backend_call_with_the_words_of_the_loop():
    from seal_fyp_logistic_regression_amd import seal as S
    e = env("k7a2-p50_60")
    s, ctx = e["s"], e["ctx"]
    rk = e["kg"].hybrid_relin_keys(s.alpha)
    L = s.k - s.alpha
    make = lambda: [S.Ciphertext()._set(ctx.backend.from_host(HC.operand(s, "uniform", L, 3, seed=60 + i)), 3, L, 2.0 ** 40) for i in range(3)]
    loop = [e["ev"].relinearize_inplace(c, rk) for c in make()]
    ev = S.Evaluator(ctx)
    ev.be = rec = Recording(ctx.backend, ctx.primes)
    batch = ev.relinearize_many_inplace(make(), rk)
    assert rec.calls == [3]
    for b, l in zip(batch, loop):
        assert b.size() == l.size() == 2 and b.parms_id() == l.parms_id() and b.scale == l.scale
        assert np.array_equal(host(e, b.data), host(e, l.data))
    # a batch that is not uniform (one item is of size 2 already) goes item by item, as before
    mixed = make()
    mixed[1] = S.Ciphertext()._set(ctx.backend.from_host(HC.operand(s, "uniform", L, 2, seed=70)), 2, L, 2.0 ** 40)
    rec.calls.clear()
    ev.relinearize_many_inplace(mixed, rk)
    assert all(c.size() == 2 for c in mixed) and rec.calls == [1, 1]
    assert np.array_equal(host(e, mixed[0].data), host(e, loop[0].data)) and np.array_equal(host(e, mixed[2].data), host(e, loop[2].data))


def _boot_input(e, sparse):
    v = SC.sparse_input(HB.BOOT_NS) if sparse else BC.bootstrap_input()
    full = SC.tiled(v) if sparse else v
    return v, e["enc"].encrypt(e["encoder"].encode(full, BC.SCALE, parms_id=1))


def _rel_error(e, ct, v):
    got = e["encoder"].decode(e["dec"].decrypt(ct))
    return float(np.abs(got[:len(v)] - v).max() / np.abs(v).max())


_REFERENCE = {}


def reference_bootstrap(sparse):
    """algorithms.bootstrap on [60] + [50] * 13 + [60] with the same key seed and the same input: (error, level)"""
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import bootstrap as B
    if sparse not in _REFERENCE:
        from seal_fyp_logistic_regression_amd import seal as S
        primes = S.CoeffModulus.Create(BC.N, BC.CHAIN_BITS)
        plan = B.plan(BC.N, primes, BC.SCALE, slots=HB.BOOT_NS if sparse else None)
        e = SC.make("oracle", plan.galois_steps())
        v, ct = _boot_input(e, sparse)
        out = alg.bootstrap(e["ev"], ct, plan, e["gk"], e["rk"])
        _REFERENCE[sparse] = (_rel_error(e, out, v), out.parms_id(), [int(p) for p in primes])
    return _REFERENCE[sparse]


@pytest.mark.parametrize("sparse", [True, False], ids=["sparse16", "dense"])
def test_bootstrap_hybrid_on_the_twin_against_the_bootstrap_with_one_special_prime(sparse):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    e = HB.boot_env("oracle", sparse)
    plan, ev = e["plan"], e["ev"]
    v, ct = _boot_input(e, sparse)
    _, I = BC.raised_coefficients(e, ct, plan.top_level)
    print(f"[hybrid bsgs cpu] max |I| = {int(np.abs(I).max())} (K = {plan.K})")
    assert np.abs(I).max() <= plan.K                                # a condition on the input
    err_ref, level_ref, primes_ref = reference_bootstrap(sparse)
    assert [int(p) for p in e["ctx"].primes[:14]] == primes_ref[:14]  # the 14 data primes agree
    for hoist in (True, False):
        out = alg.bootstrap_hybrid(ev, ct, plan, e["hgk"], e["hrk"], e["encoded"], hoist_giants=hoist)
        assert out.size() == 2 and out.parms_id() == plan.result_level == level_ref and abs(out.scale / BC.SCALE - 1.0) < 1e-12
        err = _rel_error(e, out, v)
        print(f"[hybrid bsgs cpu] {'sparse' if sparse else 'dense'} bootstrap_hybrid, giants {'hoisted' if hoist else 'not hoisted'}: "
              f"error {err:.3e} of the largest value, bootstrap with one special prime {err_ref:.3e}")
        assert 0 < err <= BC.CAP and err <= 2 * err_ref
    if sparse:
        from seal_fyp_logistic_regression_amd import bootstrap as B
        other = B.plan(BC.N, e["ctx"].primes, BC.SCALE, slots=HB.BOOT_NS, special=1)
        with pytest.raises(ValueError, match="special"):
            alg.bootstrap_hybrid(ev, ct, other, e["hgk"], e["hrk"])
        with pytest.raises(ValueError, match="last prime"):
            alg.bootstrap_hybrid(ev, out, plan, e["hgk"], e["hrk"])


def test_capi_declares_the_symbol_and_the_build_lists_the_sources(tmp_path):
    from seal_fyp_logistic_regression_amd import _build, capi
    assert capi.HYBRID_BSGS_SYMBOLS == ["hefx_hybrid_bsgs_hoisted"]
    assert "hefx_hybrid_bsgs.hip" in _build.SOURCES and "../../include/hefx_hybrid_bsgs.h" in _build.HEADERS
    text = open(os.path.join(ROOT, "include", "hefx_hybrid_bsgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(hefx_[a-z_0-9]+)\s*\(", src))) == capi.HYBRID_BSGS_SYMBOLS, "header and capi.py disagree"
    others = (capi.EXPORTED_SYMBOLS, capi.HYBRID_SYMBOLS, capi.HYBRID_HOIST_SYMBOLS, capi.ENCAPS_SYMBOLS, capi.DFT_SYMBOLS, capi.BOOTSTRAP_SYMBOLS)
    assert all(not set(capi.HYBRID_BSGS_SYMBOLS) & set(t) for t in others)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.library_path()], text=True)
    assert set(capi.HYBRID_BSGS_SYMBOLS) <= set(re.findall(r" T (hefx_[a-z_0-9]+)", out))
    c = tmp_path / "t.c"
    c.write_text('#include "hefx_hybrid_bsgs.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
