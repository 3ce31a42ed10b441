"""Hoisted hybrid key switching without a GPU (include/hefx_hybrid_hoist.h): seal.py's host statement against the independent
model of tests/hybrid_hoist_cases.py, the model against what is already pinned (element 1 with a real key is
HC.apply_galois_model), the noise bound under real keys, the decode errors of the combine and of the hybrid DFT against the
op-by-op hybrid composition, the front end's refusals and the C surface."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import hybrid_cases as HC
from tests import hybrid_hoist_cases as HH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_SEED = 3
STATEMENT_SETS = ("k7a2-p50_60", "k8a3-above60", "k7a4-d40_s60", "k4a1-p50_60")
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


@pytest.mark.parametrize("name,L", [(n, L) for n in STATEMENT_SETS for L in HC.sets()[n].levels])
def test_the_host_statement_is_the_model_word_for_word(name, L):
    from seal_fyp_logistic_regression_amd import seal as S
    s = HC.sets()[name]
    be = HC.twin(s)
    cts, elts, keys, pts = HH.case(s, L)
    rot, comb = HH.case_models(s, L)
    got = S.hybrid_hoist_host(be, s.primes, s.alpha, L, cts, elts, keys)
    assert len(got) == len(rot) == 6
    for t, (g, w) in enumerate(zip(got, rot)):
        assert np.array_equal(g, w), (name, L, "rotation", t)
    got = S.hybrid_hoist_host(be, s.primes, s.alpha, L, cts, elts, keys, pts)
    assert len(got) == len(comb) == 2
    for o, (g, w) in enumerate(zip(got, comb)):
        assert np.array_equal(g, w), (name, L, "output", o)


@pytest.mark.parametrize("name", STATEMENT_SETS)
def test_element_one_with_a_real_key_is_the_unhoisted_switch_and_other_elements_are_not(name):
    """at g = 1 nothing is permuted: the words of HC.apply_galois_model; at g = 3 the words DIFFER (the uncorrected base
    conversion does not commute with the automorphism's sign flips) -- the header says so"""
    s = HC.sets()[name]
    be, L = HC.twin(s), max(s.levels)
    ct, key = HC.operand(s, "uniform", L, 2, seed=77), HC.random_key(s, HC.SEED)
    one, three = HH.rotate_model(be, s.primes, s.alpha, L, [ct], [1, 3], [key, key])
    assert np.array_equal(one, HC.apply_galois_model(be, s.primes, s.alpha, L, ct, 1, key))
    # (at alpha = 1 too: a flipped coefficient is q_i - x before the lift and -(x mod q_m) after it, q_i mod q_m apart)
    assert not np.array_equal(three, HC.apply_galois_model(be, s.primes, s.alpha, L, ct, 3, key)), name


@pytest.mark.parametrize("name", ["k7a2-p50_60", "k8a3-above60"])
def test_a_combine_of_one_term_with_the_plaintext_one_is_the_hoisted_rotation(name):
    s = HC.sets()[name]
    be, L = HC.twin(s), max(s.levels)
    cts, elts, keys, _ = HH.case(s, L)
    rot, _ = HH.case_models(s, L)
    one = HH.plaintext(s, "one", 0)
    for t in (0, 1, 5):     # the identity term of source 0, element 3 of source 0, the conjugation of source 1
        row = [None] * 6
        row[t] = one
        assert np.array_equal(HH.combine_model(be, s.primes, s.alpha, L, cts, elts, keys, [row])[0], rot[t]), (name, t)


def noise_cases():
    out = []
    for name in STATEMENT_SETS:
        s = HC.sets()[name]
        for L in s.levels:
            B, Q = HC.noise_bound(s, L)
            if s.alpha > 1 and 4 * B < Q:
                out.append((name, L))
    return out


@pytest.mark.parametrize("name,L", noise_cases())
def test_the_hoisted_rotation_keeps_the_noise_bound_under_real_keys(name, L):
    """HC.noise_bound unchanged: |pi_g(ext_j)| < alpha D_j(L) still.  Measured through HC.switch_noise in exact integers."""
    e = env(name)
    s, be, N = e["s"], e["ctx"].backend, e["s"].N
    sk = e["kg"].secret_key().host
    B, Q = HC.noise_bound(s, L)
    elts = [3, 9, 2 * N - 1]
    keys = [host(e, e["gk"].hybrid_key(g)) for g in elts]
    worst = 0
    for kind in ("uniform", "max"):
        ct = HC.operand(s, kind, L, 2, seed=41 + L)
        for elt, out in zip(elts, HH.rotate_model(be, s.primes, s.alpha, L, [ct], elts, keys)):
            noise, Q_ = HC.switch_noise(s, L, "galois", elt, ct, out, sk)
            assert Q_ == Q
            worst = max(worst, noise)
    print(f"[hybrid hoist cpu] {name} L = {L}: noise {worst} (bound {B})")
    assert 0 < worst <= B


def decode_err(e, ct, want):
    return float(np.abs(e["encoder"].decode(e["dec"].decrypt(ct)) - want).max())


def test_decode_of_the_combine_against_the_op_by_op_composition():
    """steps (0, 1, 2), random weights in [-1, 1], level k - alpha, scale 2^40: hoisted <= 2 x op-by-op (both are dominated by
    the same encryption noise; the factor absorbs the second noise draw of the rotations) and <= 1e-3 of the largest value"""
    e = env("k7a2-p50_60")
    s, ev, encoder = e["s"], e["ev"], e["encoder"]
    top, n, scale = s.k - s.alpha, s.N // 2, 2.0 ** 40
    rng = np.random.default_rng(23)
    v = rng.uniform(-1.0, 1.0, n)
    w = rng.uniform(-1.0, 1.0, (3, n))
    want = sum(w[i] * np.roll(v, -i) for i in range(3))
    ct = e["enc"].encrypt(encoder.encode(v, scale, parms_id=top))
    hoisted = ev.plain_combine_hoisted([ct], [0, 1, 2], [[encoder.encode(w[i], scale, parms_id=s.k) for i in range(3)]], e["gk"])[0]
    assert hoisted.size() == 2 and hoisted.parms_id() == top and hoisted.scale == scale * scale
    rots = [ct] + [ev.rotate_vector(ct, i, e["gk"]) for i in (1, 2)]
    plain = ev.add_many([ev.multiply_plain(r, encoder.encode(w[i], scale, parms_id=top)) for i, r in enumerate(rots)])
    err_h, err_o, largest = decode_err(e, hoisted, want), decode_err(e, plain, want), float(np.abs(want).max())
    print(f"[hybrid hoist cpu] combine at {s.name}: decode error hoisted {err_h:.3e}, op by op {err_o:.3e}, largest value {largest:.3f}")
    assert 0 < err_h <= 2 * err_o and err_h <= CAP * largest
    assert not np.array_equal(host(e, hoisted.data), host(e, plain.data))     # one rounding per output: other words


def _op_by_op_stage(ev, xs, stage, table, gk):
    """algorithms._dft_stage on hybrid keys op by op: rotate_vector per baby and giant step, plain_combine, add_many, rescale"""
    nb, ng = len(stage.babies), len(stage.giants)
    rots = [x.copy() if b == 0 else ev.rotate_vector(x, b, gk) for x in xs for b in stage.babies]
    rows = []
    for c in range(stage.outputs):
        for gi in range(ng):
            row = [None] * (len(xs) * nb)
            for src, mat in {"split": [(0, c)], "lockstep": [(c, 0)], "merge": [(0, 0), (1, 1)], "single": [(0, 0)]}[stage.mode]:
                row[src * nb:(src + 1) * nb] = table[mat][gi]
            rows.append(row)
    inner = ev.plain_combine(rots, rows)
    moved = [x if g == 0 else ev.rotate_vector(x, g, gk) for x, g in zip(inner, list(stage.giants) * stage.outputs)]
    return ev.rescale_to_next_many_inplace([moved[c * ng] if ng == 1 else ev.add_many(moved[c * ng:(c + 1) * ng]) for c in range(stage.outputs)])


def _op_by_op(ev, xs, plan, tables, gk, conjugate):
    for stage, table in zip(plan.stages, tables):
        xs = _op_by_op_stage(ev, xs, stage, table, gk)
    return [ev.add(x, ev.complex_conjugate(x, gk)) for x in xs] if conjugate else xs


DFT_LEVELS = HH.DFT_LEVELS


def dft_env():
    return HH.dft_env("oracle")


def dft_programs(e, which):
    """(the hybrid program, the op-by-op program, the input values, the expected values) of the dense or the packed round trip"""
    hybrid, c2s, s2c, z, want = HH.dft_program(e, which)
    ev, gk, encoder, top = e["ev"], e["gk"], e["encoder"], e["top"]

    def op_by_op(ct):
        mid = _op_by_op(ev, [ct], c2s, c2s.encode(encoder, top), gk, True)
        return _op_by_op(ev, mid, s2c, s2c.encode(encoder, top - DFT_LEVELS), gk, False)[0]
    return lambda ct: hybrid(ct)[1], op_by_op, z, want


@pytest.mark.parametrize("which", ["dense", "packed"])
def test_decode_of_the_hybrid_dft_round_trip_against_plan_apply_and_the_op_by_op_run(which):
    """coeffs_to_slots_hybrid then slots_to_coeffs_hybrid (and the packed pair) against plan.apply: the error is at most twice
    that of the same plans run op by op with the same hybrid keys, and at most 1e-3 of the largest expected value"""
    e = dft_env()
    hybrid, op_by_op, z, want = dft_programs(e, which)
    ct = e["enc"].encrypt(e["encoder"].encode(z, 2.0 ** 40, parms_id=e["top"]))
    got_h, got_o = hybrid(ct), op_by_op(ct)
    assert got_h.size() == 2 and got_h.parms_id() == got_o.parms_id() == e["top"] - 2 * DFT_LEVELS
    assert abs(got_h.scale - got_o.scale) <= 2.0 ** -40 * got_o.scale
    err_h, err_o, largest = decode_err(e, got_h, want), decode_err(e, got_o, want), float(np.abs(want).max())
    print(f"[hybrid hoist cpu] {which} DFT round trip: decode error hybrid {err_h:.3e}, op by op {err_o:.3e}, largest value {largest:.3e}")
    assert 0 < err_h <= 2 * err_o and err_h <= CAP * largest


def test_the_front_end_refuses_and_the_old_composites_still_do():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import seal as S
    e = env("k7a2-p50_60")
    s, be, ev, gk, encoder = e["s"], e["ctx"].backend, e["ev"], e["gk"], e["encoder"]
    top = s.k - s.alpha
    at = lambda L: S.Ciphertext()._set(be.from_host(HC.operand(s, "uniform", L, 2, seed=2) if L <= top else
                                                    np.zeros((2, L, s.N), dtype=np.uint64)), 2, L, 2.0 ** 40)
    ct = at(top)
    key_pt = encoder.encode(np.ones(4), 2.0 ** 40, parms_id=s.k)
    with pytest.raises(ValueError, match=r"level <= k - alpha = 5"):
        ev.rotate_hoisted([at(top + 1)], [1], gk)
    with pytest.raises(ValueError, match=r"level <= k - alpha = 5"):
        ev.plain_combine_hoisted([at(top + 1)], [1], [[key_pt]], gk)
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.rotate_hoisted([ct], [1, 3], gk)
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.plain_combine_hoisted([ct], [0, 3], [[key_pt, key_pt]], gk)
    with pytest.raises(ValueError, match="key-level plaintexts"):
        ev.plain_combine_hoisted([ct], [0, 1], [[key_pt, encoder.encode(np.ones(4), 2.0 ** 40, parms_id=top)]], gk)
    with pytest.raises(ValueError, match="an output has no term"):
        ev.plain_combine_hoisted([ct], [0, 1], [[key_pt, None], [None, None]], gk)
    with pytest.raises(ValueError, match="one plaintext"):
        ev.plain_combine_hoisted([ct], [0, 1], [[key_pt]], gk)
    with pytest.raises(TypeError, match="HybridKeys"):
        ev.rotate_hoisted([ct], [1], e["kg"].galois_keys([1]))
    # rotate_hoisted: one list per input, a step of zero is a copy
    out = ev.rotate_hoisted([ct, ct], [0, 1], gk)
    assert [len(r) for r in out] == [2, 2] and np.array_equal(host(e, out[0][0].data), host(e, ct.data))
    assert np.array_equal(host(e, out[0][1].data), host(e, out[1][1].data))
    for call in (lambda: alg.coeffs_to_slots(ev, ct, None, gk), lambda: alg.slots_to_coeffs(ev, ct, ct, None, gk),
                 lambda: alg.coeffs_to_slots_packed(ev, ct, None, gk), lambda: alg.slots_to_coeffs_packed(ev, ct, None, gk),
                 lambda: alg.linear_transform_plain(ev, ct, [None, None], gk)):
        with pytest.raises(TypeError, match=r"with HybridKeys \(alpha = 2\) is not supported"):
            call()
    with pytest.raises(TypeError, match="HybridKeys"):
        alg.coeffs_to_slots_hybrid(ev, ct, dft_env()["plans"]["c2s"], e["kg"].galois_keys([1]))


def test_plan_encode_without_extended_returns_the_words_it_returned():
    """the default is the former code path, and extended=True has the same words in the stage's rows with all k rows present"""
    e = dft_env()
    plan, encoder, top, k = e["plans"]["pc2s"], e["encoder"], e["top"], e["s"].k
    be = e["ctx"].backend
    default, explicit, extended = plan.encode(encoder, top), plan.encode(encoder, top, extended=False), plan.encode(encoder, top, extended=True)
    seen = 0
    for i, st in enumerate(plan.stages):
        L = top - i
        todo = [st.rotated(c, g, b) for c in range(len(st.mats)) for g in st.giants for b in st.babies]
        reps = plan.n // st.n
        former = iter(encoder.encode_many([np.tile(v, reps) if reps > 1 else v for v in todo if v is not None], st.scale(), L))
        for c in range(len(st.mats)):
            for gi in range(len(st.giants)):
                for bi in range(len(st.babies)):
                    a, b, x = default[i][c][gi][bi], explicit[i][c][gi][bi], extended[i][c][gi][bi]
                    assert (a is None) == (b is None) == (x is None) == (st.rotated(c, st.giants[gi], st.babies[bi]) is None)
                    if a is None:
                        continue
                    f = next(former)
                    wa = np.asarray(be.to_host(a.data)).reshape(L, -1)
                    assert a.parms_id() == b.parms_id() == L and x.parms_id() == k and a.scale == b.scale == x.scale == f.scale == st.scale()
                    assert np.array_equal(wa, np.asarray(be.to_host(f.data)).reshape(L, -1))
                    assert np.array_equal(wa, np.asarray(be.to_host(b.data)).reshape(L, -1))
                    assert np.array_equal(wa, np.asarray(be.to_host(x.data)).reshape(k, -1)[:L])
                    seen += 1
    assert seen > 0


def test_capi_declares_the_two_symbols_and_the_build_lists_the_sources(tmp_path):
    from seal_fyp_logistic_regression_amd import _build, capi
    assert capi.HYBRID_HOIST_SYMBOLS == ["hefx_hybrid_plain_combine_hoisted", "hefx_hybrid_rotate_hoisted_batch"]
    assert "hefx_hybrid_hoist.hip" in _build.SOURCES and "../../include/hefx_hybrid_hoist.h" in _build.HEADERS
    text = open(os.path.join(ROOT, "include", "hefx_hybrid_hoist.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(hefx_[a-z_0-9]+)\s*\(", src))) == capi.HYBRID_HOIST_SYMBOLS, "header and capi.py disagree"
    others = (capi.EXPORTED_SYMBOLS, capi.HYBRID_SYMBOLS, capi.ENCAPS_SYMBOLS, capi.DFT_SYMBOLS, capi.BOOTSTRAP_SYMBOLS)
    assert all(not set(capi.HYBRID_HOIST_SYMBOLS) & set(t) for t in others)
    assert int(re.search(r"#define HEFX_HYBRID_HOIST_MAX_TERMS (\d+)", text).group(1)) == capi.HYBRID_HOIST_MAX_TERMS
    assert int(re.search(r"#define HEFX_HYBRID_HOIST_MAX_OUT (\d+)", text).group(1)) == capi.HYBRID_HOIST_MAX_OUT
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.library_path()], text=True)
    assert set(capi.HYBRID_HOIST_SYMBOLS) <= set(re.findall(r" T (hefx_[a-z_0-9]+)", out))
    c = tmp_path / "t.c"
    c.write_text('#include "hefx_hybrid_hoist.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
