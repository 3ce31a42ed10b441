"""hefx_scalar_combine (include/hefx_poly.h) and algorithms.evaluate_polynomial on the GPU.

hefx_scalar_combine, word for word against
  * the composition it replaces, on the engine: hefx_mod_drop of every higher input, one scalar plaintext per weight,
    hefx_multiply_plain, hefx_add_many, hefx_add_plain (and once with the plaintexts made by hefx_ckks_encode_scalar from
    float weights, which also holds poly.weight_residue to the encoder's words, wide path included);
  * the integer statement of the header in Python integers: (sum_k w[g][k][j] * in[k][p][j][x] + [p == 0] c[g][j]) mod q_j.
One dimension varies at a time around size 2, L 2, m 3, G 1 at N = 1024: size 2 and 3; L 1, 2, 3; m 1, 3, 4, 5 (the unroll
tail), 33 and 65 (one and two folds, then a tail); G 1, 3, 16 (tiles of 1, 4 and two of 8); inputs of mixed levels; with and
without constants; everything at q - 1 on eight 61-bit primes at N = 4096 with m = 65 (the accumulator's worst case across a
fold); primes on both sides of 2^40 - 2^23, 2^41 and 2^60 in one call.
Refusals leave the outputs as they were; the entry returns while its stream is shut and its host arrays may be reused at once.

evaluate_polynomial (degrees 3, 7 and 31, both bases, both rescale divisions) and predict_cipher_weights(poly="ps") give the
words of the same host code on the oracle-backed twin, which has no scalar_combine and composes every COMBINE op by op.
Key switching needs N >= 2048 on the engine, so these run at N = 2048 (N = 4096 on the LR chain)."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import policy_sets
from tests.test_gpu_composites import make

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENGINES = {}


def engine(N, primes):
    from seal_fyp_logistic_regression_amd import Engine
    key = (N, tuple(primes))
    if key not in _ENGINES:
        _ENGINES[key] = Engine(N, list(primes))
    return _ENGINES[key]


def base_primes(N=1024):
    """a 60-bit prime, 40-bit primes, a 60-bit special prime: the layout of the engine's parameter sets"""
    from seal_fyp_logistic_regression_amd import seal as S
    return S.CoeffModulus.Create(N, [60, 40, 40, 40, 40, 60])


def uniform(rng, primes, size, rows, N):
    out = np.empty((size, rows, N), dtype=np.uint64)
    for j in range(rows):
        out[:, j] = rng.integers(0, primes[j], (size, N), dtype=np.uint64)
    return out


def model(ins, L, wres, cres, primes):
    """the header's statement in Python integers"""
    G, m = wres.shape[:2]
    size, N = ins[0].shape[0], ins[0].shape[2]
    outs = []
    for g in range(G):
        out = np.empty((size, L, N), dtype=np.uint64)
        for j in range(L):
            acc = np.zeros((size, N), dtype=object)
            for k in range(m):
                acc = acc + ins[k][:, j].astype(object) * int(wres[g, k, j])
            if cres is not None:
                acc[0] = acc[0] + int(cres[g, j])
            out[:, j] = (acc % primes[j]).astype(np.uint64)
        outs.append(out)
    return outs


def composed(e, L, size, dins, in_rows, wres, cres, plains=None):
    """the call-by-call sequence on the engine; plains[g][k]: device plaintexts to use instead of uploaded rows"""
    N = e.N
    low = [d if r == L else e.mod_drop(r, L, size, d) for d, r in zip(dins, in_rows)]
    outs = []
    for g in range(wres.shape[0]):
        prods = []
        for k, x in enumerate(low):
            pt = plains[g][k] if plains is not None else e.to_device(np.repeat(wres[g, k][:, None], N, axis=1))
            prods.append(e.multiply_plain(L, size, x, pt))
        acc = e.add_many(L, size, prods)
        if cres is not None:
            acc = e.add_plain(L, size, acc, e.to_device(np.repeat(cres[g][:, None], N, axis=1)))
        outs.append(acc.download())
    return outs


def run_case(N, primes, size=2, L=2, m=3, G=1, in_rows=None, consts=True, seed=1, maxed=False):
    e = engine(N, primes)
    rng = np.random.default_rng(seed)
    in_rows = list(in_rows) if in_rows is not None else [L] * m
    if maxed:
        ins = [np.stack([np.repeat(np.array([[p - 1] for p in primes[:r]], dtype=np.uint64), N, axis=1)] * size) for r in in_rows]
        wres = np.broadcast_to(np.array([p - 1 for p in primes[:L]], dtype=np.uint64), (G, m, L)).copy()
        cres = np.broadcast_to(np.array([p - 1 for p in primes[:L]], dtype=np.uint64), (G, L)).copy() if consts else None
    else:
        ins = [uniform(rng, primes, size, r, N) for r in in_rows]
        wres = np.stack([np.stack([np.array([rng.integers(0, primes[j], dtype=np.uint64) for j in range(L)]) for _ in range(m)])
                         for _ in range(G)])
        if m > 1:
            wres[0, 1] = 0   # a weight of zero is legal: a term of zero
        cres = np.stack([np.array([rng.integers(0, primes[j], dtype=np.uint64) for j in range(L)]) for _ in range(G)]) if consts else None
    dins = [e.to_device(x) for x in ins]
    outs = e.scalar_combine(L, size, dins, in_rows, wres, cres)
    got = [o.download() for o in outs]
    want = model(ins, L, wres, cres, primes)
    for g in range(G):
        assert got[g].shape == (size, L, N)
        assert np.array_equal(got[g], want[g]), ("integer model", g)
    for g, w in enumerate(composed(e, L, size, dins, in_rows, wres, cres)):
        assert np.array_equal(got[g], w.reshape(size, L, N)), ("composition", g)
    for x, d in zip(ins, dins):   # inputs are only read
        assert np.array_equal(d.download(), x)


@pytest.mark.parametrize("size", [2, 3])
def test_sizes(size):
    run_case(1024, base_primes(), size=size)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_levels(L):
    run_case(1024, base_primes(), L=L)


@pytest.mark.parametrize("m", [1, 3, 4, 5, 33, 65])
def test_terms_across_the_unroll_tail_and_the_fold(m):
    run_case(1024, base_primes(), m=m, seed=m)


@pytest.mark.parametrize("G", [1, 3, 16])
def test_outputs_across_the_tiles(G):
    run_case(1024, base_primes(), G=G, seed=10 + G)


def test_inputs_of_mixed_levels_are_read_through_their_own_stride():
    run_case(1024, base_primes(), L=2, in_rows=(2, 3, 4), size=3)
    run_case(1024, base_primes(), L=3, m=5, in_rows=(5, 3, 4, 3, 5), G=3)


def test_without_constants():
    run_case(1024, base_primes(), consts=False)
    run_case(1024, base_primes(), consts=False, G=3, m=4)


def test_everything_at_q_minus_1_on_61_bit_primes():
    """the accumulator's worst case: 65 products of (q - 1)^2, q just below 2^61, on top of the constant q - 1, across two
    folds and a tail; N = 4096 (several workgroups per row)"""
    s = policy_sets.sets()["p_min61"]
    assert s.N == 4096 and all(p >> 60 for p in s.primes[:8])
    run_case(s.N, s.primes, L=8, m=65, G=1, maxed=True)
    run_case(s.N, s.primes, L=3, m=33, G=3, maxed=True, consts=False)


def test_primes_on_both_sides_of_every_policy_bound():
    N = 1024
    P = policy_sets
    primes = [P.primes_below(P.C40_LO, N, 1)[0], P.primes_above(P.C40_LO, N, 1)[0], P.primes_below(1 << 41, N, 1)[0],
              P.primes_above(1 << 41, N, 1)[0], P.primes_below(1 << 60, N, 1)[0], P.primes_above(1 << 60, N, 1)[0],
              P.primes_below(1 << 61, N, 1)[0]]
    run_case(N, primes, L=6, m=5, G=3)
    run_case(N, primes, L=6, m=33, G=1, maxed=True)


def test_float_weights_are_the_words_of_encode_scalar():
    """poly.weight_residue == hefx_poly_weight_residue == the word hefx_ckks_encode_scalar writes (narrow and wide), and the
    composition through encoded plaintexts gives the fused call's words"""
    from seal_fyp_logistic_regression_amd import capi, poly
    N, primes, L, size = 1024, base_primes(), 3, 2
    e = engine(N, primes)
    rng = np.random.default_rng(5)
    weights = [(1.20069, 2.0 ** 40), (-0.81562, 2.0 ** 80), (1e-5, 2.0 ** 40), (-1.0, 1099511627775.0), (0.5, 1.0), (-2.5, 1.0),
               (3.0, 2.0 ** 63), (-4.19407, 2.0 ** 79.3)]
    m = len(weights)
    wres = np.empty((1, m, L), dtype=np.uint64)
    plains = []
    for k, (v, s) in enumerate(weights):
        pt = e.ckks_encode_scalar(L, [v], s)
        words = pt.download().reshape(L, N)
        assert (words == words[:, :1]).all()
        for j in range(L):
            assert poly.weight_residue(v, s, primes[j]) == int(words[j, 0]) == capi.lib().hefx_poly_weight_residue(v, s, primes[j]), (v, s, j)
        wres[0, k] = words[:, 0]
        plains.append(pt.view(0, (L, N)))
    ins = [uniform(rng, primes, size, L, N) for _ in range(m)]
    dins = [e.to_device(x) for x in ins]
    cpt = e.ckks_encode_scalar(L, [-1.0], 2.0 ** 80).download().reshape(L, N)
    cres = cpt[None, :, 0].copy()
    got = e.scalar_combine(L, size, dins, [L] * m, wres, cres)[0].download()
    assert np.array_equal(got, composed(e, L, size, dins, [L] * m, wres, cres, plains=[plains])[0].reshape(size, L, N))
    assert np.array_equal(got, model(ins, L, wres, cres, primes)[0])


# ---- refusals: HEFX_ERR_INVALID, nothing written ---------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    N, primes, L, size, m = 1024, base_primes(), 2, 2, 3
    e = engine(N, primes)
    rng = np.random.default_rng(9)
    ins = [uniform(rng, primes, size, L + 1, N) for _ in range(m)]
    junk = rng.integers(0, 1 << 63, (17, size, L, N), dtype=np.uint64)

    def fresh():
        return [e.to_device(x) for x in ins], [e.to_device(j) for j in junk]

    def weights(G):
        return np.ones((G, m, L), dtype=np.uint64)

    def refused(match, dins, outs, rows, w, c=None):
        with pytest.raises(ValueError, match=match):
            e.scalar_combine(L, size, dins, rows, w, c, outs=outs)
        e.sync()
        for o, j in zip(outs, junk):
            assert np.array_equal(o.download(), j)
        for d, x in zip(dins, ins):
            assert np.array_equal(d.download(), x)

    rows = [L + 1] * m
    dins, outs = fresh()
    # an output that shares bytes with an input: the rows beyond the L that are read still count
    big = e.to_device(rng.integers(0, 1 << 40, (2 * size * (L + 1) * N,), dtype=np.uint64))
    d1 = big.view(0, (size, L + 1, N))
    e.copy_raw(d1.ptr, dins[1].ptr, dins[1].nbytes)
    before = big.download()
    for off in (0, N // 2, (size * (L + 1) - 1) * N + N - 2):   # the exact alias, a shifted one, the input's last two words
        o = big.view(off, (size, L, N))
        with pytest.raises(ValueError, match="overlaps an input"):
            e.scalar_combine(L, size, [dins[0], d1, dins[2]], rows, weights(1), outs=[o])
        e.sync()
        assert np.array_equal(big.download(), before)
    e.scalar_combine(L, size, [dins[0], d1, dins[2]], rows, weights(1), outs=[big.view(size * (L + 1) * N, (size, L, N))])  # adjacent: fine
    # two outputs that share bytes
    dins, outs = fresh()
    pair = e.to_device(rng.integers(0, 1 << 40, (2 * size * L * N,), dtype=np.uint64))
    before = pair.download()
    with pytest.raises(ValueError, match="two outputs overlap"):
        e.scalar_combine(L, size, dins, rows, weights(2), outs=[pair.view(0, (size, L, N)), pair.view(size * L * N - 2, (size, L, N))])
    with pytest.raises(ValueError, match="two outputs overlap"):
        e.scalar_combine(L, size, dins, rows, weights(2), outs=[pair.view(0, (size, L, N)), pair.view(0, (size, L, N))])
    e.sync()
    assert np.array_equal(pair.download(), before)
    # a residue that is not below its modulus (weight, then constant)
    w = weights(1)
    w[0, 2, 1] = primes[1]
    refused("weight is not below", dins, outs[:1], rows, w)
    c = np.zeros((1, L), dtype=np.uint64)
    c[0, 0] = primes[0]
    refused("constant is not below", dins, outs[:1], rows, weights(1), c)
    w[0, 2, 1] = primes[1] - 1   # (the largest residue passes)
    e.scalar_combine(L, size, dins, rows, w, outs=[e.empty(size, L, N)])
    # an input with fewer rows than L
    refused("at least L rows", dins, outs[:1], [L + 1, L - 1, L + 1], weights(1))
    # G = 17, m = 0 and m = 257
    refused("G out of range", dins, outs[:17], rows, weights(17))
    with pytest.raises(ValueError, match="m out of range"):
        e.scalar_combine(L, size, [dins[0]] * 257, [L + 1] * 257, np.ones((1, 257, L), dtype=np.uint64), outs=outs[:1])
    e.sync()
    assert np.array_equal(outs[0].download(), junk[0])


def test_of_two_faults_the_one_checked_first_is_reported():
    """hefx_scalar_combine checks its arguments in one fixed order: of two faults in one call the message is that of the
    check that stands first in the entry.  Every operand is a window of one buffer, which no refused call may touch."""
    N, primes, L, size, m, G = 1024, base_primes(), 2, 2, 2, 2
    e = engine(N, primes)
    rows = L + 1
    blk = size * rows * N                                            # words of an input; an output is shorter
    pool = e.to_device(np.random.default_rng(12).integers(0, 1 << 40, (4 * blk,), dtype=np.uint64))
    before = pool.download()
    ins = [pool.view(k * blk, (size, rows, N)) for k in range(m)]
    outs = [pool.view((m + g) * blk, (size, L, N)) for g in range(G)]
    on = lambda k, off=0: pool.view(k * blk + off, (size, L, N))     # an output that shares bytes with input k
    null = SimpleNamespace(ptr=None)
    ok, few = [rows] * m, [rows, L - 1]
    w, c = np.ones((G, m, L), dtype=np.uint64), np.zeros((G, L), dtype=np.uint64)
    w_bad, c_bad = w.copy(), c.copy()
    w_bad[1, 1, 1], c_bad[0, 0] = primes[1], primes[0]
    cases = [
        ("scalar_combine: every input needs at least L rows", ins, few, w_bad, c, outs),
        ("scalar_combine: every input needs at least L rows", [ins[0], null], [L - 1, rows], w, c, outs),
        ("null input in scalar_combine", [null, ins[1]], few, w, c, outs),
        ("scalar_combine: a weight is not below its modulus", ins, ok, w_bad, c_bad, outs),
        ("scalar_combine: a constant is not below its modulus", ins, ok, w, c_bad, [outs[0], on(1)]),
        ("scalar_combine: an output overlaps an input (d_in, entry 0)", ins, ok, w, c, [on(1), on(0, N // 2)]),
        ("scalar_combine: two outputs overlap", ins, ok, w, c, [on(1), on(1, 2)]),
        ("scalar_combine: G out of range", ins, few, np.ones((17, m, L), dtype=np.uint64), None, [outs[0]] * 17),
    ]
    for text, ins_, rows_, w_, c_, outs_ in cases:
        with pytest.raises(ValueError) as err:
            e.scalar_combine(L, size, ins_, rows_, w_, c_, outs=outs_)
        assert str(err.value) == text
    e.sync()
    assert np.array_equal(pool.download(), before)


# ---- asynchrony ------------------------------------------------------------------------------------------------------------
def test_returns_while_its_stream_is_shut_and_keeps_no_host_pointer():
    from tests.hip_stream_gate import Stream
    N, primes, L, size, m, G = 1024, base_primes(), 3, 2, 5, 3
    e = engine(N, primes)
    rng = np.random.default_rng(21)
    reals = [uniform(rng, primes, size, L, N) for _ in range(m)]
    decoys = [uniform(rng, primes, size, L, N) for _ in range(m)]
    wres = np.stack([np.stack([np.array([rng.integers(1, primes[j], dtype=np.uint64) for j in range(L)]) for _ in range(m)]) for _ in range(G)])
    cres = np.stack([np.array([rng.integers(0, primes[j], dtype=np.uint64) for j in range(L)]) for _ in range(G)])
    want, want_decoy = model(reals, L, wres, cres, primes), model(decoys, L, wres, cres, primes)
    assert all((a != b).any() for a, b in zip(want, want_decoy))
    dins, stage, dec = ([e.to_device(x) for x in src] for src in (decoys, reals, decoys))
    outs = [e.to_device(rng.integers(0, 1 << 63, (size, L, N), dtype=np.uint64)) for _ in range(G)]
    snaps = [e.empty(size, L, N) for _ in range(G)]
    e.sync()
    with Stream() as S:
        gate = S.gate()
        for i, s in zip(dins, stage):
            e.copy_raw(i.ptr, s.ptr, s.nbytes, S.handle)          # the real operands arrive on S, behind the gate
        w_host, c_host = wres.copy(), cres.copy()
        e.scalar_combine(L, size, dins, [L] * m, w_host, c_host, outs=outs, stream=S.handle)
        w_host[:] = 0                                             # the host arrays were copied before the call returned
        c_host[:] = 0
        for o, s in zip(outs, snaps):
            e.copy_raw(s.ptr, o.ptr, o.nbytes, S.handle)
        for i, d in zip(dins, dec):
            e.copy_raw(i.ptr, d.ptr, d.nbytes, S.handle)          # ... and leave again on S
        assert not gate.opened, "hefx_scalar_combine waited on the host: its stream was still shut"
        e.sync(S.handle)
        assert gate.opened
    for g in range(G):
        assert np.array_equal(snaps[g].download(), want[g]) and np.array_equal(outs[g].download(), want[g])


# ---- evaluate_polynomial against the oracle-backed twin ------------------------------------------------------------------------
def words(e, ct):
    return np.asarray(e["ctx"].backend.to_host(ct.data)).reshape(ct.size(), ct.parms_id(), e["ctx"].N)


def chebyshev_interpolant(d):
    k = np.arange(d + 1)
    nodes = np.cos(np.pi * (k + 0.5) / (d + 1))
    return np.polynomial.chebyshev.chebfit(nodes, 1.0 / (1.0 + np.exp(-6.0 * nodes)), d)


@pytest.mark.parametrize("d", [3, 7, 31])
def test_evaluate_polynomial_same_words_as_the_twin(d, rescale_mode):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    N = 2048
    bits_ = [60, 40, 40, 40, 60] if d <= 7 else [60, 40, 40, 40, 40, 40, 60]
    x = np.linspace(-1.0, 1.0, N // 2)
    if d <= 7:
        power = np.array(alg.SIGMOID_COEFFS[d])
        cases = [("power", power), ("chebyshev", np.polynomial.chebyshev.poly2cheb(power))]
        want = {b: np.polynomial.polynomial.polyval(x, power) for b, _ in cases}
    else:
        cheb = chebyshev_interpolant(d)
        power = np.zeros(d + 1)
        power[[0, 1, 3, 17, 31]] = [0.5, 1.25, -0.75, 0.5, -0.375]   # sparse: chunks that vanish, chunks that are one monomial
        cases = [("power", power), ("chebyshev", cheb)]
        want = {"power": np.polynomial.polynomial.polyval(x, power), "chebyshev": np.polynomial.chebyshev.chebval(x, cheb)}
    res = {}
    for kind in ("gpu", "oracle"):
        e = make(N, bits_, kind, seed=3)
        assert (getattr(e["ctx"].backend, "scalar_combine", None) is not None) == (kind == "gpu")
        ct = e["enc"].encrypt(e["encoder"].encode(x, 2.0 ** 40))
        res[kind] = (e, [alg.evaluate_polynomial(e["ev"], ct, c, e["rk"], basis=b) for b, c in cases])
    (eg, rg), (eo, ro) = res["gpu"], res["oracle"]
    for (basis, _), g, o in zip(cases, rg, ro):
        depth = int(np.ceil(np.log2(d + 1)))
        assert g.size() == o.size() == 2 and g.parms_id() == o.parms_id() == len(bits_) - 1 - depth and g.scale == o.scale
        assert np.array_equal(words(eg, g), words(eo, o)), (d, basis)
        err = float(np.abs(eg["encoder"].decode(eg["dec"].decrypt(g)).real - want[basis]).max())
        print(f"[gpu poly] degree {d} {basis} {rescale_mode}: max slot error {err:.3e}")
        assert err < 1e-6   # (a sanity bound on the decryption, far above the noise: the criterion is the words)


def test_predict_ps_same_words_as_the_twin_and_no_worse_than_horner():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from tests import lr_gradient_cases as C
    shape = (3, 4)
    X, w, y = C.inputs(*shape)
    coeffs = alg.SIGMOID_COEFFS[3]
    z = np.array([C.plain_dot_product(X[i], w, shape[1])[i] for i in range(shape[0])])
    want = sum(c * z ** k for k, c in enumerate(coeffs))
    out = {}
    for kind in ("gpu", "oracle"):
        e = make(4096, C.LR_BITS, kind, seed=C.KEY_SEED)
        feats, _, _, cw = C.encrypt_inputs(e, X, w, y)
        run = lambda p: alg.predict_cipher_weights(e["ev"], e["encoder"], e["enc"], feats, cw, shape[1], C.SCALE, e["gk"], e["rk"], poly=p)
        out[kind] = (e, run("ps"), run("horner") if kind == "gpu" else None)
    (eg, pg, hg), (eo, po, _) = out["gpu"], out["oracle"]
    assert C.compare(eg, pg, eo, po) == []
    assert pg.parms_id() == hg.parms_id() + 1 and pg.scale == C.SCALE   # two levels instead of three, the scale tracked
    err = lambda ct: float(np.abs(eg["encoder"].decode(eg["dec"].decrypt(ct))[:shape[0]].real - want).max())
    e_ps, e_h = err(pg), err(hg)
    print(f"[gpu poly] predict (3, 4): max slot error ps {e_ps:.3e}, horner {e_h:.3e}")
    assert e_ps <= 2 * e_h


def test_poly_selftest_runs_to_its_end():
    exe = os.path.join(ROOT, "drivers", "_ref", "poly_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "drivers"), "_ref/poly_selftest"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "POLY SELFTEST PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
