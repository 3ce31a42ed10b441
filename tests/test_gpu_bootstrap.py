"""hefx_product_combine (include/hefx_bootstrap.h), algorithms.evaluate_polynomial_many and algorithms.bootstrap on the GPU.

hefx_product_combine, word for word against
  * the integer statement of the header in Python integers (tests/bootstrap_cases.product_model);
  * the composition it replaces, on the engine: hefx_mod_drop of every higher operand, hefx_multiply (hefx_square for a == b)
    per product, hefx_multiply_plain by the constant polynomial of each weight at size 3 / size 2, hefx_add_many per size, the
    size-2 sum added into the first two polynomials, hefx_add_plain of the constant.
One dimension varies at a time around L 2, n 1, P 1, m 1 at N = 1024: L 1, 2, 3; n 1, 2, 5; P 1, 2, 5 and 16, 17 (the fold
interval is 16 products: 16 runs without a fold when no linear term follows, 17 folds once); m 0, 1, 3 and 30, 31 (with P = 1
the 31st linear term is the first behind a fold); a square; operands of mixed levels; with and without the constant;
everything at q - 1 on 61-bit primes at N = 4096 across a fold; primes on both sides of 2^40 - 2^23, 2^41 and 2^60 in one call.
Refusals leave the outputs as they were; the entry returns while its stream is shut and its host arrays may be reused at once.

evaluate_polynomial_many (degree 31 Chebyshev, degree 7 power, two ciphertexts, both rescale divisions) gives the words of the
same host code on the oracle-backed twin, which has no product_combine and composes every node op by op; lazy=False gives the
words of evaluate_polynomial.  bootstrap: a one-prime ciphertext under a Hamming-weight-32 key comes back word for word the
twin's, one level above the bottom, and is squared once more.  Key switching needs N >= 2048 on the engine."""
import numpy as np
import pytest

from tests import bootstrap_cases as BC
from tests import policy_sets
from tests.test_gpu_poly import base_primes, engine, uniform

pytestmark = pytest.mark.gpu


def const_poly(e, res):
    return e.to_device(np.repeat(np.asarray(res, dtype=np.uint64)[:, None], e.N, axis=1))


def composed(e, L, dA, a_rows, dB, b_rows, dl, lin_rows, ures, wres, cres):
    """one item, call by call on the engine"""
    N = e.N
    low = lambda d, r: d if r == L else e.mod_drop(r, L, 2, d)
    terms3 = []
    for p in range(len(dA)):
        a = low(dA[p], a_rows[p])
        t = e.square(L, a) if dA[p] is dB[p] else e.multiply(L, a, low(dB[p], b_rows[p]))
        terms3.append(e.multiply_plain(L, 3, t, const_poly(e, ures[p])))
    acc = terms3[0] if len(terms3) == 1 else e.add_many(L, 3, terms3)
    if dl:
        terms2 = [e.multiply_plain(L, 2, low(d, r), const_poly(e, wres[k])) for k, (d, r) in enumerate(zip(dl, lin_rows))]
        lin2 = terms2[0] if len(terms2) == 1 else e.add_many(L, 2, terms2)
        out = e.empty(3, L, N)
        e.add(L, 2, acc.view(0, (2, L, N)), lin2, out=out.view(0, (2, L, N)))
        e.copy_raw(out.ptr + 16 * L * N, acc.ptr + 16 * L * N, 8 * L * N)
        acc = out
    if cres is not None:
        acc = e.add_plain(L, 3, acc, const_poly(e, cres))
    return acc.download().reshape(3, L, N)


def residues(rng, primes, count, L, maxed=False):
    if maxed:
        return np.broadcast_to(np.array([p - 1 for p in primes[:L]], dtype=np.uint64), (count, L)).copy()
    return np.array([[rng.integers(0, primes[j], dtype=np.uint64) for j in range(L)] for _ in range(count)],
                    dtype=np.uint64).reshape(count, L)


def run_case(N, primes, L=2, n=1, P=1, m=1, a_rows=None, b_rows=None, lin_rows=None, const=True, square=(), seed=1, maxed=False):
    e = engine(N, primes)
    rng = np.random.default_rng(seed)
    a_rows = list(a_rows) if a_rows is not None else [L] * P
    b_rows = list(b_rows) if b_rows is not None else [L] * P
    lin_rows = list(lin_rows) if lin_rows is not None else [L] * m
    assert all(a_rows[p] == b_rows[p] for p in square)   # a square is ONE operand: one row count
    draw = (lambda r: np.stack([np.repeat(np.array([[p - 1] for p in primes[:r]], dtype=np.uint64), N, axis=1)] * 2)) if maxed \
        else (lambda r: uniform(rng, primes, 2, r, N))
    A = [[draw(a_rows[p]) for p in range(P)] for _ in range(n)]
    B = [[A[i][p] if p in square else draw(b_rows[p]) for p in range(P)] for i in range(n)]
    Lin = [[draw(lin_rows[k]) for k in range(m)] for _ in range(n)]
    ures, wres = residues(rng, primes, P, L, maxed), residues(rng, primes, m, L, maxed)
    if m > 1 and not maxed:
        wres[1] = 0   # a weight of zero is legal: a term of zero
    cres = residues(rng, primes, 1, L, maxed)[0] if const else None
    dA = [[e.to_device(x) for x in row] for row in A]
    dB = [[dA[i][p] if p in square else e.to_device(B[i][p]) for p in range(P)] for i in range(n)]
    dL = [[e.to_device(x) for x in row] for row in Lin]
    outs = e.product_combine(L, dA, a_rows, dB, b_rows, ures, dL, lin_rows, wres if m else None, cres)
    assert len(outs) == n
    for i in range(n):
        got = outs[i].download()
        assert got.shape == (3, L, N)
        assert np.array_equal(got, BC.product_model(A[i], B[i], Lin[i], ures, wres, cres, L, primes)), ("integer model", i)
        assert np.array_equal(got, composed(e, L, dA[i], a_rows, dB[i], b_rows, dL[i], lin_rows, ures, wres, cres)), ("composition", i)
    for row, drow in zip(A + B + Lin, dA + dB + dL):   # inputs are only read
        for x, d in zip(row, drow):
            assert np.array_equal(d.download(), x)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_levels(L):
    run_case(1024, base_primes(), L=L)


@pytest.mark.parametrize("n", [1, 2, 5])
def test_items_in_lockstep(n):
    run_case(1024, base_primes(), n=n, seed=20 + n)


@pytest.mark.parametrize("P", [1, 2, 5, 16, 17])
def test_products_across_the_pair_loop_and_the_fold(P):
    run_case(1024, base_primes(), P=P, seed=30 + P)
    if P >= 16:
        run_case(1024, base_primes(), P=P, m=0, seed=60 + P)   # 16 products and nothing behind them: no fold at all


@pytest.mark.parametrize("m", [0, 1, 3, 30, 31])
def test_linear_terms_across_the_fold(m):
    run_case(1024, base_primes(), m=m, seed=40 + m)


def test_a_square_reads_one_operand_twice():
    run_case(1024, base_primes(), square=(0,))
    run_case(1024, base_primes(), P=3, n=2, m=2, square=(1,), seed=7)


def test_operands_of_mixed_levels_are_read_through_their_own_stride():
    run_case(1024, base_primes(), L=2, P=2, m=2, a_rows=(3, 2), b_rows=(2, 4), lin_rows=(4, 3), n=2)
    run_case(1024, base_primes(), L=3, P=3, m=1, a_rows=(5, 3, 4), b_rows=(4, 3, 3), lin_rows=(5,), square=(1,), seed=3)


def test_without_the_constant():
    run_case(1024, base_primes(), const=False)
    run_case(1024, base_primes(), const=False, P=3, m=0, n=2)


def test_everything_at_q_minus_1_on_61_bit_primes():
    """the accumulators' worst case: every factor q - 1, q just below 2^61, on top of the constant q - 1, across a fold in the
    products (17) and in the linear terms (P = 1, m = 31); N = 4096 (several workgroups per row)"""
    s = policy_sets.sets()["p_min61"]
    assert s.N == 4096 and all(p >> 60 for p in s.primes[:4])
    run_case(s.N, s.primes, L=4, P=17, m=3, maxed=True)
    run_case(s.N, s.primes, L=3, P=16, m=32, n=2, maxed=True)
    run_case(s.N, s.primes, L=3, P=1, m=31, maxed=True, const=False)


def test_primes_on_both_sides_of_every_policy_bound():
    N = 1024
    P = policy_sets
    primes = [P.primes_below(P.C40_LO, N, 1)[0], P.primes_above(P.C40_LO, N, 1)[0], P.primes_below(1 << 41, N, 1)[0],
              P.primes_above(1 << 41, N, 1)[0], P.primes_below(1 << 60, N, 1)[0], P.primes_above(1 << 60, N, 1)[0],
              P.primes_below(1 << 61, N, 1)[0]]
    run_case(N, primes, L=6, P=5, m=3, n=2)
    run_case(N, primes, L=6, P=17, m=1, maxed=True)


# ---- refusals: HEFX_ERR_INVALID, nothing written ---------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    N, primes, L, P, m, n = 1024, base_primes(), 2, 2, 1, 2
    e = engine(N, primes)
    rng = np.random.default_rng(9)
    rows = L + 1
    A = [[uniform(rng, primes, 2, rows, N) for _ in range(P)] for _ in range(n)]
    B = [[uniform(rng, primes, 2, rows, N) for _ in range(P)] for _ in range(n)]
    Lin = [[uniform(rng, primes, 2, rows, N) for _ in range(m)] for _ in range(n)]
    junk = rng.integers(0, 1 << 63, (n, 3, L, N), dtype=np.uint64)
    up = lambda M: [[e.to_device(x) for x in r] for r in M]
    dA, dB, dL = up(A), up(B), up(Lin)
    ones = lambda c: np.ones((c, L), dtype=np.uint64)

    def call(outs, dA_=None, dB_=None, dL_=None, ar=None, br=None, lr=None, u=None, w=None, c=None):
        e.product_combine(L, dA_ or dA, ar or [rows] * P, dB_ or dB, br or [rows] * P, ones(P) if u is None else u,
                          dL_ or dL, lr or [rows] * m, ones(m) if w is None else w, c, outs=outs)

    def refused(match, **kw):
        outs = [e.to_device(j) for j in junk]
        with pytest.raises(ValueError, match=match):
            call(outs, **kw)
        e.sync()
        for o, j in zip(outs, junk):
            assert np.array_equal(o.download(), j)

    # an output that shares bytes with an operand of ANOTHER item: the rows beyond the L that are read still count
    big = e.to_device(rng.integers(0, 1 << 40, (2 * 3 * rows * N,), dtype=np.uint64))
    d1 = big.view(0, (2, rows, N))
    before = big.download()
    for which in ("a", "b", "lin"):
        dA2 = [dA[0], [dA[1][0], d1]] if which == "a" else dA
        dB2 = [dB[0], [d1, dB[1][1]]] if which == "b" else dB
        dL2 = [dL[0], [d1]] if which == "lin" else dL
        for off in (0, N // 2, (2 * rows - 1) * N + N - 2):   # the exact alias, a shifted one, the operand's last two words
            with pytest.raises(ValueError, match="overlaps an input"):
                call([big.view(off, (3, L, N)), e.empty(3, L, N)], dA_=dA2, dB_=dB2, dL_=dL2)
        e.sync()
        assert np.array_equal(big.download(), before)
    call([big.view(2 * rows * N, (3, L, N)), e.empty(3, L, N)], dA_=[dA[0], [dA[1][0], d1]])   # adjacent: fine
    # two outputs that share bytes
    pair = e.to_device(rng.integers(0, 1 << 40, (2 * 3 * L * N,), dtype=np.uint64))
    before = pair.download()
    for second in (3 * L * N - 2, 0):
        with pytest.raises(ValueError, match="two outputs overlap"):
            call([pair.view(0, (3, L, N)), pair.view(second, (3, L, N))])
    e.sync()
    assert np.array_equal(pair.download(), before)
    # residues that are not below their modulus: a product weight, a linear weight, the constant
    u = ones(P)
    u[1, 1] = primes[1]
    refused("weight is not below", u=u)
    w = ones(m)
    w[0, 0] = primes[0]
    refused("weight is not below", w=w)
    c = np.zeros(L, dtype=np.uint64)
    c[1] = primes[1]
    refused("constant is not below", c=c)
    u[1, 1] = primes[1] - 1   # (the largest residue passes)
    call([e.empty(3, L, N) for _ in range(n)], u=u)
    # row counts below L
    refused("at least L rows", ar=[rows, L - 1])
    refused("at least L rows", br=[L - 1, rows])
    refused("at least L rows", lr=[L - 1])
    # P = 33, m = 65, n = 65
    with pytest.raises(ValueError, match="P out of range"):
        e.product_combine(L, [[dA[0][0]] * 33], [rows] * 33, [[dB[0][0]] * 33], [rows] * 33, ones(33), [[]], [], None, None,
                          outs=[e.empty(3, L, N)])
    with pytest.raises(ValueError, match="m out of range"):
        e.product_combine(L, [dA[0]], [rows] * P, [dB[0]], [rows] * P, ones(P), [[dL[0][0]] * 65], [rows] * 65, ones(65), None,
                          outs=[e.empty(3, L, N)])
    with pytest.raises(ValueError, match="n out of range"):
        e.product_combine(L, [dA[0]] * 65, [rows] * P, [dB[0]] * 65, [rows] * P, ones(P), [dL[0]] * 65, [rows] * m, ones(m), None,
                          outs=[e.empty(3, L, N) for _ in range(65)])


def test_of_two_faults_the_one_checked_first_is_reported():
    """hefx_product_combine checks its arguments in one fixed order: of two faults in one call the message is that of the
    check that stands first in the entry.  Every operand is a window of one buffer, which no refused call may touch."""
    from types import SimpleNamespace
    N, primes, L, P, m, n = 1024, base_primes(), 2, 2, 2, 2
    e = engine(N, primes)
    rows = L + 1
    blk = 2 * rows * N                                               # words of an operand, and of an output: 3 L N
    pool = e.to_device(np.random.default_rng(12).integers(0, 1 << 40, (14 * blk,), dtype=np.uint64))
    before = pool.download()
    table = lambda first: [[pool.view((first + 2 * i + p) * blk, (2, rows, N)) for p in range(2)] for i in range(n)]
    dA, dB, dL = table(0), table(4), table(8)                        # operand (i, p) of A is block 2 i + p, of B 4 + 2 i + p, ...
    outs = [pool.view((12 + i) * blk, (3, L, N)) for i in range(n)]
    on = lambda block, off=0: pool.view(block * blk + off, (3, L, N))
    null = SimpleNamespace(ptr=None)
    ok, few = [rows] * 2, [rows, L - 1]
    ones, c = np.ones((2, L), dtype=np.uint64), np.zeros(L, dtype=np.uint64)
    bad, c_bad = ones.copy(), c.copy()
    bad[1, 1], c_bad[1] = primes[1], primes[1]
    cases = [
        ("product_combine: every operand needs at least L rows", dict(ar=few, u=bad)),
        ("product_combine: every operand needs at least L rows", dict(lr=[L - 1, rows], br=few)),
        ("product_combine: every operand needs at least L rows", dict(ar=few, dB=[[dB[0][0], null], dB[1]])),
        ("product_combine: every linear term needs at least L rows", dict(lr=[L - 1, rows], w=bad)),
        ("null linear term in product_combine", dict(dL=[dL[0], [null, dL[1][1]]], w=bad)),
        ("product_combine: a weight is not below its modulus", dict(u=bad, c=c_bad)),
        ("product_combine: a weight is not below its modulus", dict(w=bad, c=c_bad)),
        ("product_combine: a constant is not below its modulus", dict(c=c_bad, outs=[outs[0], on(1)])),
        ("product_combine: an output overlaps an input (d_b, entry 0)", dict(outs=[on(4 + 2), on(1)])),
        ("product_combine: an output overlaps an input (d_a, entry 1)", dict(outs=[on(8), on(3)])),
        ("product_combine: two outputs overlap", dict(outs=[on(0), on(0, 2)])),
    ]
    for text, kw in cases:
        with pytest.raises(ValueError) as err:
            e.product_combine(L, kw.get("dA", dA), kw.get("ar", ok), kw.get("dB", dB), kw.get("br", ok), kw.get("u", ones),
                              kw.get("dL", dL), kw.get("lr", ok), kw.get("w", ones), kw.get("c", c), outs=kw.get("outs", outs))
        assert str(err.value) == text
    e.sync()
    assert np.array_equal(pool.download(), before)


# ---- asynchrony ------------------------------------------------------------------------------------------------------------
def test_returns_while_its_stream_is_shut_and_keeps_no_host_pointer():
    from tests.hip_stream_gate import Stream
    N, primes, L, P, m, n = 1024, base_primes(), 3, 2, 2, 2
    e = engine(N, primes)
    rng = np.random.default_rng(21)
    draw = lambda: [[uniform(rng, primes, 2, L, N) for _ in range(2 * P + m)] for _ in range(n)]
    reals, decoys = draw(), draw()
    ures, wres, cres = residues(rng, primes, P, L), residues(rng, primes, m, L), residues(rng, primes, 1, L)[0]
    split = lambda row: (row[:P], row[P:2 * P], row[2 * P:])
    want = [BC.product_model(*split(r), ures, wres, cres, L, primes) for r in reals]
    assert all((w != BC.product_model(*split(d), ures, wres, cres, L, primes)).any() for w, d in zip(want, decoys))
    dins, stage, dec = ([[e.to_device(x) for x in row] for row in src] for src in (decoys, reals, decoys))
    outs = [e.to_device(rng.integers(0, 1 << 63, (3, L, N), dtype=np.uint64)) for _ in range(n)]
    snaps = [e.empty(3, L, N) for _ in range(n)]
    e.sync()
    with Stream() as S:
        gate = S.gate()
        for ri, rs in zip(dins, stage):
            for i, s in zip(ri, rs):
                e.copy_raw(i.ptr, s.ptr, s.nbytes, S.handle)          # the real operands arrive on S, behind the gate
        u_host, w_host, c_host = ures.copy(), wres.copy(), cres.copy()
        e.product_combine(L, [split(r)[0] for r in dins], [L] * P, [split(r)[1] for r in dins], [L] * P, u_host,
                          [split(r)[2] for r in dins], [L] * m, w_host, c_host, outs=outs, stream=S.handle)
        u_host[:] = 0                                                 # the host arrays were copied before the call returned
        w_host[:] = 0
        c_host[:] = 0
        for o, s in zip(outs, snaps):
            e.copy_raw(s.ptr, o.ptr, o.nbytes, S.handle)
        for ri, rd in zip(dins, dec):
            for i, d in zip(ri, rd):
                e.copy_raw(i.ptr, d.ptr, d.nbytes, S.handle)          # ... and leave again on S
        assert not gate.opened, "hefx_product_combine waited on the host: its stream was still shut"
        e.sync(S.handle)
        assert gate.opened
    for i in range(n):
        assert np.array_equal(snaps[i].download(), want[i]) and np.array_equal(outs[i].download(), want[i])


# ---- composites at N = 2048 against the oracle-backed twin -------------------------------------------------------------------
@pytest.mark.parametrize("case", ["chebyshev31", "power7"])
def test_evaluate_polynomial_many_same_words_as_the_twin(case, rescale_mode):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import poly
    N = 2048
    if case == "chebyshev31":
        bits_, basis, coeffs = [60, 40, 40, 40, 40, 40, 60], "chebyshev", BC.evalmod_interpolant(31, 3)
        ref = lambda x: np.polynomial.chebyshev.chebval(x, coeffs)
    else:
        bits_, basis, coeffs = [60, 40, 40, 40, 60], "power", np.array(alg.SIGMOID_COEFFS[7])
        ref = lambda x: np.polynomial.polynomial.polyval(x, coeffs)
    xs = [np.linspace(-1.0, 1.0, N // 2), np.cos(np.arange(N // 2))]
    res = {}
    for kind in ("gpu", "oracle"):
        e = BC.make(N, bits_, kind, seed=3)
        assert (getattr(e["ctx"].backend, "product_combine", None) is not None) == (kind == "gpu")
        cts = [e["enc"].encrypt(e["encoder"].encode(x, 2.0 ** 40)) for x in xs]
        lazy = alg.evaluate_polynomial_many(e["ev"], cts, coeffs, e["rk"], basis=basis, lazy=True)
        eager = alg.evaluate_polynomial_many(e["ev"], cts, coeffs, e["rk"], basis=basis, lazy=False) if kind == "gpu" else None
        single = [alg.evaluate_polynomial(e["ev"], c, coeffs, e["rk"], basis=basis) for c in cts] if kind == "gpu" else None
        res[kind] = (e, lazy, eager, single)
    (eg, lg, gg, sg), (eo, lo, _, _) = res["gpu"], res["oracle"]
    plan = poly.plan(coeffs, basis, eg["ctx"].primes[:len(bits_) - 1], 2.0 ** 40)
    assert plan.relinearizations(True) < plan.muls   # something was deferred: the fused node ran
    for i, x in enumerate(xs):
        assert lg[i].size() == lo[i].size() == 2 and lg[i].parms_id() == lo[i].parms_id() == plan.result_level
        assert lg[i].scale == lo[i].scale == gg[i].scale == sg[i].scale
        assert np.array_equal(BC.words(eg, lg[i]), BC.words(eo, lo[i])), (case, "lazy", i)
        assert np.array_equal(BC.words(eg, gg[i]), BC.words(eg, sg[i])), (case, "lazy=False against evaluate_polynomial", i)
        for name, ct in (("lazy", lg[i]), ("eager", gg[i])):
            err = float(np.abs(eg["encoder"].decode(eg["dec"].decrypt(ct)).real - ref(x)).max())
            print(f"[gpu bootstrap] {case} {name} {rescale_mode} item {i}: max slot error {err:.3e}")
            assert err < 1e-6   # (a sanity bound on the decryption, far above the noise: the criterion is the words)


def test_bootstrap_same_words_as_the_twin_and_one_more_product():
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import bootstrap as B
    from seal_fyp_logistic_regression_amd import seal as S
    v = BC.bootstrap_input()
    plan = B.plan(BC.N, S.CoeffModulus.Create(BC.N, BC.CHAIN_BITS), BC.SCALE)
    res = {}
    for kind in ("gpu", "oracle"):
        e = BC.make(BC.N, BC.CHAIN_BITS, kind, seed=BC.KEY_SEED, hamming_weight=BC.HAMMING_WEIGHT,
                    galois_steps=plan.galois_steps(), conjugate=True)
        ct = e["enc"].encrypt(e["encoder"].encode(v, BC.SCALE, parms_id=1))
        assert ct.parms_id() == 1
        if kind == "gpu":   # a condition on the input: the key's integer part fits the plan
            _, I = BC.raised_coefficients(e, ct, plan.top_level)
            print(f"[gpu bootstrap] max |I| = {int(np.abs(I).max())} (K = {plan.K})")
            assert np.abs(I).max() <= 12
        out = alg.bootstrap(e["ev"], ct, plan, e["gk"], e["rk"], plan.encode(e["encoder"]))
        res[kind] = (e, ct, out)
    (eg, cg, og), (eo, co, oo) = res["gpu"], res["oracle"]
    assert np.array_equal(BC.words(eg, cg), BC.words(eo, co))
    assert og.size() == oo.size() == 2 and og.parms_id() == oo.parms_id() == plan.result_level == 2 and og.scale == oo.scale
    assert abs(og.scale / BC.SCALE - 1.0) < 1e-12   # ct's scale, as a computed value
    assert np.array_equal(BC.words(eg, og), BC.words(eo, oo))
    err = float(np.abs(eg["encoder"].decode(eg["dec"].decrypt(og)).real - v).max())
    sq = eg["ev"].rescale_to_next_inplace(eg["ev"].relinearize_inplace(eg["ev"].square(og), eg["rk"]))
    err2 = float(np.abs(eg["encoder"].decode(eg["dec"].decrypt(sq)).real - v * v).max())
    print(f"[gpu bootstrap] decode error {err:.3e}, after one more square {err2:.3e} (cap {BC.CAP:g})")
    assert sq.parms_id() == 1 and err <= BC.CAP and err2 <= 2 * BC.CAP   # (x + e)^2 - x^2 = 2 x e + e^2, |x| <= 1
