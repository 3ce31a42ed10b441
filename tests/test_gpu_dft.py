"""hefx_plain_combine (include/hefx_dft.h) and algorithms.coeffs_to_slots / slots_to_coeffs on the GPU.

hefx_plain_combine, word for word against
  * the header's statement in Python integers: (sum over the non-null k of pt[g][k][j][x] * in[k][p][j][x]) mod q_j;
  * hefx_multiply_plain_sum on the same pointers, output by output (the path it replaces).
One dimension varies at a time around L 2, m 3, G 1 at N = 1024: L 1, 2, 3; m 1, 3, 4, 5 (the unroll tail); G 1, 2, 3, 4, 5, 8,
9 and 17.  The width of a tile of outputs is chosen by the call's wave count, and at N = 1024 every tile is one output wide:
the widths 2, 4 and 8, both sides of every change of width, padded last tiles and one tile against several run at N = 32768,
L = 8, where the integer model is checked on sampled slots and the old entry in full.  A sparse matrix with an output of a
single term, an input no output uses, an input only ANOTHER tile's outputs use and a NULL in every unroll position and in the
tail; everything at q - 1 with m = 33 and m = 65 on the 61-bit set at N = 4096 (the accumulator's worst case on both sides
of a fold); primes on both sides of 2^40 - 2^23, 2^41 and 2^60 in one call.
Refusals leave the outputs as they were; the entry returns while its stream is shut and its pointer array may be reused at once.

The transforms (CoeffToSlot, SlotToCoeff, the round trip) give on the engine, word for word, the ciphertexts of the same plan
run OP BY OP on the oracle-backed twin -- single rotations, multiply_plain, add, rescale, conjugation -- under both rescale
divisions, and pass the decode gate of tests/test_dft_cpu.py (error <= 1e-3 * max|expected|).  Parameters, seeds and plan are
those of the CPU test except the ring: key switching needs N >= 2048 on the engine, so these run at N = 2048."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import policy_sets
from tests.test_gpu_composites import make
from tests.test_gpu_poly import base_primes, engine, uniform

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model(ins, pts, rows, L, primes, cols=None):
    """the header's statement in Python integers; rows[g][k]: index into pts or None; cols: the slots to compute (all)"""
    cols = np.arange(ins[0].shape[2]) if cols is None else cols
    outs = []
    for r in rows:
        out = np.empty((2, L, len(cols)), dtype=np.uint64)
        for j in range(L):
            acc = np.zeros((2, len(cols)), dtype=object)
            for k, t in enumerate(r):
                if t is not None:
                    acc = acc + ins[k][:, j, cols].astype(object) * pts[t][j, cols].astype(object)[None, :]
            out[:, j] = (acc % primes[j]).astype(np.uint64)
        outs.append(out)
    return outs


def big_primes():
    """N = 32768, eight data rows: L * N / 128 = 2048 waves a tile, where the tile rule (hefx_capi.cpp, plain_combine_tile:
    the widest of 8, 4, 2, 1 outputs that still gives the call 4096 waves) takes width 1 for G <= 2, 2 for G = 3 and 4, 4 for
    G = 5 .. 8 and 8 from G = 9 up; at N = 1024 every tile is one output wide"""
    from seal_fyp_logistic_regression_amd import seal as S
    return S.CoeffModulus.Create(32768, [60] + [40] * 7 + [60])


def run_case(N, primes, L=2, m=3, G=1, rows=None, seed=1, maxed=False, sample=None):
    """sample: check the integer model on that many random slots only (large N); the old entry is compared in full"""
    e = engine(N, primes)
    rng = np.random.default_rng(seed)
    if rows is None:
        rows = [[(g * m + k) % 7 for k in range(m)] for g in range(G)]   # dense; seven plaintexts stand in several places
    npts = 1 + max(t for r in rows for t in r if t is not None)
    if maxed:
        top = np.repeat(np.array([[p - 1] for p in primes[:L]], dtype=np.uint64), N, axis=1)
        ins, pts = [np.stack([top, top])] * m, [top] * npts
    else:
        ins = [uniform(rng, primes, 2, L, N) for _ in range(m)]
        pts = [uniform(rng, primes, 1, L, N)[0] for _ in range(npts)]
    dins, dpts = [e.to_device(x) for x in ins], [e.to_device(p) for p in pts]
    matrix = [[None if t is None else dpts[t] for t in r] for r in rows]
    got = [o.download() for o in e.plain_combine(L, dins, matrix)]
    if maxed:   # every word of a row is the same number: (terms * (q - 1)^2) mod q
        want = [np.stack([np.repeat(np.array([[sum(t is not None for t in r) * (p - 1) ** 2 % p] for p in primes[:L]],
                                             dtype=np.uint64), N, axis=1)] * 2) for r in rows]
    else:
        cols = None if sample is None else np.sort(rng.choice(N, sample, replace=False))
        want = model(ins, pts, rows, L, primes, cols)
    for g, r in enumerate(rows):
        assert got[g].shape == (2, L, N)
        assert np.array_equal(got[g] if maxed or sample is None else got[g][:, :, cols], want[g]), ("integer model", g)
        terms = [k for k, t in enumerate(r) if t is not None]   # the same pointers through the entry it replaces
        old = e.multiply_plain_sum(L, 2, [dins[k] for k in terms], [matrix[g][k] for k in terms])[0].download()
        assert np.array_equal(got[g], old.reshape(2, L, N)), ("multiply_plain_sum", g)
    for x, d in zip(ins + pts, dins + dpts):   # operands are only read
        assert np.array_equal(d.download(), x)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_levels(L):
    run_case(1024, base_primes(), L=L)


@pytest.mark.parametrize("m", [1, 3, 4, 5])
def test_terms_across_the_unroll_tail(m):
    run_case(1024, base_primes(), m=m, seed=m)


@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 8, 9, 17])
def test_outputs_across_the_tiles_of_one(G):
    run_case(1024, base_primes(), G=G, seed=10 + G)


@pytest.mark.parametrize("G", [2, 3, 4, 5, 8, 9, 16, 17])
def test_outputs_on_both_sides_of_every_tile_width(G):
    """widths 1 | 2 | 2 | 4 | 4 | 8 | 8 | 8 (big_primes): both sides of every change of width, a last tile that is padded
    (3, 5, 9, 17) and one that is full, one tile and several"""
    run_case(32768, big_primes(), L=8, m=5, G=G, seed=40 + G, sample=48)


def test_sparse_matrix():
    """m = 9 (two unrolled groups and a tail of one), G = 10: an output with a single term (0), an input no output uses (4), an
    input only the outputs 8 and 9 use (7), a NULL in each of the four unroll positions of both groups and in the tail, an
    output whose only terms sit in the tail and the second group.  At N = 1024 in ten tiles of one output; at N = 32768,
    L = 8 in a tile of eight and a padded second one, which alone reads input 7"""
    X = None
    rows = [[X, X, X, X, X, X, 0, X, X],
            [0, X, 1, 2, X, 3, 4, X, 5],
            [X, 0, 1, X, X, X, 2, X, 3],
            [0, 1, X, 2, X, 3, X, X, X],
            [0, 1, 2, 3, X, 4, 5, X, 6],
            [X, X, X, X, X, X, X, X, 2],
            [6, X, X, 5, X, X, 4, X, X],
            [X, 3, X, X, X, 2, X, X, 1],
            [1, X, X, X, X, X, X, 2, X],
            [X, X, 3, X, X, 4, X, 5, 6]]
    assert all(any(r[k] is None for r in rows) for k in range(9)) and all(r[4] is None for r in rows)
    assert all(r[7] is None for r in rows[:8]) and any(r[7] is not None for r in rows[8:])
    run_case(1024, base_primes(), L=3, m=9, G=10, rows=rows, seed=77)
    run_case(32768, big_primes(), L=8, m=9, G=10, rows=rows, seed=78, sample=32)


@pytest.mark.parametrize("m", [33, 65])
def test_everything_at_q_minus_1_on_61_bit_primes(m):
    """the accumulator's worst case: m products of (q - 1)^2, q just below 2^61, across one fold (33) and two (65) and a tail;
    N = 4096; dense and with NULLs that move the terms against the fold positions"""
    s = policy_sets.sets()["p_min61"]
    assert s.N == 4096 and all(p >> 60 for p in s.primes[:8])
    run_case(s.N, s.primes, L=8 if m == 65 else 3, m=m, G=1, maxed=True)
    rows = [[0] * m, [None if k % 5 == 2 else 0 for k in range(m)], [0 if k >= 31 else None for k in range(m)]]
    run_case(s.N, s.primes, L=2, m=m, G=3, rows=rows, maxed=True)


def test_primes_on_both_sides_of_every_policy_bound():
    N = 1024
    P = policy_sets
    primes = [P.primes_below(P.C40_LO, N, 1)[0], P.primes_above(P.C40_LO, N, 1)[0], P.primes_below(1 << 41, N, 1)[0],
              P.primes_above(1 << 41, N, 1)[0], P.primes_below(1 << 60, N, 1)[0], P.primes_above(1 << 60, N, 1)[0],
              P.primes_below(1 << 61, N, 1)[0]]
    run_case(N, primes, L=6, m=5, G=3)
    run_case(N, primes, L=7, m=33, G=1, maxed=True)


# ---- refusals: nothing written ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    from seal_fyp_logistic_regression_amd import capi
    N, primes, L, m = 1024, base_primes(), 2, 3
    e = engine(N, primes)
    rng = np.random.default_rng(9)
    ins = [uniform(rng, primes, 2, L, N) for _ in range(m)]
    pts = [uniform(rng, primes, 1, L, N)[0] for _ in range(m)]
    junk = rng.integers(0, 1 << 63, (3, 2, L, N), dtype=np.uint64)
    dins, dpts = [e.to_device(x) for x in ins], [e.to_device(p) for p in pts]
    outs = [e.to_device(j) for j in junk]
    null = SimpleNamespace(ptr=None)

    def refused(match, ins_, matrix, outs_, level=L, exc=ValueError):
        with pytest.raises(exc, match=match):
            e.plain_combine(level, ins_, matrix, outs=outs_)
        e.sync()
        for o, j in zip(outs, junk):
            assert np.array_equal(o.download(), j)
        for d, x in zip(dins + dpts, ins + pts):
            assert np.array_equal(d.download(), x)

    refused("an output has no term", dins, [dpts, [None] * m], outs[:2])
    refused("null input", [dins[0], null, dins[2]], [dpts], outs[:1])
    refused("null output", dins, [dpts, dpts], [outs[0], null])
    refused("level L out of range", dins, [dpts], outs[:1], level=0)
    refused("level L out of range", dins, [dpts], outs[:1], level=len(primes) + 1)
    refused("m out of range", [dins[0]] * 257, [[dpts[0]] * 257], outs[:1])
    refused("G out of range", dins, [dpts] * 65, [outs[0]] * 65)
    with pytest.raises(ValueError, match="m out of range"):
        capi.check(capi.lib().hefx_plain_combine(e._h, L, 0, capi.ptr_array([dins[0].ptr]), 1, capi.ptr_array([dpts[0].ptr]),
                                                 capi.ptr_array([outs[0].ptr]), None))
    # 256 + 64 * 256 + 64 pointers do not fit a descriptor slot: UNSUPPORTED, before anything is submitted
    many = e.empty_many(64, (2, L, N))
    refused("do not fit a descriptor slot", [dins[0]] * 256, [[dpts[0]] * 256] * 64, many, exc=capi.HefxError)
    # an output that shares bytes with an input: the exact alias, a shifted one, the input's last two words
    big = e.to_device(rng.integers(0, 1 << 40, (2 * 2 * L * N,), dtype=np.uint64))
    d1 = big.view(0, (2, L, N))
    e.copy_raw(d1.ptr, dins[1].ptr, dins[1].nbytes)
    before = big.download()
    for off in (0, N // 2, 2 * L * N - 2):
        with pytest.raises(ValueError, match=r"overlaps an input \(d_in, entry 1\)"):
            e.plain_combine(L, [dins[0], d1, dins[2]], [dpts], outs=[big.view(off, (2, L, N))])
        e.sync()
        assert np.array_equal(big.download(), before)
    e.plain_combine(L, [dins[0], d1, dins[2]], [dpts], outs=[big.view(2 * L * N, (2, L, N))])   # adjacent: fine
    # ... with a plaintext: its first and its last two words (a plaintext is half an output long)
    big = e.to_device(rng.integers(0, 1 << 40, (3 * 2 * L * N,), dtype=np.uint64))
    p1 = big.view(2 * L * N, (L, N))
    e.copy_raw(p1.ptr, dpts[1].ptr, dpts[1].nbytes)
    before = big.download()
    for off in (2 * L * N, 3 * L * N - 2, 2):
        with pytest.raises(ValueError, match=r"overlaps an input \(d_pts, entry 4\)"):
            e.plain_combine(L, dins, [dpts, [None, p1, None]], outs=[outs[0], big.view(off, (2, L, N))])
        e.sync()
        assert np.array_equal(big.download(), before) and np.array_equal(outs[0].download(), junk[0])
    e.plain_combine(L, dins, [[None, p1, None]], outs=[big.view(0, (2, L, N))])                  # adjacent in front: fine
    # two outputs that share bytes
    pair = e.to_device(rng.integers(0, 1 << 40, (2 * 2 * L * N,), dtype=np.uint64))
    before = pair.download()
    for second in (2 * L * N - 2, 0):
        with pytest.raises(ValueError, match="two outputs overlap"):
            e.plain_combine(L, dins, [dpts, dpts], outs=[pair.view(0, (2, L, N)), pair.view(second, (2, L, N))])
    e.sync()
    assert np.array_equal(pair.download(), before)
    for o, j in zip(outs, junk):
        assert np.array_equal(o.download(), j)


def test_of_two_faults_the_one_checked_first_is_reported():
    """hefx_plain_combine checks its arguments in one fixed order: of two faults in one call the message is that of the
    check that stands first in the entry.  Every operand is a window of one buffer, which no refused call may touch."""
    N, primes, L, m, G = 1024, base_primes(), 2, 2, 2
    e = engine(N, primes)
    blk = 2 * L * N                                                  # words of an input and of an output; a plaintext is half
    pool = e.to_device(np.random.default_rng(12).integers(0, 1 << 40, (6 * blk,), dtype=np.uint64))
    before = pool.download()
    ins = [pool.view(k * blk, (2, L, N)) for k in range(m)]
    pts = [pool.view(2 * blk + k * (blk // 2), (L, N)) for k in range(4)]
    outs = [pool.view((4 + g) * blk, (2, L, N)) for g in range(G)]
    on = lambda word: pool.view(word, (2, L, N))
    null = SimpleNamespace(ptr=None)
    full, holes = [pts[:2], pts[2:]], [[None, None], pts[2:]]
    cases = [
        ("plain_combine: an output has no term", ins, holes, [outs[0], null]),
        ("null output in plain_combine", ins, [pts[:2], [None, None]], [null, outs[1]]),
        ("null input in plain_combine", [ins[0], null], holes, outs),
        ("plain_combine: G out of range", [ins[0], null], [pts[:2]] * 65, [outs[0]] * 65),
        ("plain_combine: an output overlaps an input (d_in, entry 0)", ins, full, [on(blk), on(0)]),
        ("plain_combine: an output overlaps an input (d_in, entry 1)", ins, full, [on(2 * blk + 3 * (blk // 2) - 2), on(blk + 2)]),
        ("plain_combine: two outputs overlap", ins, full, [on(blk), on(blk + 2)]),
    ]
    for text, ins_, matrix, outs_ in cases:
        with pytest.raises(ValueError) as err:
            e.plain_combine(L, ins_, matrix, outs=outs_)
        assert str(err.value) == text
    e.sync()
    assert np.array_equal(pool.download(), before)


# ---- asynchrony ------------------------------------------------------------------------------------------------------------
def test_returns_while_its_stream_is_shut_and_keeps_no_host_pointer():
    import ctypes as C
    from seal_fyp_logistic_regression_amd import capi
    from tests.hip_stream_gate import Stream
    N, primes, L, m, G = 1024, base_primes(), 3, 5, 10
    e = engine(N, primes)
    rng = np.random.default_rng(21)
    reals = [uniform(rng, primes, 2, L, N) for _ in range(m)]
    decoys = [uniform(rng, primes, 2, L, N) for _ in range(m)]
    pts = [uniform(rng, primes, 1, L, N)[0] for _ in range(4)]
    rows = [[None if (g + k) % 3 == 0 else (g + 2 * k) % 4 for k in range(m)] for g in range(G)]
    want, want_decoy = model(reals, pts, rows, L, primes), model(decoys, pts, rows, L, primes)
    assert all((a != b).any() for a, b in zip(want, want_decoy))
    dins, stage, dec = ([e.to_device(x) for x in src] for src in (decoys, reals, decoys))
    dpts = [e.to_device(p) for p in pts]
    outs = [e.to_device(rng.integers(0, 1 << 63, (2, L, N), dtype=np.uint64)) for _ in range(G)]
    snaps = [e.empty(2, L, N) for _ in range(G)]
    e.sync()
    with Stream() as S:
        gate = S.gate()
        for i, s in zip(dins, stage):
            e.copy_raw(i.ptr, s.ptr, s.nbytes, S.handle)          # the real operands arrive on S, behind the gate
        in_arr = (C.c_void_p * m)(*[d.ptr for d in dins])
        pt_arr = (C.c_void_p * (G * m))(*[None if t is None else dpts[t].ptr for r in rows for t in r])
        out_arr = (C.c_void_p * G)(*[o.ptr for o in outs])
        capi.check(capi.lib().hefx_plain_combine(e._h, L, m, in_arr, G, pt_arr, out_arr, S.handle))
        for arr in (in_arr, pt_arr, out_arr):                    # the pointer arrays were copied before the call returned
            C.memset(arr, 0, C.sizeof(arr))
        for o, s in zip(outs, snaps):
            e.copy_raw(s.ptr, o.ptr, o.nbytes, S.handle)
        for i, d in zip(dins, dec):
            e.copy_raw(i.ptr, d.ptr, d.nbytes, S.handle)          # ... and leave again on S
        assert not gate.opened, "hefx_plain_combine waited on the host: its stream was still shut"
        e.sync(S.handle)
        assert gate.opened
    for g in range(G):
        assert np.array_equal(snaps[g].download(), want[g]) and np.array_equal(outs[g].download(), want[g])


# ---- the transforms against the same plan run op by op on the oracle-backed twin ----------------------------------------------
N_T, LEVELS, SCALE, CAP = 2048, 3, 2.0 ** 40, 1e-3
BITS = [60] + [40] * 7 + [60]


def words(e, ct):
    return np.asarray(e["ctx"].backend.to_host(ct.data)).reshape(ct.size(), ct.parms_id(), e["ctx"].N)


def stage_op_by_op(ev, xs, stage, table, gk):
    """dft.Stage, one evaluator call per operation: rotate_vector, multiply_plain, add, rescale_to_next"""
    rots = [[x if b == 0 else ev.rotate_vector(x, b, gk) for b in stage.babies] for x in xs]
    outs = []
    for c in range(stage.outputs):
        feeds = [(0, c)] if stage.mode == "split" else [(c, 0)] if stage.mode == "lockstep" else [(0, 0), (1, 1)]
        acc = None
        for gi, g in enumerate(stage.giants):
            inner = None
            for src, mat in feeds:
                for bi in range(len(stage.babies)):
                    pt = table[mat][gi][bi]
                    if pt is not None:
                        t = ev.multiply_plain(rots[src][bi], pt)
                        inner = t if inner is None else ev.add(inner, t)
            moved = inner if g == 0 else ev.rotate_vector(inner, g, gk)
            acc = moved if acc is None else ev.add(acc, moved)
        outs.append(ev.rescale_to_next_inplace(acc))
    return outs


def plan_op_by_op(ev, xs, plan, tables, gk):
    from seal_fyp_logistic_regression_amd import dft
    for stage, table in zip(plan.stages, tables):
        xs = stage_op_by_op(ev, xs, stage, table, gk)
    return [ev.add(x, ev.complex_conjugate(x, gk)) for x in xs] if plan.direction == dft.C2S else xs


def transform_inputs():
    from seal_fyp_logistic_regression_amd import dft
    from tests.test_dft_cpu import dense_U
    n = N_T // 2
    rng = np.random.default_rng(2026)
    z = np.sqrt(rng.uniform(0, 1, n)) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
    U = dense_U(N_T)
    m = 2.0 / N_T * (U.conj().T @ z).real
    R = dft.bit_reversal(n)
    xa, xb = rng.uniform(-1.0 / n, 1.0 / n, n), rng.uniform(-1.0 / n, 1.0 / n, n)
    coeffs = np.empty(N_T)
    coeffs[R], coeffs[n + R] = xa, xb
    return z, m[:n][R], m[n:][R], xa, xb, U @ coeffs


def gate(e, name, ct, want, mode):
    got = e["encoder"].decode(e["dec"].decrypt(ct))
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"[gpu dft] {name} ({mode}): max error / max|expected| = {rel:.3e}")
    assert rel <= CAP, (name, rel)


def test_transforms_same_words_as_the_plan_op_by_op_on_the_twin(rescale_mode):
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import dft
    from seal_fyp_logistic_regression_amd import seal as S
    q = S.CoeffModulus.Create(N_T, BITS)
    top = len(q) - 1
    plans = {"c2s": dft.plan(N_T, LEVELS, dft.C2S, [q[top - 1 - i] for i in range(LEVELS)]),
             "s2c": dft.plan(N_T, LEVELS, dft.S2C, [q[top - 1 - i] for i in range(LEVELS)]),
             "back": dft.plan(N_T, LEVELS, dft.S2C, [q[top - LEVELS - 1 - i] for i in range(LEVELS)])}
    steps = sorted(set(plans["c2s"].galois_steps()) | set(plans["s2c"].galois_steps()))
    z, a, b, xa, xb, zs = transform_inputs()
    res = {}
    for kind in ("gpu", "oracle"):
        e = make(N_T, BITS, kind, seed=3, galois_steps=steps + [0])   # (step 0 is SEAL's name for the conjugation key)
        assert (getattr(e["ctx"].backend, "plain_combine", None) is not None) == (kind == "gpu")
        assert e["ctx"].primes == q and e["gk"].has_key(2 * N_T - 1)
        ev, gk = e["ev"], e["gk"]
        tables = {"c2s": plans["c2s"].encode(e["encoder"], top), "s2c": plans["s2c"].encode(e["encoder"], top),
                  "back": plans["back"].encode(e["encoder"], top - LEVELS)}
        ct = e["enc"].encrypt(e["encoder"].encode(z, SCALE))
        ca, cb = (e["enc"].encrypt(e["encoder"].encode(x, SCALE)) for x in (xa, xb))
        if kind == "gpu":
            c2s = alg.coeffs_to_slots(ev, ct, plans["c2s"], gk, encoded=tables["c2s"])
            s2c = alg.slots_to_coeffs(ev, ca, cb, plans["s2c"], gk, encoded=tables["s2c"])
            back = alg.slots_to_coeffs(ev, c2s[0], c2s[1], plans["back"], gk, encoded=tables["back"])
        else:
            c2s = plan_op_by_op(ev, [ct], plans["c2s"], tables["c2s"], gk)
            (s2c,) = plan_op_by_op(ev, [ca, cb], plans["s2c"], tables["s2c"], gk)
            (back,) = plan_op_by_op(ev, list(c2s), plans["back"], tables["back"], gk)
        res[kind] = (e, list(c2s) + [s2c, back])
    (eg, cg), (eo, co) = res["gpu"], res["oracle"]
    names = ["coeffs_to_slots a", "coeffs_to_slots b", "slots_to_coeffs", "round trip"]
    levels = [top - LEVELS, top - LEVELS, top - LEVELS, top - 2 * LEVELS]
    for name, g, o, lv in zip(names, cg, co, levels):
        assert g.size() == o.size() == 2 and g.parms_id() == o.parms_id() == lv and g.scale == o.scale, name
        assert np.array_equal(words(eg, g), words(eo, o)), name
    gate(eg, "coeffs_to_slots a", cg[0], a.astype(np.complex128), rescale_mode)
    gate(eg, "coeffs_to_slots b", cg[1], b.astype(np.complex128), rescale_mode)
    gate(eg, "slots_to_coeffs", cg[2], zs, rescale_mode)
    gate(eg, "round trip", cg[3], z, rescale_mode)


def test_dft_selftest_runs_to_its_end():
    exe = os.path.join(ROOT, "drivers", "_ref", "dft_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "drivers"), "_ref/dft_selftest"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DFT SELFTEST PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
