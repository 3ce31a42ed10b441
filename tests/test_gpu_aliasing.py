"""The aliasing rule of the C-ABI on the GPU (include/hefx.h per entry, INTEGRATION.md "Aliasing", tests/aliasing_cases.py):
the in-place forms an entry serves give the oracle's out-of-place words, the overlaps it refuses come back as
HEFX_ERR_INVALID with nothing written and nothing counted, and the same layout moved to exactly adjacent views runs and
gives the oracle's words.  Bar: bit-exact uint64 words, no tolerance.

Every buffer of a case is a view of ONE allocation with a margin as large as the case's largest buffer on both sides, so
no case -- refused, accepted, or wrongly accepted -- can reach memory outside its own slab.  N = 2048 with
coeff_modulus_create(2048, [50, 30, 30, 50]) (k = 4: L = 3 and 2), the smallest ring that rescales and key-switches."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import aliasing_cases as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, BITS = 2048, [50, 30, 30, 50]
_made = {}


def _env(n=N, bits=tuple(BITS)):
    """(oracle, engine) of a parameter set, made once"""
    if (n, bits) not in _made:
        from oracle import oracle as O
        from seal_fyp_logistic_regression_amd import Engine
        primes = O.coeff_modulus_create(n, list(bits))
        _made[(n, bits)] = (O.Oracle(n, primes), Engine(n, primes))
    return _made[(n, bits)]


def _lib():
    from seal_fyp_logistic_regression_amd import capi
    return capi.lib(), capi.ptr_array, capi


def _top(o, L, npoly):
    """every word q_j - 1: the largest canonical residue"""
    a = np.zeros((npoly, L, o.N), dtype=np.uint64)
    for j in range(L):
        a[:, j, :] = o.primes[j] - 1
    return a


def _rand_key(o, seed):
    return o.uniform(o.k, 2 * (o.k - 1), seed).reshape(o.k - 1, 2, o.k, o.N)


def _engine_constants():
    """(ADD_MANY_GROUP, TABLE_MAX) from the engine's sources, not from literals"""
    from tests.test_gpu_multiply_sum import _table_slice
    src = open(os.path.join(ROOT, "seal_fyp_logistic_regression_amd", "csrc", "hefx_internal.h")).read()
    return int(re.search(r"ADD_MANY_GROUP = (\d+)", src).group(1)), _table_slice()


# ---- one slab, views, moves -----------------------------------------------------------------------------------------
class Case:
    """Buffers (name, words, host data or None for an output) packed back to back in one slab, in the order given -- the
    ACCEPTED layout: every view exactly adjacent to its neighbours.  place(moves) gives the device pointers of the layout
    with some buffers moved: {"x": ("row_into", "y")} puts x where y's last row starts (x and y share one row of N words,
    or less when x is shorter), {"x": ("on", "y")} puts x at y's first word."""

    def __init__(self, e, o, bufs, seed=1):
        self.e, self.o = e, o
        self.names = [b[0] for b in bufs]
        self.words = {b[0]: int(b[1]) for b in bufs}
        self.margin = max(self.words.values())
        self.at, pos = {}, self.margin
        for name in self.names:
            self.at[name] = pos
            pos += self.words[name]
        rng = np.random.default_rng(seed)
        self.host = rng.integers(0, 1 << 63, size=pos + self.margin, dtype=np.uint64)  # canary everywhere, outputs included
        for name, words, data in bufs:
            if data is not None:
                self.host[self.at[name]:self.at[name] + words] = np.ascontiguousarray(data, dtype=np.uint64).reshape(-1)
        self.dev = e.to_device(self.host)

    def offsets(self, moves=None):
        at = dict(self.at)
        for x, (how, y) in (moves or {}).items():
            at[x] = self.at[y] + (self.words[y] - self.o.N if how == "row_into" else 0)
            assert 0 <= at[x] and at[x] + self.words[x] <= self.host.size  # inside the slab, whatever the engine does
        return at

    def place(self, moves=None):
        return {k: self.dev.ptr + 8 * v for k, v in self.offsets(moves).items()}

    def unchanged(self):
        return (self.dev.download() == self.host).all()


def _refused(case, call, moves, ks):
    lib, _, capi = _lib()
    before = case.e.ks_stats() if ks else None
    rc = call(case.place(moves))
    case.e.sync()
    msg = lib.hefx_last_error().decode()
    assert rc == capi.HEFX_ERR_INVALID, (moves, rc, msg)
    assert re.search("overlap|alias|independent", msg), (moves, msg)
    assert case.unchanged(), moves
    if ks:
        assert case.e.ks_stats() == before, moves


def _accepted(case, call, want):
    """the adjacent layout runs; want: {output name: words}.  Everything else in the slab -- inputs, margins -- is unchanged"""
    _, _, capi = _lib()
    capi.check(call(case.place()))
    expect = case.host.copy()
    for name, words in want.items():
        expect[case.at[name]:case.at[name] + case.words[name]] = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    got = case.dev.download()
    for name in want:
        s = slice(case.at[name], case.at[name] + case.words[name])
        assert (got[s] == expect[s]).all(), name
    assert (got == expect).all()


def _standard_moves(ins, outs, exact=(), cross=()):
    """an output one row into an input, an input one row into an output, two outputs one row apart; exact: (out, in) pairs
    that are refused even when equal; cross: (out, in) pairs of DIFFERENT items made equal"""
    moves = []
    for x in outs:
        for y in ins:
            moves += [{x: ("row_into", y)}, {y: ("row_into", x)}]
    for x, y in zip(outs[1:], outs[:-1]):
        moves.append({x: ("row_into", y)})
    moves += [{x: ("on", y)} for x, y in list(exact) + list(cross)]
    return moves


# ---- served: element-wise in place ----------------------------------------------------------------------------------
@pytest.mark.parametrize("size,count", [(2, 1), (3, 1), (2, 3), (3, 3)])
def test_elementwise_in_place(size, count):
    """hefx_add / hefx_sub / hefx_negate / hefx_add_plain / hefx_multiply_plain with d_out == d_a and d_out == d_b, and
    add(a, a, out = a): the oracle's out-of-place words, the other operand untouched"""
    o, e = _env()
    lib, _, capi = _lib()
    L, h = 3, e._h
    ctw = size * L * N
    a = np.stack([o.uniform(L, size, 100 + 10 * size + c) for c in range(count)])
    b = np.stack([_top(o, L, size)] + [o.uniform(L, size, 200 + 10 * size + c) for c in range(1, count)])  # item 0: all q - 1
    pt = o.uniform(L, 1, 300)[0]
    pt[1, :] = o.primes[1] - 1

    def per_ct(f, *xs):
        return np.stack([f(*[x[c] for x in xs]) for c in range(count)])

    ops = {
        "hefx_add": (lambda p, out: lib.hefx_add(h, L, size, count, p["a"], p["b"], out, None), lambda: per_ct(o.add, a, b), "ab"),
        "hefx_sub": (lambda p, out: lib.hefx_sub(h, L, size, count, p["a"], p["b"], out, None), lambda: per_ct(o.sub, a, b), "ab"),
        "hefx_negate": (lambda p, out: lib.hefx_negate(h, L, size, count, p["a"], out, None), lambda: per_ct(o.negate, a), "a"),
        "hefx_multiply_plain": (lambda p, out: lib.hefx_multiply_plain(h, L, size, count, p["a"], p["pt"], out, None),
                                lambda: per_ct(lambda x: o.multiply_plain(x, pt), a), "a"),
    }
    if count == 1:
        ops["hefx_add_plain"] = (lambda p, out: lib.hefx_add_plain(h, L, size, p["a"], p["pt"], out, None),
                                 lambda: per_ct(lambda x: o.add_plain(x, pt), a), "a")
    for name, (call, want, in_place_on) in ops.items():
        assert A.RULES[name]["kind"] == A.IN_PLACE
        for target in in_place_on:
            case = Case(e, o, [("a", count * ctw, a), ("b", count * ctw, b), ("pt", L * N, pt)], seed=size + count)
            p = case.place()
            capi.check(call(p, p[target]))
            _accepted(case, lambda _: 0, {target: want()})  # the target holds the result; a / b / pt otherwise untouched
    # add(a, a, out = a) = 2a, and sub(b, b, out = b) = 0
    case = Case(e, o, [("a", count * ctw, a), ("b", count * ctw, b)], seed=9)
    p = case.place()
    capi.check(lib.hefx_add(h, L, size, count, p["a"], p["a"], p["a"], None))
    capi.check(lib.hefx_sub(h, L, size, count, p["b"], p["b"], p["b"], None))
    _accepted(case, lambda _: 0, {"a": per_ct(o.add, a, a), "b": np.zeros_like(b)})
    e.check_transparent()  # (the products above are not transparent; leaves the flag clean for later tests)


def test_elementwise_refusals():
    """hefx_add, hefx_sub, hefx_negate, hefx_add_plain, hefx_multiply_plain: any overlap other than the exact in-place form"""
    o, e = _env()
    lib, _, _ = _lib()
    L, size, h = 3, 2, e._h
    ctw = size * L * N
    a, b, pt = o.uniform(L, size, 1), _top(o, L, size), o.uniform(L, 1, 3)[0]
    bufs = [("a", ctw, a), ("b", ctw, b), ("pt", L * N, pt), ("out", ctw, None)]
    specs = [
        (lambda p: lib.hefx_add(h, L, size, 1, p["a"], p["b"], p["out"], None), ["a", "b"], lambda: o.add(a, b)),
        (lambda p: lib.hefx_sub(h, L, size, 1, p["a"], p["b"], p["out"], None), ["a", "b"], lambda: o.sub(a, b)),
        (lambda p: lib.hefx_negate(h, L, size, 1, p["a"], p["out"], None), ["a"], lambda: o.negate(a)),
        (lambda p: lib.hefx_add_plain(h, L, size, p["a"], p["pt"], p["out"], None), ["a", "pt"], lambda: o.add_plain(a, pt)),
        (lambda p: lib.hefx_multiply_plain(h, L, size, 1, p["a"], p["pt"], p["out"], None), ["a", "pt"], lambda: o.multiply_plain(a, pt)),
    ]
    for call, ins, want in specs:
        case = Case(e, o, bufs)
        for moves in _standard_moves(ins, ["out"], exact=[("out", "pt")] if "pt" in ins else []):
            _refused(case, call, moves, ks=False)
        _accepted(case, call, {"out": want()})
    e.check_transparent()


def test_addsub_batch_in_place():
    """hefx_add_batch / hefx_sub_batch: in place on a, in place on b, one shared read-only b; refused: an output on ANOTHER
    item's operand, two outputs one row apart, an output one row into another item's b"""
    o, e = _env()
    lib, arr, capi = _lib()
    L, size, n, h = 3, 2, 3, e._h
    ctw = size * L * N
    As = [o.uniform(L, size, 400 + i) for i in range(n)]
    Bs = [_top(o, L, size)] + [o.uniform(L, size, 500 + i) for i in range(1, n)]
    bufs = [(f"a{i}", ctw, As[i]) for i in range(n)] + [(f"b{i}", ctw, Bs[i]) for i in range(n)] + [(f"o{i}", ctw, None) for i in range(n)]
    for entry, f, op in (("hefx_add_batch", lib.hefx_add_batch, o.add), ("hefx_sub_batch", lib.hefx_sub_batch, o.sub)):
        assert A.RULES[entry]["kind"] == A.IN_PLACE

        def call(p, outs="o", bs=None):
            return f(h, L, size, n, arr([p[f"a{i}"] for i in range(n)]), arr([p[bs or f"b{i}"] for i in range(n)]),
                     arr([p[f"{outs}{i}"] for i in range(n)]), None)

        case = Case(e, o, bufs)
        for moves in _standard_moves(["a0", "b1"], ["o0", "o1", "o2"], cross=[("o0", "a1"), ("o1", "b2"), ("o2", "o0")]):
            _refused(case, call, moves, ks=False)
        _accepted(case, call, {f"o{i}": op(As[i], Bs[i]) for i in range(n)})
        case = Case(e, o, bufs)  # in place on a
        _accepted(case, lambda p: call(p, outs="a"), {f"a{i}": op(As[i], Bs[i]) for i in range(n)})
        case = Case(e, o, bufs)  # in place on b
        _accepted(case, lambda p: call(p, outs="b"), {f"b{i}": op(As[i], Bs[i]) for i in range(n)})
        case = Case(e, o, bufs)  # one shared read-only b, in place on a
        _accepted(case, lambda p: call(p, outs="a", bs="b0"), {f"a{i}": op(As[i], Bs[0]) for i in range(n)})
        case = Case(e, o, bufs)  # ... which may not be an output
        _refused(case, lambda p: call(p, outs="b", bs="b0"), None, ks=False)


# ---- served: add_many with the output among the inputs --------------------------------------------------------------
_pool = {}


def _add_many_pool():
    """150 ciphertexts (size 2, L = 3; the first one all q - 1) and the running sums of the first n of them, once"""
    if not _pool:
        o, _ = _env()
        bufs = [_top(o, 3, 2)] + [o.uniform(3, 2, 600 + i) for i in range(1, 150)]
        sums, acc = [None], None
        for b in bufs:
            acc = b.copy() if acc is None else o.add(acc, b)
            sums.append(acc)
        _pool["bufs"], _pool["sums"] = bufs, sums
    return _pool["bufs"], _pool["sums"]


def _weighted_sum(o, L, bufs, mult):
    """sum_k mult[k] * bufs[k] mod q_j per row, in Python integers"""
    out = np.zeros_like(bufs[0])
    for j in range(L):
        acc = sum(int(m) * b[:, j, :].astype(object) for b, m in zip(bufs, mult))
        out[:, j, :] = (acc % o.primes[j]).astype(np.uint64)
    return out


def _run_add_many(o, e, L, size, bufs, order, out_index, want):
    """in[t] = bufs[order[t]]; once out of place, once with out = bufs[out_index]; the other buffers untouched"""
    lib, arr, capi = _lib()
    words = size * L * o.N
    case = Case(e, o, [(f"v{k}", words, b) for k, b in enumerate(bufs)] + [("out", words, None)], seed=len(order))
    p = case.place()
    ins = arr([p[f"v{k}"] for k in order])
    capi.check(lib.hefx_add_many(e._h, L, size, len(order), ins, p["out"], None))
    _accepted(case, lambda _: 0, {"out": want})
    capi.check(lib.hefx_add_many(e._h, L, size, len(order), ins, p[f"v{out_index}"], None))
    _accepted(case, lambda _: 0, {"out": want, f"v{out_index}": want})


@pytest.mark.parametrize("n,i", A.ADD_MANY_IN_PLACE)
def test_add_many_in_place(n, i):
    """hefx_add_many(v[0..n), out = v[i]) on both sides of every path of add_many_impl: one launch (n <= ADD_MANY_GROUP), two
    launches (the second accumulates into out: before the fix an out among the second launch's inputs had already been
    overwritten with the first partial sum when it was read), the table level"""
    group, table_max = _engine_constants()
    assert 2 * group < max(c[0] for c in A.ADD_MANY_IN_PLACE) <= table_max
    assert {(n_ <= group, n_ <= 2 * group) for n_, _ in A.ADD_MANY_IN_PLACE} == {(True, True), (False, True), (False, False)}
    o, e = _env()
    bufs, sums = _add_many_pool()
    _run_add_many(o, e, 3, 2, bufs[:n], list(range(n)), i, sums[n])


def test_add_many_in_place_on_a_repeated_input():
    """n = 60 from a pool of four buffers, out the one that sits at positions 1, 50 and 59: read by both launches"""
    group, _ = _engine_constants()
    o, e = _env()
    bufs, _ = _add_many_pool()
    n, at = A.ADD_MANY_POOL_N, A.ADD_MANY_POOL_OUT_AT
    assert group < n <= 2 * group and at[0] < group <= at[1]
    order = [3 if t in at else t % 3 for t in range(n)]
    mult = [order.count(k) for k in range(4)]
    _run_add_many(o, e, 3, 2, bufs[:4], order, 3, _weighted_sum(o, 3, bufs[:4], mult))


def test_add_many_in_place_beyond_the_pointer_table():
    """n = TABLE_MAX + 1 (more pointers than a descriptor-ring slot holds) from a pool of four, out the last input; N = 1024,
    L = 1, size 1"""
    _, table_max = _engine_constants()
    o, e = _env(1024, (50,))
    n = table_max + 1
    bufs = [_top(o, 1, 1)] + [o.uniform(1, 1, 700 + i) for i in range(1, 4)]
    order = [t % 3 for t in range(n - 1)] + [3]
    mult = [order.count(k) for k in range(4)]
    _run_add_many(o, e, 1, 1, bufs, order, 3, _weighted_sum(o, 1, bufs, mult))
    # and with out in the middle of the list as well as at its end
    order[table_max // 2] = 3
    mult = [order.count(k) for k in range(4)]
    _run_add_many(o, e, 1, 1, bufs, order, 3, _weighted_sum(o, 1, bufs, mult))


def test_add_many_refuses_a_partial_overlap():
    o, e = _env()
    lib, arr, _ = _lib()
    bufs, sums = _add_many_pool()
    words = 2 * 3 * N
    case = Case(e, o, [(f"v{k}", words, bufs[k]) for k in range(3)] + [("out", words, None)])
    call = lambda p: lib.hefx_add_many(e._h, 3, 2, 3, arr([p["v0"], p["v1"], p["v2"]]), p["out"], None)  # noqa: E731
    for moves in _standard_moves(["v0", "v2"], ["out"]):
        _refused(case, call, moves, ks=False)
    _accepted(case, call, {"out": sums[3]})


# ---- refused: the entries that serve no alias at all -----------------------------------------------------------------
def _specs(o, e):
    """name -> (buffers, call, inputs, outputs, exact, cross, want, ks).  exact: (out, in) pairs refused although equal;
    cross: (out, in) pairs of different items made equal."""
    from tests.oracle_backend import OracleBackend
    lib, arr, _ = _lib()
    h, L, k = e._h, 3, o.k
    LN, c2, c3 = L * N, 2 * L * N, 3 * L * N
    ob = OracleBackend(o.N, o.primes)
    ob.rescale_rounded = e.rescale_rounded
    a = [o.uniform(L, 2, 10 + i) for i in range(4)]
    a[1] = _top(o, L, 2)
    t3 = [o.multiply(a[0], a[1]), o.multiply(a[2], a[3])]
    pts = [o.uniform(L, 1, 20 + i)[0] for i in range(4)]
    key = _rand_key(o, 30)
    dkey = e.to_device(key)
    _made["keep"] = dkey
    sk, pk = o.uniform(k, 1, 31)[0], o.uniform(k, 2, 32)
    key32 = bytes(range(32))
    S = {}
    S["hefx_multiply"] = ([("a", c2, a[0]), ("b", c2, a[1]), ("o", c3, None)],
                          lambda p: lib.hefx_multiply(h, L, p["a"], p["b"], p["o"], None), ["a", "b"], ["o"], [("o", "a"), ("o", "b")], [],
                          lambda: {"o": o.multiply(a[0], a[1])}, False)
    S["hefx_square"] = ([("a", c2, a[1]), ("o", c3, None)], lambda p: lib.hefx_square(h, L, p["a"], p["o"], None), ["a"], ["o"],
                        [("o", "a")], [], lambda: {"o": o.multiply(a[1], a[1])}, False)
    S["hefx_multiply_batch"] = (
        [("a0", c2, a[0]), ("a1", c2, a[1]), ("b0", c2, a[2]), ("b1", c2, a[3]), ("o0", c3, None), ("o1", c3, None)],
        lambda p: lib.hefx_multiply_batch(h, L, 2, arr([p["a0"], p["a1"]]), arr([p["b0"], p["b1"]]), arr([p["o0"], p["o1"]]), None),
        ["a0", "a1", "b1"], ["o0", "o1"], [("o0", "a0")], [("o0", "a1"), ("o1", "b0"), ("o1", "o0")],
        lambda: {"o0": o.multiply(a[0], a[2]), "o1": o.multiply(a[1], a[3])}, False)
    mp = [("c0", c2, a[0]), ("c1", c2, a[1]), ("p0", LN, pts[0]), ("p1", LN, pts[1]), ("o0", c2, None), ("o1", c2, None)]
    S["hefx_multiply_plain_batch"] = (
        mp, lambda p: lib.hefx_multiply_plain_batch(h, L, 2, 2, arr([p["c0"], p["c1"]]), arr([p["p0"], p["p1"]]), arr([p["o0"], p["o1"]]), None),
        ["c0", "c1", "p1"], ["o0", "o1"], [("o0", "c0")], [("o0", "c1"), ("o1", "p0"), ("o1", "o0")],
        lambda: {"o0": o.multiply_plain(a[0], pts[0]), "o1": o.multiply_plain(a[1], pts[1])}, False)
    ms = [(f"c{i}", c2, a[i]) for i in range(4)] + [(f"p{i}", LN, pts[i]) for i in range(4)] + [("o0", c2, None), ("o1", c2, None)]
    S["hefx_multiply_plain_sum"] = (
        ms, lambda p: lib.hefx_multiply_plain_sum(h, L, 2, 4, 2, arr([p[f"c{i}"] for i in range(4)]), arr([p[f"p{i}"] for i in range(4)]),
                                                  arr([p["o0"], p["o1"]]), None),
        ["c0", "c3", "p2"], ["o0", "o1"], [("o0", "c1")], [("o0", "c2"), ("o1", "c0"), ("o0", "p3"), ("o1", "o0")],
        lambda: {"o0": o.add(o.multiply_plain(a[0], pts[0]), o.multiply_plain(a[1], pts[1])),
                 "o1": o.add(o.multiply_plain(a[2], pts[2]), o.multiply_plain(a[3], pts[3]))}, False)
    two = np.stack([a[0], a[1]])  # count = 2, size 2
    rs = [("in", 2 * c2, two), ("out", 2 * 2 * (L - 1) * N, None)]
    S["hefx_rescale_to_next"] = (rs, lambda p: lib.hefx_rescale_to_next(h, L, 2, 2, p["in"], p["out"], None), ["in"], ["out"], [("out", "in")], [],
                                 lambda: {"out": np.stack([ob.rescale(L, 2, x) for x in two])}, False)
    S["hefx_rescale_to_next_mode"] = (rs, lambda p: lib.hefx_rescale_to_next_mode(h, L, 2, 2, p["in"], p["out"], 0, None), ["in"], ["out"],
                                      [("out", "in")], [], lambda: {"out": np.stack([o.rescale(x, rounded=False) for x in two])}, False)
    S["hefx_rescale_to_next_batch"] = (
        [("i0", c3, t3[0]), ("i1", c3, t3[1]), ("o0", 3 * (L - 1) * N, None), ("o1", 3 * (L - 1) * N, None)],
        lambda p: lib.hefx_rescale_to_next_batch(h, L, 3, 2, arr([p["i0"], p["i1"]]), arr([p["o0"], p["o1"]]), None),
        ["i0", "i1"], ["o0", "o1"], [("o0", "i0")], [("o0", "i1"), ("o1", "o0")],
        lambda: {"o0": ob.rescale(L, 3, t3[0]), "o1": ob.rescale(L, 3, t3[1])}, False)
    S["hefx_mod_drop"] = ([("in", c2, a[0]), ("out", 2 * 2 * N, None)], lambda p: lib.hefx_mod_drop(h, L, 2, 2, p["in"], p["out"], None),
                          ["in"], ["out"], [("out", "in")], [], lambda: {"out": o.mod_drop(a[0], 2)}, False)
    S["hefx_galois_permute"] = ([("in", LN, pts[0]), ("out", LN, None)], lambda p: lib.hefx_galois_permute(h, 3, p["in"], L, p["out"], None),
                                ["in"], ["out"], [("out", "in")], [], lambda: {"out": np.stack([o.apply_galois_ntt(3, r) for r in pts[0]])}, False)
    S["hefx_decrypt"] = ([("ct", c2, a[0]), ("sk", LN, sk[:L]), ("out", LN, None)],
                         lambda p: lib.hefx_decrypt(h, L, 2, p["ct"], p["sk"], p["out"], None), ["ct", "sk"], ["out"], [("out", "ct"), ("out", "sk")],
                         [], lambda: {"out": ob.decrypt(L, 2, a[0], sk)}, False)
    S["hefx_encrypt"] = ([("pk", 2 * k * N, pk), ("plain", LN, pts[0]), ("out", c2, None)],
                         lambda p: lib.hefx_encrypt(h, L, p["pk"], p["plain"], key32, 5, p["out"], None), ["pk", "plain"], ["out"],
                         [("out", "plain"), ("out", "pk")], [], lambda: {"out": ob.encrypt(L, pk, pts[0], key32, 5)}, False)
    S["hefx_encrypt_batch"] = (
        [("pk", 2 * k * N, pk), ("p0", LN, pts[0]), ("p1", LN, pts[1]), ("o0", c2, None), ("o1", c2, None)],
        lambda p: lib.hefx_encrypt_batch(h, L, 2, p["pk"], arr([p["p0"], p["p1"]]), key32, 7, arr([p["o0"], p["o1"]]), None),
        ["pk", "p0", "p1"], ["o0", "o1"], [("o0", "p0")], [("o0", "p1"), ("o1", "o0")],
        lambda: {"o0": ob.encrypt(L, pk, pts[0], key32, 7), "o1": ob.encrypt(L, pk, pts[1], key32, 8)}, False)
    S["hefx_relinearize"] = ([("ct3", c3, t3[0]), ("ct2", c2, None)], lambda p: lib.hefx_relinearize(h, L, p["ct3"], dkey.ptr, p["ct2"], None),
                             ["ct3"], ["ct2"], [("ct2", "ct3")], [], lambda: {"ct2": o.relinearize(t3[0], key)}, True)
    S["hefx_relinearize_batch"] = (
        [("i0", c3, t3[0]), ("i1", c3, t3[1]), ("o0", c2, None), ("o1", c2, None)],
        lambda p: lib.hefx_relinearize_batch(h, L, 2, arr([p["i0"], p["i1"]]), dkey.ptr, arr([p["o0"], p["o1"]]), None),
        ["i0", "i1"], ["o0", "o1"], [("o0", "i0")], [("o0", "i1"), ("o1", "o0")],
        lambda: {"o0": o.relinearize(t3[0], key), "o1": o.relinearize(t3[1], key)}, True)
    return S


_NO_ALIAS = ["hefx_multiply", "hefx_square", "hefx_multiply_batch", "hefx_multiply_plain_batch", "hefx_multiply_plain_sum",
             "hefx_rescale_to_next", "hefx_rescale_to_next_mode", "hefx_rescale_to_next_batch", "hefx_mod_drop", "hefx_galois_permute",
             "hefx_decrypt", "hefx_encrypt", "hefx_encrypt_batch", "hefx_relinearize", "hefx_relinearize_batch"]


@pytest.mark.parametrize("name", _NO_ALIAS)
def test_refusals(name):
    """an output one row into an input, an input one row into an output, two outputs one row apart, an output ON another
    item's input, the exact alias: HEFX_ERR_INVALID, a message that says "overlap", every buffer unchanged, no key switch
    counted.  Then the same buffers exactly adjacent: accepted, the oracle's words."""
    o, e = _env()
    assert A.RULES[name]["kind"] == A.NO_OVERLAP
    bufs, call, ins, outs, exact, cross, want, ks = _specs(o, e)[name]
    case = Case(e, o, bufs)
    for moves in _standard_moves(ins, outs, exact, cross):
        _refused(case, call, moves, ks)
    _accepted(case, call, want())


def test_keygen_kswitch_refusals():
    """hefx_keygen_kswitch: the key may reach into neither secret key; adjacent, it is the key a separate buffer receives"""
    o, e = _env()
    lib, _, capi = _lib()
    k = o.k
    sk, new_sk = o.uniform(k, 1, 41)[0], o.uniform(k, 1, 42)[0]
    key32 = bytes(range(7, 39))
    call = lambda p: lib.hefx_keygen_kswitch(e._h, p["sk"], p["new"], key32, 3, p["out"], None)  # noqa: E731
    case = Case(e, o, [("sk", k * N, sk), ("new", k * N, new_sk), ("out", (k - 1) * 2 * k * N, None)])
    for moves in _standard_moves(["sk", "new"], ["out"]):
        _refused(case, call, moves, ks=False)
    apart = e.keygen_kswitch(e.to_device(sk), e.to_device(new_sk), key32, 3).download()
    _accepted(case, call, {"out": apart})


# ---- the plain linear transforms and the hoisted batch, d = 3 ---------------------------------------------------------
def _lt_env():
    from oracle import oracle as O
    o, e = _env()
    L, d = 3, 3
    steps = [1, 2, -d]
    elts = [O.galois_elt_from_step(N, s) for s in steps]
    key = _rand_key(o, 50)
    if "ltkey" not in _made:
        _made["ltkey"] = e.to_device(key)
    rot = lambda ct, step: o.apply_galois(ct, elts[steps.index(step)], key)  # noqa: E731
    return o, e, L, d, elts, key, _made["ltkey"], rot


def _lt_plain_want(o, rot, ct, diags, d):
    ct_new = o.add(ct, rot(ct, -d))
    acc = o.multiply_plain(ct_new, diags[0])
    for l in range(1, d):
        acc = o.add(acc, o.multiply_plain(rot(ct_new, l), diags[l]))
    return acc


@pytest.mark.parametrize("name", ["hefx_linear_transform_plain", "hefx_linear_transform_plain_hoisted", "hefx_linear_transform_plain_many",
                                  "hefx_linear_transform_plain_bsgs", "hefx_linear_transform_plain_hoisted2",
                                  "hefx_linear_transform_plain_hoisted2_sparse", "hefx_rotate_hoisted_batch"])
def test_linear_transform_refusals(name):
    """an output equal to d_ct, an output one row into a diagonal (and the other standard overlaps), for _many two equal
    outputs: refused before a key switch is counted; adjacent views: the words of the op-by-op sequence over the oracle"""
    from seal_fyp_logistic_regression_amd import capi
    o, e, L, d, elts, key, dkey, rot = _lt_env()
    lib, arr = capi.lib(), capi.ptr_array
    assert A.RULES[name]["kind"] == A.NO_OVERLAP
    h, k = e._h, o.k
    LN, c2 = L * N, 2 * L * N
    ct = [o.uniform(L, 2, 60), _top(o, L, 2)]
    diags = [o.uniform(L, 1, 70 + i)[0] for i in range(2 * d)]
    kdiags = [o.uniform(k, 1, 80 + i)[0] for i in range(d)]  # key-level plaintexts of the double-hoisted forms
    ke, kk = capi.u32_array(elts), arr([dkey.ptr] * 3)
    dnames = [f"d{i}" for i in range(d)]
    one = [("ct", c2, ct[0])] + [(f"d{i}", LN, diags[i]) for i in range(d)] + [("out", c2, None)]
    onek = [("ct", c2, ct[0])] + [(f"d{i}", k * N, kdiags[i]) for i in range(d)] + [("out", c2, None)]
    dp = lambda p: arr([p[x] for x in dnames])  # noqa: E731
    std = (["ct"] + dnames, ["out"], [("out", "ct")], [])
    if name in ("hefx_linear_transform_plain", "hefx_linear_transform_plain_hoisted"):
        f = getattr(lib, name)
        bufs, (ins, outs, exact, cross) = one, std
        call = lambda p: f(h, L, p["ct"], d, dp(p), 3, ke, kk, p["out"], None)  # noqa: E731
        want = lambda: {"out": _lt_plain_want(o, rot, ct[0], diags, d)}  # noqa: E731
    elif name == "hefx_linear_transform_plain_many":
        bufs = [("ct0", c2, ct[0]), ("ct1", c2, ct[1])] + [(f"d{i}", LN, diags[i]) for i in range(2 * d)] + [("o0", c2, None), ("o1", c2, None)]
        ins, outs, exact, cross = ["ct0", "ct1", "d0", "d5"], ["o0", "o1"], [("o0", "ct0")], [("o1", "ct0"), ("o1", "o0")]
        call = lambda p: lib.hefx_linear_transform_plain_many(h, L, 2, arr([p["ct0"], p["ct1"]]), d, arr([p[f"d{i}"] for i in range(2 * d)]),  # noqa: E731
                                                              3, ke, kk, arr([p["o0"], p["o1"]]), None)
        want = lambda: {"o0": _lt_plain_want(o, rot, ct[0], diags[:d], d), "o1": _lt_plain_want(o, rot, ct[1], diags[d:], d)}  # noqa: E731
    elif name == "hefx_linear_transform_plain_bsgs":
        bufs, (ins, outs, exact, cross) = one, std
        call = lambda p: lib.hefx_linear_transform_plain_bsgs(h, L, p["ct"], d, 2, dp(p), 3, ke, kk, 1, p["out"], None)  # noqa: E731

        def want():  # n1 = 2: inner_0 = ct_new d0 + rot_1(ct_new) d1, inner_1 = ct_new d2; out = inner_0 + rot_2(inner_1)
            ct_new = o.add(ct[0], rot(ct[0], -d))
            inner0 = o.add(o.multiply_plain(ct_new, diags[0]), o.multiply_plain(rot(ct_new, 1), diags[1]))
            return {"out": o.add(inner0, rot(o.multiply_plain(ct_new, diags[2]), 2))}
    elif name in ("hefx_linear_transform_plain_hoisted2", "hefx_linear_transform_plain_hoisted2_sparse"):
        bufs, (ins, outs, exact, cross) = onek, std
        steps = (C.c_int * d)(0, 1, 2)
        if name.endswith("sparse"):
            call = lambda p: lib.hefx_linear_transform_plain_hoisted2_sparse(h, L, p["ct"], d, d, steps, dp(p), 3, ke, kk, p["out"], None)  # noqa: E731
        else:
            call = lambda p: lib.hefx_linear_transform_plain_hoisted2(h, L, p["ct"], d, dp(p), 3, ke, kk, p["out"], None)  # noqa: E731
        want = lambda: {"out": o.lt_double_hoisted_core(o.add(ct[0], rot(ct[0], -d)), kdiags, elts[:2], [key, key])}  # noqa: E731
    else:  # hefx_rotate_hoisted_batch: three rotations of one source, fused plaintexts
        bufs = [("ct", c2, ct[0])] + [(f"d{i}", LN, diags[i]) for i in range(d)] + [(f"o{i}", c2, None) for i in range(d)]
        ins, outs, exact, cross = ["ct", "d0", "d2"], ["o0", "o1", "o2"], [("o0", "ct")], [("o2", "ct"), ("o1", "d2"), ("o2", "o0")]
        call = lambda p: lib.hefx_rotate_hoisted_batch(h, L, p["ct"], 3, ke, kk, dp(p), arr([p[f"o{i}"] for i in range(d)]), None)  # noqa: E731
        want = lambda: {f"o{i}": o.rotate_mulplain(ct[0], elts[i], key, diags[i]) for i in range(d)}  # noqa: E731
    case = Case(e, o, bufs)
    for moves in _standard_moves(ins, outs, exact, cross):
        _refused(case, call, moves, ks=True)
    if name == "hefx_rotate_hoisted_batch":  # one item, no plaintext: ks_run's check runs for one item too
        lone = lambda p: lib.hefx_rotate_hoisted_batch(h, L, p["ct"], 1, ke, kk, None, arr([p["o0"]]), None)  # noqa: E731
        for moves in ({"o0": ("row_into", "ct")}, {"ct": ("row_into", "o0")}, {"o0": ("on", "ct")}):
            _refused(case, lone, moves, ks=True)
    _accepted(case, call, want())


# ---- the key-switch host path: one rule for every n, the rotations and the sums as one list of outputs -------------------
def _ks_refused_then_accepted(case, call, moves, want):
    for m in moves:
        _refused(case, call, m, ks=True)
    _accepted(case, call, want)


def test_apply_galois_one_item():
    """hefx_apply_galois: d_ct_out == d_ct_in is served from a scratch copy; an output one row into the input (or the input
    one row into the output) computed wrong words silently before the check ran for one item -- now refused"""
    o, e, L, d, elts, key, dkey, rot = _lt_env()
    lib, _, capi = _lib()
    assert A.RULES["hefx_apply_galois"]["kind"] == A.IN_PLACE
    c2 = 2 * L * N
    ct = _top(o, L, 2)
    call = lambda p, out="out": lib.hefx_apply_galois(e._h, L, p["in"], elts[0], dkey.ptr, p[out], None)  # noqa: E731
    case = Case(e, o, [("in", c2, ct), ("out", c2, None)])
    _ks_refused_then_accepted(case, call, [{"out": ("row_into", "in")}, {"in": ("row_into", "out")}], {"out": rot(ct, 1)})
    case = Case(e, o, [("in", c2, ct), ("out", c2, None)])
    _accepted(case, lambda p: call(p, "in"), {"in": rot(ct, 1)})


@pytest.mark.parametrize("name", ["hefx_apply_galois_batch", "hefx_rotate_multiply_plain_batch"])
def test_key_switch_batch_aliasing(name):
    """n = 2: an item's own in-place rotation is served; the standard overlaps, the cross pair d_ct_out[1] == d_ct_in[0] and
    an output on a plaintext are refused"""
    o, e, L, d, elts, key, dkey, rot = _lt_env()
    lib, arr, capi = _lib()
    assert A.RULES[name]["kind"] == A.IN_PLACE
    LN, c2 = L * N, 2 * L * N
    cts = [o.uniform(L, 2, 90), _top(o, L, 2)]
    pts = [o.uniform(L, 1, 92 + i)[0] for i in range(2)]
    ke, kk = capi.u32_array(elts[:2]), arr([dkey.ptr] * 2)
    fused = name == "hefx_rotate_multiply_plain_batch"
    bufs = [("i0", c2, cts[0]), ("i1", c2, cts[1])] + ([("p0", LN, pts[0]), ("p1", LN, pts[1])] if fused else []) + [("o0", c2, None), ("o1", c2, None)]

    def call(p, outs="o"):
        ins, oo = arr([p["i0"], p["i1"]]), arr([p[f"{outs}0"], p[f"{outs}1"]])
        if fused:
            return lib.hefx_rotate_multiply_plain_batch(e._h, L, 2, ins, ke, kk, arr([p["p0"], p["p1"]]), oo, None)
        return lib.hefx_apply_galois_batch(e._h, L, 2, ins, ke, kk, oo, None)

    want = [o.rotate_mulplain(cts[i], elts[i], key, pts[i]) if fused else rot(cts[i], i + 1) for i in range(2)]
    moves = _standard_moves(["i0", "i1"] + (["p1"] if fused else []), ["o0", "o1"], exact=[("o0", "p0")] if fused else [],
                            cross=[("o1", "i0")] + ([("o1", "p0")] if fused else []))
    _ks_refused_then_accepted(Case(e, o, bufs), call, moves, {"o0": want[0], "o1": want[1]})
    _accepted(Case(e, o, bufs), lambda p: call(p, "i"), {"i0": want[0], "i1": want[1]})
    e.check_transparent()


def _rotate_add_bufs(o, L):
    c2 = 2 * L * N
    cts = [o.uniform(L, 2, 110), _top(o, L, 2)]
    accs = [_top(o, L, 2), o.uniform(L, 2, 111)]
    bufs = [("i0", c2, cts[0]), ("i1", c2, cts[1]), ("a0", c2, accs[0]), ("a1", c2, accs[1])] + [(x, c2, None) for x in ("s0", "s1", "o0", "o1")]
    return cts, accs, bufs


def test_apply_galois_add_batch_aliasing():
    """hefx_apply_galois_add_batch, n = 2: d_acc_out[i] == d_acc_in[i] and d_ct_out[i] == d_ct_in[i] are served (together); a
    sum on the other item's sum, on a rotation output or on an input, d_acc_in[i] one row into d_acc_out[i] and
    d_acc_in[0] == d_acc_out[1] are refused"""
    o, e, L, d, elts, key, dkey, rot = _lt_env()
    lib, arr, capi = _lib()
    assert A.RULES["hefx_apply_galois_add_batch"]["kind"] == A.IN_PLACE
    cts, accs, bufs = _rotate_add_bufs(o, L)
    ke, kk = capi.u32_array(elts[:2]), arr([dkey.ptr] * 2)

    def call(p, sums="s", outs="o"):
        return lib.hefx_apply_galois_add_batch(e._h, L, 2, arr([p["i0"], p["i1"]]), ke, kk, arr([p["a0"], p["a1"]]),
                                               arr([p[f"{sums}0"], p[f"{sums}1"]]), arr([p[f"{outs}0"], p[f"{outs}1"]]), None)

    r = [rot(cts[i], i + 1) for i in range(2)]
    s = [o.add(accs[i], r[i]) for i in range(2)]
    moves = _standard_moves(["i0", "a1"], ["o0", "o1", "s0", "s1"], cross=[("s1", "s0"), ("s0", "o1"), ("s1", "o1"), ("s0", "i1"), ("s1", "i1"), ("a0", "s1")])
    moves += [{"a0": ("row_into", "s0")}, {"a1": ("row_into", "s1")}]
    _ks_refused_then_accepted(Case(e, o, bufs), call, moves, {"o0": r[0], "o1": r[1], "s0": s[0], "s1": s[1]})
    _accepted(Case(e, o, bufs), lambda p: call(p, "a", "i"), {"i0": r[0], "i1": r[1], "a0": s[0], "a1": s[1]})


def test_rotate_add_chain_aliasing():
    """hefx_rotate_add_chain, n = 2, steps = 3 (level 1 through the front door, one level in each ping-pong direction): any two
    of the 2n outputs overlapping are refused; d_ct_out[i] == d_ct_in[i] is served; the words are the oracle's rotate and add,
    step by step"""
    import itertools
    o, e, L, d, elts, key, dkey, rot = _lt_env()
    lib, arr, capi = _lib()
    assert A.RULES["hefx_rotate_add_chain"]["kind"] == A.IN_PLACE
    cts, accs, bufs = _rotate_add_bufs(o, L)
    ke, kk = capi.u32_array(elts[:2]), arr([dkey.ptr] * 2)

    def call(p, outs="o"):
        return lib.hefx_rotate_add_chain(e._h, L, 2, arr([p["i0"], p["i1"]]), ke, kk, arr([p["a0"], p["a1"]]), arr([p["s0"], p["s1"]]),
                                         arr([p[f"{outs}0"], p[f"{outs}1"]]), 3, None)

    t, a = list(cts), list(accs)
    for _ in range(3):
        t = [rot(t[i], i + 1) for i in range(2)]
        a = [o.add(a[i], t[i]) for i in range(2)]
    moves = [{x: (how, y)} for x, y in itertools.combinations(["o0", "o1", "s0", "s1"], 2) for how in ("row_into", "on")]
    _ks_refused_then_accepted(Case(e, o, bufs), call, moves, {"o0": t[0], "o1": t[1], "s0": a[0], "s1": a[1]})
    _accepted(Case(e, o, bufs), lambda p: call(p, "i"), {"i0": t[0], "i1": t[1], "s0": a[0], "s1": a[1]})


def test_apply_galois_forest_refusals():
    """hefx_apply_galois_forest, three nodes -- a root, its child, a second root with a fused plaintext: outputs on one another,
    on an external input or on the plaintext are refused; adjacent, the words of the node-by-node rotations"""
    o, e, L, d, elts, key, dkey, rot = _lt_env()
    lib, arr, capi = _lib()
    assert A.RULES["hefx_apply_galois_forest"]["kind"] == A.NO_OVERLAP
    LN, c2 = L * N, 2 * L * N
    ext = [o.uniform(L, 2, 120), _top(o, L, 2)]
    pt = o.uniform(L, 1, 121)[0]
    bufs = [("e0", c2, ext[0]), ("e2", c2, ext[1]), ("p2", LN, pt)] + [(f"o{i}", c2, None) for i in range(3)]
    parent = (C.c_int32 * 3)(-1, 0, -1)
    ke, kk = capi.u32_array([elts[0], elts[1], elts[1]]), arr([dkey.ptr] * 3)
    call = lambda p: lib.hefx_apply_galois_forest(e._h, L, 3, parent, arr([p["e0"], None, p["e2"]]), ke, kk, arr([None, None, p["p2"]]),  # noqa: E731
                                                  arr([p["o0"], p["o1"], p["o2"]]), None)
    moves = _standard_moves(["e0", "e2", "p2"], ["o0", "o1", "o2"], exact=[("o0", "e0"), ("o2", "e2"), ("o2", "p2")],
                            cross=[("o1", "o0"), ("o2", "o0"), ("o1", "e2"), ("o0", "p2")])
    n0 = rot(ext[0], 1)
    _ks_refused_then_accepted(Case(e, o, bufs), call, moves, {"o0": n0, "o1": rot(n0, 2), "o2": o.rotate_mulplain(ext[1], elts[1], key, pt)})
    e.check_transparent()


def test_linear_transform_cipher_refusals():
    """hefx_linear_transform_cipher, d = 3: d_out3 on d_ct or on a diagonal and a diagonal one row into d_out3 are refused;
    adjacent, the words of rotate, multiply and the sum of the products over the oracle"""
    o, e, L, d, elts, key, dkey, rot = _lt_env()
    lib, arr, capi = _lib()
    assert A.RULES["hefx_linear_transform_cipher"]["kind"] == A.NO_OVERLAP
    c2, c3 = 2 * L * N, 3 * L * N
    ct = o.uniform(L, 2, 130)
    diags = [_top(o, L, 2)] + [o.uniform(L, 2, 131 + i) for i in range(1, d)]
    bufs = [("ct", c2, ct)] + [(f"g{i}", c2, diags[i]) for i in range(d)] + [("out", c3, None)]
    ke, kk = capi.u32_array(elts), arr([dkey.ptr] * 3)
    call = lambda p: lib.hefx_linear_transform_cipher(e._h, L, p["ct"], d, arr([p[f"g{i}"] for i in range(d)]), 3, ke, kk, p["out"], None)  # noqa: E731
    ct_new = o.add(ct, rot(ct, -d))
    want = o.multiply(ct_new, diags[0])
    for l in range(1, d):
        want = o.add(want, o.multiply(rot(ct_new, l), diags[l]))
    moves = _standard_moves(["ct"] + [f"g{i}" for i in range(d)], ["out"], exact=[("out", "ct"), ("out", "g0"), ("out", "g2")])
    _ks_refused_then_accepted(Case(e, o, bufs), call, moves, {"out": want})
    # wrong in two ways at once -- a null Galois key AND the result on an operand: every linear transform checks the aliasing
    # rule before the keys ("The linear transforms' host path"), so the overlap is what is reported; nothing is written
    case = Case(e, o, bufs)
    no_key = lambda p: lib.hefx_linear_transform_cipher(e._h, L, p["ct"], d, arr([p[f"g{i}"] for i in range(d)]), 3, ke,  # noqa: E731
                                                        arr([dkey.ptr, None, dkey.ptr]), p["out"], None)
    before = e.ks_stats()
    for m, text in [({"out": ("on", "ct")}, "overlap"), ({"out": ("row_into", "g1")}, "overlap"), (None, "null Galois key")]:
        with pytest.raises(ValueError, match=text):
            capi.check(no_key(case.place(m)))
        e.sync()
        assert case.unchanged() and e.ks_stats() == before, m


def test_multiply_sum_refusals():
    """hefx_multiply_sum, n = 4, group = 2: an output on an input of the other group and two outputs one row apart (and the
    other standard overlaps) are refused; adjacent, the sums of the oracle's products"""
    o, e = _env()
    lib, arr, _ = _lib()
    assert A.RULES["hefx_multiply_sum"]["kind"] == A.NO_OVERLAP
    L = 3
    c2, c3 = 2 * L * N, 3 * L * N
    a = [_top(o, L, 2)] + [o.uniform(L, 2, 140 + i) for i in range(1, 4)]
    b = [_top(o, L, 2)] + [o.uniform(L, 2, 150 + i) for i in range(1, 4)]
    bufs = [(f"a{i}", c2, a[i]) for i in range(4)] + [(f"b{i}", c2, b[i]) for i in range(4)] + [("o0", c3, None), ("o1", c3, None)]
    call = lambda p: lib.hefx_multiply_sum(e._h, L, 4, 2, arr([p[f"a{i}"] for i in range(4)]), arr([p[f"b{i}"] for i in range(4)]),  # noqa: E731
                                           arr([p["o0"], p["o1"]]), None)
    moves = _standard_moves(["a0", "a3", "b2"], ["o0", "o1"], exact=[("o0", "a1")], cross=[("o0", "a2"), ("o1", "b0"), ("o1", "o0")])
    want = {f"o{g}": o.add(o.multiply(a[2 * g], b[2 * g]), o.multiply(a[2 * g + 1], b[2 * g + 1])) for g in range(2)}
    _ks_refused_then_accepted(Case(e, o, bufs), call, moves, want)
