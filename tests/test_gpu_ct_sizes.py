"""GPU parity of the ciphertext product and relinearisation for ciphertexts of ANY size (hefx_multiply_sizes[_batch],
multiply_sizes_kernel; hefx_relinearize_sizes[_batch]) and of their front ends.  Bar: bit-exact uint64 RNS words against
oracle.Oracle.multiply / a Python loop of Oracle.switch_key, no tolerance; decrypted values at the project's tolerance for
products at scale 2^30."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 2), (2, 3), (3, 3), (4, 2), (5, 4), (8, 9), (15, 2)]

_made = {}


def _mixed_chain(N):
    """a mixed 40- / 60-bit chain (CoeffModulus::Create), special prime last"""
    from seal_fyp_logistic_regression_amd.seal import CoeffModulus
    return CoeffModulus.Create(N, [60, 40, 40, 60])


def _mk(name):
    """(oracle, engine, L): 'mixed2048_chain' / 'mixed8192_chain' at their top data level, or a policy set of
    tests/policy_sets.py over ALL its primes (the element-wise kernels take any L <= k)"""
    if name not in _made:
        from oracle import oracle as O
        from seal_fyp_logistic_regression_amd import Engine
        if name.endswith("_chain"):
            N = int(name[len("mixed"):-len("_chain")])
            primes = _mixed_chain(N)
            L = len(primes) - 1
        else:
            from tests import policy_sets
            s = policy_sets.sets()[name]
            N, primes, L = s.N, s.primes, s.k
        _made[name] = (O.Oracle(N, primes), Engine(N, primes), L)
    return _made[name]


def _policy_names():
    """every set of tests/policy_sets.py, at the size the engine can build it (its GPU size: the toy rings of 16 / 32
    coefficients are below the engine's smallest degree).  Among them the many-row sets f41_wide (62 rows) and lsweep (17),
    which take the row index w >> (log N - 1) far past a handful of rows, the 41- / 42-bit classes and log N = 15."""
    from tests import policy_sets
    return sorted(policy_sets.sets())


POLICY = _policy_names()
assert {"f41_wide", "lsweep", "f41", "i42", "c40_edge", "seal_deep", "small_p", "mixed2048", "straddle60", "p_min61"} <= set(POLICY)
# rings above 4096: the shapes that take each body of the kernel once more -- a compile-time one, the other operand order,
# the run-time loop at its widest -- so that a case stays within seconds (the host reference is the cost)
SHAPES_BIG = [(3, 2), (2, 3), (8, 9)]


# ------------------------------------------------------------------------------------------------------------------
# 1. the product
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed2048_chain", "mixed8192_chain"] + POLICY)
def test_product_word_for_word(name):
    """every shape of the issue (policy sets on rings above 4096: SHAPES_BIG), a square with d_a == d_b, and (2, 2) against
    hefx_multiply"""
    o, e, L = _mk(name)
    shapes = SHAPES if o.N <= 4096 or name.endswith("_chain") else SHAPES_BIG
    host = {s: o.uniform(L, s, 7000 + s) for s in sorted({x for sh in shapes for x in sh} | {2, 3, 8})}
    dev = {s: e.to_device(x) for s, x in host.items()}
    other = {s: o.uniform(L, s, 7100 + s) for s in host}
    for sa, sb in shapes:
        b, db = (other[sb], e.to_device(other[sb]))
        out = e.multiply_sizes(L, sa, dev[sa], sb, db)
        assert out.shape == (sa + sb - 1, L, o.N)
        assert (out.download() == o.multiply(host[sa], b)).all(), (name, sa, sb)
    for s in (3, 8):  # squares: the same buffer on both sides
        assert (e.multiply_sizes(L, s, dev[s], s, dev[s]).download() == o.multiply(host[s], host[s])).all(), (name, s)
    got = e.multiply_sizes(L, 2, dev[2], 2, e.to_device(other[2])).download()
    assert (got == e.multiply(L, dev[2], e.to_device(other[2])).download()).all()
    assert (got == o.multiply(host[2], other[2])).all()


# ------------------------------------------------------------------------------------------------------------------
# 2. the largest residues
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 9), (2, 15), (2, 2)])
def test_accumulator_holds_at_the_largest_residues(shape):
    """every input word q_j - 1 with primes just below 2^61: (q-1)^2 = 1 mod q, so output k is the number of pairs
    i + j = k, mod q -- Python integers, no backend.  The twin of test_fold_intervals_hold_at_the_largest_residues.
    (2, 2) -- outputs 1, 2, 1 -- also through hefx_multiply, hefx_square and a hefx_multiply_batch of three: one kernel
    family behind all of them."""
    o, e, L = _mk("p_min61")
    assert sum(p > 1 << 60 for p in o.primes[:L]) >= 8
    sa, sb = shape

    def top(size):
        x = np.zeros((size, L, o.N), dtype=np.uint64)
        for j in range(L):
            x[:, j, :] = o.primes[j] - 1
        return e.to_device(x)

    da, db = top(sa), top(sb)
    results = [e.multiply_sizes(L, sa, da, sb, db)]
    if shape == (2, 2):
        results += [e.multiply(L, da, db), e.square(L, da)] + e.multiply_batch(L, [da, db, da], [db, db, da])
    for which, out in enumerate(results):
        got = out.download()
        for k in range(sa + sb - 1):
            terms = sum(1 for i in range(sa) if 0 <= k - i < sb)
            for j in range(L):
                assert (got[k, j] == terms % o.primes[j]).all(), (shape, which, k, j)


# ------------------------------------------------------------------------------------------------------------------
# 3. the batch form
# ------------------------------------------------------------------------------------------------------------------
def test_batch_of_seven_with_a_repeated_operand():
    o, e, L = _mk("mixed8192_chain")
    A = [o.uniform(L, 3, 7200 + i) for i in range(7)]
    B = [o.uniform(L, 3, 7300 + i) for i in range(2)]
    dA, dB = [e.to_device(x) for x in A], [e.to_device(x) for x in B]
    outs = e.multiply_sizes_batch(L, 3, dA, 3, [dB[i % 2] for i in range(7)])
    for i, out in enumerate(outs):
        assert (out.download() == o.multiply(A[i], B[i % 2])).all(), i


def test_batch_whose_items_outgrow_one_pass_of_the_grid():
    """C3 (N = 16384, L = 5): 40960 records per polynomial against the 64 x 256 lanes an item of the pointer-table twin
    gets, so every lane walks its grid stride; a compile-time shape and a run-time one"""
    from oracle import oracle as O
    from seal_fyp_logistic_regression_amd import Engine
    from seal_fyp_logistic_regression_amd.seal import CoeffModulus
    N = 16384
    primes = CoeffModulus.Create(N, [60, 40, 40, 40, 40, 60])
    o, e, L = O.Oracle(N, primes), Engine(N, primes), 5
    assert L * N // 2 > 64 * 256
    for sa, sb in ((3, 2), (5, 4)):
        A = [o.uniform(L, sa, 7800 + 10 * sa + i) for i in range(3)]
        B = [o.uniform(L, sb, 7900 + 10 * sb + i) for i in range(2)]
        dA, dB = [e.to_device(x) for x in A], [e.to_device(x) for x in B]
        outs = e.multiply_sizes_batch(L, sa, dA, sb, [dB[i % 2] for i in range(3)])
        for i, out in enumerate(outs):
            assert (out.download() == o.multiply(A[i], B[i % 2])).all(), (sa, sb, i)
    e.close()


def test_batch_that_crosses_a_pointer_table_slice():
    """N = 2048, L = 2, shape (3, 2): more items than one descriptor-ring slot holds triples, inputs from a pool of five,
    outputs distinct; the first and last item of each slice and 32 sampled items against the oracle"""
    from tests.test_gpu_multiply_sum import _table_slice
    from oracle import oracle as O
    from seal_fyp_logistic_regression_amd import Engine
    N = 2048
    primes = _mixed_chain(N)[:2] + _mixed_chain(N)[-1:]
    o, e, L = O.Oracle(N, primes), Engine(N, primes), 2
    slice_ = _table_slice() // 3
    n = slice_ + 37
    A = [o.uniform(L, 3, 7400 + i) for i in range(5)]
    B = [o.uniform(L, 2, 7500 + i) for i in range(5)]
    dA, dB = [e.to_device(x) for x in A], [e.to_device(x) for x in B]
    ia, ib = (lambda i: i % 5), (lambda i: (3 * i + i // 5) % 5)
    outs = e.multiply_sizes_batch(L, 3, [dA[ia(i)] for i in range(n)], 2, [dB[ib(i)] for i in range(n)])
    rng = np.random.default_rng(3)
    picks = {0, slice_ - 1, slice_, n - 1} | {int(x) for x in rng.integers(0, n, 32)}
    prod = {}
    for i in sorted(picks):
        key = (ia(i), ib(i))
        if key not in prod:
            prod[key] = o.multiply(A[key[0]], B[key[1]])
        assert (outs[i].download() == prod[key]).all(), i
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. relinearisation
# ------------------------------------------------------------------------------------------------------------------
class _Relin:
    """one ring: oracle, engine, a secret key, the keys of s^2 .. s^4 from Oracle.gen_kswitch_key"""

    def __init__(self, N):
        from oracle import oracle as O
        from seal_fyp_logistic_regression_amd import Engine
        primes = _mixed_chain(N)
        self.o, self.e, self.N, self.k = O.Oracle(N, primes), Engine(N, primes), N, len(primes)
        o = self.o
        sk = o.gen_secret(11)
        power, self.keys = sk, {}
        for p in range(2, 5):
            power = o.multiply_plain(power[None], sk)[0]
            key = np.zeros((self.k - 1, 2, self.k, N), dtype=np.uint64)
            O.lib().orc_gen_kswitch_key(o._h, sk, np.ascontiguousarray(power), 900 + p, key)
            self.keys[p] = key
        self.dkeys = {p: self.e.to_device(k) for p, k in self.keys.items()}

    def want(self, ct, size_out):
        """SEAL's relinearize_internal as a Python loop of Oracle.switch_key: from the top, polynomial t with the key of
        s^t into (c0, c1)"""
        o, size_in = self.o, ct.shape[0]
        head = np.ascontiguousarray(ct[:2])
        for t in range(size_in - 1, size_out - 1, -1):
            head = o.switch_key(head, ct[t], self.keys[t])
        return np.concatenate([head, ct[2:size_out]]) if size_out > 2 else head

    def key_list(self, size_in):
        return [self.dkeys.get(p) for p in range(2, size_in)]


_relin = {}


def _rl(N):
    if N not in _relin:
        _relin[N] = _Relin(N)
    return _relin[N]


@pytest.mark.parametrize("N", [2048, 8192])
def test_relinearize_word_for_word(N):
    """size_in 3, 4, 5 -> 2 and 5 -> 3, at the top level and one below; size_in = 3 equals hefx_relinearize"""
    r = _rl(N)
    o, e = r.o, r.e
    for L in (r.k - 1, r.k - 2):
        for size_in, size_out in ((3, 2), (4, 2), (5, 2), (5, 3)):
            ct = o.uniform(L, size_in, 7600 + 10 * size_in + size_out + L)
            got = e.relinearize_sizes(L, size_in, size_out, e.to_device(ct), r.key_list(size_in))
            assert got.shape == (size_out, L, N)
            assert (got.download() == r.want(ct, size_out)).all(), (N, L, size_in, size_out)
            if size_in == 3:
                assert (got.download() == e.relinearize(L, e.to_device(ct), r.dkeys[2]).download()).all()


@pytest.mark.parametrize("n", [1, 8, 40])
def test_relinearize_batches(n):
    """1, 8 and 40 items: the pair path, the small path and a regular chunk of the key switch; 4 -> 2 and 5 -> 3"""
    r = _rl(2048)
    o, e, L = r.o, r.e, r.k - 1
    for size_in, size_out in ((4, 2), (5, 3)):
        cts = o.uniform(L, size_in * n, 7700 + n + size_in).reshape(n, size_in, L, r.N)
        outs = e.relinearize_sizes_batch(L, size_in, size_out, [e.to_device(c) for c in cts], r.key_list(size_in))
        for i in sorted({0, n // 2, n - 1}):
            assert (outs[i].download() == r.want(cts[i], size_out)).all(), (n, size_in, i)
        if n == 8:  # every item once
            for i in range(n):
                assert (outs[i].download() == r.want(cts[i], size_out)).all(), (n, size_in, i)


def test_relinearize_batch_longer_than_one_staging_group():
    """more items than one staging group holds (include/hefx.h: floor(1 GiB / (6 L N 8 B)) items per group): the groups
    go through the same blocks one after the other.  N = 2048, L = 2, 4 -> 2; inputs from a pool of five, outputs
    distinct; the first and last item of each group and 12 sampled items against the oracle loop"""
    r = _rl(2048)
    o, e, L = r.o, r.e, 2
    group = (1 << 30) // (6 * L * r.N * 8)
    n = group + 29
    pool = [o.uniform(L, 4, 7950 + i) for i in range(5)]
    dpool = [e.to_device(x) for x in pool]
    want = [r.want(x, 2) for x in pool]
    outs = e.relinearize_sizes_batch(L, 4, 2, [dpool[i % 5] for i in range(n)], r.key_list(4))
    rng = np.random.default_rng(4)
    for i in sorted({0, group - 1, group, n - 1} | {int(x) for x in rng.integers(0, n, 12)}):
        assert (outs[i].download() == want[i % 5]).all(), i


# ------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_anything_is_written():
    from seal_fyp_logistic_regression_amd import capi
    r = _rl(2048)
    o, e, L, N = r.o, r.e, r.k - 1, r.N
    lib, arr = capi.lib(), capi.ptr_array
    canary = o.uniform(L, 20, 5).reshape(-1)
    big = e.to_device(canary)                       # sentinel: every output below is a view into it
    a2, a3, a9 = (e.to_device(o.uniform(L, s, 6 + s)) for s in (2, 3, 9))
    one = e.to_device(o.uniform(L, 1, 9))
    keys = arr([k.ptr for k in r.key_list(5)])
    pw = L * N

    def refused(rc, text):
        e.sync()
        assert rc == capi.HEFX_ERR_INVALID, rc
        assert text in lib.hefx_last_error().decode(), lib.hefx_last_error().decode()
        assert (big.download() == canary).all()

    out = big.view(0, (17, L, N))
    refused(lib.hefx_multiply_sizes(e._h, L, 1, one.ptr, 2, a2.ptr, out.ptr, None), "at least 2")
    refused(lib.hefx_multiply_sizes(e._h, L, 2, a2.ptr, 1, one.ptr, out.ptr, None), "at least 2")
    refused(lib.hefx_multiply_sizes(e._h, L, 9, a9.ptr, 9, a9.ptr, out.ptr, None), "HEFX_CT_SIZE_MAX = 16")
    refused(lib.hefx_multiply_sizes_batch(e._h, L, 1, 9, arr([a9.ptr]), 9, arr([a9.ptr]), arr([out.ptr]), None),
            "HEFX_CT_SIZE_MAX = 16")
    # an output that reaches into an input: views of one allocation
    in_view = big.view(0, (3, L, N))
    refused(lib.hefx_multiply_sizes(e._h, L, 3, in_view.ptr, 2, a2.ptr, big.view(3 * pw - N, (4, L, N)).ptr, None), "overlaps")
    refused(lib.hefx_multiply_sizes(e._h, L, 2, a2.ptr, 3, big.view(4 * pw - 8, (3, L, N)).ptr, big.view(0, (4, L, N)).ptr, None),
            "overlaps")
    refused(lib.hefx_multiply_sizes_batch(e._h, L, 2, 3, arr([a3.ptr, a3.ptr]), 2, arr([a2.ptr, a2.ptr]),
                                          arr([big.view(0, (4, L, N)).ptr, big.view(4 * pw - 2, (4, L, N)).ptr]), None), "overlap")
    # relinearisation: sizes, a missing key entry, overlap
    ct5 = big.view(5 * pw, (5, L, N))
    out2 = big.view(0, (2, L, N))
    refused(lib.hefx_relinearize_sizes(e._h, L, 5, 5, ct5.ptr, keys, out2.ptr, None), "size_out < size_in")
    refused(lib.hefx_relinearize_sizes(e._h, L, 3, 4, ct5.ptr, keys, out2.ptr, None), "size_out < size_in")
    refused(lib.hefx_relinearize_sizes(e._h, L, 5, 1, ct5.ptr, keys, out2.ptr, None), "size_out < size_in")
    refused(lib.hefx_relinearize_sizes(e._h, L, 17, 2, ct5.ptr, keys, out2.ptr, None), "HEFX_CT_SIZE_MAX = 16")
    holed = arr([r.dkeys[2].ptr, None, r.dkeys[4].ptr])
    refused(lib.hefx_relinearize_sizes(e._h, L, 5, 2, ct5.ptr, holed, out2.ptr, None), "missing")
    refused(lib.hefx_relinearize_sizes(e._h, L, 5, 2, ct5.ptr, keys, big.view(5 * pw - N, (2, L, N)).ptr, None), "overlaps")
    # ... and what IS fine: the key of s^2 may be absent for 5 -> 3, adjacent views are no overlap
    ct = canary[5 * pw:10 * pw].reshape(5, L, N)
    sep = e.empty(3, L, N)
    lower = arr([None, r.dkeys[3].ptr, r.dkeys[4].ptr])
    capi.check(lib.hefx_relinearize_sizes(e._h, L, 5, 3, ct5.ptr, lower, sep.ptr, None))
    assert (sep.download() == r.want(ct, 3)).all()
    with pytest.raises(ValueError, match="overlaps"):
        e.multiply_sizes(L, 3, in_view, 2, a2, out=big.view(3 * pw - N, (4, L, N)))
    got = e.multiply_sizes(L, 3, in_view, 2, a2, out=big.view(3 * pw, (4, L, N))).download()
    assert (got == o.multiply(canary[:3 * pw].reshape(3, L, N), a2.download())).all()


# ------------------------------------------------------------------------------------------------------------------
# 6. a caller-owned stream held shut by a gate
# ------------------------------------------------------------------------------------------------------------------
def test_new_entries_on_a_caller_owned_stream():
    """both new entries (single and batch form) behind the host-function gate, under the decoy protocol of
    tests/test_gpu_streams.py: each call returns while the stream is shut, and snapshots and outputs are the oracle's"""
    from tests.hip_stream_gate import Stream
    from tests.test_gpu_streams import Op, run_gated
    r = _rl(2048)
    o, e, L, N = r.o, r.e, r.k - 1, r.N

    class W:
        pass

    w = W()
    w.e, w.o, w.k, w.S = e, o, r.k, Stream()
    seeds = iter(range(8000, 9000))
    w.junk = lambda shape: o.uniform(shape[-2], int(np.prod(shape[:-2], dtype=np.int64)) if len(shape) > 2 else 1,
                                     next(seeds)).reshape(shape)
    ct = lambda size: o.uniform(L, size, next(seeds))
    a, b, da, db = ct(3), ct(4), ct(3), ct(4)
    c5, d5 = ct(5), ct(5)
    A, B, DA, DB = [ct(3) for _ in range(3)], [ct(2) for _ in range(3)], [ct(3) for _ in range(3)], [ct(2) for _ in range(3)]
    C4, D4 = [ct(4) for _ in range(9)], [ct(4) for _ in range(9)]
    keys5, keys4 = r.key_list(5), r.key_list(4)
    # warm: the staging workspace and the key switch's scratch exist before the gate shuts (their growth does not wait
    # for the device either, but the first use also loads code objects)
    e.relinearize_sizes_batch(L, 5, 2, [e.to_device(ct(5)) for _ in range(9)], keys5)
    e.sync()
    ops = [
        Op(w, "multiply_sizes", [a, b], [da, db], [o.multiply(a, b)], [o.multiply(da, db)],
           lambda i, t, s: e.multiply_sizes(L, 3, i[0], 4, i[1], out=t[0], stream=s)),
        Op(w, "multiply_sizes_batch", A + B, DA + DB, [o.multiply(x, y) for x, y in zip(A, B)],
           [o.multiply(x, y) for x, y in zip(DA, DB)],
           lambda i, t, s: e.multiply_sizes_batch(L, 3, i[:3], 2, i[3:], outs=t, stream=s)),
        Op(w, "relinearize_sizes", [c5], [d5], [r.want(c5, 2)], [r.want(d5, 2)],
           lambda i, t, s: e.relinearize_sizes(L, 5, 2, i[0], keys5, out=t[0], stream=s)),
        Op(w, "relinearize_sizes 5 -> 3", [c5], [d5], [r.want(c5, 3)], [r.want(d5, 3)],
           lambda i, t, s: e.relinearize_sizes(L, 5, 3, i[0], keys5, out=t[0], stream=s), c_name="hefx_relinearize_sizes"),
        Op(w, "relinearize_sizes_batch", C4, D4, [r.want(x, 2) for x in C4], [r.want(x, 2) for x in D4],
           lambda i, t, s: e.relinearize_sizes_batch(L, 4, 2, i, keys4, outs=t, stream=s)),
    ]
    try:
        run_gated(w, ops)
    finally:
        w.S.destroy()


# ------------------------------------------------------------------------------------------------------------------
# 7. the front end
# ------------------------------------------------------------------------------------------------------------------
def test_xyz_without_intermediate_relinearisation(rescale_mode):
    """Evaluator on the engine against the oracle twin that has the new methods: x * y * z as a size-4 ciphertext, one
    relinearize_inplace with relin_keys(2), two rescales -- same words, sizes, levels and scales; both the size-4 ciphertext
    and the relinearised one decrypt to x * y * z (atol 1e-2 at scale 2^30, inputs in [-1, 1]: the tolerance of
    tests/test_multiply_sum_cpu.py for decrypted products, which tests/test_ct_sizes_cpu.py holds the twin to)"""
    from tests.ct_sizes_backend import make, xyz, VALUES
    res = {}
    for kind in ("gpu", "oracle"):
        e = make(4096, [50, 30, 30, 30, 50], kind, seed=5)
        res[kind] = (e, xyz(e))
    (eg, sg), (eo, so) = res["gpu"], res["oracle"]
    assert hasattr(eg["ctx"].backend, "engine")
    host = lambda e, c: np.asarray(e["ctx"].backend.to_host(c.data)).reshape(c.size(), c.parms_id(), e["ctx"].N)
    for tag in ("size4", "relin", "rescaled"):
        g, t = sg[tag], so[tag]
        assert g.size() == t.size() and g.parms_id() == t.parms_id() and g.scale == t.scale, tag
        assert (host(eg, g) == host(eo, t)).all(), tag
    assert sg["size4"].size() == 4 and sg["relin"].size() == 2 and sg["rescaled"].parms_id() == sg["relin"].parms_id() - 2
    want = VALUES[0] * VALUES[1] * VALUES[2]
    for tag in ("size4", "relin", "rescaled"):
        got = eg["encoder"].decode(eg["dec"].decrypt(sg[tag]))[:len(want)].real
        assert np.allclose(got, want, atol=1e-2), (tag, np.abs(got - want).max())


def test_unequal_size_add_and_sub_on_the_device():
    from tests.ct_sizes_backend import make
    res = {}
    for kind in ("gpu", "oracle"):
        e = make(4096, [50, 30, 30, 50], kind, seed=6)
        ev, scale = e["ev"], 2.0 ** 30
        x = e["enc"].encrypt(e["encoder"].encode([0.5, -0.25], scale))
        y = e["enc"].encrypt(e["encoder"].encode([0.125, 0.75], scale))
        p = ev.multiply(x, y)                                   # size 3, scale^2
        x2 = e["enc"].encrypt(e["encoder"].encode([0.5, -0.25], scale * scale))
        res[kind] = [np.asarray(e["ctx"].backend.to_host(c.data)).reshape(3, c.parms_id(), -1)
                     for c in (ev.add(p, x2), ev.add(x2, p), ev.sub(p, x2), ev.sub(x2, p))]
    for g, t in zip(res["gpu"], res["oracle"]):
        assert (g == t).all()


# ------------------------------------------------------------------------------------------------------------------
# 8. the C++ shim
# ------------------------------------------------------------------------------------------------------------------
def test_ct_sizes_selftest_driver():
    """drivers/ct_sizes_selftest.cpp through include/seal/seal.h: multiply (3,2) and (3,3), relinearise with relin_keys(3),
    a save / load round trip of that key set and evaluation with the loaded keys, unequal-size add; lazy and live modes
    give the same words"""
    exe = os.path.join(ROOT, "drivers", "_ref", "ct_sizes_selftest")
    if not os.path.exists(exe):  # our own source: build it where it is missing
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "drivers"), "_ref/ct_sizes_selftest"], check=False)
    assert os.path.exists(exe), "drivers/_ref/ct_sizes_selftest could not be built (make -C drivers _ref/ct_sizes_selftest)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SELFTEST PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout
