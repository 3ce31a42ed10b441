"""The batched element-wise and product entries ACROSS a pointer-table slice (one descriptor-ring slot): hefx_add_batch,
hefx_sub_batch, hefx_multiply_batch, hefx_multiply_plain_batch, hefx_rescale_to_next_batch, the grouped sums
hefx_multiply_plain_sum / hefx_multiply_sum over several groups, and the limit of a group longer than a slot.  Every
boundary comes from the engine's sources (_table_slice).  N = 2048, L = 2: the smallest ring rescale accepts; inputs from a
pool of five buffers, outputs distinct.  Bar: bit-exact uint64 RNS words against the oracle, no tolerance."""
import numpy as np
import pytest

from tests.test_gpu_multiply_sum import _table_slice

pytestmark = pytest.mark.gpu

N, L = 2048, 2
_made = {}


def _mk():
    """(oracle, engine, five size-2 ciphertexts A, five more B, five plaintexts P -- host words, then their uploads)"""
    if not _made:
        from oracle import oracle as O
        from seal_fyp_logistic_regression_amd import Engine
        from seal_fyp_logistic_regression_amd.seal import CoeffModulus
        chain = CoeffModulus.Create(N, [60, 40, 40, 60])
        primes = chain[:2] + chain[-1:]
        o, e = O.Oracle(N, primes), Engine(N, primes)
        A = [o.uniform(L, 2, 8100 + i) for i in range(5)]
        B = [o.uniform(L, 2, 8200 + i) for i in range(5)]
        P = [o.uniform(L, 1, 8300 + i)[0] for i in range(5)]
        _made["x"] = (o, e, A, B, P, *([e.to_device(x) for x in X] for X in (A, B, P)))
    return _made["x"]


def _ia(i):
    return i % 5


def _ib(i):
    return (3 * i + i // 5) % 5  # every (ia, ib) pair occurs; never slab order


def _picks(n, slice_, extra, seed):
    """the first and last item of each slice and `extra` seeded random ones"""
    assert 0 < slice_ < n <= 2 * slice_
    return sorted({0, slice_ - 1, slice_, n - 1} | {int(x) for x in np.random.default_rng(seed).integers(0, n, extra)})


@pytest.mark.parametrize("entry", ["add_batch", "sub_batch", "sub_batch_in_place", "multiply_batch", "multiply_plain_batch",
                                   "rescale_batch_floor", "rescale_batch_round"])
def test_batch_entry_across_a_table_slice(entry):
    """n = items per slice + 37 through the pointer-table path; items {0, slice - 1, slice, n - 1} and 32 sampled ones word
    for word.  sub_batch_in_place: out[i] is d_a[i] (n distinct first operands: the sums of an add_batch)."""
    o, e, A, B, P, dA, dB, dP = _mk()
    rescale = entry.startswith("rescale")
    slice_ = _table_slice() // (2 if rescale else 3)
    n = slice_ + 37
    As, Bs = [dA[_ia(i)] for i in range(n)], [dB[_ib(i)] for i in range(n)]
    assert not e.contiguous(As) and not e.contiguous(Bs)
    cache = {}

    def want(i, f):
        key = (_ia(i), _ib(i))
        if key not in cache:
            cache[key] = f(*key)
        return cache[key]

    if entry == "add_batch":
        outs, f = e.add_batch(L, 2, As, Bs), lambda a, b: o.add(A[a], B[b])
    elif entry == "sub_batch":
        outs, f = e.sub_batch(L, 2, As, Bs), lambda a, b: o.sub(A[a], B[b])
    elif entry == "sub_batch_in_place":
        sums = e.add_batch(L, 2, As, Bs)
        outs = e.sub_batch(L, 2, sums, [dA[_ib(i)] for i in range(n)], outs=sums)
        assert all(x is y for x, y in zip(outs, sums))
        f = lambda a, b: o.sub(o.add(A[a], B[b]), A[b])
    elif entry == "multiply_batch":
        outs, f = e.multiply_batch(L, As, Bs), lambda a, b: o.multiply(A[a], B[b])
    elif entry == "multiply_plain_batch":
        outs, f = e.multiply_plain_batch(L, 2, As, [dP[_ib(i)] for i in range(n)]), lambda a, b: o.multiply_plain(A[a], P[b])
    else:
        rounded, before = entry.endswith("round"), e.rescale_rounded
        e.set_rescale_rounded(rounded)
        try:
            outs = e.rescale_batch(L, 2, As)
        finally:
            e.set_rescale_rounded(before)
        f = lambda a, b: o.rescale(A[a], rounded=rounded)
    assert len(outs) == n
    for i in _picks(n, slice_, 32, 5):
        assert (outs[i].download() == want(i, f)).all(), (entry, i)


@pytest.mark.parametrize("entry", ["multiply_plain_sum", "multiply_sum"])
def test_grouped_sums_across_a_table_slice(entry):
    """groups of 3 (2 * 3 + 1 pointers each), 20 groups more than one slot holds, the last group ragged; the first group, the
    last group of slice one, the first of slice two, the last group and 16 sampled ones against multiply[_plain] per term,
    then add"""
    o, e, A, B, P, dA, dB, dP = _mk()
    group = 3
    gps = _table_slice() // (2 * group + 1)
    groups = gps + 20
    n = group * groups - 1
    assert n % group and (n + group - 1) // group == groups
    As = [dA[_ia(i)] for i in range(n)]
    plain = entry == "multiply_plain_sum"
    if plain:
        outs = e.multiply_plain_sum(L, 2, As, [dP[_ib(i)] for i in range(n)], group)
    else:
        outs = e.multiply_sum(L, As, [dB[_ib(i)] for i in range(n)], group)
    assert len(outs) == groups
    term = {}
    for g in _picks(groups, gps, 16, 6):
        acc = None
        for i in range(g * group, min(n, (g + 1) * group)):
            key = (_ia(i), _ib(i))
            if key not in term:
                term[key] = o.multiply_plain(A[key[0]], P[key[1]]) if plain else o.multiply(A[key[0]], B[key[1]])
            acc = term[key] if acc is None else o.add(acc, term[key])
        assert (outs[g].download() == acc).all(), (entry, g)


def test_a_group_of_more_than_96_slot_sized_parts_is_refused_by_both_sums():
    """n = group = 96 * ((slot - 1) // 2) + 1 terms: 97 slot-sized parts, one more than hefx_add_many sums without a scratch
    level of its own.  hefx_multiply_plain_sum and hefx_multiply_sum both return HEFX_ERR_UNSUPPORTED before anything is
    submitted; the output keeps its words.  (Before the two entries shared one long-group rule the plain form did not
    refuse: it summed its parts through a scratch level that lay on the parts.)"""
    from seal_fyp_logistic_regression_amd import capi
    o, e, A, B, P, dA, dB, dP = _mk()
    lib = capi.lib()
    n = 96 * ((_table_slice() - 1) // 2) + 1
    canary = o.uniform(L, 3, 8400)
    out = e.to_device(canary)
    cts, pts, outs = capi.ptr_array([dA[0].ptr] * n), capi.ptr_array([dP[0].ptr] * n), capi.ptr_array([out.ptr])
    for rc in (lib.hefx_multiply_plain_sum(e._h, L, 2, n, n, cts, pts, outs, None),
               lib.hefx_multiply_sum(e._h, L, n, n, cts, cts, outs, None)):
        assert rc == capi.HEFX_ERR_UNSUPPORTED, (rc, lib.hefx_last_error())
        assert b"group too long" in lib.hefx_last_error()
        e.sync()
        assert (out.download() == canary).all()
