"""Every C-ABI entry on a CALLER-OWNED stream (include/hefx.h: "asynchronous on that stream", "ordered on the caller's stream").

The default stream is the one stream on which a wrong-stream bug cannot show: the legacy default stream synchronises with
every blocking stream, so an internal copy or launch issued on stream 0 instead of the caller's still lands in order.
Here every entry runs on a non-blocking stream S that a GATE (tests/hip_stream_gate.py: a host function that sleeps, then
sets `opened`) holds shut while the host submits behind it -- the host-function gate, not the fallback producer.

The DECOY protocol, the same for every case (class Op):
  before the gate   everything is uploaded (hefx_upload synchronises).  Every buffer the entry READS holds a decoy -- a
                    valid operand of the same shape from another seed -- and the real operand waits in a staging buffer;
                    every output buffer holds a decoy too.
  behind the gate   on S, in this order: (1) hefx_copy staging -> inputs, (2) the entry, (3) hefx_copy outputs -> snapshots,
                    (4) hefx_copy decoys -> inputs.
  then              `not gate.opened` (the entry returned while S was still shut) for every entry hefx.h does not list as
                    waiting on the host; hefx_stream_sync(S); snapshot AND output against oracle.Oracle on the real
                    operands, word for word.
(1) catches any internal step that runs ahead of S (stream 0, an unforked internal stream): it reads decoys.  (4) catches
internal streams that were not joined back to S: the entry would still be reading when its inputs change.  (3) catches
outputs written after the call's place in S.  Every case first asserts that the oracle gives other words on the decoys.

Shown to detect, once, on two planted defects built outside the tree (an element-wise launch on stream 0; ks_run without the
wait for its internal streams' join events): both fail here by mismatch."""
import json
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "appendix_b.json")))
C2 = next((s["N"], [int(p, 16) for p in s["primes"]]) for s in GOLD["sets"] if s["name"] == "C2")
C5 = (32768, [0xfffffffff840001, 0xffff940001, 0xffffb20001, 0xffffc40001, 0xffffe80001, 0xffffffffffc0001])

# The entries of include/hefx.h that may wait on the host -- exactly the list of its conventions block
# (test_header_names_every_host_blocking_entry).  Every OTHER entry must return while its stream is still shut.
HOST_BLOCKING = {
    # always, by their purpose
    "hefx_upload", "hefx_download", "hefx_stream_sync", "hefx_check_transparent", "hefx_ckks_decode", "hefx_event_elapsed_ms",
    "hefx_ks_fallback_count", "hefx_profile_begin", "hefx_profile_end", "hefx_context_destroy",
    # on the first use of a Galois element on the exactly hoisted path
    "hefx_rotate_hoisted_batch", "hefx_apply_galois_batch", "hefx_rotate_multiply_plain_batch", "hefx_apply_galois_add_batch",
    "hefx_rotate_add_chain", "hefx_apply_galois_forest", "hefx_linear_transform_plain", "hefx_linear_transform_plain_many",
    "hefx_linear_transform_plain_hoisted", "hefx_linear_transform_plain_bsgs", "hefx_linear_transform_cipher",
    # when a call outgrows a buffer that cannot be retired while in use
    "hefx_multiply_plain", "hefx_ckks_encode", "hefx_ckks_encode_batch", "hefx_free",
}
# ... of which these wait only on the FIRST USE of an element / of a size: the cases below that are not such a first use
# hold them to `not gate.opened` like everything else
FIRST_USE_ONLY = HOST_BLOCKING - {"hefx_upload", "hefx_download", "hefx_stream_sync", "hefx_check_transparent", "hefx_ckks_decode",
                                  "hefx_event_elapsed_ms", "hefx_ks_fallback_count", "hefx_profile_begin", "hefx_profile_end",
                                  "hefx_context_destroy"}


def test_header_names_every_host_blocking_entry():
    """the conventions block of hefx.h lists the entries that wait on the host BY NAME, and states the two-stream rule; the
    exemption list of this module is that list"""
    text = open(os.path.join(ROOT, "include", "hefx.h")).read()
    block = text[text.index("Conventions"):text.index("#ifndef HEFX_H")]
    start = block.index("The entries that DO wait on the host")
    listed = set(re.findall(r"hefx_[a-z0-9_]+", block[start:block.index("Besides these")]))
    assert listed == HOST_BLOCKING, (sorted(listed - HOST_BLOCKING), sorted(HOST_BLOCKING - listed))
    rule = " ".join(block[block.index("One context, one order"):].replace("*", " ").split())
    assert "belong to the CONTEXT, not to the stream" in rule and "ordered with events" in rule
    assert "UNORDERED streams" in rule and "a context per stream" in rule


# ------------------------------------------------------------------------------------------------------------------
# the world: one engine, one oracle, one caller-owned stream, shared references
# ------------------------------------------------------------------------------------------------------------------
class World:
    def __init__(self, N, primes, L):
        from oracle import oracle as O
        from seal_fyp_logistic_regression_amd import Engine
        from tests.hip_stream_gate import Stream
        self.e = Engine(N, primes)
        self.O, self.o, self.N, self.primes, self.k, self.L = O, O.Oracle(N, primes), N, list(primes), len(primes), L
        self.S = Stream()
        self._seed = 10_000
        self._rot = {}
        rng = np.random.default_rng(N + L)
        self.keys = [self.key(31 + i) for i in range(3)]
        self.dkeys = [self.e.to_device(k) for k in self.keys]
        # item i of every key-switch batch: ciphertext A[i] (decoy B[i]) rotated by elts[i] with keys[ki[i]]
        self.elts = [int(2 * rng.integers(1, N) + 1) for _ in range(640)]
        self.ki = [int(rng.integers(3)) for _ in range(640)]

    def close(self):
        self.S.destroy()
        self.e.close()

    def seed(self):
        self._seed += 1
        return self._seed

    def ct(self, size=2, L=None):
        return self.o.uniform(L or self.L, size, self.seed())

    def cts(self, n, size=2, L=None):
        """n ciphertexts as one array [n][size][L][N]"""
        L = L or self.L
        return self.o.uniform(L, size * n, self.seed()).reshape(n, size, L, self.N)

    def pt(self, L=None):
        return self.o.uniform(L or self.L, 1, self.seed())[0]

    def pts(self, n, L=None):
        L = L or self.L
        return self.o.uniform(L, n, self.seed()).reshape(n, L, self.N)

    def key(self, seed):
        return self.o.uniform(self.k, 2 * (self.k - 1), seed).reshape(self.k - 1, 2, self.k, self.N)

    def junk(self, shape):
        """canonical residues of the shape [..][rows][N] (an output's decoy filling)"""
        rows = shape[-2]
        assert rows <= self.k
        n = int(np.prod(shape[:-2], dtype=np.int64)) if len(shape) > 2 else 1
        return self.o.uniform(rows, n, self.seed()).reshape(shape)

    def rot(self, tag, ct, elt, ki):
        """o.apply_galois, computed once per tag"""
        if tag not in self._rot:
            self._rot[tag] = self.o.apply_galois(np.ascontiguousarray(ct), elt, self.keys[ki])
        return self._rot[tag]


@pytest.fixture(scope="module")
def w():
    world = World(*C2, L=3)
    yield world
    world.close()


def views(dev, n):
    """the n equal parts of a device array [n][...]"""
    words = dev.nwords // n
    return [dev.view(i * words, dev.shape[1:]) for i in range(n)]


class Op:
    """One entry under the decoy protocol.  reals / decoys: the arrays the entry reads (same shapes); want: the oracle's
    outputs on the reals (None: not checked -- the sampled items of a large batch), want_decoy: on the decoys, for at least
    one output; call(ins, outs, stream) submits the entry; inplace: indices of the inputs that ARE the outputs."""

    def __init__(self, w, name, reals, decoys, want, want_decoy, call, inplace=None, out_shapes=None, c_name=None):
        e = w.e
        self.w, self.name, self.call, self.want, self.c_name = w, name, call, list(want), c_name
        differs = []
        for a, b in zip(want, want_decoy):  # a decoy result may be given for sampled items only: {index: words}
            if isinstance(b, dict):
                differs += [(a[i] != x).any() for i, x in b.items()]
            else:
                differs.append((a != b).any())
        assert differs and all(differs), f"{name}: the decoys give the real operands' words -- the case would pass vacuously"
        self.ins = [e.to_device(d) for d in decoys]
        self.stage = [e.to_device(r) for r in reals]
        self.dec = [e.to_device(d) for d in decoys]
        self.inplace = inplace
        if inplace is None:
            shapes = out_shapes or [x.shape for x in want]
            self.outs = [e.to_device(w.junk(s)) for s in shapes]
        else:
            self.outs = [self.ins[i] for i in inplace]
        self.snaps = [e.empty(*o.shape) for o in self.outs]

    def submit(self, stream):
        e = self.w.e
        for i, s in zip(self.ins, self.stage):
            e.copy_raw(i.ptr, s.ptr, s.nbytes, stream)       # (1)
        self.call(self.ins, self.outs, stream)               # (2)
        for o, s in zip(self.outs, self.snaps):
            e.copy_raw(s.ptr, o.ptr, o.nbytes, stream)       # (3)
        for i, d in zip(self.ins, self.dec):
            e.copy_raw(i.ptr, d.ptr, d.nbytes, stream)       # (4)

    def check(self):
        for j, want in enumerate(self.want):
            for what, buf in (("snapshot", self.snaps[j]),) + ((("output", self.outs[j]),) if self.inplace is None else ()):
                got = buf.download()
                if isinstance(want, dict):  # sampled items of a batch: {index: words}
                    for i, x in want.items():
                        assert (got[i] == x).all(), (self.name, what, j, i)
                elif want is not None:
                    assert (got.reshape(want.shape) == want).all(), (self.name, what, j)


def run_gated(w, ops, exempt=False, stream=None, hold=None):
    """all `ops` behind ONE gate on the world's stream; none of them may have waited for the stream unless `exempt`.
    hold: seconds the gate stays shut, for the cases whose submission is long on the HOST (the time each submission took is
    printed: a submission that outlasts the gate without waiting for anything looks like one that waited)"""
    import time
    S = stream or w.S
    gate = S.gate(*([hold] if hold else []))
    for op in ops:
        t0 = time.perf_counter()
        op.submit(S.handle)
        print(f"[streams] {op.name}: submitted in {(time.perf_counter() - t0) * 1e3:.1f} ms of host time, gate {'open' if gate.opened else 'shut'}")
        if not exempt:
            assert not gate.opened, f"{op.name} ({op.c_name or 'hefx_' + op.name}) waited on the host: its stream was still shut"
    w.e.sync(S.handle)
    assert gate.opened
    for op in ops:
        op.check()


# ------------------------------------------------------------------------------------------------------------------
# element-wise entries and table users, one gate per group
# ------------------------------------------------------------------------------------------------------------------
def test_basic_arithmetic(w):
    o, e, L = w.o, w.e, w.L
    a, b, da, db, p, dp = w.ct(), w.ct(), w.ct(), w.ct(), w.pt(), w.pt()
    ops = [
        Op(w, "add", [a, b], [da, db], [o.add(a, b)], [o.add(da, db)], lambda i, t, s: e.add(L, 2, i[0], i[1], out=t[0], stream=s)),
        Op(w, "sub", [a, b], [da, db], [o.sub(a, b)], [o.sub(da, db)], lambda i, t, s: e.sub(L, 2, i[0], i[1], out=t[0], stream=s)),
        Op(w, "negate", [a], [da], [o.negate(a)], [o.negate(da)], lambda i, t, s: e.negate(L, 2, i[0], out=t[0], stream=s)),
        Op(w, "add_plain", [a, p], [da, dp], [o.add_plain(a, p)], [o.add_plain(da, dp)],
           lambda i, t, s: e.add_plain(L, 2, i[0], i[1], out=t[0], stream=s)),
    ]
    run_gated(w, ops)


def test_multiply_plain_and_the_transparent_flag(w):
    """the flag is set by multiply_plain on S and read and cleared by check_transparent on ITS stream argument: a product
    by zero on S, then check_transparent(S) raises (it may block: a documented blocker), a second check passes"""
    from seal_fyp_logistic_regression_amd.capi import TransparentCiphertextError
    o, e, L = w.o, w.e, w.L
    a, da, p, dp = w.ct(), w.ct(), w.pt(), w.pt()
    e.check_transparent(w.S.handle)  # (whatever earlier tests left)
    run_gated(w, [Op(w, "multiply_plain", [a, p], [da, dp], [o.multiply_plain(a, p)], [o.multiply_plain(da, dp)],
                     lambda i, t, s: e.multiply_plain(L, 2, i[0], i[1], out=t[0], stream=s))])
    e.check_transparent(w.S.handle)  # a non-zero product leaves the flag down
    zero = np.zeros_like(p)
    op = Op(w, "multiply_plain by zero", [a, zero], [da, dp], [o.multiply_plain(a, zero)], [o.multiply_plain(da, dp)],
            lambda i, t, s: e.multiply_plain(L, 2, i[0], i[1], out=t[0], stream=s))
    gate = w.S.gate()
    op.submit(w.S.handle)
    assert not gate.opened
    with pytest.raises(TransparentCiphertextError):
        e.check_transparent(w.S.handle)
    assert gate.opened  # it waited for S: the product ran before the flag was read
    e.check_transparent(w.S.handle)
    e.sync(w.S.handle)
    op.check()


def test_products_and_level_changes(w):
    o, e, L = w.o, w.e, w.L
    a, b, da, db = w.ct(), w.ct(), w.ct(), w.ct()
    ops = [
        Op(w, "multiply", [a, b], [da, db], [o.multiply(a, b)], [o.multiply(da, db)],
           lambda i, t, s: e.multiply(L, i[0], i[1], out=t[0], stream=s)),
        Op(w, "square", [a], [da], [o.multiply(a, a)], [o.multiply(da, da)], lambda i, t, s: e.square(L, i[0], out=t[0], stream=s)),
        Op(w, "mod_drop", [a], [da], [o.mod_drop(a, 2)], [o.mod_drop(da, 2)], lambda i, t, s: e.mod_drop(L, 2, 2, i[0], out=t[0], stream=s)),
    ]
    run_gated(w, ops)


def test_rescale_in_both_divisions(w):
    """rescale_common borrows the context's scratch"""
    o, e, L = w.o, w.e, w.L
    a, da = w.ct(3), w.ct(3)
    ops = [Op(w, f"rescale_to_next_mode({r})", [a], [da], [o.rescale(a, rounded=r)], [o.rescale(da, rounded=r)],
              lambda i, t, s, r=r: e.rescale_to_next(L, 3, i[0], out=t[0], stream=s, rounded=r), c_name="hefx_rescale_to_next_mode")
           for r in (False, True)]
    r0 = e.rescale_rounded
    ops.append(Op(w, "rescale_to_next", [a], [da], [o.rescale(a, rounded=r0)], [o.rescale(da, rounded=r0)],
                  lambda i, t, s: e.rescale_to_next(L, 3, i[0], out=t[0], stream=s)))
    run_gated(w, ops)


def _sum(o, cts):
    acc = cts[0].copy()
    for c in cts[1:]:
        acc = o.add(acc, c)
    return acc


def test_sums_and_reduction(w):
    """add_many at 5 inputs (by-value pointer groups) and at 150 (device pointer table through a ring slot, partial sums in
    scratch); reduce_canonical in place"""
    o, e, L = w.o, w.e, w.L
    ops = []
    for n in (5, 150):
        a, da = w.cts(n), w.cts(n)
        ops.append(Op(w, f"add_many({n})", [a], [da], [_sum(o, list(a))], [_sum(o, list(da))],
                      lambda i, t, s, n=n: e.add_many(L, 2, views(i[0], n), out=t[0], stream=s)))
    # sums of 8 canonical residues, not yet reduced (the all-reduce's intermediate)
    parts, dparts = w.cts(8), w.cts(8)
    raw, draw = parts.sum(axis=0, dtype=np.uint64), dparts.sum(axis=0, dtype=np.uint64)
    red = lambda x: np.stack([x[:, j, :] % np.uint64(w.primes[j]) for j in range(L)], axis=1)
    assert (red(raw) == _sum(o, list(parts))).all()
    ops.append(Op(w, "reduce_canonical", [raw], [draw], [_sum(o, list(parts))], [_sum(o, list(dparts))],
                  lambda i, t, s: e.reduce_canonical(L, 2, i[0], addends=8, stream=s), inplace=[0]))
    run_gated(w, ops)


def test_batches_over_pointer_tables(w):
    o, e, L, n = w.o, w.e, w.L, 7
    a, b, da, db, p, dp = w.cts(n), w.cts(n), w.cts(n), w.cts(n), w.pts(n), w.pts(n)
    a3, da3 = w.cts(n, 3), w.cts(n, 3)
    st = lambda f, *xs: np.stack([f(*[x[i] for x in xs]) for i in range(n)])
    r0 = e.rescale_rounded
    tab = lambda f: (lambda i, t, s: f(i, views(t[0], n), s))
    ops = [
        Op(w, "add_batch", [a, b], [da, db], [st(o.add, a, b)], [st(o.add, da, db)],
           tab(lambda i, t, s: capi_batch(e, "hefx_add_batch", L, 2, views(i[0], n), views(i[1], n), t, s))),
        Op(w, "sub_batch", [a, b], [da, db], [st(o.sub, a, b)], [st(o.sub, da, db)],
           tab(lambda i, t, s: e.sub_batch(L, 2, views(i[0], n), views(i[1], n), outs=t, stream=s))),
        Op(w, "multiply_plain_batch", [a, p], [da, dp], [st(o.multiply_plain, a, p)], [st(o.multiply_plain, da, dp)],
           tab(lambda i, t, s: e.multiply_plain_batch(L, 2, views(i[0], n), views(i[1], n), outs=t, stream=s))),
        Op(w, "multiply_batch", [a, b], [da, db], [st(o.multiply, a, b)], [st(o.multiply, da, db)],
           tab(lambda i, t, s: e.multiply_batch(L, views(i[0], n), views(i[1], n), outs=t, stream=s))),
        Op(w, "rescale_to_next_batch", [a3], [da3], [st(lambda x: o.rescale(x, rounded=r0), a3)],
           [st(lambda x: o.rescale(x, rounded=r0), da3)],
           tab(lambda i, t, s: capi_batch(e, "hefx_rescale_to_next_batch", L, 3, views(i[0], n), None, t, s))),
    ]
    run_gated(w, ops)


def capi_batch(e, fn, L, size, As, Bs, outs, stream):
    """hefx_add_batch / hefx_rescale_to_next_batch with given outputs (the Engine wrappers allocate theirs)"""
    from seal_fyp_logistic_regression_amd import capi
    args = [e._h, L, size, len(As), capi.ptr_array([a.ptr for a in As])]
    if Bs is not None:
        args.append(capi.ptr_array([b.ptr for b in Bs]))
    capi.check(getattr(capi.lib(), fn)(*args, capi.ptr_array([o.ptr for o in outs]), stream))


def _ragged(n, group):
    return [list(range(g, min(n, g + group))) for g in range(0, n, group)]


def test_grouped_plain_sum_ragged(w):
    o, e, L, n, group = w.o, w.e, w.L, 11, 4  # groups of 4, 4, 3
    a, da, p, dp = w.cts(n), w.cts(n), w.pts(n), w.pts(n)
    ref = lambda c, q: np.stack([_sum(o, [o.multiply_plain(c[i], q[i]) for i in g]) for g in _ragged(n, group)])
    run_gated(w, [Op(w, "multiply_plain_sum", [a, p], [da, dp], [ref(a, p)], [ref(da, dp)],
                     lambda i, t, s: e.multiply_plain_sum(L, 2, views(i[0], n), views(i[1], n), group=group, outs=views(t[0], 3), stream=s))])


def test_grouped_ciphertext_sum_ragged_and_one_group_of_40(w):
    o, e, L = w.o, w.e, w.L
    ops = []
    for n, group in ((11, 4), (40, 40)):
        a, b, da, db = w.cts(n), w.cts(n), w.cts(n), w.cts(n)
        groups = _ragged(n, group)
        ref = lambda x, y, groups=groups: np.stack([_sum(o, [o.multiply(x[i], y[i]) for i in g]) for g in groups])
        ops.append(Op(w, f"multiply_sum({n}, group {group})", [a, b], [da, db], [ref(a, b)], [ref(da, db)],
                      lambda i, t, s, n=n, group=group, ng=len(groups): e.multiply_sum(
                          L, views(i[0], n), views(i[1], n), group=group, outs=views(t[0], ng), stream=s), c_name="hefx_multiply_sum"))
    run_gated(w, ops)


def test_transforms_in_place(w):
    """no separate output: (1) stages, (3) snapshots, (4) overwrites with the decoy after the snapshot"""
    o, e, L = w.o, w.e, w.L
    a, da = w.ct(), w.ct()
    fwd = lambda x: np.stack([np.stack([o.ntt_fwd(j, x[p, j]) for j in range(L)]) for p in range(2)])
    inv = lambda x: np.stack([np.stack([o.ntt_inv(j, x[p, j]) for j in range(L)]) for p in range(2)])
    run_gated(w, [Op(w, "ntt_forward", [a], [da], [fwd(a)], [fwd(da)], lambda i, t, s: e.ntt_forward(i[0], 2, L, stream=s), inplace=[0]),
                  Op(w, "ntt_inverse", [a], [da], [inv(a)], [inv(da)], lambda i, t, s: e.ntt_inverse(i[0], 2, L, stream=s), inplace=[0])])


# ------------------------------------------------------------------------------------------------------------------
# key switch
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(w):
    """A[i] / B[i]: the real and the decoy ciphertext of item i, accumulators, plaintexts -- and the oracle's rotations,
    computed once and shared by every key-switch case"""
    n = 40
    p = dict(A=w.cts(n), B=w.cts(n), accA=w.cts(n), accB=w.cts(n), ptA=w.pts(n), ptB=w.pts(n))
    p["rot"] = lambda i: w.rot(("A", i), p["A"][i], w.elts[i], w.ki[i])
    p["rotB0"] = lambda: w.rot(("B", 0), p["B"][0], w.elts[0], w.ki[0])
    return p


def _ks_ops(w, pool, n):
    """apply_galois_batch, rotate_multiply_plain_batch, apply_galois_add_batch over items 0..n-1 (and the single-item
    entries at n = 1)"""
    o, e, L = w.o, w.e, w.L
    A, B, accA, accB, ptA, ptB = (pool[k][:n] for k in ("A", "B", "accA", "accB", "ptA", "ptB"))
    elts, keys = w.elts[:n], [w.dkeys[j] for j in w.ki[:n]]
    rots = np.stack([pool["rot"](i) for i in range(n)])
    rotB0 = pool["rotB0"]()
    first = lambda x: {0: x}
    ops = [
        Op(w, f"apply_galois_batch({n})", [A], [B], [rots], [first(rotB0)],
           lambda i, t, s: e.apply_galois_batch(L, views(i[0], n), elts, keys, outs=views(t[0], n), stream=s)),
        Op(w, f"rotate_multiply_plain_batch({n})", [A, ptA], [B, ptB], [np.stack([o.multiply_plain(rots[i], ptA[i]) for i in range(n)])],
           [first(o.multiply_plain(rotB0, ptB[0]))],
           lambda i, t, s: e.rotate_multiply_plain_batch(L, views(i[0], n), elts, keys, views(i[1], n), outs=views(t[0], n), stream=s)),
        Op(w, f"apply_galois_add_batch({n})", [A, accA], [B, accB], [rots, np.stack([o.add(accA[i], rots[i]) for i in range(n)])],
           [first(rotB0), first(o.add(accB[0], rotB0))],
           lambda i, t, s: e.apply_galois_add_batch(L, views(i[0], n), elts, keys, views(i[1], n), outs=views(t[0], n),
                                                    acc_outs=views(t[1], n), stream=s)),
    ]
    if n == 1:
        ops.append(Op(w, "apply_galois", [A[0]], [B[0]], [rots[0]], [rotB0],
                      lambda i, t, s: e.apply_galois(L, i[0], elts[0], keys[0], out=t[0], stream=s)))
        # the in-place rotation (c_in == c_out: the kernels read a scratch copy)
        ops.append(Op(w, "apply_galois in place", [A[0]], [B[0]], [rots[0]], [rotB0],
                      lambda i, t, s: e.apply_galois(L, i[0], elts[0], keys[0], out=i[0], stream=s), inplace=[0], c_name="hefx_apply_galois"))
        a3, b3, rk = w.ct(3), w.ct(3), w.keys[0]
        ops.append(Op(w, "relinearize", [a3], [b3], [o.relinearize(a3, rk)], [o.relinearize(b3, rk)],
                      lambda i, t, s: e.relinearize(L, i[0], w.dkeys[0], out=t[0], stream=s)))
    return ops


@pytest.mark.parametrize("n", [1, 8, 40])
def test_key_switch_batches(w, pool, n):
    """n = 1: the pair path (descriptors in the kernel arguments); 8: the small path; 40: a regular chunk, descriptors
    through a ring slot.  Distinct sources, so nothing is hoisted: no first use, nothing may wait."""
    before = w.e.ks_stats()
    run_gated(w, _ks_ops(w, pool, n))
    assert w.e.ks_stats()["hoisted"] == before["hoisted"]


def test_rotate_hoisted_batch_twice_then_a_one_source_batch(w, pool):
    """40 rotations of ONE source.  The first use of their elements builds the flip-mask tables and may wait on the host (the
    documented exemption); the second call must not.  Then the same batch through hefx_apply_galois_batch, which hoists by
    itself (ks_stats) and finds the tables."""
    o, e, L, n = w.o, w.e, w.L, 40
    src, dsrc = pool["A"][0], pool["B"][0]
    elts, kis = w.elts[100:100 + n], w.ki[100:100 + n]
    keys = [w.dkeys[j] for j in kis]
    rots = np.stack([w.rot(("H", i), src, elts[i], kis[i]) for i in range(n)])
    decoy = {0: w.rot(("HB", 0), dsrc, elts[0], kis[0])}
    mk = lambda name: Op(w, name, [src], [dsrc], [rots], [decoy],
                         lambda i, t, s: e.rotate_hoisted_batch(L, i[0], elts, keys, outs=views(t[0], n), stream=s),
                         out_shapes=[rots.shape], c_name="hefx_rotate_hoisted_batch")
    assert "hefx_rotate_hoisted_batch" in FIRST_USE_ONLY
    run_gated(w, [mk("rotate_hoisted_batch, first use")], exempt=True)
    run_gated(w, [mk("rotate_hoisted_batch, second use")])
    before = e.ks_stats()
    srcs, dsrcs = np.stack([src] * 1), np.stack([dsrc] * 1)
    run_gated(w, [Op(w, "apply_galois_batch of one source", [srcs], [dsrcs], [rots], [decoy],
                     lambda i, t, s: e.apply_galois_batch(L, [i[0]] * n, elts, keys, outs=views(t[0], n), stream=s),
                     out_shapes=[rots.shape], c_name="hefx_apply_galois_batch")])
    after = e.ks_stats()
    assert after["hoisted"] - before["hoisted"] == n and e.ks_fallback_count() == 0


def test_a_batch_split_over_the_internal_streams(w):
    """600 items at C2 are two chunks (512 + 88): ks_run forks its two internal streams from S and joins them back.  The
    fork is what (1) checks -- a chunk that ran ahead would read decoys -- and the join is what (4) checks.  Sampled items
    against the oracle: both ends of both chunks (items are processed grouped by key, so every index matters equally).
    What the first call of such a batch costs the HOST -- 560 gather tables built and uploaded, a scratch buffer of 1.7 GB
    from hipMalloc: a quarter of a second and more on a loaded machine, none of it a wait for the stream -- is spent by one
    ungated call on the default stream (decoys in, the snapshot buffer out); scratch growth behind a gate is the subject of
    test_a_fresh_context_grows_its_scratch_behind_the_gate."""
    import time
    o, e, L, n = w.o, w.e, w.L, 600
    A, B = w.cts(n), w.cts(n)
    elts, kis = w.elts[:n], w.ki[:n]
    keys = [w.dkeys[j] for j in kis]
    rng = np.random.default_rng(7)
    idx = sorted({0, 1, 87, 88, 299, 511, 512, 513, 598, 599} | set(int(x) for x in rng.integers(0, n, 6)))
    want = {i: o.apply_galois(A[i], elts[i], w.keys[kis[i]]) for i in idx}
    decoy = {0: o.apply_galois(B[0], elts[0], w.keys[kis[0]])}
    op = Op(w, "apply_galois_batch(600)", [A], [B], [want], [decoy],
            lambda i, t, s: e.apply_galois_batch(L, views(i[0], n), elts, keys, outs=views(t[0], n), stream=s),
            out_shapes=[A.shape], c_name="hefx_apply_galois_batch")
    t0 = time.perf_counter()
    e.apply_galois_batch(L, views(op.ins[0], n), elts, keys, outs=views(op.snaps[0], n))
    print(f"[streams] first call of the 600-item batch, default stream: {(time.perf_counter() - t0) * 1e3:.1f} ms of host time")
    e.sync()
    before = e.ks_stats()
    run_gated(w, [op])
    after = e.ks_stats()
    assert after["chunks"] - before["chunks"] >= 2 and after["calls"] - before["calls"] == 1


# ------------------------------------------------------------------------------------------------------------------
# chains and forests
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 24, 40])
def test_rotate_add_chain(w, n):
    """steps = 4; n = 8: one lane (S alone), 24: three lanes (S and both internal streams, forked and joined), 40: the wide
    path (a regular batch per level).  Chains are checked at both ends of every lane."""
    o, e, L, steps = w.o, w.e, w.L, 4
    A, B, accA, accB = w.cts(n), w.cts(n), w.cts(n), w.cts(n)
    elts, kis = w.elts[200:200 + n], w.ki[200:200 + n]
    keys = [w.dkeys[j] for j in kis]

    def chain(ct, acc, i):
        for _ in range(steps):
            ct = o.apply_galois(ct, elts[i], w.keys[kis[i]])
            acc = o.add(acc, ct)
        return ct, acc

    idx = sorted({0, n // 3 - 1, n // 3, 2 * n // 3 - 1, 2 * n // 3, n - 1} | ({1, 2, 3, 4, 5, 6} if n == 8 else set()))
    got = {i: chain(A[i], accA[i], i) for i in idx}
    d0 = chain(B[0], accB[0], 0)
    run_gated(w, [Op(w, f"rotate_add_chain({n})", [A, accA], [B, accB], [{i: g[0] for i, g in got.items()}, {i: g[1] for i, g in got.items()}],
                     [{0: d0[0]}, {0: d0[1]}],
                     lambda i, t, s: e.rotate_add_chain(L, views(i[0], n), elts, keys, views(i[1], n), steps, outs=views(t[0], n),
                                                        acc_outs=views(t[1], n), stream=s),
                     out_shapes=[A.shape, A.shape])])


def test_apply_galois_forest_on_two_lanes():
    """the 156-node forest of test_apply_galois_forest_bit_exact_vs_node_by_node (N = 4096): above the 96-node bound, so the
    subtrees run on two lanes -- S and an internal stream, forked after (1) and joined before (3)"""
    from oracle import oracle as O
    N, primes = 4096, O.coeff_modulus_create(4096, [50, 30, 30, 50])
    w = World(N, primes, L=len(primes) - 1)
    try:
        o, e, L = w.o, w.e, w.L
        steps = [1, -1, 2, -2, 4, 8]
        elt_of = {s: O.galois_elt_from_step(N, s) for s in steps}
        keys = {s: w.key(40 + i) for i, s in enumerate(steps)}
        dkeys = {s: e.to_device(k) for s, k in keys.items()}
        nroots, fan, depth = 12, 3, 3
        rng = np.random.default_rng(nroots * 100 + fan)
        parents, step_of, src_of, level = [], [], [], []
        for r in range(nroots):
            parents.append(-1), step_of.append(steps[r % len(steps)]), src_of.append(r % 2), level.append(len(parents) - 1)
        for _ in range(depth - 1):
            nxt = []
            for p in level:
                for f in range(fan):
                    parents.append(p), step_of.append(steps[int(rng.integers(len(steps)))]), src_of.append(None), nxt.append(len(parents) - 1)
            level = nxt
        n = len(parents)
        assert n == 156
        has_pt = [i % 3 == 1 for i in range(n)]
        srcs, dsrcs, pts, dpts = w.cts(2), w.cts(2), w.pts(n), w.pts(n)

        def ref(src, pt, only=None):
            want = {}
            for i in range(n) if only is None else only:
                x = src[src_of[i]] if parents[i] < 0 else want[parents[i]]
                s = step_of[i]
                want[i] = o.rotate_mulplain(x, elt_of[s], keys[s], pt[i]) if has_pt[i] else o.apply_galois(x, elt_of[s], keys[s])
            return want

        want, decoy = ref(srcs, pts), ref(dsrcs, dpts, only=[1])
        call = lambda i, t, s: e.apply_galois_forest(
            L, parents, [views(i[0], 2)[x] if x is not None else None for x in src_of], [elt_of[x] for x in step_of],
            [dkeys[x] for x in step_of], [p if has_pt[j] else None for j, p in enumerate(views(i[1], n))], outs=views(t[0], n), stream=s)
        # the first use of the six elements may build flip-mask tables (a wide one-source depth hoists): once ungated
        warm = Op(w, "apply_galois_forest, first use", [srcs, pts], [dsrcs, dpts], [want], [decoy], call, out_shapes=[(n, 2, L, N)],
                  c_name="hefx_apply_galois_forest")
        run_gated(w, [warm], exempt=True)
        run_gated(w, [Op(w, "apply_galois_forest", [srcs, pts], [dsrcs, dpts], [want], [decoy], call, out_shapes=[(n, 2, L, N)])])
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------------------------
# linear transforms at d = 16, C2
# ------------------------------------------------------------------------------------------------------------------
D = 16


@pytest.fixture(scope="module")
def lt(w):
    """Galois keys (uniform words: the arithmetic is the same) -- the default set (3^(+-2^i), 2N-1: rotations are NAF chains)
    and a direct key for every step the hoisted / baby-step forms need; operands and their decoys"""
    o, O, N = w.o, w.O, w.N
    default = o.default_galois_elts()
    direct = sorted({O.galois_elt_from_step(N, s) for s in [-D] + list(range(1, D))})
    hk = {elt: w.key(5000 + elt) for elt in sorted(set(default) | set(direct))}
    dk = {elt: w.e.to_device(k) for elt, k in hk.items()}
    sel = lambda elts: (elts, {x: hk[x] for x in elts}, [dk[x] for x in elts])
    return dict(naf=sel(default), direct=sel(direct), ct=w.ct(), ctB=w.ct(), ct2=w.ct(), ct2B=w.ct(),
                diag=w.pts(2 * D), diagB=w.pts(2 * D), cdiag=w.cts(D), cdiagB=w.cts(D),
                kdiag=w.pts(D, L=w.k), kdiagB=w.pts(D, L=w.k))


def _ct_new(o, ct, gk):
    return o.add(ct, o.rotate_vector(ct, -D, gk))


def _lt_plain(o, ct, diag, gk):
    """helper.h:237-262 op by op"""
    cn = _ct_new(o, ct, gk)
    return _sum(o, [o.multiply_plain(cn, diag[0])] + [o.multiply_plain(o.rotate_vector(cn, l, gk), diag[l]) for l in range(1, D)])


def test_linear_transform_plain_and_many(w, lt):
    o, e, L = w.o, w.e, w.L
    elts, gk, dks = lt["naf"]
    d1, d1B = lt["diag"][:D], lt["diagB"][:D]
    a = _lt_plain(o, lt["ct"], d1, gk)
    b = _lt_plain(o, lt["ct2"], lt["diag"][D:], gk)
    aB = _lt_plain(o, lt["ctB"], d1B, gk)
    two, twoB = np.stack([lt["ct"], lt["ct2"]]), np.stack([lt["ctB"], lt["ct2B"]])
    ops = [
        Op(w, "linear_transform_plain", [lt["ct"], d1], [lt["ctB"], d1B], [a], [aB],
           lambda i, t, s: e.linear_transform_plain(L, i[0], views(i[1], D), elts, dks, out=t[0], stream=s)),
        Op(w, "linear_transform_plain_many", [two, lt["diag"]], [twoB, lt["diagB"]], [np.stack([a, b])], [{0: aB}],
           lambda i, t, s: e.linear_transform_plain_many(L, views(i[0], 2), views(i[1], 2 * D), elts, dks, outs=views(t[0], 2), stream=s)),
    ]
    run_gated(w, ops)


def test_linear_transform_cipher(w, lt):
    """the forest without fused products, then one hefx_multiply_sum over (ct_new, rotations) x diagonals"""
    o, e, L = w.o, w.e, w.L
    elts, gk, dks = lt["naf"]

    def ref(ct, cd):
        cn = _ct_new(o, ct, gk)
        return _sum(o, [o.multiply(cn, cd[0])] + [o.multiply(o.rotate_vector(cn, l, gk), cd[l]) for l in range(1, D)])

    run_gated(w, [Op(w, "linear_transform_cipher", [lt["ct"], lt["cdiag"]], [lt["ctB"], lt["cdiagB"]], [ref(lt["ct"], lt["cdiag"])],
                     [ref(lt["ctB"], lt["cdiagB"])],
                     lambda i, t, s: e.linear_transform_cipher(L, i[0], views(i[1], D), elts, dks, out=t[0], stream=s))])


def test_linear_transform_plain_hoisted(w, lt):
    """direct keys (the entry refuses NAF chains); 15 rotations of ct_new: the latency path, same words"""
    o, e, L = w.o, w.e, w.L
    elts, gk, dks = lt["direct"]
    d1, d1B = lt["diag"][:D], lt["diagB"][:D]
    run_gated(w, [Op(w, "linear_transform_plain_hoisted", [lt["ct"], d1], [lt["ctB"], d1B], [_lt_plain(o, lt["ct"], d1, gk)],
                     [_lt_plain(o, lt["ctB"], d1B, gk)],
                     lambda i, t, s: e.linear_transform_plain(L, i[0], views(i[1], D), elts, dks, out=t[0], stream=s, hoisted=True))])


def test_linear_transform_plain_hoisted2_sparse(w, lt):
    """the double-hoisted transform over a subset of the diagonals, against the oracle's statement of that algorithm; its
    descriptors travel through a ring slot since this module exists -- it used to wait for the stream on every call"""
    o, e, L, O, N = w.o, w.e, w.L, w.O, w.N
    assert L == w.k - 1
    elts, gk, dks = lt["direct"]
    steps = [0, 1, 3, 4, 9, 15]
    kd, kdB = lt["kdiag"][:len(steps)], lt["kdiagB"][:len(steps)]
    selts = [O.galois_elt_from_step(N, s) for s in steps[1:]]
    ref = lambda ct, dg: o.lt_double_hoisted_core(_ct_new(o, ct, gk), list(dg), selts, [gk[x] for x in selts])
    assert "hefx_linear_transform_plain_hoisted2_sparse" not in HOST_BLOCKING
    run_gated(w, [Op(w, "linear_transform_plain_hoisted2_sparse", [lt["ct"], kd], [lt["ctB"], kdB], [ref(lt["ct"], kd)], [ref(lt["ctB"], kdB)],
                     lambda i, t, s: e.linear_transform_plain_hoisted2_sparse(L, i[0], D, steps, views(i[1], len(steps)), elts, dks,
                                                                              out=t[0], stream=s))])


def test_linear_transform_plain_bsgs(w, lt):
    """n1 = 4: baby steps 1..3 (one batch), inner sums (hefx_multiply_plain_sum), giant steps 4, 8, 12, add_many"""
    o, e, L = w.o, w.e, w.L
    elts, gk, dks = lt["direct"]
    n1, n2 = 4, 4
    d1, d1B = lt["diag"][:D], lt["diagB"][:D]

    def ref(ct, dg):
        cn = _ct_new(o, ct, gk)
        rots = [cn] + [o.rotate_vector(cn, i, gk) for i in range(1, n1)]
        inner = [_sum(o, [o.multiply_plain(rots[i], dg[j * n1 + i]) for i in range(n1)]) for j in range(n2)]
        return _sum(o, inner[:1] + [o.rotate_vector(inner[j], j * n1, gk) for j in range(1, n2)])

    run_gated(w, [Op(w, "linear_transform_plain_bsgs", [lt["ct"], d1], [lt["ctB"], d1B], [ref(lt["ct"], d1)], [ref(lt["ctB"], d1B)],
                     lambda i, t, s: e.linear_transform_plain_bsgs(L, i[0], views(i[1], D), n1, elts, dks, hoisted=True, out=t[0], stream=s))])


# ------------------------------------------------------------------------------------------------------------------
# front end
# ------------------------------------------------------------------------------------------------------------------
def test_front_end(w):
    """encode (host arrays overwritten right after the call returns, the gate still shut), encrypt, encrypt_batch, sampling,
    decrypt behind one gate; decode, which blocks, last"""
    from seal_fyp_logistic_regression_amd import capi
    from tests.oracle_backend import OracleBackend
    o, e, L, N = w.o, w.e, w.L, w.N
    ob = OracleBackend(N, w.primes)
    key32, scale = bytes(range(7, 39)), 2.0 ** 30
    S = w.S.handle
    # constant slot vectors encode to constant polynomials: exact in floating point, so the oracle's words are the engine's
    vals = [3.0, -7.0, 11.0, 0.5]
    want_pt = [o.encode(L, np.full(N // 2, v), scale) for v in vals]
    assert (want_pt[0] != o.encode(L, np.full(N // 2, 99.0), scale)).any()
    one = np.full(N // 2, vals[0])
    many = np.stack([np.full(N // 2, v) for v in vals[1:]])
    d_one, d_many = e.to_device(w.junk((1, L, N))), e.to_device(w.junk((3, L, N)))
    e.ckks_encode(L, one, scale)  # (the encoder's tables: first use, on the default stream)
    # encrypt / decrypt operands
    pk, pkB = w.junk((2, w.k, N)), w.junk((2, w.k, N))
    plains, plainsB = w.pts(6), w.pts(6)
    sk, skB = w.junk((w.k, N)), w.junk((w.k, N))
    ct, ctB = w.ct(), w.ct()
    enc = lambda pk_, pl, sid: ob.encrypt(L, pk_, pl, key32, sid)
    ops = [
        Op(w, "encrypt", [pk, plains[0]], [pkB, plainsB[0]], [enc(pk, plains[0], 77)], [enc(pkB, plainsB[0], 77)],
           lambda i, t, s: e.encrypt(L, i[0], i[1], key32, 77, out=t[0], stream=s)),
        Op(w, "encrypt_batch", [pk, plains[1:]], [pkB, plainsB[1:]], [np.stack([enc(pk, plains[1 + j], 200 + j) for j in range(5)])],
           [{0: enc(pkB, plainsB[1], 200)}],
           lambda i, t, s: e.encrypt_batch(L, i[0], views(i[1], 5), key32, 200, outs=views(t[0], 5), stream=s)),
        Op(w, "decrypt", [ct, sk], [ctB, skB], [ob.decrypt(L, 2, ct, sk)], [ob.decrypt(L, 2, ctB, skB)],
           lambda i, t, s: e.decrypt(L, 2, i[0], i[1], out=t[0], stream=s)),
    ]
    d_smp = e.to_device(w.junk((2, L, N)))
    want_smp = o.sample("uniform", key32, 5, 2, L, 0)
    gate = w.S.gate()
    capi.check(capi.lib().hefx_ckks_encode(e._h, L, one.ctypes.data, None, N // 2, 1, scale, d_one.ptr, S))
    one[:] = 99.0
    assert not gate.opened, "hefx_ckks_encode waited for the stream"
    capi.check(capi.lib().hefx_ckks_encode_batch(e._h, L, many.ctypes.data, None, N // 2, 3, scale,
                                                 capi.ptr_array([v.ptr for v in views(d_many, 3)]), S))
    many[:] = 99.0
    assert not gate.opened, "hefx_ckks_encode_batch waited for the stream"
    e.sample("uniform", key32, 5, 2, L, 0, out=d_smp, stream=S)
    assert not gate.opened, "hefx_sample_uniform waited for the stream"
    for op in ops:
        op.submit(S)
        assert not gate.opened, op.name
    e.sync(S)
    assert gate.opened
    assert (d_one.download()[0] == want_pt[0]).all(), "ckks_encode: not the values the host array held at the call"
    for j in range(3):
        assert (d_many.download()[j] == want_pt[1 + j]).all(), ("ckks_encode_batch", j)
    assert (d_smp.download() == want_smp).all()
    for op in ops:
        op.check()
    # decode blocks: last.  Its values are those of the default-stream call (held to the exact reference elsewhere)
    dpt = e.to_device(np.stack(want_pt))
    gate = w.S.gate()
    got = e.ckks_decode(L, dpt, scale, count=4, stream=S)
    assert gate.opened and (got == e.ckks_decode(L, dpt, scale, count=4)).all()
    assert np.abs(got[:, 0].real - np.array(vals)).max() < 1e-6


# ------------------------------------------------------------------------------------------------------------------
# scratch growth, pool, two streams, N = 32768, and the default stream afterwards
# ------------------------------------------------------------------------------------------------------------------
def test_a_fresh_context_grows_its_scratch_behind_the_gate():
    """a new engine has no scratch: batches of 3, 20, 70 and 300 rotations behind ONE gate, no sync in between -- the buffer
    is outgrown and retired three times while the work that uses the old ones has not even started.  The gather tables of
    the 300 elements are built beforehand (hefx_galois_permute: no scratch involved), so that what the host does behind the
    gate is the scratch's hipMalloc calls and the submissions; the gate stays shut for a second, since those allocations
    (64 MiB to half a gigabyte) take their time on a loaded machine without waiting for any stream."""
    w = World(*C2, L=3)
    try:
        o, e, L = w.o, w.e, w.L
        row, tmp = e.to_device(w.junk((1, w.N))), e.empty(1, w.N)
        for elt in sorted(set(w.elts[:300])):
            e.galois_permute(elt, row, 1, out=tmp)
        e.sync()
        ops = []
        for n in (3, 20, 70, 300):
            A, B = w.cts(n), w.cts(n)
            elts, kis = w.elts[:n], w.ki[:n]
            idx = sorted({0, n - 1, n // 2})
            ops.append(Op(w, f"apply_galois_batch({n})", [A], [B], [{i: o.apply_galois(A[i], elts[i], w.keys[kis[i]]) for i in idx}],
                          [{0: o.apply_galois(B[0], elts[0], w.keys[kis[0]])}],
                          lambda i, t, s, n=n, elts=elts, kis=kis: e.apply_galois_batch(
                              L, views(i[0], n), elts, [w.dkeys[j] for j in kis], outs=views(t[0], n), stream=s),
                          out_shapes=[A.shape], c_name="hefx_apply_galois_batch"))
        run_gated(w, ops, hold=1.0)
    finally:
        w.close()


def test_pool_recycles_a_block_in_stream_order(w):
    """hefx_free parks a block without synchronising and the next hefx_malloc of the size hands it out again: op A into a
    fresh block, free, malloc (the same address), op B into it -- all behind the gate.  The snapshot taken between the two
    holds A's result, the block B's: the contract is stream order"""
    from seal_fyp_logistic_regression_amd.engine import DeviceArray
    o, e, L, S = w.o, w.e, w.L, w.S.handle
    a, b, c, d = (e.to_device(x) for x in (w.ct(), w.ct(), w.ct(), w.ct()))
    ha, hb, hc, hd = (x.download() for x in (a, b, c, d))
    snap = e.empty(2, L, w.N)
    blk = DeviceArray(e, (2, L, w.N))
    addr = blk.ptr
    gate = w.S.gate()
    e.add(L, 2, a, b, out=blk, stream=S)
    e.copy_raw(snap.ptr, blk.ptr, blk.nbytes, S)
    blk.free()
    blk2 = DeviceArray(e, (2, L, w.N))
    assert blk2.ptr == addr, "the pool did not hand the parked block out again"
    e.sub(L, 2, c, d, out=blk2, stream=S)
    assert not gate.opened, "hefx_malloc / hefx_free waited for the stream"
    e.sync(S)
    want_a, want_b = o.add(ha, hb), o.sub(hc, hd)
    assert (want_a != want_b).any()
    assert (snap.download() == want_a).all() and (blk2.download() == want_b).all()


def test_two_streams_ordered_by_the_caller(w, pool):
    """the contract case of hefx_malloc's comment and of the two-stream rule: the producer on S1 (gated), an event recorded
    on S1, S2 made to wait for it (hipStreamWaitEvent), the consumer -- a key-switch batch -- on S2"""
    from tests.hip_stream_gate import Stream
    o, e, L, n = w.o, w.e, w.L, 8
    A, B = pool["A"][:n], pool["B"][:n]
    elts, keys = w.elts[:n], [w.dkeys[j] for j in w.ki[:n]]
    x = w.cts(n)
    # producer: d_in = x + (A - x) = A, computed on S1 from staged operands; consumer rotates d_in on S2
    delta = np.stack([o.sub(A[i], x[i]) for i in range(n)])
    dx, ddelta = e.to_device(x), e.to_device(delta)
    d_in, d_out = e.to_device(B), e.to_device(w.junk((n, 2, L, w.N)))
    want = np.stack([pool["rot"](i) for i in range(n)])
    assert (want[0] != pool["rotB0"]()).any()
    ev = e.event()
    with Stream() as S2:
        gate = w.S.gate()
        e.add(L, 2, dx, ddelta, out=d_in, count=n, stream=w.S.handle)
        e.event_record(ev, w.S.handle)
        S2.wait_event(ev)
        e.apply_galois_batch(L, views(d_in, n), elts, keys, outs=views(d_out, n), stream=S2.handle)
        assert not gate.opened
        e.sync(S2.handle)
        assert gate.opened, "S2 did not wait for the producer's event"
        assert (d_out.download() == want).all()
        e.sync(w.S.handle)
    e.event_destroy(ev)


def test_flip_mask_builder_borrows_the_scratch_at_32768():
    """N = 32768: the flip-mask tables' transform is out of place THROUGH the context's scratch buffer, on the caller's
    stream, in front of a batch whose chunks use the same buffer.  34 rotations of one source (the smallest batch that
    hoists) on a fresh context; first use, so the call may wait on the host -- the words must be the oracle's"""
    N, primes = C5
    w = World(N, primes, L=2)
    try:
        o, e, L, n = w.o, w.e, w.L, 34
        src, dsrc = w.ct(), w.ct()
        elts, kis = w.elts[:n], w.ki[:n]
        idx = [0, 16, 33]
        want = {i: o.apply_galois(src, elts[i], w.keys[kis[i]]) for i in idx}
        decoy = {0: o.apply_galois(dsrc, elts[0], w.keys[kis[0]])}
        before = e.ks_stats()
        run_gated(w, [Op(w, "rotate_hoisted_batch at N = 32768", [src], [dsrc], [want], [decoy],
                         lambda i, t, s: e.rotate_hoisted_batch(L, i[0], elts, [w.dkeys[j] for j in kis], outs=views(t[0], n), stream=s),
                         out_shapes=[(n, 2, L, N)], c_name="hefx_rotate_hoisted_batch")], exempt=True)
        assert e.ks_stats()["hoisted"] - before["hoisted"] == n and e.ks_fallback_count() == 0
    finally:
        w.close()


def test_default_stream_after_the_foreign_streams(w, pool):
    """after everything above: a default-stream batch on the same context still gives the oracle's words -- no ring slot or
    event was left in a bad state by the caller-owned streams"""
    e, L, n = w.e, w.L, 40
    e.sync(w.S.handle)
    outs = e.apply_galois_batch(L, [e.to_device(pool["A"][i]) for i in range(n)], w.elts[:n], [w.dkeys[j] for j in w.ki[:n]])
    for i in range(n):
        assert (outs[i].download() == pool["rot"](i)).all(), i
