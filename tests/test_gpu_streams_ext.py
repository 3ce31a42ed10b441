"""The stream-taking entries of the EXTENSION headers on a CALLER-OWNED stream, under the decoy protocol of
tests/test_gpu_streams.py (class Op, run_gated: operands staged behind a gate, outputs snapshotted behind the call, decoys
restored behind the snapshot): hefx_hybrid.h, hefx_hybrid_hoist.h, hefx_hybrid_bsgs.h, hefx_refresh.h, hefx_encaps.h.  The
`..._return_while_their_stream_is_held_shut` tests of the entries' own modules prove that the host did not wait; with every
operand in place before the gate they cannot see a launch or a descriptor copy on the wrong stream, nor an entry that is still
reading behind its place in the stream.  These can.  Cases, references and the coverage table: tests/stream_ext_cases.py, held to
non-vacuity and to the engine's thresholds without a GPU by tests/test_stream_ext_cpu.py.

Single entries are held to `not gate.opened`.  The sequences put several calls behind one gate: a wrap of the descriptor ring
(exempt: call 33 waits for slot 0, as the headers allow), scratch growth that retires the buffer a queued call still uses, the
scratch shared with a hefx_apply_galois_batch forked onto the internal streams, a 1030-item call of two chunks, and two streams
ordered by the caller with an event.

Shown to detect, once, on two planted defects built outside the tree, each ONE transform(...) launch moved to stream 0 -- the
forward transform of the converted data rows (ext), which dereferences nothing from the call's table: wrong words, no wrong
address.  Both runs failed by mismatch (the snapshot of the first op checked), nothing else:
  1. in hybrid_run: 4 of the 10 tests -- test_the_hybrid_entries_at_two_digits_the_last_one_partial (the three-item Galois
     batch), test_scratch_growth_behind_the_gate_retires_a_buffer_in_use (the one-item call), test_the_scratch_shared_with_a_
     batch_forked_onto_the_internal_streams (the hybrid batch) and test_two_streams_ordered_by_the_caller.  The cases at L = 1
     (two chunks, the ring) and at `big` (alpha = 2, L = 2) passed, and rightly: with ONE digit every data row is the digit's
     own, its word is the input's and the result of that transform is never read (hefx_hybrid.h, step 3).
  2. in hybrid_hoist_run: test_the_hybrid_entries_at_two_digits_the_last_one_partial, at hefx_hybrid_rotate_hoisted_batch (the
     first hoisted op; the check stops there).  `big` passed for the reason above; no other test runs that function."""
import time

import numpy as np
import pytest

from tests import hybrid_cases as HC
from tests import stream_ext_cases as SX

pytestmark = pytest.mark.gpu


class ExtWorld:
    """what test_gpu_streams.Op asks of a world: .e, .S, .junk(shape), .seed() -- one engine over a prime list, one caller-owned
    stream"""

    def __init__(self, N, primes):
        from seal_fyp_logistic_regression_amd import Engine
        from tests.hip_stream_gate import Stream
        self.e, self.N, self.primes = Engine(N, [int(p) for p in primes]), N, [int(p) for p in primes]
        self.S = Stream()
        self._seed = 40_000
        self._floor = min(self.primes)

    def seed(self):
        self._seed += 1
        return self._seed

    def junk(self, shape):
        """an output's decoy filling: words below the smallest prime are canonical in every row"""
        return np.random.default_rng(self.seed()).integers(0, self._floor, shape, dtype=np.uint64)

    def close(self):
        self.S.destroy()
        self.e.close()


def hybrid_world(name):
    s = HC.sets()[name]
    return ExtWorld(s.N, s.primes)


@pytest.fixture(scope="module")
def w():
    world = hybrid_world(SX.SET)
    yield world
    world.close()


def op(w, case, call=None):
    from tests.test_gpu_streams import Op
    call = call or (lambda i, t, s: case.call(w.e, i, t, s))
    return Op(w, case.name, case.reals, case.decoys, case.want, case.want_decoy, call, inplace=case.inplace, out_shapes=case.out_shapes,
              c_name=case.c_name)


def gated(w, ops, **kw):
    from tests.test_gpu_streams import run_gated
    run_gated(w, ops, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# single entries: one gate per header group
# ---------------------------------------------------------------------------------------------------------------------
def test_the_hybrid_entries_at_two_digits_the_last_one_partial(w):
    """k8a3-p50_60, L = 5: three Galois items out of place on two keys, one exact in-place item, three relinearisations, the key
    generation, both hoisted entries (the identity term with a NULL key among the elements, G = 2) and the hoisted giant steps
    (G = 4, O = 2, two giant keys) -- ciphertexts, plaintexts, keys and secrets all decoyed"""
    names = ("galois_batch", "galois_in_place", "relin_batch", "keygen", "rotate_hoisted", "plain_combine_hoisted", "bsgs_hoisted")
    gated(w, [op(w, c) for name in names for c in SX.flat(name)])


def test_a_call_of_two_chunks(w):
    """1030 items at L = 1: two descriptor slots, two launch sequences through the same scratch; items 0, 1023, 1024, 1029 and
    their neighbours against the model"""
    gated(w, [op(w, SX.chunked())])


def test_the_split_transforms_at_n_32768():
    """the set `big`: one Galois item, one relinearisation, one hoisted call of one source and three elements -- every transform src != dst"""
    world = hybrid_world(SX.BIG)
    try:
        gated(world, [op(world, c) for name in ("big_galois", "big_relin", "big_rotate_hoisted") for c in SX.flat(name)])
    finally:
        world.close()


def test_mod_raise_refresh_and_refresh_batch():
    """the shapes of tests/test_gpu_refresh.py's gate test; the ciphertexts, sk and pk decoyed"""
    world = ExtWorld(SX.REFRESH_N, SX.refresh_primes())
    try:
        gated(world, [op(world, SX.mod_raise()), op(world, SX.refresh()), op(world, SX.refresh_batch())])
    finally:
        world.close()


def test_switch_key_collapse_key_and_raise_switch():
    """the shapes of tests/test_gpu_encaps.py's gate test; hefx_raise_switch reads the collapsed key that hefx_collapse_key's
    case writes on the same stream just before -- until the stream runs that buffer holds the collapse case's output decoy"""
    from tests import encaps_cases as EC
    world = ExtWorld(EC.N, SX.encaps_primes())
    try:
        collapse, rs = op(world, SX.collapse_key()), SX.raise_switch()
        ckey = collapse.outs[0]
        gated(world, [op(world, SX.switch_key()), collapse, op(world, rs, lambda i, t, s: rs.call(world.e, i, t, s, ckey))])
    finally:
        world.close()


# ---------------------------------------------------------------------------------------------------------------------
# sequences: several calls behind one gate
# ---------------------------------------------------------------------------------------------------------------------
def test_sixty_five_calls_wrap_the_descriptor_ring(w):
    """every hybrid call copies its table through one of KS_RING = 32 slots of a pinned mirror: 65 one-item calls behind one gate
    use slot 0 three times.  Call 33 must wait for call 1's slot (the headers allow a wait on a full ring): exempt.  Every call's
    snapshot and output against the model -- a slot reused before its copy had run would hand a kernel another call's table"""
    ops = [op(w, c) for c in SX.ring_wrap()]
    assert len(ops) == SX.RING_CALLS
    gated(w, ops, exempt=True)


def test_scratch_growth_behind_the_gate_retires_a_buffer_in_use():
    """a fresh context: a one-item call takes the 64 MiB floor, then a call sized from hybrid_cases.item_rows outgrows it while
    the first is still queued behind the gate.  The gate stays shut for a second: the hipMalloc of the grown buffer takes its time
    on a loaded machine without waiting for any stream (test_a_fresh_context_grows_its_scratch_behind_the_gate)"""
    world = hybrid_world(SX.SET)
    try:
        gated(world, [op(world, c) for c in SX.scratch_growth()], hold=1.0)
    finally:
        world.close()


def test_the_scratch_shared_with_a_batch_forked_onto_the_internal_streams(w):
    """on one stream: a hybrid batch, hefx_apply_galois_batch of 600 items (two chunks: ks_run forks its internal streams from S
    and joins them back, in the scratch the hybrid entries carve), hefx_hybrid_relinearize_batch, hefx_hybrid_bsgs_hoisted.  What
    the first call of the 600-item batch costs the HOST (gather tables, a larger scratch) is spent by one ungated call on the
    default stream, as test_a_batch_split_over_the_internal_streams does"""
    e = w.e
    ks = SX.ks_split()
    n, L = ks.n, ks.L
    key = e.to_device(ks.key)
    call = lambda i, t, s: e.apply_galois_batch(L, SX.parts(i[0], n), ks.elts, [key] * n, outs=SX.parts(t[0], n), stream=s)
    split = op(w, ks, call)
    t0 = time.perf_counter()
    e.apply_galois_batch(L, SX.parts(split.ins[0], n), ks.elts, [key] * n, outs=SX.parts(split.snaps[0], n))
    print(f"[streams ext] first call of the 600-item batch, default stream: {(time.perf_counter() - t0) * 1e3:.1f} ms of host time")
    e.sync()
    before = e.ks_stats()
    gated(w, [op(w, SX.galois_batch()), split, op(w, SX.relin_batch()), op(w, SX.bsgs_hoisted())])
    after = e.ks_stats()
    assert after["chunks"] - before["chunks"] >= 2 and after["calls"] - before["calls"] == 1


def test_two_streams_ordered_by_the_caller(w):
    """a hybrid call on S1 (gated, its input staged behind the gate), an event recorded on S1, S2 made to wait for it, then a
    hybrid call on S2 that reads S1's output: the two-stream rule of hefx.h (test_gpu_streams.test_two_streams_ordered_by_the_caller)"""
    from tests.hip_stream_gate import Stream
    t, e = SX.two_streams(), w.e
    s, L, N = t["s"], t["L"], t["s"].N
    assert (t["want"] != t["want_decoy"]).any()
    keys = [e.to_device(k) for k in t["K"]]
    d_in, stage = e.to_device(t["B"]), e.to_device(t["A"])
    d_mid, d_out = e.to_device(w.junk((2, L, N))), e.to_device(w.junk((2, L, N)))
    ev = e.event()
    with Stream() as S2:
        gate = w.S.gate()
        e.copy_raw(d_in.ptr, stage.ptr, stage.nbytes, w.S.handle)
        e.hybrid_apply_galois_batch(s.alpha, L, [d_in], [3], [keys[0]], outs=[d_mid], stream=w.S.handle)
        e.event_record(ev, w.S.handle)
        S2.wait_event(ev)
        e.hybrid_apply_galois_batch(s.alpha, L, [d_mid], [2 * N - 1], [keys[1]], outs=[d_out], stream=S2.handle)
        assert not gate.opened
        e.sync(S2.handle)
        assert gate.opened, "S2 did not wait for the producer's event"
        assert (d_out.download() == t["want"]).all()
        e.sync(w.S.handle)
    e.event_destroy(ev)


def test_default_stream_after_the_foreign_streams(w):
    """after everything above: a default-stream call on the same context still gives the model's words"""
    e, c = w.e, SX.galois_batch()
    e.sync(w.S.handle)
    ins, keys, out = e.to_device(c.reals[0]), e.to_device(c.reals[1]), e.to_device(w.junk(c.want[0].shape))
    c.call(e, [ins, keys], [out], None)
    assert (out.download() == c.want[0]).all()
