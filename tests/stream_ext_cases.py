"""Shared cases of tests/test_stream_ext_cpu.py and tests/test_gpu_streams_ext.py (TEST INFRASTRUCTURE): the stream-taking entries
of the EXTENSION headers (include/hefx_*.h other than hefx.h) under the decoy protocol of tests/test_gpu_streams.py.  Pure numpy
and models, no GPU: per case the real operands, the decoy operands (same shapes, other seeds) and the expected words on both,
and how the entry is called on an engine.  The coverage table at the end names, for every such entry, where it is held to
stream order.

THE REFERENCES of the expected words, none of them the engine:
    hybrid entries      the integer models of tests/hybrid_cases.py, tests/hybrid_hoist_cases.py and tests/hybrid_bsgs_cases.py
    hefx_hybrid_keygen  the key composed on the oracle twin from the header's statement (keygen_model): the twin's sampler
                        and transforms, the arithmetic in Python integers
    hefx_mod_raise      refresh_cases.lift
    hefx_refresh(_batch) the composition the header states -- decrypt, mod-raise, encrypt with the same key32 and stream id --
                        on OracleBackend.decrypt, refresh_cases.lift and OracleBackend.encrypt: every step has a reference
                        outside the engine, none comes from the engine on the default stream
    hefx_switch_key     oracle.Oracle.apply_galois with the element 1
    hefx_collapse_key, hefx_raise_switch   encaps_cases.collapse_model, encaps_cases.raise_switch_model
    hefx_apply_galois_batch (the split batch of the shared-scratch sequence)   oracle.Oracle.apply_galois

THE DECOYS.  Every buffer an entry reads is an input of its case: ciphertexts and plaintexts everywhere, the switching keys in
the hybrid cases (they are read late, in the MAC: step (4) of the protocol, which restores the decoys behind the call, is what
catches an entry that is still reading), sk / new_sk / pk where an entry reads them.  hefx_raise_switch reads the collapsed key
that hefx_collapse_key's case has just written on the same stream: that buffer holds the collapse case's output decoy until the
stream runs.

hefx_ckks_encode_wide, hefx_ckks_encode_wide_batch and hefx_ckks_encode_scalar are declared in include/hefx.h, not in an
extension header, and their values (h_re, h_im, h_values) are HOST memory: they are outside this table (the decoy protocol
stages device operands; tests/test_gpu_streams.py treats the host-value encodes by overwriting the host array)."""
import os
import re

import numpy as np

from tests import hybrid_bsgs_cases as HB
from tests import hybrid_cases as HC
from tests import hybrid_hoist_cases as HH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SET = "k8a3-p50_60"     # N = 2048, k = 8, alpha = 3; L = 5: two digits, the last one partial
L_TOP = 5
BIG = "big"             # N = 32768, k = 4, alpha = 2, L = 2: every transform goes src != dst
KEY32 = bytes(range(7, 39))

# the launch rules of the engine the sequence cases lean on, restated beside those of tests/hybrid_cases.py
KS_MAX_CHUNK = HC.KS_MAX_CHUNK         # hefx_internal.h  constexpr int KS_MAX_CHUNK = 1024
KS_RING = 32                           # hefx_internal.h:91  constexpr int KS_RING = 32
SCRATCH_FLOOR_BYTES = 64 << 20         # hefx_capi.cpp, ensure_scratch: at least (size_t)8 << 20 words
RING_CALLS = 2 * KS_RING + 1           # 65 one-item calls: call 33 waits for slot 0, call 65 takes it a third time
CHUNKED_N = 1030                       # at L = 1 a chunk takes KS_MAX_CHUNK items: 1024 + 6
CHUNKED_SAMPLES = (0, 1, 2, 511, 1023, 1024, 1025, 1029)
KS_SPLIT_N, KS_SPLIT_L = 600, 2        # hefx_apply_galois_batch: chunks of 512 below N = 16384, so 512 + 88 on two internal streams
KS_SPLIT_SAMPLES = (0, 1, 87, 88, 299, 511, 512, 513, 598, 599)


def grow_items(s, L):
    """items of the second call of the scratch-growth case: the first number past the floor, and a few more"""
    return SCRATCH_FLOOR_BYTES // (HC.item_rows(s.N, s.alpha, L) * s.N * 8) + 8


class Case:
    """One entry under the decoy protocol: the arguments of test_gpu_streams.Op, with call(e, ins, outs, stream) taking the
    engine.  want / want_decoy: one array per output buffer, or {index: words} for the sampled items of a slab; they have the
    same structure, so that `differs` can hold EVERY checked output to the non-vacuity condition."""

    def __init__(self, name, c_name, reals, decoys, want, want_decoy, call, inplace=None, out_shapes=None):
        self.name, self.c_name, self.reals, self.decoys, self.want, self.want_decoy = name, c_name, reals, decoys, want, want_decoy
        self.call, self.inplace, self.out_shapes = call, inplace, out_shapes
        assert len(reals) == len(decoys) and all(r.shape == d.shape and r.dtype == d.dtype == np.uint64 for r, d in zip(reals, decoys)), name
        assert len(want) == len(want_decoy), name

    def differs(self):
        """per checked output: do the decoys give other words than the real operands?"""
        out = []
        for a, b in zip(self.want, self.want_decoy):
            if isinstance(a, dict):
                assert sorted(a) == sorted(b), self.name
                out += [bool((a[i] != b[i]).any()) for i in a]
            else:
                out.append(bool((a != b).any()))
        return out


def parts(dev, n):
    """the n equal parts of a device array [n][...] (test_gpu_streams.views)"""
    words = dev.nwords // n
    return [dev.view(i * words, dev.shape[1:]) for i in range(n)]


def canonical(primes, rows, front, N, seed):
    """[*front][len(rows)][N] uniform canonical words, row r below primes[rows[r]]"""
    rng = np.random.default_rng(seed)
    out = np.empty(tuple(front) + (len(rows), N), dtype=np.uint64)
    for r, j in enumerate(rows):
        out[..., r, :] = rng.integers(0, int(primes[j]), tuple(front) + (N,), dtype=np.uint64)
    return out


def hkeys(s, seeds):
    return np.stack([HC.random_key(s, sd) for sd in seeds])


_CACHE = {}


def cached(f):
    def g(*a):
        if (f.__name__, a) not in _CACHE:
            _CACHE[f.__name__, a] = f(*a)
        return _CACHE[f.__name__, a]
    g.__name__ = f.__name__
    return g


# ---------------------------------------------------------------------------------------------------------------------
# hefx_hybrid.h
# ---------------------------------------------------------------------------------------------------------------------
TRIO_ELTS = lambda N: [3, 2 * N - 1, 1]
TRIO_KEY = (0, 1, 0)


@cached
def trio(name, L, side):
    """the operands of three Galois items -- the elements 3, 2N - 1 and 1, the second on a key of its own -- and of three
    relinearisations with key 0, real (side 0) or decoy (side 1): dict(A [3][2][L][N], A3 [3][3][L][N], K [2][dnum][2][k][N])"""
    s, base = HC.sets()[name], 1000 * side + 10 * L
    return dict(A=np.stack([HC.operand(s, "uniform", L, 2, seed=base + 50 + i) for i in range(3)]),
                A3=np.stack([HC.operand(s, "uniform", L, 3, seed=base + 60 + i) for i in range(3)]), K=hkeys(s, (base + 11, base + 12)))


@cached
def gal(name, L, side, i):
    """the model's words of Galois item i of the trio, once per process"""
    s, t = HC.sets()[name], trio(name, L, side)
    return HC.apply_galois_model(HC.twin(s), s.primes, s.alpha, L, t["A"][i], TRIO_ELTS(s.N)[i], t["K"][TRIO_KEY[i]])


@cached
def rel(name, L, side, i):
    s, t = HC.sets()[name], trio(name, L, side)
    return HC.relinearize_model(HC.twin(s), s.primes, s.alpha, L, t["A3"][i], t["K"][0])


def _galois_call(s, L, n):
    elts, which = TRIO_ELTS(s.N), TRIO_KEY

    def call(e, i, t, st):
        ins, keys = parts(i[0], 3), parts(i[1], 2)
        e.hybrid_apply_galois_batch(s.alpha, L, [ins[j % 3] for j in range(n)], [elts[j % 3] for j in range(n)],
                                    [keys[which[j % 3]] for j in range(n)], outs=parts(t[0], n), stream=st)
    return call


def galois_batch(name=SET, L=L_TOP):
    """three items out of place, elements 3, 2N - 1 and 1, two keys"""
    s, r, d = HC.sets()[name], trio(name, L, 0), trio(name, L, 1)
    want = lambda side: np.stack([gal(name, L, side, i) for i in range(3)])
    return Case(f"hybrid_apply_galois_batch(3) at {name}", "hefx_hybrid_apply_galois_batch", [r["A"], r["K"]], [d["A"], d["K"]],
                [want(0)], [want(1)], _galois_call(s, L, 3))


def galois_in_place(name=SET, L=L_TOP):
    """one exact in-place item: the output IS the input"""
    s, r, d = HC.sets()[name], trio(name, L, 0), trio(name, L, 1)
    return Case(f"hybrid_apply_galois_batch in place at {name}", "hefx_hybrid_apply_galois_batch", [r["A"][0], r["K"][0]], [d["A"][0], d["K"][0]],
                [gal(name, L, 0, 0)], [gal(name, L, 1, 0)],
                lambda e, i, t, st: e.hybrid_apply_galois_batch(s.alpha, L, [i[0]], [3], [i[1]], outs=[i[0]], stream=st), inplace=[0])


def galois_one(name=SET, L=L_TOP, item=0):
    """one item out of place (the set at N = 32768, the first call of the scratch-growth case, the ring)"""
    s, r, d = HC.sets()[name], trio(name, L, 0), trio(name, L, 1)
    elt, ki = TRIO_ELTS(s.N)[item], TRIO_KEY[item]
    return Case(f"hybrid_apply_galois_batch(1) at {name}, L = {L}, element {elt}", "hefx_hybrid_apply_galois_batch",
                [r["A"][item], r["K"][ki]], [d["A"][item], d["K"][ki]], [gal(name, L, 0, item)], [gal(name, L, 1, item)],
                lambda e, i, t, st: e.hybrid_apply_galois_batch(s.alpha, L, [i[0]], [elt], [i[1]], outs=[t[0]], stream=st))


def galois_many(n, samples, name=SET, L=L_TOP):
    """n items that cycle through the trio's inputs, elements and keys; sampled checks"""
    s, r, d = HC.sets()[name], trio(name, L, 0), trio(name, L, 1)
    assert all(0 <= i < n for i in samples)
    return Case(f"hybrid_apply_galois_batch({n}) at {name}, L = {L}", "hefx_hybrid_apply_galois_batch", [r["A"], r["K"]], [d["A"], d["K"]],
                [{i: gal(name, L, 0, i % 3) for i in samples}], [{i: gal(name, L, 1, i % 3) for i in samples}], _galois_call(s, L, n),
                out_shapes=[(n, 2, L, s.N)])


def relin_batch(n=3, name=SET, L=L_TOP):
    s, r, d = HC.sets()[name], trio(name, L, 0), trio(name, L, 1)
    want = lambda side: np.stack([rel(name, L, side, i) for i in range(n)])
    return Case(f"hybrid_relinearize_batch({n}) at {name}", "hefx_hybrid_relinearize_batch", [r["A3"][:n], r["K"][0]], [d["A3"][:n], d["K"][0]],
                [want(0)], [want(1)],
                lambda e, i, t, st: e.hybrid_relinearize_batch(s.alpha, L, parts(i[0], n), i[1], outs=parts(t[0], n), stream=st))


def keygen_model(s, sk, new_sk, key32, stream_id):
    """the key of include/hefx_hybrid.h on the twin: key[j] = (-(a_j s + e_j) + F_j (.) s', a_j), a the uniform draw of dnum
    polynomials from sub-stream 2 id, e the noise from 2 id + 1 (transformed by the twin), F_j[m] = P mod q_m on digit j's rows"""
    be, q, k, D = HC.twin(s), [int(p) for p in s.primes], s.k, s.k - s.alpha
    a = be.sample("uniform", key32, 2 * stream_id, s.dnum, k)
    e = be.ntt_forward(be.sample("noise", key32, 2 * stream_id + 1, s.dnum, k), s.dnum, k, 0)
    P = int(np.prod(q[D:], dtype=object))
    out = np.empty((s.dnum, 2, k, s.N), dtype=np.uint64)
    for j in range(s.dnum):
        for m in range(k):
            f = P % q[m] if j * s.alpha <= m < min((j + 1) * s.alpha, D) else 0
            c0 = (f * new_sk[m].astype(object) - a[j, m].astype(object) * sk[m].astype(object) - e[j, m].astype(object)) % q[m]
            out[j, 0, m], out[j, 1, m] = c0.astype(np.uint64), a[j, m]
    return out


@cached
def keygen(name=SET):
    """any canonical words are a secret to the arithmetic: both secrets uniform, both decoyed"""
    s = HC.sets()[name]
    sec = [canonical(s.primes, range(s.k), (), s.N, 300 + i) for i in range(4)]
    return Case(f"hybrid_keygen at {name}", "hefx_hybrid_keygen", sec[:2], sec[2:], [keygen_model(s, sec[0], sec[1], KEY32, 7)],
                [keygen_model(s, sec[2], sec[3], KEY32, 7)],
                lambda e, i, t, st: e.hybrid_keygen(s.alpha, i[0], i[1], KEY32, 7, out=t[0], stream=st))


# ---------------------------------------------------------------------------------------------------------------------
# hefx_hybrid_hoist.h and hefx_hybrid_bsgs.h: two sources, the baby elements {1 with a NULL key, 3, 2N - 1}; the terms are
# computed once per side and shared by the three entries
# ---------------------------------------------------------------------------------------------------------------------
def _pts(s, rows, holes, seed):
    """plaintext table [rows][6] with one structural zero per row, and the live plaintexts stacked [rows * 5][k][N]"""
    live = np.stack([HH.plaintext(s, "uniform", seed + i) for i in range(5 * rows)])
    it = iter(live)
    return [[None if t == holes[o] else next(it) for t in range(6)] for o in range(rows)], live


def _table(stack, rows, holes):
    """the pointer table of a call from the device views of the live plaintexts, row-major as _pts stacked them"""
    it = iter(stack)
    return [[None if t == holes[o] else next(it) for t in range(6)] for o in range(rows)]


COMBINE_HOLES, BSGS_HOLES = (4, 0), (4, 0, 3, 1)


@cached
def hoist(name, L, side, n):
    s = HC.sets()[name]
    be, base = HC.twin(s), 2000 * side + 31 * L
    C = np.stack([HC.operand(s, "uniform", L, 2, seed=base + i) for i in range(n)])
    K = hkeys(s, (base + 5, base + 6))
    elts = [1, 3, 2 * s.N - 1]
    terms = HH.terms_model(be, s.primes, s.alpha, L, list(C), elts, [None, K[0], K[1]])
    return dict(C=C, K=K, elts=elts, terms=terms)


def rotate_hoisted(name=SET, L=L_TOP, n=2):
    s, be = HC.sets()[name], HC.twin(HC.sets()[name])
    r, d = hoist(name, L, 0, n), hoist(name, L, 1, n)
    md = lambda h: np.stack([HH.mod_down_model(be, s.primes, s.alpha, L, A) for A in h["terms"]])

    def call(e, i, t, st):
        keys = parts(i[1], 2)
        e.hybrid_rotate_hoisted_batch(s.alpha, L, parts(i[0], n), r["elts"], [None, keys[0], keys[1]], outs=parts(t[0], 3 * n), stream=st)
    return Case(f"hybrid_rotate_hoisted_batch at {name}", "hefx_hybrid_rotate_hoisted_batch", [r["C"], r["K"]], [d["C"], d["K"]], [md(r)], [md(d)], call)


def plain_combine_hoisted(name=SET, L=L_TOP):
    """G = 2 outputs over the six terms, one structural zero each"""
    s, be = HC.sets()[name], HC.twin(HC.sets()[name])
    r, d = hoist(name, L, 0, 2), hoist(name, L, 1, 2)
    (pr, lr), (pd, ld) = _pts(s, 2, COMBINE_HOLES, 4000), _pts(s, 2, COMBINE_HOLES, 5000)
    want = lambda h, p: np.stack([HH.mod_down_model(be, s.primes, s.alpha, L, B) for B in HB.sums_model(s.primes, s.alpha, L, h["terms"], p)])

    def call(e, i, t, st):
        keys = parts(i[1], 2)
        e.hybrid_plain_combine_hoisted(s.alpha, L, parts(i[0], 2), r["elts"], [None, keys[0], keys[1]], _table(parts(i[2], 10), 2, COMBINE_HOLES),
                                       outs=parts(t[0], 2), stream=st)
    return Case(f"hybrid_plain_combine_hoisted at {name}", "hefx_hybrid_plain_combine_hoisted", [r["C"], r["K"], lr], [d["C"], d["K"], ld],
                [want(r, pr)], [want(d, pd)], call)


def bsgs_hoisted(name=SET, L=L_TOP):
    """the shape of hybrid_bsgs_cases.case: G = 4 inner sums, O = 2 outputs, giant elements 3 and 2N - 1 on two giant keys"""
    s, be = HC.sets()[name], HC.twin(HC.sets()[name])
    r, d = hoist(name, L, 0, 2), hoist(name, L, 1, 2)
    (pr, lr), (pd, ld) = _pts(s, 4, BSGS_HOLES, 6000), _pts(s, 4, BSGS_HOLES, 7000)
    gelts, dest = [1, 3, 1, 2 * s.N - 1], list(HB.DEST)
    gr, gd = hkeys(s, (8001, 8002)), hkeys(s, (9001, 9002))

    def want(h, p, g):
        sums = HB.sums_model(s.primes, s.alpha, L, h["terms"], p)
        Ws = [HB.giant_model(be, s.primes, s.alpha, L, B, ge, K) for B, ge, K in zip(sums, gelts, [None, g[0], None, g[1]])]
        return np.stack(HB.outputs_model(be, s.primes, s.alpha, L, Ws, dest))

    def call(e, i, t, st):
        keys, gk = parts(i[1], 2), parts(i[3], 2)
        e.hybrid_bsgs_hoisted(s.alpha, L, parts(i[0], 2), r["elts"], [None, keys[0], keys[1]], _table(parts(i[2], 20), 4, BSGS_HOLES), gelts,
                              [None, gk[0], None, gk[1]], dest, outs=parts(t[0], 2), stream=st)
    return Case(f"hybrid_bsgs_hoisted at {name}", "hefx_hybrid_bsgs_hoisted", [r["C"], r["K"], lr, gr], [d["C"], d["K"], ld, gd],
                [want(r, pr, gr)], [want(d, pd, gd)], call)


# ---------------------------------------------------------------------------------------------------------------------
# sequences on the hybrid entries
# ---------------------------------------------------------------------------------------------------------------------
def chunked():
    """hefx_hybrid_apply_galois_batch at L = 1 with 1030 items: two descriptor slots, two launch sequences through one scratch"""
    s = HC.sets()[SET]
    assert HC.chunk_of(s.N, s.alpha, 1) == KS_MAX_CHUNK < CHUNKED_N
    return galois_many(CHUNKED_N, CHUNKED_SAMPLES, L=1)


def ring_wrap():
    """65 one-item calls at L = 1, every one checked: the three items of the trio in turn"""
    return [galois_one(L=1, item=j % 3) for j in range(RING_CALLS)]


def scratch_growth():
    """(a one-item call, a call of grow_items items): on a fresh context the first fits the 64 MiB ensure_scratch allocates at
    least, the second does not, so its growth retires the buffer the first still has queued"""
    s = HC.sets()[SET]
    n = grow_items(s, L_TOP)
    return [galois_one(), galois_many(n, sorted({0, 1, 2, n // 2, n - 2, n - 1}))]


@cached
def two_streams(name=SET, L=L_TOP):
    """item 0 of the trio on S1, its result rotated again by 2N - 1 with key 1 on S2: dict(A, B the real and the decoy input of
    the first call, K the two keys, want the second call's words, want_decoy those the decoy input would give)"""
    s, be = HC.sets()[name], HC.twin(HC.sets()[name])
    r, d = trio(name, L, 0), trio(name, L, 1)
    second = lambda x: HC.apply_galois_model(be, s.primes, s.alpha, L, x, 2 * s.N - 1, r["K"][1])
    first_decoy = HC.apply_galois_model(be, s.primes, s.alpha, L, d["A"][0], 3, r["K"][0])
    return dict(s=s, L=L, A=r["A"][0], B=d["A"][0], K=r["K"], want=second(gal(name, L, 0, 0)), want_decoy=second(first_decoy))


@cached
def ks_split(name=SET):
    """hefx_apply_galois_batch (the scheme of hefx.h) on the hybrid context: 600 distinct sources at L = 2, three elements, one
    key [k-1][2][k][N] -- two chunks, forked onto the internal streams, in the scratch the hybrid entries use.  Sampled against
    oracle.Oracle; the sources are decoyed"""
    s = HC.sets()[name]
    o, n, L = HC.twin(s).o, KS_SPLIT_N, KS_SPLIT_L
    A, B = (canonical(s.primes, range(L), (n, 2), s.N, sd) for sd in (610, 611))
    key = np.stack([canonical(s.primes, range(s.k), (2,), s.N, 620 + j) for j in range(s.k - 1)])
    elts = [(3, 2 * s.N - 1, 5)[i % 3] for i in range(n)]
    want = lambda X: {i: o.apply_galois(np.ascontiguousarray(X[i]), elts[i], key) for i in KS_SPLIT_SAMPLES}
    case = Case(f"apply_galois_batch({n}) split over the internal streams", "hefx_apply_galois_batch", [A], [B], [want(A)], [want(B)], None,
                out_shapes=[A.shape])
    case.key, case.elts, case.L, case.n = key, elts, L, n
    return case


# ---------------------------------------------------------------------------------------------------------------------
# hefx_refresh.h at the shapes of tests/test_gpu_refresh.py's gate test: the LR chain at N = 1024, L_in = 2, L_out = 8, 3 items
# ---------------------------------------------------------------------------------------------------------------------
REFRESH_N, REFRESH_LIN, REFRESH_LOUT, REFRESH_COUNT, REFRESH_SID = 1024, 2, 8, 3, 9


@cached
def refresh_primes():
    from seal_fyp_logistic_regression_amd import seal as S
    from tests import lr_gradient_cases as G
    return [int(p) for p in S.CoeffModulus.Create(REFRESH_N, G.LR_BITS)]


def mod_raise():
    from tests import refresh_cases as R
    primes = refresh_primes()
    a, b = (R.crafted_words(primes, REFRESH_LIN, REFRESH_N, REFRESH_COUNT, seed=sd) for sd in (5, 6))
    lift = lambda x: R.lift(x, primes, REFRESH_LIN, REFRESH_LOUT)
    return Case("mod_raise", "hefx_mod_raise", [a], [b], [lift(a)], [lift(b)],
                lambda e, i, t, st: e.mod_raise(REFRESH_LIN, REFRESH_LOUT, i[0], count=REFRESH_COUNT, out=t[0], stream=st))


@cached
def _refresh_operands(side):
    primes, k, N = refresh_primes(), len(refresh_primes()), REFRESH_N
    cts = canonical(primes, range(REFRESH_LIN), (REFRESH_COUNT, 2), N, 700 + side)
    sk, pk = canonical(primes, range(k), (), N, 710 + side), canonical(primes, range(k), (2,), N, 720 + side)
    return cts, sk, pk


@cached
def refresh_model(side, item):
    """the header's composition on the references: OracleBackend.decrypt at L_in, refresh_cases.lift, OracleBackend.encrypt at
    L_out with KEY32 and the stream id REFRESH_SID + item"""
    from tests import refresh_cases as R
    from tests.oracle_backend import OracleBackend
    primes = refresh_primes()
    cts, sk, pk = _refresh_operands(side)
    be = OracleBackend(REFRESH_N, primes)
    pt = be.decrypt(REFRESH_LIN, 2, cts[item], sk)
    pt = R.lift(np.asarray(pt)[None], primes, REFRESH_LIN, REFRESH_LOUT)[0]
    return np.asarray(be.encrypt(REFRESH_LOUT, pk, pt, KEY32, REFRESH_SID + item)).reshape(2, REFRESH_LOUT, REFRESH_N)


def refresh():
    (cr, skr, pkr), (cd, skd, pkd) = _refresh_operands(0), _refresh_operands(1)
    return Case("refresh", "hefx_refresh", [cr[0], skr, pkr], [cd[0], skd, pkd], [refresh_model(0, 0)], [refresh_model(1, 0)],
                lambda e, i, t, st: e.refresh(REFRESH_LIN, 2, REFRESH_LOUT, i[0], i[1], i[2], KEY32, REFRESH_SID, out=t[0], stream=st))


def refresh_batch():
    n = REFRESH_COUNT
    (cr, skr, pkr), (cd, skd, pkd) = _refresh_operands(0), _refresh_operands(1)
    want = lambda side: np.stack([refresh_model(side, i) for i in range(n)])
    return Case("refresh_batch", "hefx_refresh_batch", [cr, skr, pkr], [cd, skd, pkd], [want(0)], [want(1)],
                lambda e, i, t, st: e.refresh_batch(REFRESH_LIN, 2, REFRESH_LOUT, parts(i[0], n), i[1], i[2], KEY32, REFRESH_SID,
                                                    outs=parts(t[0], n), stream=st))


# ---------------------------------------------------------------------------------------------------------------------
# hefx_encaps.h at the shapes of tests/test_gpu_encaps.py's gate test: the chain "wide0" at N = 2048, the top level
# ---------------------------------------------------------------------------------------------------------------------
@cached
def encaps_primes():
    from seal_fyp_logistic_regression_amd import seal as S
    from tests import encaps_cases as EC
    return [int(p) for p in S.CoeffModulus.Create(EC.N, EC.CHAINS["wide0"])]


@cached
def _encaps_operands(side):
    from tests import encaps_cases as EC
    primes = encaps_primes()
    k, top = len(primes), len(primes) - 1
    ct1, key = EC.random_operands(EC.N, primes, 800 + side)
    return ct1, key, canonical(primes, range(top), (2,), EC.N, 810 + side), top


def switch_key():
    from tests import encaps_cases as EC
    from tests.oracle_backend import OracleBackend
    o = OracleBackend(EC.N, encaps_primes()).o
    (_, kr, cr, top), (_, kd, cd, _) = _encaps_operands(0), _encaps_operands(1)
    return Case("switch_key", "hefx_switch_key", [cr, kr], [cd, kd], [o.apply_galois(cr, 1, kr)], [o.apply_galois(cd, 1, kd)],
                lambda e, i, t, st: e.switch_key(top, i[0], i[1], out=t[0], stream=st))


def collapse_key():
    from tests import encaps_cases as EC
    primes = encaps_primes()
    (_, kr, _, top), (_, kd, _, _) = _encaps_operands(0), _encaps_operands(1)
    return Case("collapse_key", "hefx_collapse_key", [kr], [kd], [EC.collapse_model(kr, primes, top)], [EC.collapse_model(kd, primes, top)],
                lambda e, i, t, st: e.collapse_key(top, i[0], out=t[0], stream=st))


def raise_switch():
    """call(e, ins, outs, stream, ckey): ckey is the OUTPUT buffer of collapse_key's case, written on the same stream just before;
    the expected words are raise_switch_model's on the real key (it collapses the key itself), the decoys' on the decoy
    ciphertext and the decoy key"""
    from tests import encaps_cases as EC
    from tests.oracle_backend import OracleBackend
    primes = encaps_primes()
    be = OracleBackend(EC.N, primes)
    (c1r, kr, _, top), (c1d, kd, _, _) = _encaps_operands(0), _encaps_operands(1)
    return Case("raise_switch", "hefx_raise_switch", [c1r], [c1d], [EC.raise_switch_model(be, primes, top, c1r, kr)],
                [EC.raise_switch_model(be, primes, top, c1d, kd)],
                lambda e, i, t, st, ckey: e.raise_switch(top, i[0], ckey, out=t[0], stream=st))


# ---------------------------------------------------------------------------------------------------------------------
# every case by name (builders: the models run when a case is first asked for), and the coverage table
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    "galois_batch": galois_batch, "galois_in_place": galois_in_place, "relin_batch": relin_batch, "keygen": keygen,
    "rotate_hoisted": rotate_hoisted, "plain_combine_hoisted": plain_combine_hoisted, "bsgs_hoisted": bsgs_hoisted,
    "chunked": chunked,
    "big_galois": lambda: galois_one(BIG, 2), "big_relin": lambda: relin_batch(1, BIG, 2), "big_rotate_hoisted": lambda: rotate_hoisted(BIG, 2, 1),
    "ring_wrap": ring_wrap, "scratch_growth": scratch_growth, "ks_split": ks_split,
    "mod_raise": mod_raise, "refresh": refresh, "refresh_batch": refresh_batch,
    "switch_key": switch_key, "collapse_key": collapse_key, "raise_switch": raise_switch,
}


def flat(name):
    """the Case objects of a named case (a sequence case is several)"""
    c = CASES[name]()
    return list(c) if isinstance(c, (list, tuple)) else [c]


BFV = ("not yet: the hefx_bfv object owns its working basis, tables and scratch (hefx_bfv.h, 'Scratch and streams'), not the "
       "context's ring and scratch these cases press on; its coefficient-form operands need decoys and models of their own")
COVERAGE = {
    # include/hefx_hybrid.h
    "hefx_hybrid_keygen": ["keygen"],
    "hefx_hybrid_apply_galois_batch": ["galois_batch", "galois_in_place", "chunked", "big_galois", "ring_wrap", "scratch_growth"],
    "hefx_hybrid_relinearize_batch": ["relin_batch", "big_relin"],
    # include/hefx_hybrid_hoist.h, include/hefx_hybrid_bsgs.h
    "hefx_hybrid_rotate_hoisted_batch": ["rotate_hoisted", "big_rotate_hoisted"],
    "hefx_hybrid_plain_combine_hoisted": ["plain_combine_hoisted"],
    "hefx_hybrid_bsgs_hoisted": ["bsgs_hoisted"],
    # include/hefx_refresh.h, include/hefx_encaps.h
    "hefx_mod_raise": ["mod_raise"], "hefx_refresh": ["refresh"], "hefx_refresh_batch": ["refresh_batch"],
    "hefx_switch_key": ["switch_key"], "hefx_collapse_key": ["collapse_key"], "hefx_raise_switch": ["raise_switch"],
    # held to the same protocol (decoys staged behind a gate, restored behind the call) by their own modules
    "hefx_plain_combine": "tests/test_gpu_dft.py", "hefx_scalar_combine": "tests/test_gpu_poly.py", "hefx_product_combine": "tests/test_gpu_bootstrap.py",
    # include/hefx_bfv.h
    "hefx_bfv_multiply": BFV, "hefx_bfv_decrypt_round": BFV, "hefx_bfv_scale_plain_add": BFV, "hefx_bfv_lift_plain": BFV,
    "hefx_bfv_noise_budget": BFV, "hefx_bfv_batch_encode": BFV, "hefx_bfv_batch_decode": BFV,
}


def extension_headers():
    inc = os.path.join(ROOT, "include")
    return sorted(os.path.join(inc, f) for f in os.listdir(inc) if re.fullmatch(r"hefx_\w+\.h", f))


def stream_entries(path):
    """the names of the declarations of a header that take `void *stream`"""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(hefx_\w+)\s*\(([^;{}]*?)\)\s*;", text) if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))]
