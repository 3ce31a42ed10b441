"""The reference's composite HE algorithms (its L3 layer), restated over the seal.py API mirror so that the same
code drives the HIP engine (product) and, in tests, the oracle-backed twin.  Each function follows the
reference line by line in WHAT it calls and in which order -- results must be bit-identical -- but is free in HOW
the calls are batched: independent rotations of one ciphertext go to the engine as one batch.

Citations are /root/reference/helper.h unless noted.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import operator

import numpy as np

from . import poly as _poly
from .seal import Ciphertext, CKKSEncoder, Evaluator, HybridEncapsKeys, HybridKeys, KSwitchKeys, Plaintext


def _kswitch_only(fn):
    """The fused composites -- the linear transforms, the plain_combine / product_combine pipelines, the bootstrap -- run kernels
    that know the one-special-prime key layout: given seal.HybridKeys they refuse before anything is computed.  (The DFT has
    forms of its own on hybrid keys: coeffs_to_slots_hybrid, slots_to_coeffs_hybrid and their _packed_hybrid forms, below.)"""
    import functools

    @functools.wraps(fn)
    def checked(*args, **kwargs):
        for a in (*args, *kwargs.values()):
            if isinstance(a, HybridKeys):
                raise TypeError(f"{fn.__name__} with HybridKeys (alpha = {a.alpha}) is not supported: hybrid key switching serves "
                                "Evaluator.rotate_vector, apply_galois, complex_conjugate, relinearize and switch_key only")
        return fn(*args, **kwargs)
    return checked


# ---- plain data prep (L0) -------------------------------------------------------------------
def get_diagonal(position: int, U: np.ndarray) -> np.ndarray:
    """helper.h:175-195: U(0,l), U(1,l+1), ... wrapping around."""
    n = U.shape[0]
    return np.array([U[i, (i + position) % n] for i in range(n)], dtype=U.dtype)


def get_all_diagonals(U: np.ndarray) -> np.ndarray:
    """helper.h:198-209"""
    return np.stack([get_diagonal(i, U) for i in range(U.shape[0])])


# ---- linear transforms ----------------------------------------------------------------------
def _rotations_of_many(ev: Evaluator, cts: Sequence[Ciphertext], steps: Sequence[int], gal_keys: KSwitchKeys,
                       pts_per_input: Sequence[Sequence[Plaintext]] = None) -> List[List[Ciphertext]]:
    """[[rotate_vector(ct, l) for l in steps] for ct in cts] over SEAL's NAF plans, for one or more inputs of one level and
    size 2.  Identical (source payload, Galois element) pairs are computed once -- the key switch is deterministic, so
    sharing cannot change a bit.  pts_per_input[t][i] (optional): multiply_plain of input t's rotation by steps[i], fused
    into the last key switch of its plan (hefx_rotate_multiply_plain_batch).

    Where the backend has it, the NAF forests of all inputs go out in ONE engine call (hefx_apply_galois_forest takes any
    number of roots: the depths of the forests run side by side, so k inputs cost the dependent launch sequences of one,
    and the engine schedules depth batches, subtrees on lanes and hoisted depths itself).  Other backends, and a single key
    switch, run depth by depth, each engine call one batch of an input's independent key switches.  Step 0 has an empty
    plan: its result is the input's copy, times its plaintext.  Inputs of mixed level or size are served one by one.

    The plaintext checks are Evaluator._plain_product_scale's, per input over all its plaintexts, made after the rotation
    plans (a missing Galois key raises first) and BEFORE anything is submitted.  Every single fault raises what
    multiply_plain + add_many raise op by op; of two simultaneous faults the one multiply_plain reports first is raised."""
    be = ev.be
    fused = pts_per_input is not None
    if len(cts) > 1 and (len({c.parms_id() for c in cts}) != 1 or any(c.size() != 2 for c in cts)):
        return [_rotations_batched(ev, c, steps, gal_keys, pts_per_input[t] if fused else None) for t, c in enumerate(cts)]
    plans = [ev.rotation_plan(s, gal_keys) for s in steps]
    if not cts or not plans:
        return [[] for _ in cts]
    L = cts[0].parms_id()
    if fused:
        for ct, pts in zip(cts, pts_per_input):
            ev._plain_product_scale(L, ct.scale, pts, L)
    leaves = []  # [input][step] -> payload of the plan's last node (None: step 0)
    if hasattr(be, "apply_galois_forest") and len(cts) * sum(len(p) for p in plans) > 1:
        parents, ext, elts, node_pts = [], [], [], []
        for t, ct in enumerate(cts):
            index, row = {}, []
            for i, p in enumerate(plans):
                c = -1
                for depth, elt in enumerate(p):
                    fuse = fused and depth == len(p) - 1
                    key = (c, elt, i if fuse else -1)
                    j = index.get(key)
                    if j is None:
                        j = index[key] = len(parents)
                        parents.append(c), ext.append(ct.data if c < 0 else None), elts.append(elt)
                        node_pts.append(pts_per_input[t][i].data if fuse else None)
                    c = j
                row.append(c)
            leaves.append(row)
        outs = be.apply_galois_forest(L, parents, ext, elts, [gal_keys.key(e) for e in elts], node_pts if fused else None)
        leaves = [[outs[j] if j >= 0 else None for j in row] for row in leaves]
    else:
        for t, ct in enumerate(cts):
            cur = [ct.data if p else None for p in plans]
            for depth in range(max(len(p) for p in plans)):
                jobs, owner = {}, {}   # (id(source), element, fused owner) -> (source, element, plaintext); step -> its job
                for i, p in enumerate(plans):
                    if depth < len(p):
                        fuse = fused and depth == len(p) - 1
                        owner[i] = key = (id(cur[i]), p[depth], i if fuse else -1)
                        jobs.setdefault(key, (cur[i], p[depth], pts_per_input[t][i].data if fuse else None))
                done = {}
                for with_pt in (False, True):
                    ks = [k for k, job in jobs.items() if (job[2] is not None) == with_pt]
                    if ks:
                        src, el, pt = zip(*[jobs[k] for k in ks])
                        keys = [gal_keys.key(e) for e in el]
                        o = be.rotate_multiply_plain_batch(L, list(src), list(el), keys, list(pt)) if with_pt else \
                            be.apply_galois_batch(L, list(src), list(el), keys)
                        done.update(zip(ks, o))
                for i, key in owner.items():
                    cur[i] = done[key]
            leaves.append(cur)
    res = []
    for t, ct in enumerate(cts):
        row = []
        for i, data in enumerate(leaves[t]):
            if data is None:  # step 0: rotate_vector returns its input unchanged
                row.append(ev.multiply_plain(ct.copy(), pts_per_input[t][i]) if fused else ct.copy())
            else:
                row.append(Ciphertext()._set(data, 2, L, ct.scale * pts_per_input[t][i].scale if fused else ct.scale))
        res.append(row)
    return res


def _rotations_batched(ev: Evaluator, ct: Ciphertext, steps: Sequence[int], gal_keys: KSwitchKeys,
                       pts: Sequence[Plaintext] = None) -> List[Ciphertext]:
    """rotate_vector(ct, l) for every l in `steps`, times pts[i] when given: _rotations_of_many for one input"""
    return _rotations_of_many(ev, [ct], steps, gal_keys, None if pts is None else [pts])[0]


_PT_PTR = operator.attrgetter("data.ptr")


def _native_args(gal_keys: KSwitchKeys, operands: Sequence):
    """(elements, key payloads, operand payloads) in the form the native entry points take -- the one place that knows the
    HIP engine from the other backends.  There the tables are C arrays: the operands' built in one C-level pass, the two
    of the key set built once and kept on it (512 keys: 0.1 ms of Python per call otherwise, with the GPU idle) until keys
    are added or replaced.  Other backends get plain lists.  Missing keys / too large steps come back from the engine
    with SEAL's messages (ValueError)."""
    elts = sorted(gal_keys.keys)
    keys = [gal_keys.key(e) for e in elts]
    if not keys or not hasattr(keys[0], "ptr"):
        return elts, keys, [x.data for x in operands]
    from .engine import ptr_array, u32_array
    # fingerprint: elements AND payload addresses -- a key replaced under an existing element, or one removed and another
    # added, must not leave the native transform on the old payloads (0.03 ms at 512 keys against 0.1 ms for the C arrays)
    mark = (tuple(elts), tuple(k.ptr for k in keys))
    cache = getattr(gal_keys, "_native_args", None)
    if cache is None or cache[0] != mark:
        cache = gal_keys._native_args = (mark, u32_array(elts), ptr_array(list(mark[1])), keys)  # keys: kept alive
    return cache[1], cache[2], ptr_array(list(map(_PT_PTR, operands)))


def _direct_elts(ev: Evaluator, steps: Sequence[int], gal_keys: KSwitchKeys, what: str) -> List[int]:
    """the Galois element of every step, for the forms that run one key switch per rotation (the native entries make this
    check themselves)"""
    plans = [ev.rotation_plan(s, gal_keys) for s in steps]
    if any(len(p) != 1 for p in plans):
        raise ValueError(f"{what} needs a direct Galois key for every step")
    return [p[0] for p in plans]


def _duplicate(ev: Evaluator, ct: Ciphertext, d: int, gal_keys: KSwitchKeys) -> Ciphertext:
    return ev.add(ct, ev.rotate_vector(ct, -d, gal_keys))            # helper.h:244-247


@_kswitch_only
def linear_transform_plain(ev: Evaluator, ct: Ciphertext, U_diagonals: Sequence[Plaintext],
                           gal_keys: KSwitchKeys, hoisted: bool = False) -> Ciphertext:
    """Linear_Transform_Plain, helper.h:237-262 (= linear_transformation2.cpp:149-174).

    hoisted=2 is the double-hoisted fast mode: U_diagonals must be KEY-LEVEL plaintexts (encoder.encode(..., parms_id =
    context.key_parms_id())), ct at the top data level; the products are accumulated over the extended basis and modded
    down once (hefx_linear_transform_plain_hoisted2) -- per rotation only a gathered key MAC remains.

    hoisted=True asks for SURVEY 8f rank 3 explicitly: the d-1 rotations of ct_new share one digit decomposition
    (hefx_rotate_hoisted_batch); it needs a direct Galois key per step (keygen.galois_keys(steps)).  Since round 4 the
    hoisted form is EXACT -- the engine adds the term by which SEAL's positive digit lifts differ from the signed ones
    (DESIGN.md "Exact hoisting") -- so this is bit-identical to the reference's sequence with those keys, and the plain
    call (hoisted=False) takes the same path by itself whenever more than 32 rotations share a source."""
    d = len(U_diagonals)
    if hoisted == 2:
        return _linear_transform_plain_hoisted2(ev, ct, d, None, U_diagonals, gal_keys)
    native = getattr(ev.be, "linear_transform_plain", None)
    if native is not None:  # the HIP engine runs the whole transform behind one C-ABI call, same bits
        return _linear_transform_plain_native(ev, native, ct, U_diagonals, gal_keys, bool(hoisted))
    if hoisted:
        return _linear_transform_plain_hoisted(ev, ct, U_diagonals, gal_keys)
    ct_new = _duplicate(ev, ct, d, gal_keys)                         # :244-247  fill with duplicate
    res = [ev.multiply_plain(ct_new, U_diagonals[0])]                # :250
    res += _rotations_batched(ev, ct_new, list(range(1, d)), gal_keys, U_diagonals[1:])   # :252-257
    return ev.add_many(res)                                          # :259


def _linear_transform_plain_hoisted2(ev: Evaluator, ct: Ciphertext, d: int, steps: Sequence[int],
                                     pts: Sequence[Plaintext], gal_keys: KSwitchKeys) -> Ciphertext:
    """double hoisting (one mod-down for the whole transform) over the diagonals `steps` of a d x d matrix (steps[0] == 0;
    None: all d of them, the dense entry): KEY-LEVEL plaintexts, ct at the top data level, direct keys for the other steps"""
    ctx, be, L = ev.ctx, ev.be, ct.parms_id()
    if ct.size() != 2:
        raise ValueError("encrypted size must be 2")
    if L != ctx.first_parms_id():
        raise ValueError("double hoisting is built for the top data level")
    scale = ev._plain_product_scale(L, ct.scale, pts, ctx.k)
    dense = steps is None
    steps = list(range(d)) if dense else steps
    native = getattr(be, "linear_transform_plain" if dense else "linear_transform_plain_hoisted2_sparse", None)
    if native is not None:  # plans, key checks and everything else behind one C-ABI call (errors come back as ValueError)
        elts, keys, diag = _native_args(gal_keys, pts)
        data = native(L, ct.data, diag, elts, keys, hoisted=2) if dense else native(L, ct.data, d, steps, diag, elts, keys)
    else:  # the oracle twin: regular -d rotation, then the oracle's statement of the double-hoisted core
        elts = _direct_elts(ev, steps[1:], gal_keys, "hoisted linear transform")
        ct_new = _duplicate(ev, ct, d, gal_keys)
        data = be.lt_double_hoisted_core(ct_new.data, [p.data for p in pts], elts, [gal_keys.key(e) for e in elts])
    return Ciphertext()._set(data, 2, L, scale)


def _linear_transform_plain_hoisted(ev: Evaluator, ct: Ciphertext, U_diagonals: Sequence[Plaintext],
                                    gal_keys: KSwitchKeys) -> Ciphertext:
    """hoisted=True on a backend without the native transform: the d-1 rotations of ct_new as one hoisted batch"""
    d, L = len(U_diagonals), ct.parms_id()
    elts = _direct_elts(ev, range(1, d), gal_keys, "hoisted linear transform")
    scale = ev._plain_product_scale(L, ct.scale, U_diagonals, L)
    ct_new = _duplicate(ev, ct, d, gal_keys)                         # helper.h:244-247, regular rotation
    res = [ev.multiply_plain(ct_new, U_diagonals[0])]                # :250
    outs = ev.be.rotate_hoisted_batch(L, ct_new.data, elts, [gal_keys.key(e) for e in elts],
                                      [p.data for p in U_diagonals[1:]])
    res += [Ciphertext()._set(o, 2, L, scale) for o in outs]
    return ev.add_many(res)                                          # :259


def _linear_transform_plain_native(ev: Evaluator, native, ct: Ciphertext, U_diagonals: Sequence[Plaintext],
                                   gal_keys: KSwitchKeys, hoisted: bool = False) -> Ciphertext:
    """Same checks and bookkeeping as the op-by-op path (SEAL's exceptions), arithmetic in hefx_linear_transform_plain
    (hoisted: hefx_linear_transform_plain_hoisted, which also checks the keys)."""
    L = ct.parms_id()
    if ct.size() != 2:
        raise ValueError("encrypted size must be 2")
    scale = ev._plain_product_scale(L, ct.scale, U_diagonals, L)
    elts, keys, diag = _native_args(gal_keys, U_diagonals)
    data = native(L, ct.data, diag, elts, keys, **({"hoisted": True} if hoisted else {}))
    return Ciphertext()._set(data, 2, L, scale)


@_kswitch_only
def linear_transforms_plain_many(ev: Evaluator, cts: Sequence[Ciphertext], diag_sets: Sequence[Sequence[Plaintext]],
                                 gal_keys: KSwitchKeys) -> List[Ciphertext]:
    """[Linear_Transform_Plain(cts[t], diag_sets[t], gal_keys) for t] -- INDEPENDENT transforms of one dimension, e.g.
    the sigma transform of ctA and the tau transform of ctB (matrix_multiplication.cpp:22-25).  On the HIP engine they run
    in lockstep behind one call (hefx_linear_transform_plain_many: every dependent launch sequence carries the items of all
    inputs); per input the operations and their order are those of linear_transform_plain -- same bits, which is also what
    every other backend (and mixed shapes) gets from the loop."""
    native = getattr(ev.be, "linear_transform_plain_many", None)
    d = len(diag_sets[0]) if diag_sets else 0
    same = (len(cts) > 1 and len(cts) == len(diag_sets) and all(len(ds) == d for ds in diag_sets)
            and all(c.size() == 2 and c.parms_id() == cts[0].parms_id() for c in cts)
            and len({id(c.data) for c in cts}) == len(cts))
    if native is None or not same or len(cts) > 64:
        return [linear_transform_plain(ev, c, ds, gal_keys) for c, ds in zip(cts, diag_sets)]
    L = cts[0].parms_id()
    scales = [ev._plain_product_scale(L, c.scale, ds, L) for c, ds in zip(cts, diag_sets)]   # SEAL's checks, transform by transform
    elts, keys, flat = _native_args(gal_keys, [p for ds in diag_sets for p in ds])
    outs = native(L, [c.data for c in cts], flat, elts, keys)
    return [Ciphertext()._set(o, 2, L, s) for o, s in zip(outs, scales)]


# ---- baby-step / giant-step form of Linear_Transform_Plain -----------------------------------
# With l = j*n1 + i (i < n1 baby, j < n2 giant):
#   sum_l diag_l (.) rot_l(v)  =  sum_j rot_(j*n1)( sum_i rot_(-j*n1)(diag_l) (.) rot_i(v) )
# so a d x d transform needs n1-1 (hoisted) + n2-1 key switches instead of d-1, and n1+n2-1 Galois keys instead of d
# (d = 1000: 63 and 64 against 999 and 1000), at the price of diagonals that are rotated in the clear before they
# are encoded.  A different operation sequence than helper.h:237-262, so NOT its noise bits: same decryption, checked
# bit-for-bit against the same composition on the oracle-backed twin.
def bsgs_split(d: int, n1: int = None):
    """(n1, n2) with n1*n2 >= d; default n1 = ceil(sqrt(d))"""
    if n1 is None:
        n1 = max(1, int(np.ceil(np.sqrt(d))))
    return n1, (d + n1 - 1) // n1


def bsgs_steps(d: int, n1: int = None) -> List[int]:
    """rotation steps the transform needs direct Galois keys for (keygen.galois_keys(bsgs_steps(d)))"""
    n1, n2 = bsgs_split(d, n1)
    return [-d] + list(range(1, n1)) + [j * n1 for j in range(1, n2)]


def bsgs_diagonals(diagonals: np.ndarray, n1: int = None) -> List[np.ndarray]:
    """diagonals[l] (length d, helper.h:198-209) shifted right by (l // n1) * n1 slots -- what
    linear_transform_plain_bsgs expects, still in the clear; encode each with the ciphertext's scale and level."""
    d = len(diagonals)
    n1, _ = bsgs_split(d, n1)
    out = []
    for l in range(d):
        shift = (l // n1) * n1
        v = np.zeros(shift + d, dtype=np.asarray(diagonals[l]).dtype)
        v[shift:] = diagonals[l]
        out.append(v)
    return out


@_kswitch_only
def linear_transform_plain_bsgs(ev: Evaluator, ct: Ciphertext, shifted_diagonals: Sequence[Plaintext],
                                gal_keys: KSwitchKeys, n1: int = None, hoisted: bool = True) -> Ciphertext:
    """Linear_Transform_Plain (helper.h:237-262) in baby-step / giant-step form; `shifted_diagonals` are the
    encodings of bsgs_diagonals(...), gal_keys must hold direct keys for bsgs_steps(d, n1).  hoisted=True shares the
    digit decomposition of ct_new over the baby rotations (hefx_rotate_hoisted_batch)."""
    be, L = ev.be, ct.parms_id()
    d = len(shifted_diagonals)
    n1, n2 = bsgs_split(d, n1)
    if d + n1 * n2 > ev.ctx.N // 2:  # the shifted diagonals and the rotated duplicate must not wrap around
        raise ValueError("baby-step/giant-step transform: dimension too large for the slot count")
    native = getattr(be, "linear_transform_plain_bsgs", None)
    if native is not None:  # the HIP engine: the whole composition behind one C-ABI call, same bits as the lines below
        if ct.size() != 2:
            raise ValueError("encrypted size must be 2")
        scale = ev._plain_product_scale(L, ct.scale, shifted_diagonals, L)
        elts, keys, diag = _native_args(gal_keys, shifted_diagonals)
        return Ciphertext()._set(native(L, ct.data, diag, n1, elts, keys, hoisted), 2, L, scale)
    baby = list(range(1, n1))
    elts = _direct_elts(ev, baby + [j * n1 for j in range(1, n2)], gal_keys, "baby-step/giant-step transform")
    ct_new = _duplicate(ev, ct, d, gal_keys)                         # helper.h:244-247
    if hoisted and baby:
        data = be.rotate_hoisted_batch(L, ct_new.data, elts[:n1 - 1], [gal_keys.key(e) for e in elts[:n1 - 1]])
        rots = [ct_new] + [Ciphertext()._set(x, 2, L, ct_new.scale) for x in data]
    else:
        rots = [ct_new] + _rotations_batched(ev, ct_new, baby, gal_keys)
    # inner sums: group j = sum_i rots[i] (.) diag'[j*n1 + i], all groups in one pass
    inner = ev.multiply_plain_sum([rots[l % n1] for l in range(d)], list(shifted_diagonals), group=n1)
    if n2 > 1:
        outs = be.apply_galois_batch(L, [c.data for c in inner[1:]], elts[n1 - 1:],
                                     [gal_keys.key(e) for e in elts[n1 - 1:]])
        inner = inner[:1] + [Ciphertext()._set(x, 2, L, inner[0].scale) for x in outs]
    return ev.add_many(inner)


@_kswitch_only
def linear_transform_cipher(ev: Evaluator, ct: Ciphertext, U_diagonals: Sequence[Ciphertext],
                            gal_keys: KSwitchKeys) -> Ciphertext:
    """Linear_Transform_Cipher, helper.h:212-234: ct x ct products are NOT relinearized (size-3 sum)."""
    d = len(U_diagonals)
    native = getattr(ev.be, "linear_transform_cipher", None)
    if native is not None and d:  # the HIP engine: the whole composition behind one C-ABI call, same bits as below
        return _linear_transform_cipher_native(ev, native, ct, U_diagonals, gal_keys)
    ct_new = _duplicate(ev, ct, d, gal_keys)                         # :216-219
    rots = _rotations_batched(ev, ct_new, list(range(1, d)), gal_keys)
    res = [ev.multiply(ct_new, U_diagonals[0])]                      # :222
    res += [ev.multiply(r, U_diagonals[l + 1]) for l, r in enumerate(rots)]   # :227-228
    return ev.add_many(res)                                          # :231


def _linear_transform_cipher_native(ev: Evaluator, native, ct: Ciphertext, U_diagonals: Sequence[Ciphertext],
                                    gal_keys: KSwitchKeys) -> Ciphertext:
    """The checks of the op-by-op path (SEAL's exceptions: rotate_vector, multiply per diagonal, add_many), arithmetic in
    hefx_linear_transform_cipher; missing keys / too large steps come back from the engine with SEAL's messages.
    One difference in ORDER, as in _linear_transform_plain_native: the operand checks run here, before the engine plans
    the rotations, so an input with two faults -- say a missing Galois key AND a diagonal at another scale -- raises the
    operand's exception where the loop, which rotates first, raises the key's.  Every single fault raises what the loop
    raises."""
    L = ct.parms_id()
    if ct.size() != 2:
        raise ValueError("encrypted size must be 2")
    for u in U_diagonals:                                            # Evaluator::multiply(rotation, diagonal)
        ev._check_same(ct, u)
        if u.size() != 2:
            raise ValueError("multiply: only size-2 operands are supported (all reference call sites)")
        ev._check_scale(ct.scale * u.scale, L)
    scale = ct.scale * U_diagonals[0].scale
    for u in U_diagonals[1:]:                                        # Evaluator::add_many over the products
        if not ev._close(scale, ct.scale * u.scale):
            raise ValueError("scale mismatch")
    elts, keys, diag = _native_args(gal_keys, U_diagonals)
    return Ciphertext()._set(native(L, ct.data, diag, elts, keys), 3, L, scale)


def linear_transform_ciphermatrix_plainvector(ev: Evaluator, pt_rotations: Sequence[Plaintext],
                                              U_diagonals: Sequence[Ciphertext]) -> Ciphertext:
    """Linear_Transform_CipherMatrix_PlainVector, helper.h:265-278."""
    n = len(pt_rotations)                                            # :271 multiply_plain, :275 add_many -- one pass
    return ev.multiply_plain_sum(list(U_diagonals[:n]), list(pt_rotations))[0]


def c_matrix_encode(ev: Evaluator, matrix: Sequence[Ciphertext], gal_keys: KSwitchKeys) -> Ciphertext:
    """C_Matrix_Encode, helper.h:307-322: sum_i rotate(row_i, -i*n)."""
    n = len(matrix)
    rots = [matrix[0].copy()] + [ev.rotate_vector(matrix[i], -i * n, gal_keys) for i in range(1, n)]
    return ev.add_many(rots)


def c_matrix_decode(ev: Evaluator, encoder: CKKSEncoder, matrix: Ciphertext, dimension: int, scale: float,
                    gal_keys: KSwitchKeys) -> List[Ciphertext]:
    """C_Matrix_Decode, helper.h:325-360: mask row i, rotate it back."""
    out = []
    for i in range(dimension):
        mask = np.zeros(dimension * dimension)
        mask[i * dimension:(i + 1) * dimension] = 1
        row = ev.multiply_plain(matrix, encoder.encode(mask, scale, parms_id=matrix.parms_id()))
        if i:
            ev.rotate_vector_inplace(row, i * dimension, gal_keys)
        out.append(row)
    return out


def cipher_dot_product(ev: Evaluator, ctA: Ciphertext, ctB: Ciphertext, size: int, relin_keys: KSwitchKeys,
                       gal_keys: KSwitchKeys) -> Ciphertext:
    """cipher_dot_product, helper.h:416-502.  The rotate-by-1 chain is inherently sequential and is kept so:
    rotating by i directly would give different noise bits."""
    mult = ev.multiply(ctA, ctB)                                     # :432
    ev.relinearize_inplace(mult, relin_keys)                         # :440
    ev.rescale_to_next_inplace(mult)                                 # :441
    zero_filled = ev.rotate_vector(mult, -size, gal_keys)            # :455
    dup = ev.add(mult, zero_filled)                                  # :464
    for _ in range(1, size):                                         # :472-476
        ev.rotate_vector_inplace(dup, 1, gal_keys)
        ev.add_inplace(mult, dup)
    mult.scale = 2.0 ** int(np.log2(mult.scale))                     # :489 "manual rescale"
    return mult


def compute_all_powers(ev: Evaluator, ct: Ciphertext, degree: int, relin_keys: KSwitchKeys) -> List[Ciphertext]:
    """compute_all_powers, helper.h:505-547 (= polynomial.cpp:56-96): x^i = x^cand * x^(i-cand), minimal depth."""
    powers: List[Ciphertext] = [None] * (degree + 1)
    powers[1] = ct
    levels = [0] * (degree + 1)
    for i in range(2, degree + 1):
        minimum, cand = i, -1
        for j in range(1, i // 2 + 1):
            k = i - j
            newlevel = max(levels[j], levels[k]) + 1
            if newlevel < minimum:
                cand, minimum = j, newlevel
        levels[i] = minimum
        a, b = powers[cand].copy(), powers[i - cand].copy()
        target = min(a.parms_id(), b.parms_id())
        ev.mod_switch_to_inplace(a, target)                          # :537
        ev.mod_switch_to_inplace(b, target)
        p = ev.multiply(a, b)                                        # :539
        ev.relinearize_inplace(p, relin_keys)                        # :541
        ev.rescale_to_next_inplace(p)                                # :543
        powers[i] = p
    return powers


def _zero_like(ev: Evaluator, ct: Ciphertext) -> Ciphertext:
    """the zero ciphertext at ct's size / level / scale (a rank's contribution when it owns no unit)"""
    return ev.sub(ct, ct)


def _matmul_step3(ev: Evaluator, ctA0: Ciphertext, ctB0: Ciphertext, ctAk: List[Ciphertext],
                  ctBk: List[Ciphertext], include_ab: bool = True) -> Ciphertext:
    """matrix_multiplication.cpp:69-129: rescale the transforms, A0*B0 + sum_k A_k*B_k -- or one rank's share of that sum
    (parallel.py): ctAk / ctBk are the transforms this rank owns, and include_ab says whether A0*B0 is counted here (the
    serial product: all n-1 and True).  The rescales are independent, so they are one launch over their list; the products
    and the chain of add_inplace (:127-128) are one fused sum (Evaluator.multiply_sum: no product is written) to which
    ctAB is added -- canonical residues of the same integers, hence the same bits.  Every product is held to ctAB's
    level and scale HERE, whether or not ctAB is counted, so that a mismatch raises on every rank before any of them
    enters the all-reduce; the share carries ctAB's scale, as the serial sum carries its first addend's."""
    ev.rescale_to_next_many_inplace(list(ctAk) + list(ctBk))         # :69-73 (one launch pair over both families)
    ctAB = ev.multiply(ctA0, ctB0)                                   # :104
    ev.mod_switch_to_next_inplace(ctAB)                              # :112
    for c in ctAk + ctBk:
        c.scale = 2.0 ** int(np.log2(c.scale))                       # :117-121 "manual rescale"
    for a, b in zip(ctAk, ctBk):                                     # add_inplace(ctAB, A_k * B_k), :127-128
        ev._check_same(ctAB, a)
        if not ev._close(ctAB.scale, a.scale * b.scale):
            raise ValueError("scale mismatch")
    if not ctAk:
        return ctAB if include_ab else _zero_like(ev, ctAB)
    share = ev.multiply_sum(ctAk, ctBk)[0]                           # :123-129 (products and their sum in one pass)
    share.scale = ctAB.scale
    return ev.add(ctAB, share) if include_ab else share


def _linear_transforms_of_one_input(ev: Evaluator, ct: Ciphertext, diag_sets: Sequence[Sequence[Plaintext]],
                                    gal_keys: KSwitchKeys) -> List[Ciphertext]:
    """[Linear_Transform_Plain(ct, diags, gal_keys) for diags in diag_sets] (matrix_multiplication.cpp:40-43: the n-1
    transforms V_k of ctA0, W_k of ctB0).  Every one of them starts by forming the same ct_new = ct + rotate(ct, -d)
    and the same rotations rotate(ct_new, l) -- deterministic functions of ct -- so they are formed ONCE and each
    transform keeps only its sum of plaintext products (helper.h:250-259) -- the bits of the transform-by-transform
    loop with (n-1)x fewer key switches."""
    return _linear_transforms_of_inputs(ev, [ct], [diag_sets], gal_keys)[0]


def _linear_transforms_of_inputs(ev: Evaluator, cts: Sequence[Ciphertext],
                                 diag_sets_per_input: Sequence[Sequence[Sequence[Plaintext]]],
                                 gal_keys: KSwitchKeys) -> List[List[Ciphertext]]:
    """[_linear_transforms_of_one_input(ct, sets) for ct, sets] with the rotations of ALL inputs formed together
    (matrix_multiplication.cpp:40-43: the V_k of ctA0 and the W_k of ctB0 are independent of one another): the -d rotations
    as one batch, the rotation forests in one call, every plaintext product and sum in one pass.  Per input the same
    operations in the same order: same bits.  Several inputs run together where the backend has the forest entry and all
    transforms have one dimension, else one by one; one input whose transforms differ in dimension runs them one by one."""
    ds = {len(x) for s in diag_sets_per_input for x in s}
    together = len(cts) > 1 and all(diag_sets_per_input) and len(diag_sets_per_input) == len(cts) and len(ds) == 1 and \
        hasattr(ev.be, "apply_galois_forest")
    if len(cts) > 1 and not together:
        return [_linear_transforms_of_one_input(ev, c, s, gal_keys) for c, s in zip(cts, diag_sets_per_input)]
    if len(ds) != 1:
        return [[linear_transform_plain(ev, c, x, gal_keys) for x in s] for c, s in zip(cts, diag_sets_per_input)]
    d = ds.pop()
    if together:
        dup = _rotations_of_many(ev, cts, [-d], gal_keys)             # helper.h:244
        ct_news = [ev.add(c, r[0]) for c, r in zip(cts, dup)]         # :247
    else:
        ct_news = [_duplicate(ev, cts[0], d, gal_keys)]               # :244-247
    rots = _rotations_of_many(ev, ct_news, list(range(1, d)), gal_keys)   # :255
    terms_ct, terms_pt, counts = [], [], []
    for ct_new, rr, sets in zip(ct_news, rots, diag_sets_per_input):
        full = [ct_new] + rr
        terms_ct += [full[l] for _ in sets for l in range(d)]
        terms_pt += [s[l] for s in sets for l in range(d)]
        counts.append(len(sets))
    sums = ev.multiply_plain_sum(terms_ct, terms_pt, group=d)          # :250, :256, :259
    out, at = [], 0
    for k in counts:
        out.append(sums[at:at + k])
        at += k
    return out


def cc_matrix_multiplication(ev: Evaluator, ctA: Ciphertext, ctB: Ciphertext, dimension: int,
                             U_sigma: Sequence[Plaintext], U_tau: Sequence[Plaintext],
                             V_diagonals: Sequence[Sequence[Plaintext]], W_diagonals: Sequence[Sequence[Plaintext]],
                             gal_keys: KSwitchKeys) -> Ciphertext:
    """CC_Matrix_Multiplication, /root/reference/matrix_multiplication.cpp:11-132 (Jiang et al. 2018/1041)."""
    # Step 1's two transforms are independent of one another, and so are Step 2's two families: each pair runs in
    # lockstep (round 6) -- 2 x (1 + NAF depth) dependent launch sequences for the whole product instead of 4 x
    ctA0, ctB0 = linear_transforms_plain_many(ev, [ctA, ctB], [U_sigma, U_tau], gal_keys)    # :22, :25
    if dimension > 1:
        ctAk, ctBk = _linear_transforms_of_inputs(ev, [ctA0, ctB0], [V_diagonals, W_diagonals], gal_keys)   # :42, :43
    else:
        ctAk, ctBk = [], []
    return _matmul_step3(ev, ctA0, ctB0, ctAk, ctBk)


# ---- the matrix product restricted to the non-zero diagonals ------------------------------------
# The permutation matrices of CC_Matrix_Multiplication have 2n-1 (sigma), n (tau), 2 (phi_k) and 1 (psi_k) non-zero
# diagonals out of n^2; the reference adds 1e-8 to every entry (matrix_multiplication.cpp:239-297) so that SEAL does
# not refuse the all-zero ones as transparent, and rotates for all n^2.  Dropping them changes the result by those
# epsilons only (below CKKS noise) -- a fast mode, not the reference's bits: 2n * n^2 rotations become 3n + 3(n-1) - 1.
def matmul_permutation_matrices(n: int):
    """U_sigma, U_tau, [V_k], [W_k] (k = 1..n-1) on the row-major flattening: helper.h:702-851 (get_U_sigma, get_U_tau,
    get_V_k, get_W_k), i.e. sigma, tau, phi^k, psi^k of Jiang et al. 2018/1041."""
    d = n * n
    Us, Ut = np.zeros((d, d)), np.zeros((d, d))
    for i in range(n):
        for j in range(n):
            Us[n * i + j, n * i + (i + j) % n] = 1
            Ut[n * i + j, n * ((i + j) % n) + j] = 1
    V, W = [], []
    for k in range(1, n):
        Vk, Wk = np.zeros((d, d)), np.zeros((d, d))
        for i in range(n):
            for j in range(n):
                Vk[n * i + j, n * i + (j + k) % n] = 1
                Wk[n * i + j, n * ((i + k) % n) + j] = 1
        V.append(Vk)
        W.append(Wk)
    return Us, Ut, V, W


def nonzero_diagonals(U: np.ndarray) -> dict:
    """{l: l-th diagonal (helper.h:175-195)} for the diagonals of U that are not identically zero"""
    n = U.shape[0]
    idx = np.arange(n)
    out = {}
    for l in range(n):
        dg = U[idx, (idx + l) % n]
        if dg.any():
            out[l] = dg
    return out


def matmul_permutation_diagonals(n: int):
    """nonzero_diagonals of the four families of matmul_permutation_matrices(n), built directly from the index maps
    (the dense d x d matrices take 134 MB each at n = 64): ({l: diag} for sigma, for tau, [for phi^k], [for psi^k])"""
    d = n * n

    def collect(entries):
        out = {}
        for r, c in entries:
            out.setdefault((c - r) % d, np.zeros(d))[r] = 1.0
        return dict(sorted(out.items()))

    ij = [(i, j) for i in range(n) for j in range(n)]
    sigma = collect((n * i + j, n * i + (i + j) % n) for i, j in ij)
    tau = collect((n * i + j, n * ((i + j) % n) + j) for i, j in ij)
    phi = [collect((n * i + j, n * i + (j + k) % n) for i, j in ij) for k in range(1, n)]
    psi = [collect((n * i + j, n * ((i + k) % n) + j) for i, j in ij) for k in range(1, n)]
    return sigma, tau, phi, psi


def _sparse_products(ev: Evaluator, ct_new: Ciphertext, terms, gal_keys: KSwitchKeys,
                     hoisted: bool = False) -> List[Ciphertext]:
    """[diag (.) rot_l(ct_new) for (l, diag) in terms], the rotations as one batch (fused with their products);
    hoisted=True shares the digit decomposition of ct_new (direct Galois keys, hefx_rotate_hoisted_batch)"""
    rot = [(i, l, p) for i, (l, p) in enumerate(terms) if l]
    out = [None] * len(terms)
    for i, (l, p) in enumerate(terms):
        if not l:
            out[i] = ev.multiply_plain(ct_new, p)                    # :250
    if hoisted and rot:
        L = ct_new.parms_id()
        elts = _direct_elts(ev, [l for _, l, _ in rot], gal_keys, "hoisted rotation")
        scale = ev._plain_product_scale(L, ct_new.scale, [p for _, _, p in rot], L)
        data = ev.be.rotate_hoisted_batch(L, ct_new.data, elts, [gal_keys.key(x) for x in elts],
                                          [p.data for _, _, p in rot])
        for (i, _, _), x in zip(rot, data):
            out[i] = Ciphertext()._set(x, 2, L, scale)
        return out
    for (i, _, _), c in zip(rot, _rotations_batched(ev, ct_new, [l for _, l, _ in rot], gal_keys,
                                                    [p for _, _, p in rot])):   # :252-257
        out[i] = c
    return out


@_kswitch_only
def linear_transform_plain_sparse(ev: Evaluator, ct: Ciphertext, d: int, diagonals: dict,
                                  gal_keys: KSwitchKeys, hoisted: bool = False) -> Ciphertext:
    """Linear_Transform_Plain (helper.h:237-262) of a d x d matrix given by its non-zero diagonals {l: Plaintext}"""
    if not diagonals:
        raise ValueError("encrypteds cannot be empty")
    if hoisted == 2:  # double hoisting, see _linear_transform_plain_hoisted2: diagonal 0 must be present
        if 0 not in diagonals:
            raise ValueError("double hoisting over a subset of diagonals needs diagonal 0")
        steps = [0] + sorted(l for l in diagonals if l)
        return _linear_transform_plain_hoisted2(ev, ct, d, steps, [diagonals[l] for l in steps], gal_keys)
    ct_new = _duplicate(ev, ct, d, gal_keys)
    return ev.add_many(_sparse_products(ev, ct_new, sorted(diagonals.items()), gal_keys, hoisted))   # :259


def cc_matrix_multiplication_sparse(ev: Evaluator, ctA: Ciphertext, ctB: Ciphertext, dimension: int, U_sigma: dict,
                                    U_tau: dict, V_diagonals: Sequence[dict], W_diagonals: Sequence[dict],
                                    gal_keys: KSwitchKeys, hoisted: bool = False) -> Ciphertext:
    """CC_Matrix_Multiplication (matrix_multiplication.cpp:11-132) over the non-zero diagonals only.  The 2(n-1)
    Step-2 transforms read the same two duplicated ciphertexts, so all their rotations go out as two batches.
    hoisted=True (direct Galois keys for every step) runs the 2n-1 / n rotations of the sigma / tau transforms on one
    shared digit decomposition each; hoisted=2 additionally mods them down once per transform (U_sigma / U_tau then
    hold KEY-LEVEL plaintexts, see _linear_transform_plain_hoisted2; Step 2 stays single-hoisted)."""
    d = dimension * dimension
    ctA0 = linear_transform_plain_sparse(ev, ctA, d, U_sigma, gal_keys, hoisted)   # :22
    ctB0 = linear_transform_plain_sparse(ev, ctB, d, U_tau, gal_keys, hoisted)     # :25
    ctAk = _sparse_transforms_of_one_input(ev, ctA0, d, V_diagonals, gal_keys)     # :42
    ctBk = _sparse_transforms_of_one_input(ev, ctB0, d, W_diagonals, gal_keys)     # :43
    return _matmul_step3(ev, ctA0, ctB0, ctAk, ctBk)


def _sparse_transforms_of_one_input(ev: Evaluator, ct0: Ciphertext, d: int, diag_dicts: Sequence[dict],
                                    gal_keys: KSwitchKeys) -> List[Ciphertext]:
    """[linear_transform_plain_sparse(ct0, d, diags) for diags in diag_dicts] (matrix_multiplication.cpp:40-43 over the
    non-zero diagonals): the transforms read the same duplicated ciphertext, so the rotations they need go out as one
    batch and -- when every transform has the same number of diagonals (phi^k: 2, psi^k: 1) -- all sums in one pass."""
    if not diag_dicts:
        return []
    ct_new = _duplicate(ev, ct0, d, gal_keys)
    terms = [(l, p) for diags in diag_dicts for l, p in sorted(diags.items())]
    counts = {len(diags) for diags in diag_dicts}
    if len(counts) == 1:
        steps = sorted({l for l, _ in terms if l})
        rot = dict(zip(steps, _rotations_batched(ev, ct_new, steps, gal_keys)))
        rot[0] = ct_new
        return ev.multiply_plain_sum([rot[l] for l, _ in terms], [p for _, p in terms], group=counts.pop())
    prods = _sparse_products(ev, ct_new, terms, gal_keys)
    cts, pos = [], 0
    for diags in diag_dicts:
        cts.append(ev.add_many(prods[pos:pos + len(diags)]))
        pos += len(diags)
    return cts


# ---- polynomial evaluation and encrypted logistic regression (logistic_regression_ckks.cpp) -------------------
def tree_cipher(ev: Evaluator, encoder: CKKSEncoder, encryptor, ctx: Ciphertext, degree: int, scale: float,
                coeffs: Sequence[float], relin_keys: KSwitchKeys) -> Ciphertext:
    """Tree_cipher, /root/reference/logistic_regression_ckks.cpp:55-137 (= polynomial.cpp:233-359)."""
    plain = [None if coeffs[i] == 0 else encoder.encode(float(coeffs[i]), scale) for i in range(degree + 1)]  # :71-83
    powers = compute_all_powers(ev, ctx, degree, relin_keys)                                              # :93
    result = encryptor.encrypt(plain[0])                                                                   # :102
    for i in range(1, degree + 1):                                                                         # :110
        ev.mod_switch_to_inplace(plain[i], powers[i].parms_id())                                          # :113
        temp = ev.multiply_plain(powers[i], plain[i])                                                      # :116
        ev.rescale_to_next_inplace(temp)                                                                   # :119
        ev.mod_switch_to_inplace(result, temp.parms_id())                                                  # :122
        result.scale = 2.0 ** int(np.log2(result.scale))                                                   # :126-127
        temp.scale = 2.0 ** int(np.log2(result.scale))
        ev.add_inplace(result, temp)                                                                       # :130
    return result


def horner_cipher(ev: Evaluator, encoder: CKKSEncoder, encryptor, ctx: Ciphertext, degree: int,
                  coeffs: Sequence[float], scale: float, relin_keys: KSwitchKeys) -> Ciphertext:
    """Horner_cipher, /root/reference/logistic_regression_ckks.cpp:139-205."""
    plain = [encoder.encode(float(coeffs[i]), scale) for i in range(degree + 1)]                          # :147-157
    temp = encryptor.encrypt(plain[degree])                                                                # :162
    ctx = ctx.copy()
    for i in range(degree - 1, -1, -1):                                                                    # :168
        if ctx.parms_id() > temp.parms_id():                                                               # :172-182
            ev.mod_switch_to_inplace(ctx, temp.parms_id())
        elif ctx.parms_id() < temp.parms_id():
            ev.mod_switch_to_inplace(temp, ctx.parms_id())
        ev.multiply_inplace(temp, ctx)                                                                     # :184
        ev.relinearize_inplace(temp, relin_keys)                                                           # :187
        ev.rescale_to_next_inplace(temp)                                                                   # :189
        ev.mod_switch_to_inplace(plain[i], temp.parms_id())                                                # :192
        temp.scale = 2.0 ** 40                                                                             # :195 (the reference hard-codes 2^40)
        ev.add_plain_inplace(temp, plain[i])                                                               # :198
    return temp


def evaluate_polynomial(ev: Evaluator, ct: Ciphertext, coeffs: Sequence[float], relin_keys: KSwitchKeys,
                        basis: str = "power", target_scale: Optional[float] = None) -> Ciphertext:
    """sum_i coeffs[i] ct^i (basis "power") or sum_i coeffs[i] T_i(ct) ("chebyshev", slots in [-1, 1]) in
    ceil(log2(degree + 1)) levels: the Paterson-Stockmeyer plan of hefx_poly_plan (include/hefx_poly.h) executed step by
    step.  The result has that many rows fewer than ct and carries target_scale (default: ct's scale) as the plan states
    it -- scales are tracked through every product and rescale, never overwritten.  MUL: mod_switch_to the lower level,
    multiply, relinearize; COMBINE: Evaluator.scalar_combine (one fused pass on the HIP engine) and rescale_to_next;
    ADD: add.  Not the reference's Horner_cipher / Tree_cipher and not their bits: those stay as they are."""
    return _run_plan(ev, [ct], coeffs, relin_keys, basis, target_scale, lazy=False, batched=False)[0]


def evaluate_polynomial_many(ev: Evaluator, cts: Sequence[Ciphertext], coeffs: Sequence[float], relin_keys: KSwitchKeys,
                             basis: str = "power", target_scale: Optional[float] = None, lazy: bool = True) -> List[Ciphertext]:
    """evaluate_polynomial on n ciphertexts of one level and scale in lockstep: the same unchanged plan (poly.plan), every
    step one batched call over the n items.  lazy=True defers every MUL whose only reader is a COMBINE (and whose result is
    not the plan's) into that COMBINE: relinearisation is linear, so the node  sum_p u_p (a_p * b_p) + sum_k w_k ct_k + c  is
    formed at size 3 by ONE Evaluator.product_combine (hefx_product_combine on the HIP engine) and followed by one
    relinearize_many and one rescale_to_next_many -- plan.relinearizations(True) key switches per item instead of plan.muls
    (12 against 19 at degree 31).  Any other MUL runs as in evaluate_polynomial.  lazy=False gives the words of
    evaluate_polynomial per item; lazy=True gives other words (a sum relinearised once is not the sum of the parts
    relinearised one by one, only the same plaintext) at the same level and scale."""
    return _run_plan(ev, list(cts), coeffs, relin_keys, basis, target_scale, lazy, batched=True)


def _run_plan(ev: Evaluator, cts: List[Ciphertext], coeffs, relin_keys: KSwitchKeys, basis, target_scale, lazy: bool, batched: bool):
    """THE executor of a polynomial plan, on n ciphertexts of one level and scale in lockstep.  batched: every step is one
    batched Evaluator call over the items; else the single-item calls item by item, which one item is faster through."""
    if not cts:
        return []
    if any(c.size() != 2 for c in cts):
        raise ValueError("encrypted size must be 2")
    if any(c.parms_id() != cts[0].parms_id() or c.scale != cts[0].scale for c in cts):
        raise ValueError("evaluate_polynomial_many: the ciphertexts must share one level and one scale")
    plan = _poly.plan(coeffs, basis, ev.ctx.primes[:cts[0].parms_id()], cts[0].scale, target_scale)
    n, deferred = len(cts), plan.deferred() if lazy else {}
    producer = {plan.steps[i].dst: plan.steps[i] for i in deferred}   # slot -> the MUL that was not run
    slots: List[Optional[List[Ciphertext]]] = [None] * plan.nslots
    slots[0] = cts
    for i, st in enumerate(plan.steps):
        if st.op == _poly.MUL:
            if i in deferred:
                continue
            As = [ev.mod_switch_to_inplace(c.copy(), st.level) for c in slots[st.a]]
            # (a square: Evaluator.multiply sees the one payload)
            Bs = As if st.a == st.b else [ev.mod_switch_to_inplace(c.copy(), st.level) for c in slots[st.b]]
            slots[st.dst] = ev.relinearize_many_inplace(ev.multiply_many(As, Bs), relin_keys) if batched else \
                [ev.relinearize_inplace(ev.multiply(a, b), relin_keys) for a, b in zip(As, Bs)]
        elif st.op == _poly.COMBINE:
            products = [(slots[producer[t.src].a], slots[producer[t.src].b], t.coef, t.wscale) for t in st.terms if t.src in producer]
            if products:
                lin = [(slots[t.src], t.coef, t.wscale) for t in st.terms if t.src not in producer]
                outs = ev.product_combine(products, lin, st.constant, scale=st.cscale, parms_id=st.level)
                ev.relinearize_many_inplace(outs, relin_keys)
            else:
                outs = [ev.scalar_combine([slots[t.src][k] for t in st.terms], [[t.coef for t in st.terms]],
                                          [t.wscale for t in st.terms], None if st.constant is None else [st.constant],
                                          scale=st.cscale, parms_id=st.level)[0] for k in range(n)]
            slots[st.dst] = ev.rescale_to_next_many_inplace(outs) if batched else [ev.rescale_to_next_inplace(o) for o in outs]
        else:
            slots[st.dst] = ev.add_pairs(slots[st.a], slots[st.b]) if batched else [ev.add(a, b) for a, b in zip(slots[st.a], slots[st.b])]
    return slots[plan.steps[-1].dst]


# ---- EvalMod and bootstrapping (bootstrap.py plans, these run) -----------------------------------------------------------------
@_kswitch_only
def eval_mod(ev: Evaluator, cts: Sequence[Ciphertext], plan, relin_keys: KSwitchKeys, lazy: bool = True) -> List[Ciphertext]:
    """EvalMod on n ciphertexts in lockstep (the two outputs of CoeffToSlot): slots u = (I + eps) / K' in [-1, 1] become
    sin(2 pi eps), about 2 pi eps.  The Chebyshev interpolant of cos((2 pi K' u - pi / 2) / 2^r) through
    evaluate_polynomial_many, then r double angles cos 2t = 2 cos^2 t - 1, each ONE Evaluator.product_combine (P = 1, a = b,
    weight 2, constant -1), one relinearisation and one rescale: one level each, where the planner would spend two on a
    degree 2.  The weight is the integer 2 at scale 1, so a double angle takes scale s to s^2 / q; the polynomial's target
    scale (plan.poly_target_scale) is the one from which r of them end at plan.scale.  Scales are tracked, never overwritten."""
    return _eval_mod(ev, cts, plan, relin_keys, lazy)


def _eval_mod(ev: Evaluator, cts: Sequence[Ciphertext], plan, relin_keys, lazy: bool) -> List[Ciphertext]:
    """eval_mod's body: it reads relin_keys through Evaluator.relinearize_inplace / relinearize_many_inplace alone"""
    cts = list(cts)
    L = cts[0].parms_id()
    if L != plan.evalmod_level:
        raise ValueError("eval_mod: the ciphertexts are not at the level the plan was made for")
    ys = evaluate_polynomial_many(ev, cts, plan.coeffs, relin_keys, basis="chebyshev",
                                  target_scale=plan.poly_target_scale, lazy=lazy)
    for _ in range(plan.r):
        ys = ev.product_combine([(ys, ys, 2.0, 1.0)], (), -1.0)
        ev.relinearize_many_inplace(ys, relin_keys)
        ev.rescale_to_next_many_inplace(ys)
    return ys


@_kswitch_only
def bootstrap(ev: Evaluator, ct: Ciphertext, plan, gal_keys: KSwitchKeys, relin_keys: KSwitchKeys, encoded=None,
              encaps=None) -> Ciphertext:
    """CKKS bootstrapping with evaluation keys only: a size-2 ciphertext at the last prime q_0 and scale plan.scale comes back
    at level plan.result_level encrypting the same message (to the precision of bootstrap.plan), at plan.scale as a computed
    value.  Evaluator.mod_raise to the top (the plaintext becomes m + q_0 I), coeffs_to_slots with scale / (q_0 K') folded
    into its factor, eval_mod on both outputs in lockstep, slots_to_coeffs with q_0 / (2 pi scale) folded into its factor.
    plan: bootstrap.plan(...) for this context's chain; gal_keys: galois_keys(plan.galois_steps(), conjugate=True); the
    secret key must be sparse enough for plan.K (KeyGenerator(hamming_weight=...)); encoded: plan.encode(encoder).
    A sparse plan (bootstrap.plan(..., slots=ns): the message is ns values tiled over the slots) goes mod_raise, subsum,
    coeffs_to_slots_packed, eval_mod on the ONE ciphertext, slots_to_coeffs_packed; the result is ns-periodic again.
    encaps: KeyGenerator.encapsulation_keys(...) -- sparse-secret encapsulation: the main secret may then be DENSE.  The
    ciphertext is switched to the keys' sparse secret at the last prime (Evaluator.switch_key with encaps.low), raised under
    it and switched back at the top (Evaluator.raise_switch); plan.K is then a matter of the weight of THAT secret, and every
    step after the raise, like the rest of the program, runs under the main one.  None: the path above, bit for bit."""
    if isinstance(encaps, HybridEncapsKeys):
        raise TypeError("bootstrap needs the EncapsKeys of KeyGenerator.encapsulation_keys: HybridEncapsKeys "
                        "(KeyGenerator.hybrid_encapsulation_keys) go with bootstrap_hybrid")
    if ct.size() != 2 or ct.parms_id() != 1:
        raise ValueError("bootstrap: needs a size-2 ciphertext at the last prime")
    if plan.N != ev.ctx.N or list(plan.primes) != list(ev.ctx.primes):
        raise ValueError("bootstrap: the plan was made for another ring or chain")
    if not ev._close(ct.scale, plan.scale):
        raise ValueError("scale mismatch")
    if encoded is None:
        encoded = plan.encode(CKKSEncoder(ev.ctx, device_encode=False))
    if encaps is not None:
        raised = ev.raise_switch(ev.switch_key(ct, encaps.low), encaps, plan.top_level)
    else:
        raised = ev.mod_raise(ct, plan.top_level)
    if plan.sparse_slots is not None:
        x = coeffs_to_slots_packed(ev, subsum(ev, raised, plan.sparse_slots, gal_keys), plan.c2s, gal_keys, encoded[0])
        (y,) = eval_mod(ev, [x], plan, relin_keys)
        return slots_to_coeffs_packed(ev, y, plan.s2c, gal_keys, encoded[1])
    ca, cb = coeffs_to_slots(ev, raised, plan.c2s, gal_keys, encoded[0])
    ya, yb = eval_mod(ev, [ca, cb], plan, relin_keys)
    return slots_to_coeffs(ev, ya, yb, plan.s2c, gal_keys, encoded[1])


# ---- the homomorphic DFT: coefficients to slots and back (dft.py plans, these run) ------------------------------------------
def _dft_rotations(ev: Evaluator, cts: Sequence[Ciphertext], steps: Sequence[int], gal_keys: KSwitchKeys) -> List[Ciphertext]:
    """rotate_vector(cts[i], steps[i]) for every i as one batch of independent key switches; a step of zero is the input.
    Every step needs its direct Galois key (plan.galois_steps())."""
    from .seal import galois_elt_from_step
    jobs = [i for i, s in enumerate(steps) if s]
    elts = [galois_elt_from_step(steps[i], ev.ctx.N) for i in jobs]
    if any(not gal_keys.has_key(e) for e in elts):
        raise ValueError("Galois key not present")
    out = [c.copy() for c in cts]
    if jobs:
        L = cts[0].parms_id()
        datas = ev.be.apply_galois_batch(L, [cts[i].data for i in jobs], elts, [gal_keys.key(e) for e in elts])
        for i, d in zip(jobs, datas):
            out[i] = Ciphertext()._set(d, 2, L, cts[i].scale)
    return out


def _dft_stage(ev: Evaluator, xs: Sequence[Ciphertext], stage, table, gal_keys: KSwitchKeys) -> List[Ciphertext]:
    """One stage of a dft.Plan on its one or two input ciphertexts (dft.Stage states the four modes): the baby rotations of
    every input as one batch, ALL inner sums -- both chains, every giant step -- as one Evaluator.plain_combine, the giant
    rotations as one batch and their sums, one batched rescale.  table[matrix][giant][baby]: plan.encode(...)[stage].
    A packed ("single") stage's few babies of ONE ciphertext take the same apply_galois_batch: rotate_hoisted_batch, which
    shares the digit decomposition at any count, measured within 1.3 % of it at 1 and 7 rotations, L = 14 and L = 4
    (profiles/sparse_bootstrap.json, "baby_rotations")."""
    if len(xs) != stage.inputs or any(x.size() != 2 for x in xs) or len({x.parms_id() for x in xs}) != 1:
        raise ValueError("dft stage: needs %d size-2 ciphertexts of one level" % stage.inputs)
    nb, ng = len(stage.babies), len(stage.giants)
    rots = _dft_rotations(ev, [x for x in xs for _ in stage.babies], list(stage.babies) * len(xs), gal_keys)
    rows = []
    for c in range(stage.outputs):
        for gi in range(ng):
            row = [None] * (len(xs) * nb)
            # (input, matrix) pairs that feed output c
            feeds = {"split": [(0, c)], "lockstep": [(c, 0)], "merge": [(0, 0), (1, 1)], "single": [(0, 0)]}[stage.mode]
            for src, mat in feeds:
                row[src * nb:(src + 1) * nb] = table[mat][gi]
            rows.append(row)
    inner = ev.plain_combine(rots, rows)
    moved = _dft_rotations(ev, inner, list(stage.giants) * stage.outputs, gal_keys)
    outs = [moved[c * ng] if ng == 1 else ev.add_many(moved[c * ng:(c + 1) * ng]) for c in range(stage.outputs)]
    return ev.rescale_to_next_many_inplace(outs)


def _dft_run(ev: Evaluator, xs: List[Ciphertext], plan, gal_keys: KSwitchKeys, encoded) -> List[Ciphertext]:
    """the stages of a dft.Plan in turn on xs; encoded: the plan's plaintexts at the inputs' level (None: made here with a
    host encoder)"""
    if encoded is None:
        encoded = plan.encode(CKKSEncoder(ev.ctx, device_encode=False), xs[0].parms_id())
    for stage, table in zip(plan.stages, encoded):
        xs = _dft_stage(ev, xs, stage, table, gal_keys)
    return xs


@_kswitch_only
def coeffs_to_slots(ev: Evaluator, ct: Ciphertext, plan, gal_keys: KSwitchKeys, encoded=None):
    """CoeffToSlot: (ct_a, ct_b) whose slots hold the coefficients of ct's plaintext, ct_a[i] = m_R(i) / scale and
    ct_b[i] = m_(N/2 + R(i)) / scale (R: bit reversal of the N/2 slot indices, dft.bit_reversal), both plan.levels levels
    below ct and at ct's scale (tracked through every stage, not overwritten).  plan: dft.plan(N, levels, dft.C2S, ...) for
    the primes below ct's level; gal_keys: galois_keys(plan.galois_steps(), conjugate=True); encoded:
    plan.encode(encoder, ct.parms_id()), the plan's plaintexts (made here with a host encoder when not given -- a caller
    that transforms more than once passes them)."""
    from . import dft
    if plan.direction != dft.C2S or plan.N != ev.ctx.N or plan.slots is not None:
        raise ValueError("coeffs_to_slots: the plan is not a CoeffToSlot plan of this ring")
    xs = _dft_run(ev, [ct], plan, gal_keys, encoded)
    return tuple(ev.add(x, ev.complex_conjugate(x, gal_keys)) for x in xs)    # 2 Re(.)


@_kswitch_only
def slots_to_coeffs(ev: Evaluator, ct_a: Ciphertext, ct_b: Ciphertext, plan, gal_keys: KSwitchKeys, encoded=None) -> Ciphertext:
    """SlotToCoeff, the inverse map: from ct_a, ct_b with REAL slots x_a, x_b (in the bit-reversed order coeffs_to_slots
    leaves) the ciphertext whose plaintext has the coefficients scale * x_a[R^-1], scale * x_b[R^-1] -- slots
    F_s..F_1 x_a + D F_s..F_1 x_b -- plan.levels levels lower, at the inputs' scale.  plan: dft.plan(N, levels, dft.S2C, ...);
    gal_keys: galois_keys(plan.galois_steps())."""
    from . import dft
    if plan.direction != dft.S2C or plan.N != ev.ctx.N or plan.slots is not None:
        raise ValueError("slots_to_coeffs: the plan is not a SlotToCoeff plan of this ring")
    return _dft_run(ev, [ct_a, ct_b], plan, gal_keys, encoded)[0]


# ---- sparse packing: a message of ns <= N/4 slots (dft.plan_packed plans, these run) ----------------------------------------
@_kswitch_only
def subsum(ev: Evaluator, ct: Ciphertext, ns: int, gal_keys: KSwitchKeys) -> Ciphertext:
    """SubSum: x <- x + rotate_vector(x, ns 2^i) for i < log2 g, g = N / (2 ns).  The steps generate the Galois group that
    fixes the polynomials in X^g, so a plaintext t becomes g times its coefficients at the multiples of g (the slots: the sum
    of the g values at distance ns, ns-periodic); a plaintext already in that subring becomes g times itself.  log2 g
    dependent key switches, each with its sum in the key switch's epilogue where the backend has that entry
    (rotate_add_chain with one step: acc_in = ct_in); every step needs its direct Galois key."""
    from .seal import galois_elt_from_step
    N = ev.ctx.N
    if ct.size() != 2:
        raise ValueError("encrypted size must be 2")
    if ns < 2 or ns & (ns - 1) or 4 * ns > N:
        raise ValueError("subsum: slots must be a power of two in 2 .. N/4")
    L, x = ct.parms_id(), ct
    fused = getattr(ev.be, "rotate_add_chain", None)
    for i in range((N // (2 * ns)).bit_length() - 1):
        elt = galois_elt_from_step(ns << i, N)
        if not gal_keys.has_key(elt):
            raise ValueError("Galois key not present")
        if fused is not None:
            _, (data,) = fused(L, [x.data], [elt], [gal_keys.key(elt)], [x.data], 1)
            x = Ciphertext()._set(data, 2, L, x.scale)
        else:
            x = ev.add(x, ev.rotate_vector(x, ns << i, gal_keys))
    return x


def _packed_plan(ev: Evaluator, plan, direction: str, name: str):
    if plan.direction != direction or plan.N != ev.ctx.N or plan.slots is None:
        raise ValueError(name + ": the plan is not a packed plan of this direction and ring")


@_kswitch_only
def coeffs_to_slots_packed(ev: Evaluator, ct: Ciphertext, plan, gal_keys: KSwitchKeys, encoded=None) -> Ciphertext:
    """CoeffToSlot of a sparsely packed ciphertext: ct's slots are ns-periodic, z tiled (subsum's result); the ONE result has
    2 ns-periodic real slots [R a | R b] tiled, a and b the halves of the 2 ns coefficients on the stride (times the plan's
    factor), R the bit reversal of ns indices.  Every stage is one matrix on one ciphertext, and 2 Re(.) is ONE conjugation.
    plan: dft.plan_packed(N, ns, levels, dft.C2S, ...); gal_keys: galois_keys(plan.galois_steps(), conjugate=True)."""
    from . import dft
    _packed_plan(ev, plan, dft.C2S, "coeffs_to_slots_packed")
    x = _dft_run(ev, [ct], plan, gal_keys, encoded)[0]
    return ev.add(x, ev.complex_conjugate(x, gal_keys))


@_kswitch_only
def slots_to_coeffs_packed(ev: Evaluator, ct: Ciphertext, plan, gal_keys: KSwitchKeys, encoded=None) -> Ciphertext:
    """SlotToCoeff, the inverse map: from real slots [x_a | x_b] tiled to the ns-periodic slots [z | z] tiled of the plaintext
    with x_a[R^-1], x_b[R^-1] on the stride.  plan: dft.plan_packed(N, ns, levels, dft.S2C, ...)."""
    from . import dft
    _packed_plan(ev, plan, dft.S2C, "slots_to_coeffs_packed")
    return _dft_run(ev, [ct], plan, gal_keys, encoded)[0]


# ---- the homomorphic DFT on hybrid keys: one decomposition per input, one mod-down per inner sum ----------------------------
def _dft_stage_hybrid(ev: Evaluator, xs: Sequence[Ciphertext], stage, table, gal_keys: HybridKeys, hoist_giants: bool = False) -> List[Ciphertext]:
    """_dft_stage on seal.HybridKeys: the baby rotations and ALL inner sums are ONE Evaluator.plain_combine_hoisted (the baby
    step 0 is its identity term), the giant rotations one hybrid_apply_galois_batch (a step of zero is a copy), then the sums
    and one batched rescale.  table[matrix][giant][baby]: plan.encode(..., extended=True)[stage], key-level plaintexts.
    hoist_giants=True: the whole stage is ONE Evaluator.bsgs_hoisted (include/hefx_hybrid_bsgs.h) and the batched rescale -- the
    inner sum (c, gi) gets giant_steps[gi] and dest = c; the inner sums keep the extended basis and every output is rounded
    once, so these are other words with the same values."""
    from .seal import galois_elt_from_step
    if len(xs) != stage.inputs or any(x.size() != 2 for x in xs) or len({x.parms_id() for x in xs}) != 1:
        raise ValueError("dft stage: needs %d size-2 ciphertexts of one level" % stage.inputs)
    nb, ng = len(stage.babies), len(stage.giants)
    rows = []
    for c in range(stage.outputs):
        for gi in range(ng):
            row = [None] * (len(xs) * nb)
            feeds = {"split": [(0, c)], "lockstep": [(c, 0)], "merge": [(0, 0), (1, 1)], "single": [(0, 0)]}[stage.mode]
            for src, mat in feeds:
                row[src * nb:(src + 1) * nb] = table[mat][gi]
            rows.append(row)
    if hoist_giants:
        outs = ev.bsgs_hoisted(xs, list(stage.babies), rows, list(stage.giants) * stage.outputs,
                               [c for c in range(stage.outputs) for _ in range(ng)], gal_keys)
        return ev.rescale_to_next_many_inplace(outs)
    inner = ev.plain_combine_hoisted(xs, list(stage.babies), rows, gal_keys)
    steps = list(stage.giants) * stage.outputs
    jobs = [i for i, s in enumerate(steps) if s]
    elts = [galois_elt_from_step(steps[i], ev.ctx.N) for i in jobs]
    if any(not gal_keys.has_key(e) for e in elts):
        raise ValueError("Galois key not present")
    moved = [c.copy() for c in inner]
    if jobs:
        L = inner[0].parms_id()
        native = getattr(ev.be, "hybrid_apply_galois_batch", None)
        if native is not None:
            datas = native(gal_keys.alpha, L, [inner[i].data for i in jobs], elts, [gal_keys.hybrid_key(e) for e in elts])
        else:
            datas = [ev.apply_galois(inner[i], e, gal_keys).data for i, e in zip(jobs, elts)]
        for i, d in zip(jobs, datas):
            moved[i] = Ciphertext()._set(d, 2, L, inner[i].scale)
    outs = [moved[c * ng] if ng == 1 else ev.add_many(moved[c * ng:(c + 1) * ng]) for c in range(stage.outputs)]
    return ev.rescale_to_next_many_inplace(outs)


def _dft_run_hybrid(ev: Evaluator, xs: List[Ciphertext], plan, gal_keys: HybridKeys, encoded, hoist_giants: bool = False) -> List[Ciphertext]:
    if not isinstance(gal_keys, HybridKeys):
        raise TypeError("the hybrid DFT needs HybridKeys (KeyGenerator.hybrid_galois_keys)")
    if encoded is None:
        encoded = plan.encode(CKKSEncoder(ev.ctx, device_encode=False), xs[0].parms_id(), extended=True)
    for stage, table in zip(plan.stages, encoded):
        xs = _dft_stage_hybrid(ev, xs, stage, table, gal_keys, hoist_giants)
    return xs


def coeffs_to_slots_hybrid(ev: Evaluator, ct: Ciphertext, plan, gal_keys: HybridKeys, encoded=None, hoist_giants: bool = False):
    """coeffs_to_slots on hybrid keys (include/hefx_hybrid_hoist.h): the same plan, the same values, other words -- every
    inner sum is rounded once.  ct at a level <= k - alpha; gal_keys: hybrid_galois_keys(alpha, plan.galois_steps(),
    conjugate=True); encoded: plan.encode(encoder, ct.parms_id(), extended=True)."""
    from . import dft
    if plan.direction != dft.C2S or plan.N != ev.ctx.N or plan.slots is not None:
        raise ValueError("coeffs_to_slots_hybrid: the plan is not a CoeffToSlot plan of this ring")
    xs = _dft_run_hybrid(ev, [ct], plan, gal_keys, encoded, hoist_giants)
    return tuple(ev.add(x, ev.complex_conjugate(x, gal_keys)) for x in xs)    # 2 Re(.)


def slots_to_coeffs_hybrid(ev: Evaluator, ct_a: Ciphertext, ct_b: Ciphertext, plan, gal_keys: HybridKeys, encoded=None, hoist_giants: bool = False) -> Ciphertext:
    """slots_to_coeffs on hybrid keys; gal_keys: hybrid_galois_keys(alpha, plan.galois_steps())"""
    from . import dft
    if plan.direction != dft.S2C or plan.N != ev.ctx.N or plan.slots is not None:
        raise ValueError("slots_to_coeffs_hybrid: the plan is not a SlotToCoeff plan of this ring")
    return _dft_run_hybrid(ev, [ct_a, ct_b], plan, gal_keys, encoded, hoist_giants)[0]


def coeffs_to_slots_packed_hybrid(ev: Evaluator, ct: Ciphertext, plan, gal_keys: HybridKeys, encoded=None, hoist_giants: bool = False) -> Ciphertext:
    """coeffs_to_slots_packed on hybrid keys: one matrix per stage on one ciphertext, one conjugation"""
    from . import dft
    _packed_plan(ev, plan, dft.C2S, "coeffs_to_slots_packed_hybrid")
    x = _dft_run_hybrid(ev, [ct], plan, gal_keys, encoded, hoist_giants)[0]
    return ev.add(x, ev.complex_conjugate(x, gal_keys))


def slots_to_coeffs_packed_hybrid(ev: Evaluator, ct: Ciphertext, plan, gal_keys: HybridKeys, encoded=None, hoist_giants: bool = False) -> Ciphertext:
    """slots_to_coeffs_packed on hybrid keys"""
    from . import dft
    _packed_plan(ev, plan, dft.S2C, "slots_to_coeffs_packed_hybrid")
    return _dft_run_hybrid(ev, [ct], plan, gal_keys, encoded, hoist_giants)[0]


# ---- the bootstrap on hybrid keys -------------------------------------------------------------------------------------------
def subsum_hybrid(ev: Evaluator, ct: Ciphertext, ns: int, gal_keys: HybridKeys) -> Ciphertext:
    """subsum on hybrid keys: the same steps, x <- x + rotate_vector(x, ns 2^i), each a hybrid key switch and an add"""
    if not isinstance(gal_keys, HybridKeys):
        raise TypeError("subsum_hybrid needs HybridKeys (KeyGenerator.hybrid_galois_keys)")
    N = ev.ctx.N
    if ct.size() != 2:
        raise ValueError("encrypted size must be 2")
    if ns < 2 or ns & (ns - 1) or 4 * ns > N:
        raise ValueError("subsum: slots must be a power of two in 2 .. N/4")
    x = ct
    for i in range((N // (2 * ns)).bit_length() - 1):
        x = ev.add(x, ev.rotate_vector(x, ns << i, gal_keys))
    return x


def eval_mod_hybrid(ev: Evaluator, cts: Sequence[Ciphertext], plan, relin_keys: HybridKeys, lazy: bool = True) -> List[Ciphertext]:
    """eval_mod on the hybrid relinearisation key (KeyGenerator.hybrid_relin_keys): the same plan and the same steps; every
    relinearisation is from size 3, a uniform batch of them ONE hefx_hybrid_relinearize_batch."""
    if not isinstance(relin_keys, HybridKeys):
        raise TypeError("eval_mod_hybrid needs HybridKeys (KeyGenerator.hybrid_relin_keys)")
    return _eval_mod(ev, cts, plan, relin_keys, lazy)


BOOTSTRAP_HYBRID_HOIST_GIANTS = False  # the measured default of bootstrap_hybrid (profiles/hybrid_bsgs.json; README, hybrid keys)


def bootstrap_hybrid(ev: Evaluator, ct: Ciphertext, plan, gal_keys: HybridKeys, relin_keys: HybridKeys, encoded=None,
                     hoist_giants: bool = BOOTSTRAP_HYBRID_HOIST_GIANTS, encaps=None) -> Ciphertext:
    """bootstrap on hybrid evaluation keys only, dense and sparse plans: Evaluator.mod_raise to plan.top_level = k - alpha,
    subsum_hybrid (sparse plans), the hybrid CoeffToSlot (packed for sparse plans), eval_mod_hybrid, the hybrid SlotToCoeff.
    plan: bootstrap.plan(..., special=alpha) for this context's chain; gal_keys: hybrid_galois_keys(alpha,
    plan.galois_steps(), conjugate=True); relin_keys: hybrid_relin_keys(alpha); encoded: plan.encode(encoder, extended=True).
    hoist_giants: every DFT stage as ONE Evaluator.bsgs_hoisted (include/hefx_hybrid_bsgs.h) -- other words, the same values.
    encaps: KeyGenerator.hybrid_encapsulation_keys(alpha, ...) -- sparse-secret encapsulation, the main secret may then be
    DENSE: Evaluator.switch_key with encaps.low at the last prime (an ordinary key at q_0 q_(k-1)), then Evaluator.raise_switch
    to plan.top_level (include/ext/hefx_hybrid_encaps.h) in place of mod_raise; nothing else changes.  None: the words above."""
    if not isinstance(gal_keys, HybridKeys) or not isinstance(relin_keys, HybridKeys):
        raise TypeError("bootstrap_hybrid needs HybridKeys (KeyGenerator.hybrid_galois_keys, hybrid_relin_keys)")
    if encaps is not None and not isinstance(encaps, HybridEncapsKeys):
        raise TypeError("bootstrap_hybrid needs the HybridEncapsKeys of KeyGenerator.hybrid_encapsulation_keys: EncapsKeys "
                        "(KeyGenerator.encapsulation_keys) go with bootstrap")
    if ct.size() != 2 or ct.parms_id() != 1:
        raise ValueError("bootstrap: needs a size-2 ciphertext at the last prime")
    if plan.N != ev.ctx.N or list(plan.primes) != list(ev.ctx.primes):
        raise ValueError("bootstrap: the plan was made for another ring or chain")
    if not (plan.special == gal_keys.alpha == relin_keys.alpha):
        raise ValueError(f"bootstrap_hybrid: the plan has {plan.special} special primes, the keys alpha = {gal_keys.alpha} and "
                         f"{relin_keys.alpha}: make the plan with bootstrap.plan(..., special=alpha)")
    if encaps is not None and encaps.high.alpha != plan.special:
        raise ValueError(f"bootstrap_hybrid: the plan has {plan.special} special primes, the encapsulation keys alpha = "
                         f"{encaps.high.alpha}: make them with hybrid_encapsulation_keys(alpha = {plan.special})")
    if not ev._close(ct.scale, plan.scale):
        raise ValueError("scale mismatch")
    if encoded is None:
        encoded = plan.encode(CKKSEncoder(ev.ctx, device_encode=False), extended=True)
    if encaps is not None:
        raised = ev.raise_switch(ev.switch_key(ct, encaps.low), encaps, plan.top_level)
    else:
        raised = ev.mod_raise(ct, plan.top_level)
    if plan.sparse_slots is not None:
        x = coeffs_to_slots_packed_hybrid(ev, subsum_hybrid(ev, raised, plan.sparse_slots, gal_keys), plan.c2s, gal_keys, encoded[0], hoist_giants)
        (y,) = eval_mod_hybrid(ev, [x], plan, relin_keys)
        return slots_to_coeffs_packed_hybrid(ev, y, plan.s2c, gal_keys, encoded[1], hoist_giants)
    ca, cb = coeffs_to_slots_hybrid(ev, raised, plan.c2s, gal_keys, encoded[0], hoist_giants)
    ya, yb = eval_mod_hybrid(ev, [ca, cb], plan, relin_keys)
    return slots_to_coeffs_hybrid(ev, ya, yb, plan.s2c, gal_keys, encoded[1], hoist_giants)


def cipher_dot_product_many(ev: Evaluator, As: Sequence[Ciphertext], Bs: Sequence[Ciphertext], size: int,
                            relin_keys: KSwitchKeys, gal_keys: KSwitchKeys, log_sum: bool = False) -> List[Ciphertext]:
    """len(As) independent cipher_dot_product calls (helper.h:416-502) advanced in lockstep: the rotate-by-1 chain
    inside one dot product is sequential, but the chains of different rows are independent, so every step is ONE
    batched key-switch launch over all rows.  Same calls in the same order per row -> same bits as the loop at
    logistic_regression_ckks.cpp:217-220.

    log_sum=True is a fast mode (not the reference's bits): the window sum sum_{t<size} rot^t(dup) by doubling --
    S(2k) = S(k) + rot^k(S(k)), S(2k+1) = S(2k) + rot^(2k)(dup) -- i.e. about log2(size) rotations instead of size-1
    (size 8: 3 instead of 7).  Slots 0..size-1 hold the same replicated dot product as the reference's chain; slots
    size..2*size-1 differ (they carry one more copy of the products), which no caller reads."""
    be, n = ev.be, len(As)
    if n == 0:  # a rank of a row-sharded prediction that owns no row (parallel.predict_cipher_weights_sharded)
        return []
    mults = ev.multiply_many(As, Bs)                                 # :432
    ev.relinearize_many_inplace(mults, relin_keys)                   # :440
    ev.rescale_to_next_many_inplace(mults)                           # :441
    L = mults[0].parms_id()

    def rotate_all(cts, step):
        plan = ev.rotation_plan(step, gal_keys)
        data = [c.data for c in cts]
        for elt in plan:
            data = be.apply_galois_batch(L, data, [elt] * n, [gal_keys.key(elt)] * n)
        return [Ciphertext()._set(d, 2, L, c.scale) for d, c in zip(data, cts)]

    dups = ev.add_pairs(mults, rotate_all(mults, -size))             # :455, :464
    if log_sum:
        acc, k = dups, 1
        for b in bin(size)[3:]:  # the bits of size below its leading one
            acc, k = ev.add_pairs(acc, rotate_all(acc, k)), 2 * k
            if b == "1":
                acc, k = ev.add_pairs(acc, rotate_all(dups, k)), k + 1
        mults = acc
    else:
        plan1 = ev.rotation_plan(1, gal_keys)
        chain = getattr(be, "rotate_add_chain", None)
        if chain is not None and len(plan1) == 1 and size > 1:
            # :472-476 as ONE engine call (hefx_rotate_add_chain): the same key switches and sums level by level -- the
            # oracle-backed twin of the tests runs the loop below, and the bits agree
            elt, key = plan1[0], gal_keys.key(plan1[0])
            _, sums = chain(L, [c.data for c in dups], [elt] * n, [key] * n, [m.data for m in mults], size - 1)
            mults = [Ciphertext()._set(d, 2, L, m.scale) for d, m in zip(sums, mults)]
        else:
            for _ in range(1, size):                                 # :472-476
                dups = rotate_all(dups, 1)
                mults = ev.add_pairs(mults, dups)
    for m in mults:
        m.scale = 2.0 ** int(np.log2(m.scale))                       # :489 "manual rescale"
    return mults


def _check_step_level(name: str, ev: Evaluator, level: int, operands: Sequence[Ciphertext]):
    """level=s of predict_cipher_weights / lr_gradient: s must leave the step its levels, and every operand is already there"""
    if int(level) != level or not 2 <= level <= ev.ctx.first_parms_id():
        raise ValueError(name + ": level must lie between 2 and the first level")
    if any(c.parms_id() != level for c in operands):
        raise ValueError(name + ": features, labels and weights must already be at level %d" % level)


SIGMOID_COEFFS = {3: [0.5, 1.20069, 0.00001, -0.81562],
                  5: [0.5, 1.53048, 0.00001, -2.3533056, 0.00001, 1.3511295],
                  7: [0.5, 1.73496, 0.00001, -4.19407, 0.00001, 5.43402, 0.00001, -2.50739]}


def predict_cipher_weights(ev: Evaluator, encoder: CKKSEncoder, encryptor, features: Sequence[Ciphertext],
                           weights: Ciphertext, num_weights: int, scale: float, gal_keys: KSwitchKeys,
                           relin_keys: KSwitchKeys, degree: int = 3, log_sum: bool = False,
                           poly: str = "horner", level: Optional[int] = None) -> Ciphertext:
    """predict_cipher_weights, /root/reference/logistic_regression_ckks.cpp:208-266.  log_sum=True: the fast window
    sum of cipher_dot_product_many (same prediction values, not the reference's noise bits).  poly="horner" (default): the
    reference's Horner_cipher, its bits; "ps": the same sigmoid polynomial through evaluate_polynomial --
    ceil(log2(degree + 1)) levels instead of `degree`, the prediction at `scale` with nothing overwritten.
    level=None: the step starts at the first level, as the reference's does.  level=s: it starts at level s (bootstrapped
    weights come back at plan.result_level, far below the top); features and weights must already be there (ValueError)."""
    if poly not in ("horner", "ps"):
        raise ValueError("poly must be 'horner' or 'ps'")
    if level is not None:
        _check_step_level("predict_cipher_weights", ev, level, list(features) + [weights])
    num_rows = len(features)
    results = cipher_dot_product_many(ev, features, [weights] * num_rows, num_weights, relin_keys, gal_keys,
                                      log_sum)                                                             # :220
    # the reference encodes one one-hot mask per row inside the loop (:222-225, 2000 CPU FFTs per iteration); here all
    # masks go through one batched encode (one GPU launch on the HIP engine) -- same plaintexts, same order of use
    # masks go through one batched encode (one GPU launch on the HIP engine) -- same plaintexts, same order of use.
    # Encoding at the level below the top IS encode + mod_switch_to_next (:227): CKKS drops RNS rows, no arithmetic.
    top = ev.ctx.first_parms_id() if level is None else int(level)
    masks = encoder.encode_many(list(np.eye(num_rows)), scale, parms_id=top - 1)                           # :222-227
    lin = ev.multiply_plain_sum(results, masks)[0]                                                         # :229, :233
    ev.relinearize_inplace(lin, relin_keys)                                                                # :237 (no-op)
    ev.rescale_to_next_inplace(lin)                                                                        # :239
    lin.scale = 2.0 ** int(np.log2(lin.scale))                                                             # :242
    coeffs = SIGMOID_COEFFS[degree]                                                                        # :245-262
    if poly == "ps":
        return evaluate_polynomial(ev, lin, coeffs, relin_keys, "power", target_scale=scale)
    return horner_cipher(ev, encoder, encryptor, lin, len(coeffs) - 1, coeffs, scale, relin_keys)         # :264


def lr_gradient(ev: Evaluator, encoder: CKKSEncoder, encryptor, features: Sequence[Ciphertext],
                features_T: Sequence[Ciphertext], labels: Ciphertext, weights: Ciphertext, gal_keys: KSwitchKeys,
                relin_keys: KSwitchKeys, scale: float, degree: int = 3, poly: str = "horner", level: Optional[int] = None):
    """update_weights up to its manual rescale, /root/reference/logistic_regression_ckks.cpp:269-323: everything the
    training step computes before SEAL refuses it at :336.  Returns (gradient, pred_labels): the gradient after :323
    (size 2, one prime left, scale snapped to a power of two) and the operand of the sub at :288.

    Slot j < num_weights of the gradient is sum_i X[i, j] * (sigmoid(z_i) - y_i).  z_i is the dot product the
    reference's window sum leaves in slot i of row i (helper.h:455-476, masked at :222-229): all of X[i] . w for
    i <= num_weights, the terms k >= i - num_weights for the rows after that, nothing from row 2 * num_weights on --
    reproduced, not fixed.  poly: as predict_cipher_weights ("ps" leaves the prediction, and so everything after it,
    degree - ceil(log2(degree + 1)) levels higher).  level: as predict_cipher_weights; features, features_T, labels and
    weights must already be at that level, and the gradient comes out lr_step_levels(degree, poly) - 1 levels below it."""
    num_obs, num_weights = len(features), len(features_T)
    if level is not None:
        _check_step_level("lr_gradient", ev, level, list(features) + list(features_T) + [labels, weights])
    pred = predict_cipher_weights(ev, encoder, encryptor, features, weights, num_weights, scale, gal_keys,
                                  relin_keys, degree, poly=poly, level=level)                               # :282
    labels = labels.copy()
    ev.mod_switch_to_inplace(labels, pred.parms_id())                                                      # :286
    pred_labels = ev.sub(pred, labels)                                                                     # :288
    fT = [f.copy() for f in features_T]
    for f in fT:
        ev.mod_switch_to_inplace(f, pred_labels.parms_id())                                                # :298
    grads = cipher_dot_product_many(ev, fT, [pred_labels] * num_weights, num_obs, relin_keys, gal_keys)    # :299
    masks = encoder.encode_many(list(np.eye(num_weights)), scale, parms_id=grads[0].parms_id())           # :302-308
    gradient = ev.multiply_plain_sum(grads, masks)[0]                                                      # :310, :316
    ev.relinearize_inplace(gradient, relin_keys)                                                           # :319
    ev.rescale_to_next_inplace(gradient)                                                                   # :321
    gradient.scale = 2.0 ** int(np.log2(gradient.scale))                                                   # :323
    return gradient, pred_labels


def update_weights(ev: Evaluator, encoder: CKKSEncoder, encryptor, features: Sequence[Ciphertext],
                   features_T: Sequence[Ciphertext], labels: Ciphertext, weights: Ciphertext, learning_rate: float,
                   gal_keys: KSwitchKeys, relin_keys: KSwitchKeys, scale: float, degree: int = 3) -> Ciphertext:
    """update_weights, /root/reference/logistic_regression_ckks.cpp:269-345.  As committed, the reference cannot
    get past :336 with its own parameters: the gradient is at the last level (one 60-bit prime left) and the
    multiply_plain pushes the scale to 2^80 -> SEAL throws invalid_argument("scale out of bounds").  The mirror
    keeps that behaviour (ValueError from Evaluator._check_scale)."""
    num_obs = len(features)
    gradient, _ = lr_gradient(ev, encoder, encryptor, features, features_T, labels, weights, gal_keys, relin_keys,
                              scale, degree)                                                                # :275-323
    n_pt = encoder.encode(float(learning_rate) / num_obs, scale)                                           # :330-331
    ev.mod_switch_to_inplace(n_pt, gradient.parms_id())                                                    # :333
    ev.multiply_plain_inplace(gradient, n_pt)                                                              # :336  <- SEAL throws here
    new_weights = ev.sub(gradient, weights)                                                                # :341
    ev.negate_inplace(new_weights)                                                                         # :342
    return new_weights


def update_weights_refreshed(ev: Evaluator, encoder: CKKSEncoder, encryptor, decryptor, features: Sequence[Ciphertext],
                             features_T: Sequence[Ciphertext], labels: Ciphertext, weights: Ciphertext,
                             learning_rate: float, gal_keys: KSwitchKeys, relin_keys: KSwitchKeys, scale: float,
                             degree: int = 3, poly: str = "horner") -> Ciphertext:
    """A training step that ends: w - (learning_rate / num_obs) * gradient, at the first level.  A COMPLETION of the
    reference, not a mirror of it: update_weights above stops where SEAL stops (:336), because the gradient arrives with
    one prime left.  The holder of the secret key -- the reference's train_cipher has a Decryptor for exactly this
    (:348-385) -- refreshes the gradient (Decryptor.refresh: decrypt, exact lift, encrypt; no decode / encode), after which
    the reference's own lines go through, plus the rescale they omit.  poly: as lr_gradient."""
    num_obs = len(features)
    gradient, _ = lr_gradient(ev, encoder, encryptor, features, features_T, labels, weights, gal_keys, relin_keys,
                              scale, degree, poly)                                                          # :275-323
    gradient = decryptor.refresh(gradient, encryptor)                  # first level, scale 2^40: room for the product
    n_pt = encoder.encode(float(learning_rate) / num_obs, scale)                                           # :330-331
    ev.mod_switch_to_inplace(n_pt, gradient.parms_id())                                                    # :333
    ev.multiply_plain_inplace(gradient, n_pt)                                                              # :336
    ev.rescale_to_next_inplace(gradient)                               # (omitted by the reference)
    gradient.scale = 2.0 ** int(np.log2(gradient.scale))               # its own idiom, :323
    weights = weights.copy()
    ev.mod_switch_to_inplace(weights, gradient.parms_id())
    new_weights = ev.sub(gradient, weights)                                                                # :341
    ev.negate_inplace(new_weights)                                                                         # :342
    return decryptor.refresh(new_weights, encryptor)                   # back to the first level


def train_cipher(ev: Evaluator, encoder: CKKSEncoder, encryptor, decryptor, features: Sequence[Ciphertext],
                 features_T: Sequence[Ciphertext], labels: Ciphertext, weights: Ciphertext, learning_rate: float,
                 iters: int, gal_keys: KSwitchKeys, relin_keys: KSwitchKeys, scale: float, degree: int = 3,
                 poly: str = "horner") -> Ciphertext:
    """The loop of train_cipher, /root/reference/logistic_regression_ckks.cpp:356-382, over update_weights_refreshed.
    The reference refreshes by decrypt / decode ... encrypt of a last-level plaintext (:362-381) and so could not start
    a second iteration; here every step already returns first-level weights."""
    new_weights = weights                                                                                  # :354
    for _ in range(int(iters)):                                                                            # :356
        new_weights = update_weights_refreshed(ev, encoder, encryptor, decryptor, features, features_T, labels,
                                               new_weights, learning_rate, gal_keys, relin_keys, scale, degree, poly)  # :359
    return new_weights


# ---- training with evaluation keys only: the bootstrap in place of the Decryptor ----------------------------------------------
def lr_step_levels(degree: int, poly: str = "horner") -> int:
    """Levels one whole training step spends, from the level the weights start at to the updated weights: the dot product,
    the row mask, the sigmoid (`degree` levels for "horner", ceil(log2(degree + 1)) for "ps"), the gradient's dot product, the
    weight mask, and the product with learning_rate / num_obs with its rescale.  lr_gradient spends all but the last.  That
    last product needs two primes (its scale is the square of the ciphertext's until the rescale: the reference's throws at
    :336 because its gradient arrives with one), so a step that ends at level 1 starts at level 1 + lr_step_levels(...)."""
    if poly not in ("horner", "ps"):
        raise ValueError("poly must be 'horner' or 'ps'")
    if int(degree) != degree or degree < 1:
        raise ValueError("degree must be a positive integer")
    sigmoid = int(degree) if poly == "horner" else int(degree).bit_length()   # ceil(log2(degree + 1))
    return 1 + 1 + sigmoid + 1 + 1 + 1


def lr_bootstrap_galois_steps(plan, num_obs: int, num_weights: int) -> List[int]:
    """The rotation steps of ONE KeyGenerator.galois_keys(steps, conjugate=True) call for train_cipher_bootstrapped:
    plan.galois_steps() (SubSum -- the update's tiling takes the same steps --, both packed transforms) and the steps of the
    two dot products: 1 for the window sums, -num_weights and -num_obs for their zero-filled copies (helper.h:455)."""
    return sorted(set(plan.galois_steps()) | {1, -int(num_weights), -int(num_obs)})


def _check_bootstrapped_step(ev: Evaluator, plan, num_weights: int, scale: float, degree: int, poly: str) -> int:
    """the refusals of update_weights_bootstrapped that need no ciphertext; returns the level s a step starts at"""
    s = 1 + lr_step_levels(degree, poly)
    if plan.sparse_slots is None:
        raise ValueError("bootstrapped training needs a sparse plan (bootstrap.plan(..., slots=ns))")
    if plan.N != ev.ctx.N or list(plan.primes) != list(ev.ctx.primes):
        raise ValueError("bootstrap: the plan was made for another ring or chain")
    if plan.sparse_slots < num_weights:
        raise ValueError("the plan's %d slots do not hold %d weights" % (plan.sparse_slots, num_weights))
    if plan.result_level < s:
        raise ValueError("the bootstrap returns at level %d and a step needs %d: the chain is too short"
                         % (plan.result_level, s))
    if not ev._close(float(scale), plan.scale):
        raise ValueError("scale mismatch: the plan was made for another scale")
    return s


def update_weights_bootstrapped(ev: Evaluator, encoder: CKKSEncoder, encryptor, features: Sequence[Ciphertext],
                                features_T: Sequence[Ciphertext], labels: Ciphertext, weights: Ciphertext,
                                learning_rate: float, gal_keys: KSwitchKeys, relin_keys: KSwitchKeys, scale: float, plan,
                                degree: int = 3, poly: str = "ps", encoded=None, encaps=None) -> Ciphertext:
    """A training step that ends WITHOUT the secret key: w - (learning_rate / num_obs) * gradient, refreshed by one
    algorithms.bootstrap of the weights where update_weights_refreshed asks the Decryptor twice.  Every operand is at level
    s = 1 + lr_step_levels(degree, poly) and so is the result.

    plan: a sparse bootstrap.plan(N, chain, scale, slots=ns, max_value=...) with ns >= num_weights, plan.result_level >= s and
    max_value at least the largest |weight| the training reaches; encoded: plan.encode(encoder) (made here when None; a loop
    passes it).  gal_keys: galois_keys(lr_bootstrap_galois_steps(plan, num_obs, num_weights), conjugate=True); the secret key
    behind them is the sparse one bootstrap() needs.  ValueError before anything is submitted when the plan is dense, holds
    fewer slots than weights, returns below s or was made for another scale or chain, or when an operand is not at level s.

    THE INVARIANT: `weights` is ns-periodic -- its ns values tiled over the N / 2 slots (encode np.tile(w, N / 2 / ns)) --
    and so is the result.  The feature rows stay zero-padded, so the dot product's products vanish outside the first block
    and the tiling changes no value the step reads.  The gradient lives in the first block alone; subsum of a message
    confined to one block IS its tiling (log2(N / 2 ns) key switches at one prime), after which the reference's sub and negate
    (:341-342) keep the period and bootstrap() finds the subring it expects.  poly: "ps" by default -- Horner_cipher
    hard-codes the scale 2^40 (:195), at which no bootstrap chain of this engine keeps its precision.
    encaps: passed to bootstrap() -- with KeyGenerator.encapsulation_keys the secret behind every key may be dense."""
    num_obs, num_weights = len(features), len(features_T)
    s = _check_bootstrapped_step(ev, plan, num_weights, scale, degree, poly)
    _check_step_level("update_weights_bootstrapped", ev, s, list(features) + list(features_T) + [labels, weights])
    if not ev._close(weights.scale, plan.scale):
        raise ValueError("scale mismatch: the weights are not at the plan's scale")
    if encoded is None:
        encoded = plan.encode(encoder)
    gradient, _ = lr_gradient(ev, encoder, encryptor, features, features_T, labels, weights, gal_keys, relin_keys,
                              scale, degree, poly, level=s)            # :275-323, at level 2: room for the product
    new_weights = _update_and_tile(ev, encoder, gradient, weights, float(learning_rate) / num_obs, scale,
                                   plan.sparse_slots, gal_keys)
    fresh = bootstrap(ev, new_weights, plan, gal_keys, relin_keys, encoded, encaps)
    return ev.mod_switch_to_inplace(fresh, s)


def _update_and_tile(ev: Evaluator, encoder: CKKSEncoder, gradient: Ciphertext, weights: Ciphertext, rate: float,
                     scale: float, ns: int, gal_keys: KSwitchKeys) -> Ciphertext:
    """weights - rate * gradient at the last prime, ns-periodic: the gradient (level 2, first block only) times the encoded
    rate, rescaled, tiled by subsum; the weights (ns-periodic, any level) mod-switched down; the reference's sub and negate"""
    gradient = gradient.copy()
    n_pt = encoder.encode(rate, scale)                                                                     # :330-331
    ev.mod_switch_to_inplace(n_pt, gradient.parms_id())                                                    # :333
    ev.multiply_plain_inplace(gradient, n_pt)                                                              # :336
    ev.rescale_to_next_inplace(gradient)                               # (omitted by the reference)
    gradient.scale = 2.0 ** int(np.log2(gradient.scale))               # its own idiom, :323
    delta = subsum(ev, gradient, ns, gal_keys)                         # first block -> every block
    weights = weights.copy()
    ev.mod_switch_to_inplace(weights, delta.parms_id())
    new_weights = ev.sub(delta, weights)                                                                   # :341
    ev.negate_inplace(new_weights)                                                                         # :342
    return new_weights


def train_cipher_bootstrapped(ev: Evaluator, encoder: CKKSEncoder, encryptor, features: Sequence[Ciphertext],
                              features_T: Sequence[Ciphertext], labels: Ciphertext, weights: Ciphertext,
                              learning_rate: float, iters: int, gal_keys: KSwitchKeys, relin_keys: KSwitchKeys,
                              scale: float, plan, degree: int = 3, poly: str = "ps", encoded=None, encaps=None) -> Ciphertext:
    """train_cipher with evaluation keys only: `iters` times update_weights_bootstrapped, one bootstrap per iteration.
    Features, transposed features, labels and the initial weights (tiled: see update_weights_bootstrapped) may sit at any
    level from s = 1 + lr_step_levels(degree, poly) up and are mod-switched to s ONCE, here; the plan's plaintexts are
    encoded once.  The result is at level s, ns-periodic.  encaps: passed to every step's bootstrap()."""
    s = _check_bootstrapped_step(ev, plan, len(features_T), scale, degree, poly)
    operands = list(features) + list(features_T) + [labels, weights]
    if any(c.parms_id() < s for c in operands):
        raise ValueError("train_cipher_bootstrapped: features, labels and weights must be at level %d or above" % s)
    if not ev._close(weights.scale, plan.scale):
        raise ValueError("scale mismatch: the weights are not at the plan's scale")
    if encoded is None:
        encoded = plan.encode(encoder)
    features, features_T, labels, new_weights = ([ev.mod_switch_to_inplace(c.copy(), s) for c in features],
                                                 [ev.mod_switch_to_inplace(c.copy(), s) for c in features_T],
                                                 ev.mod_switch_to_inplace(labels.copy(), s),
                                                 ev.mod_switch_to_inplace(weights.copy(), s))
    for _ in range(int(iters)):
        new_weights = update_weights_bootstrapped(ev, encoder, encryptor, features, features_T, labels, new_weights,
                                                  learning_rate, gal_keys, relin_keys, scale, plan, degree, poly, encoded, encaps)
    return new_weights
