"""Host-only planner of the homomorphic DFT: CoeffToSlot and SlotToCoeff as `levels` sparse-diagonal matrix products
("Coefficients to slots and back").  Nothing here touches a device; algorithms.coeffs_to_slots and
algorithms.slots_to_coeffs run a plan.

Slot order is the encoder's, slot i <-> root zeta^(3^i), zeta = exp(2 pi i / 2N).  With n = N/2, r_j = 3^j mod 2N and
U[j][i] = zeta^(r_j i) (n x N, the decoding matrix), U = [U0 | U1]:
    U1 = D U0,   D = diag(i (-1)^j)              (generator 5 would give D = i I)
    U0 = F_s ... F_1 R,   s = log2 n             (R: bit reversal of the n indices; F_t: the butterfly factor of length 2^t)
and for REAL coefficients m = (a; b) and slots z = U m
    R a = 2 Re( (1/N) F_1^H ... F_s^H z ),   R b = 2 Re( (1/N) F_1^H ... F_s^H D^H z ),   z = F_s..F_1 (R a) + D F_s..F_1 (R b).
U0 is NOT a scaled unitary for generator 3 (U0^H U0 has entries at distance N/4 from the diagonal), which is why both
directions carry two chains of the same stage matrices and only the stage next to D differs between them.

Matrices are kept as {cyclic diagonal index: vector}: M[i][(i + d) mod n] = diag_d[i], so M x = sum_d diag_d * roll(x, -d) and
roll(x, -d) is rotate_vector(ct, d).  Nothing dense is ever formed, so a plan at N = 32768 costs what its diagonals cost."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

C2S, S2C = "coeffs_to_slots", "slots_to_coeffs"
Diags = Dict[int, np.ndarray]


# ---- the algebra of matrices given by cyclic diagonals ----------------------------------------------------------------------
def butterfly_factor(N: int, t: int) -> Diags:
    """F_t, 1 <= t <= log2(N/2): block diagonal in len x len blocks, len = 2^t; for j < len/2 rows j and j + len/2 of a block are
    (1, zeta^((r_j mod 4 len) M / (4 len))) and (1, zeta^((r_(j+len/2) mod 4 len) M / (4 len))) in columns j and j + len/2.
    (3^len = 1 mod 4 len, so the block's own row index and the global one give the same twiddle.)"""
    n, M = N // 2, 2 * N
    length, h = 1 << t, 1 << (t - 1)
    r = np.array([pow(3, j, M) for j in range(n)], dtype=np.int64)
    tw = np.exp(2j * np.pi * ((r % (4 * length)) * (M // (4 * length))) / M)
    low = (np.arange(n) % length) < h
    out: Diags = {}
    for d, v in ((0, np.where(low, 1.0, tw)), (h % n, np.where(low, tw, 0.0)), ((-h) % n, np.where(low, 0.0, 1.0))):
        out[d] = out.get(d, 0) + v.astype(np.complex128)
    return out


def matmul(A: Diags, B: Diags) -> Diags:
    """A B: (A B)_(a+b) += A_a * roll(B_b, -a)"""
    n = len(next(iter(A.values())))
    out: Diags = {}
    for a, va in A.items():
        for b, vb in B.items():
            d = (a + b) % n
            out[d] = out.get(d, 0) + va * np.roll(vb, -a)
    return {d: v for d, v in out.items() if v.any()}   # (structural zeros multiply and add to exact zeros)


def hermitian(A: Diags) -> Diags:
    n = len(next(iter(A.values())))
    return {(-d) % n: np.roll(np.conj(v), d) for d, v in A.items()}


def right_diagonal(A: Diags, g: np.ndarray) -> Diags:
    """A diag(g)"""
    return {d: v * np.roll(g, -d) for d, v in A.items()}


def left_diagonal(g: np.ndarray, A: Diags) -> Diags:
    """diag(g) A"""
    return {d: g * v for d, v in A.items()}


def dense(A: Diags) -> np.ndarray:
    """the n x n matrix of a diagonal set (tests and small sizes only)"""
    n = len(next(iter(A.values())))
    out = np.zeros((n, n), dtype=np.complex128)
    i = np.arange(n)
    for d, v in A.items():
        out[i, (i + d) % n] = v
    return out


def bit_reversal(n: int) -> np.ndarray:
    bits = n.bit_length() - 1
    return np.array([int(format(i, f"0{bits}b")[::-1], 2) if bits else 0 for i in range(n)], dtype=np.int64)


def d_vector(n: int) -> np.ndarray:
    """the diagonal of D: i (-1)^j"""
    return 1j * (-1.0) ** np.arange(n)


# ---- the baby-step / giant-step split ----------------------------------------------------------------------------------
def split(indices: Sequence[int], n: int, stride: int):
    """(babies, giants, pairs): every index is giant + baby (mod n) for exactly one (giant, baby) of `pairs`.  Babies are
    multiples k * stride, 0 <= k < nb; giants are the greedy cover of the indices by windows of nb strides, walked round the
    cycle from one of the indices (every one is tried up to 64 indices, beyond that the one after the widest cyclic gap).
    The walk and the nb kept are those that need the fewest rotations: the nonzero babies that occur plus the nonzero giants."""
    period = n // stride
    if any(d % stride for d in indices):
        raise ValueError("split: an index is not a multiple of the stride")
    ks = sorted({(d % n) // stride for d in indices})
    if len(ks) <= 64:
        starts = ks
    else:
        gaps = [((ks[(i + 1) % len(ks)] - k) % period or period, (i + 1) % len(ks)) for i, k in enumerate(ks)]
        starts = [ks[max(gaps)[1]]]
    best = None
    for start in starts:
        rel = sorted((k - start) % period for k in ks)
        for nb in range(1, rel[-1] + 2):
            giants, pairs, edge = [], [], -1
            for k in rel:
                if k > edge:
                    giants.append(k)
                    edge = k + nb - 1
                pairs.append((giants[-1], k - giants[-1]))
            cost = len({b for _, b in pairs} - {0}) + sum(1 for g in giants if (start + g) % period)
            if best is None or cost < best[0]:
                best = (cost, start, giants, pairs)
    _, start, giants, pairs = best
    to_index = lambda g: ((start + g) % period) * stride
    return (sorted({b * stride for _, b in pairs}), [to_index(g) for g in giants],
            {(to_index(g), b * stride) for g, b in pairs})


class Stage:
    """One level of the transform: `mats` (one matrix, or two where the stage touches D) over the same diagonal indices, the
    split, and the prime its rescale drops.
      mode "split"     one input, two outputs:  out_c = mats[c] x             (CoeffToSlot's first stage: F^H and F^H D^H)
      mode "lockstep"  two inputs, two outputs: out_c = mats[0] x_c
      mode "merge"     two inputs, one output:  out = mats[0] x_0 + mats[1] x_1   (SlotToCoeff's last stage: F and D F)
      mode "single"    one input, one output:   out = mats[0] x               (every stage of a packed plan, plan_packed)
    n is the period of the diagonals: the slot count, or 2 ns in a packed plan, whose vectors are n-periodic and longer."""

    def __init__(self, mode: str, mats: List[Diags], n: int, stride: int, prime: int):
        self.mode, self.mats, self.n, self.stride, self.prime = mode, mats, n, stride, int(prime)
        self.indices = sorted(set().union(*[set(m) for m in mats]))
        self.babies, self.giants, self.pairs = split(self.indices, n, stride)
        self.inputs = 1 if mode in ("split", "single") else 2
        self.outputs = 1 if mode in ("merge", "single") else 2

    def rotated(self, mat: int, giant: int, baby: int) -> Optional[np.ndarray]:
        """diagonal giant + baby of mats[mat], rotated by minus its giant step; None: a structural zero"""
        v = self.mats[mat].get((giant + baby) % self.n) if (giant, baby) in self.pairs else None
        return None if v is None else np.roll(v, giant)

    def scale(self) -> float:
        """the scale the diagonals are encoded at: the prime the stage's rescale drops, so the ciphertext's scale goes through
        the stage unchanged (tracked, not overwritten)"""
        return float(self.prime)

    def key_switches(self) -> int:
        return self.inputs * sum(1 for b in self.babies if b) + self.outputs * sum(1 for g in self.giants if g)

    def apply(self, xs: Sequence[np.ndarray]) -> List[np.ndarray]:
        """the stage in its baby/giant form on plain vectors (numpy rolls for rotations): what the ciphertexts go through.
        Vectors longer than the period meet the diagonals tiled, as the encoded plaintexts are."""
        rots = [[np.roll(x, -b) for b in self.babies] for x in xs]
        reps = len(xs[0]) // self.n
        outs = []
        for c in range(self.outputs):
            acc = 0
            for g in self.giants:
                inner = 0
                for src in range(len(xs)) if self.mode == "merge" else [c if self.mode == "lockstep" else 0]:
                    mat = src if self.mode == "merge" else (c if self.mode == "split" else 0)
                    for bi, b in enumerate(self.babies):
                        v = self.rotated(mat, g, b)
                        if v is not None:
                            inner = inner + (v if reps == 1 else np.tile(v, reps)) * rots[src][bi]
                acc = acc + np.roll(inner, -g)
            outs.append(acc)
        return outs


class Plan:
    def __init__(self, N: int, levels: int, direction: str, stages: List[Stage], factor, slots: Optional[int] = None):
        self.N, self.n, self.levels, self.direction, self.stages, self.factor = N, N // 2, levels, direction, stages, factor
        self.slots = slots   # None: the dense plan of plan(); ns: the packed plan of plan_packed(), all stages "single"

    def galois_steps(self) -> List[int]:
        """every rotation step the plan needs a direct Galois key for (CoeffToSlot needs the conjugation key on top:
        KeyGenerator.galois_keys(plan.galois_steps(), conjugate=True))"""
        return sorted({s for st in self.stages for s in st.babies + st.giants if s})

    def key_switches(self) -> int:
        """key switches of one run: the rotations of every stage, and CoeffToSlot's conjugation of every output (two; one
        in a packed plan)"""
        return sum(st.key_switches() for st in self.stages) + (self.stages[-1].outputs if self.direction == C2S else 0)

    def primes(self) -> List[int]:
        return [st.prime for st in self.stages]

    def apply(self, xs: Sequence[np.ndarray]) -> List[np.ndarray]:
        """the whole plan on plain vectors, conjugation included: [R a, R b] from [z], or [z] from [R a, R b]; a packed
        plan takes and gives ONE vector of N / 2 values, [R a | R b] tiled from [z | z] tiled or the reverse"""
        for st in self.stages:
            xs = st.apply(xs)
        return [x + np.conj(x) for x in xs] if self.direction == C2S else list(xs)

    def encode(self, encoder, parms_id: int, extended: bool = False):
        """[stage][matrix][giant][baby] -> Plaintext or None: the pre-rotated diagonals, stage i at level parms_id - i and
        scale float(q) of the prime that level's rescale drops.  The context's chain must be the one the plan was made for.
        extended: every diagonal is encoded with all k rows, a KEY-LEVEL plaintext (what Evaluator.plain_combine_hoisted
        reads: the rows of the stage's level and the special rows); the stage levels are checked as before."""
        primes = encoder.ctx.primes
        out = []
        for i, st in enumerate(self.stages):
            L = parms_id - i
            if L < 2 or primes[L - 1] != st.prime:
                raise ValueError("dft plan: the chain below parms_id does not drop the primes the plan was made for")
            todo = [(c, gi, bi, st.rotated(c, g, b)) for c in range(len(st.mats)) for gi, g in enumerate(st.giants)
                    for bi, b in enumerate(st.babies)]
            todo = [t for t in todo if t[3] is not None]
            reps = self.n // st.n   # (a packed plan's diagonals have period 2 ns: tiled over the N / 2 slots)
            pts = encoder.encode_many([t[3] if reps == 1 else np.tile(t[3], reps) for t in todo], st.scale(), encoder.ctx.k if extended else L)
            table = [[[None] * len(st.babies) for _ in st.giants] for _ in st.mats]
            for (c, gi, bi, _), p in zip(todo, pts):
                table[c][gi][bi] = p
            out.append(table)
        return out


def plan(N: int, levels: int, direction: str, primes_of_the_stages: Sequence[int], factor=1.0) -> Plan:
    """The transform of `direction` (dft.C2S or dft.S2C) in `levels` stages: the s = log2(N/2) butterfly factors in runs of
    adjacent factors, sizes as equal as possible (the longer runs first); 1/N (CoeffToSlot) and `factor` folded evenly into
    the stages; D^H folded into CoeffToSlot's first stage, D into SlotToCoeff's last.  primes_of_the_stages[i]: the prime
    stage i's rescale drops (the input's last prime first); more than `levels` of them may be given."""
    if N < 4 or N & (N - 1):
        raise ValueError("dft plan: N must be a power of two, at least 4")
    n = N // 2
    s = n.bit_length() - 1
    if direction not in (C2S, S2C):
        raise ValueError("dft plan: direction must be dft.C2S or dft.S2C")
    if not 1 <= int(levels) <= s:
        raise ValueError(f"dft plan: levels must lie in 1 .. {s}")
    levels = int(levels)
    if len(primes_of_the_stages) < levels:
        raise ValueError("dft plan: not enough primes: every stage drops one")
    # the factors in the order they are applied: F_s^H .. F_1^H (CoeffToSlot), F_1 .. F_s (SlotToCoeff)
    order = list(range(s, 0, -1)) if direction == C2S else list(range(1, s + 1))
    sizes = [s // levels + (1 if i < s % levels else 0) for i in range(levels)]
    total = complex(factor) * (1.0 / N if direction == C2S else 1.0)
    per_stage = total ** (1.0 / levels) if total.imag or total.real < 0 else total.real ** (1.0 / levels)
    stages, at = [], 0
    for i, size in enumerate(sizes):
        run = order[at:at + size]
        at += size
        M = None
        for t in run:
            F = butterfly_factor(N, t)
            F = hermitian(F) if direction == C2S else F
            M = F if M is None else matmul(F, M)
        M = {d: v * per_stage for d, v in M.items()}
        stride = 1 << (min(run) - 1)
        if direction == C2S and i == 0:
            mode, mats = "split", [M, right_diagonal(M, np.conj(d_vector(n)))]
        elif direction == S2C and i == levels - 1:
            mode, mats = "merge", [M, left_diagonal(d_vector(n), M)]
        else:
            mode, mats = "lockstep", [M]
        stages.append(Stage(mode, mats, n, stride, primes_of_the_stages[i]))
    return Plan(N, levels, direction, stages, factor)


# ---- packed plans: a message of ns <= N/4 slots, both halves in one ciphertext ------------------------------------------------
def block_matrix(blocks: Sequence[Sequence[Optional[Diags]]], ns: int) -> Diags:
    """the 2 ns x 2 ns matrix [[b00, b01], [b10, b11]] of ns x ns blocks (None: a zero block), by its cyclic diagonals of
    length 2 ns: entry (i, (i + d) mod ns) of block (r, c) lies on diagonal c ns + (i + d) mod ns - r ns - i"""
    out: Diags = {}
    i = np.arange(ns)
    for r in range(2):
        for c in range(2):
            for d, v in (blocks[r][c] or {}).items():
                e = (c * ns + (i + d) % ns - r * ns - i) % (2 * ns)
                for index in np.unique(e[v != 0]):
                    at = i[(e == index) & (v != 0)]
                    out.setdefault(int(index), np.zeros(2 * ns, dtype=np.complex128))[r * ns + at] += v[at]
    return out


def plan_packed(N: int, ns: int, levels: int, direction: str, primes_of_the_stages: Sequence[int], factor=1.0) -> Plan:
    """The transform of a sparsely packed ciphertext of the ring of degree N: a message of ns slots, 2 <= ns <= N/4, whose
    plaintext is a polynomial in Y = X^g, g = N / (2 ns).  Its N/2 slots are ns-periodic and the first ns are the slots of
    the ring of degree 2 ns (3^ns = 1 mod 4 ns), so the stage matrices are those of plan(2 ns, ...); read 2 ns-periodic,
    [z | z], both coefficient halves travel in ONE ciphertext and every stage is one 2 ns x 2 ns matrix in mode "single":
        "split" (A, B) -> [[A, 0], [B, 0]]     "lockstep" M -> [[M, 0], [0, M]]     "merge" (M0, M1) -> [[M0, M1], [M0, M1]]
    CoeffToSlot takes [z | z] to [R a | R b] with one conjugation; SlotToCoeff takes [R a | R b] to [z | z], ns-periodic
    again.  1 <= levels <= log2(ns); `factor` next to the small plan's own 1 / (2 ns): the caller folds 1 / g in where the
    input is a SubSum (bootstrap.plan does)."""
    if N < 8 or N & (N - 1):
        raise ValueError("dft plan: N must be a power of two, at least 8")
    ns = int(ns)
    if ns < 2 or ns & (ns - 1) or 4 * ns > N:
        raise ValueError("dft plan: slots must be a power of two in 2 .. N/4")
    small = plan(2 * ns, levels, direction, primes_of_the_stages, factor)
    stages = []
    for st in small.stages:
        if st.mode == "split":
            blocks = [[st.mats[0], None], [st.mats[1], None]]
        elif st.mode == "merge":
            blocks = [[st.mats[0], st.mats[1]], [st.mats[0], st.mats[1]]]
        else:
            blocks = [[st.mats[0], None], [None, st.mats[0]]]
        stages.append(Stage("single", [block_matrix(blocks, ns)], 2 * ns, st.stride, st.prime))
    return Plan(N, small.levels, direction, stages, factor, slots=ns)
