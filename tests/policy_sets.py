"""Parameter sets and operands at the engine's arithmetic-policy boundaries (host only, no GPU).

The engine picks its arithmetic per RNS prime and per level from hand-derived bounds; `policy_of` restates those rules
in Python, with the C++ line each branch mirrors, and the named sets put primes on both sides of every bound:

  forward transform   F64-c40 / F64-generic (q < 2^41), U64L (2^41 <= q < 2^60), U64 (q >= 2^60)
  key MAC             MacF (q < 2^41), MacL (integer q < 2^60 and L <= 8; lazy operands below 4q / 2q for L <= 3 / 5),
                      MacW otherwise
  input reductions    digit into target q_i > m, mod-down P < 2 q_j (lt2q), rescale q_l > q_j

`sets()` gives the sets at GPU size, `toy_sets()` the same bounds and prime counts at n = 16 / 32 for the big-int model.
The last prime of every set is the special prime.
"""
from __future__ import annotations

import numpy as np

from seal_fyp_logistic_regression_amd.seal import CoeffModulus, _is_prime

C40_LO = (1 << 40) - (1 << 23)   # the one-FMA wide reduction needs 2^40 - 2^23 < q < 2^40


# ---------------------------------------------------------------------------------------------------------------------
# primes next to a bound
# ---------------------------------------------------------------------------------------------------------------------
def primes_below(bound: int, N: int, count: int, skip: int = 0) -> list:
    """the `count` largest primes q < bound with q = 1 mod 2N, largest first, after skipping the `skip` largest"""
    out, v = [], bound - 1 - (bound - 2) % (2 * N)
    while len(out) < count + skip:
        if v < 2:
            raise ValueError("not enough primes below the bound")
        if _is_prime(v):
            out.append(v)
        v -= 2 * N
    return out[skip:]


def primes_above(bound: int, N: int, count: int) -> list:
    """the `count` smallest primes q > bound with q = 1 mod 2N, smallest first"""
    out, v = [], bound + 1 + (-bound) % (2 * N)
    while len(out) < count:
        if _is_prime(v):
            out.append(v)
        v += 2 * N
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the engine's rules, restated
# ---------------------------------------------------------------------------------------------------------------------
def fwd_policy(q: int) -> str:
    """the forward transform's arithmetic for prime q"""
    if q >> 41 == 0:                                   # hefx_capi.cpp:394  (q >> 41) == 0: FP64 policy
        c40 = (1 << 40) % q                            # hefx_capi.cpp:404-405  c40 only for 2^39 < q < 2^40 near 2^40
        return "F64-c40" if (q >> 39) == 1 and c40 < (1 << 23) else "F64-generic"
    if q >> 60:                                        # hefx_ntt.cuh:284-287  fwd_int_dispatch: mc.q >> 60 -> [0,8q)
        return "U64"
    return "U64L"                                      # hefx_ntt.cuh:288-289  [0,16q) for primes below 2^60


def mac_policy(q: int, L: int) -> tuple:
    """(MAC policy, operand slack) of target prime q in a key switch over L digits; slack: 0 canonical, 1 below 2q,
    2 below 4q (MacL only)"""
    if q >> 41 == 0:                                   # hefx_keyswitch.hip:533  T.modsf[m].q != 0.0 -> MacF
        return ("MacF", 0)
    if L <= 8 and q >> 60 == 0:                        # hefx_keyswitch.hip:535, :1739  L <= 8 && q < 2^60 -> MacL
        return ("MacL", 2 if L <= 3 else (1 if L <= 5 else 0))  # hefx_keyswitch.hip:120  mac_x_slack
    return ("MacW", 0)                                 # hefx_keyswitch.hip:537


def policy_of(q: int, L: int) -> tuple:
    """(forward policy, (MAC policy, slack)) of prime q in a key switch over L digits"""
    return fwd_policy(q), mac_policy(q, L)


def inmode_flags(primes, L: int) -> dict:
    """the values the integer-policy input reductions take in a key switch / rescale at level L:
    digit  {q_i > m}     a digit i transformed into target m != i (m a data prime below L or the special prime),
                         hefx_keyswitch.hip:303, 1029, 1372, 1594
    lt2q   {P < 2 q_j}   the mod-down remainder (< P) into data row j, hefx_keyswitch.hip:1134, 1416, 1782
    rescale {q_l > q_j}  the dropped prime's remainder into row j, hefx_keyswitch.hip:2276
    Only rows of the integer policy are counted: the FP64 policy reduces its inputs by other rules."""
    P = primes[-1]
    data = primes[:L]
    targets = list(range(L)) + [len(primes) - 1]
    is_int = lambda q: q >> 41 != 0
    digit = {primes[i] > primes[m] for i in range(L) for m in targets if m != i and is_int(primes[m])}
    lt2q = {P < 2 * q for q in data if is_int(q)}
    rescale = {data[-1] > q for q in data[:-1] if is_int(q)} if L >= 2 else set()
    return {"digit": digit, "lt2q": lt2q, "rescale": rescale}


# ---------------------------------------------------------------------------------------------------------------------
# named sets
# ---------------------------------------------------------------------------------------------------------------------
class PSet:
    def __init__(self, name, N, primes, levels, reaches=""):
        self.name, self.N, self.primes, self.levels, self.reaches = name, N, [int(p) for p in primes], tuple(levels), reaches
        assert len(set(self.primes)) == len(self.primes), name
        assert all(p % (2 * N) == 1 and p < 1 << 61 for p in self.primes), name
        assert max(self.levels) <= len(self.primes) - 1, name

    @property
    def k(self):
        return len(self.primes)

    def __repr__(self):
        return f"PSet({self.name}, N={self.N}, k={self.k}, L={self.levels})"


LSWEEP = (1, 2, 3, 4, 5, 6, 8, 9, 12, 16)


def _mixed(N):
    """one prime of every class, interleaved with the 60-bit ones; special just under 2^61.  Two 40-bit primes outside the
    c40 window: one just below it and the smallest 40-bit prime -- just below the window the one-FMA reduction would still
    be exact (a * (2^40 mod q) < 2^45.1), near 2^39 it would not (2^40 mod q is near 2^39), so only the second one tells a
    reduction that ignores the window apart"""
    p60 = primes_below(1 << 60, N, 2)
    return [p60[0], primes_above(1, N, 1)[0], primes_below(1 << 41, N, 1)[0], primes_below(1 << 40, N, 1)[0],
            primes_above(1 << 39, N, 1)[0], primes_below(C40_LO, N, 1)[0], primes_above(1 << 41, N, 1)[0],
            primes_above(1 << 60, N, 1)[0], p60[1], primes_below(1 << 61, N, 1)[0]]


def make_sets(toy_n=None):
    """the named sets; toy_n: the same bounds and prime counts at ring size toy_n (for the big-int model)"""
    def n(N):
        return toy_n or N

    S = []
    N = n(8192)
    p60 = primes_below(1 << 60, N, 2)
    S.append(PSet("f41", N, [p60[0]] + primes_below(1 << 41, N, 3) + [p60[1]], (4, 3, 1),
                  "FP64 at its top; the c32 reduction of 60-bit digits"))
    N = n(4096)
    S.append(PSet("f41_wide", N, primes_below(1 << 41, N, 61) + primes_below(1 << 60, N, 1), (31, 61),
                  "MacF sums at L = 31 and 61 (k = 62, the maximum)"))
    N = n(16384)
    p60 = primes_below(1 << 60, N, 2)
    S.append(PSet("c40_edge", N, [p60[0]] + primes_below(C40_LO, N, 2) + primes_above(C40_LO, N, 2) + [p60[1]], (5, 3),
                  "both sides of the c40 window in one launch"))
    S.append(PSet("i42", N, [p60[0]] + primes_above(1 << 41, N, 3) + [p60[1]], (4, 2),
                  "first integer primes (U64L + MacL); P >= 2 q_j: lt2q off"))
    N = n(4096)
    S.append(PSet("straddle60", N, primes_below(1 << 60, N, 2) + primes_above(1 << 60, N, 3), (4, 2),
                  "U64L / U64 and MacL / MacW side by side at L <= 8"))
    N = n(2048)
    S.append(PSet("small_p", N, primes_above(1, N, 3) + primes_below(1 << 61, N, 1), (3, 2),
                  "tiny FP64 rows; a 61-bit row reduced into them"))
    N = n(8192)
    p60 = primes_below(1 << 60, N, 2)
    S.append(PSet("p_min", N, p60 + primes_below(1 << 50, N, 1), (2, 1), "special prime below the data primes"))
    S.append(PSet("p_min40", N, p60 + primes_below(1 << 40, N, 1), (2, 1), "a 40-bit special prime below 60-bit data"))
    N = n(4096)
    S.append(PSet("p_min61", N, primes_below(1 << 61, N, 8) + primes_below(1 << 42, N, 1), (8, 5, 3),
                  "eight 61-bit digits into a 42-bit special row: the limb MAC at L = 8, 5, 3 on digits far above its prime"))
    N = n(4096)
    S.append(PSet("lsweep", N, primes_below(1 << 60, N, 17), LSWEEP, "slack 2 -> 1 -> 0, MacL -> MacW at L = 9"))
    for N0 in (2048, 16384):
        S.append(PSet(f"mixed{N0}", n(N0), _mixed(n(N0)), (9, 8, 5, 2), "per-row policy dispatch inside one launch"))
    deep = CoeffModulus.Create(32768, [60] + [40] * 19 + [60])
    if toy_n:  # at toy size every 40-bit prime SEAL hands out lies in the c40 window: keep the chain's classes instead
        win = [fwd_policy(q) == "F64-c40" for q in deep[1:20]]
        inside, outside = primes_above(C40_LO, toy_n, sum(win)), primes_below(C40_LO, toy_n, 19 - sum(win))
        deep = (primes_below(1 << 60, toy_n, 2)[1:] + [inside.pop() if w else outside.pop() for w in win]
                + primes_below(1 << 60, toy_n, 1))
    S.append(PSet("seal_deep", n(32768), deep, (20, 12, 9), "a SEAL-valid chain; L up to 20"))
    return {s.name: s for s in S}


_CACHE = {}


def sets():
    if "gpu" not in _CACHE:
        _CACHE["gpu"] = make_sets()
    return _CACHE["gpu"]


def toy_sets(toy_n=16):
    if toy_n not in _CACHE:
        _CACHE[toy_n] = make_sets(toy_n)
    return _CACHE[toy_n]


# ---------------------------------------------------------------------------------------------------------------------
# operands (payloads [npoly][L][N] uint64, NTT domain, canonical)
# ---------------------------------------------------------------------------------------------------------------------
OPERANDS = ("uniform", "ntt_max", "coef_max", "coef_max_z", "zero")
KEYS = ("uniform", "max")


def operand(o, kind, L, npoly=2, seed=1):
    """uniform: seeded; ntt_max: every NTT word q-1 (the constant polynomial -1: sparse digits); coef_max: every
    COEFFICIENT q-1 (dense digits of q_i - 1: the worst input of the forward digit transforms); coef_max_z: coef_max
    with one zero coefficient per row (dense digits that still send exact hoisting to its fallback); zero"""
    N, primes = o.N, o.primes
    if kind == "uniform":
        return o.uniform(L, npoly, seed)
    out = np.zeros((npoly, L, N), dtype=np.uint64)
    if kind == "zero":
        return out
    rng = np.random.default_rng(seed)
    for j in range(L):
        q = np.uint64(primes[j] - 1)
        if kind == "ntt_max":
            out[:, j] = q
            continue
        coef = np.full(N, q, dtype=np.uint64)
        for p in range(npoly):
            c = coef.copy()
            if kind == "coef_max_z":
                c[int(rng.integers(N))] = 0
            elif kind != "coef_max":
                raise ValueError(kind)
            out[p, j] = o.ntt_fwd(j, c)
    return out


def key(o, kind, seed=7):
    """a key-switching key [k-1][2][k][N]: uniform, or every word q_j - 1 (the MAC columns at their maximum)"""
    k, N = o.k, o.N
    if kind == "uniform":
        return o.uniform(k, 2 * (k - 1), seed).reshape(k - 1, 2, k, N)
    if kind != "max":
        raise ValueError(kind)
    row = np.asarray([p - 1 for p in o.primes], dtype=np.uint64)
    return np.ascontiguousarray(np.broadcast_to(row[None, None, :, None], (k - 1, 2, k, N)))


def plain(o, kind, rows, seed=5):
    """a plaintext / diagonal [rows][N]: uniform, or every word q_j - 1"""
    if kind == "uniform":
        return o.uniform(rows, 1, seed)[0]
    if kind != "max":
        raise ValueError(kind)
    return np.ascontiguousarray(np.broadcast_to(np.asarray([p - 1 for p in o.primes[:rows]], dtype=np.uint64)[:, None],
                                                (rows, o.N)))
