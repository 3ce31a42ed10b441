"""Shared cases of tests/test_hybrid_cpu.py and tests/test_gpu_hybrid.py (TEST INFRASTRUCTURE): hybrid key switching -- the
integer statement of include/hefx_hybrid.h in Python integers over a backend's own row transforms, the parameter sets, the
operands and the noise bound.

THE SETS.  N = 2048, the smallest ring with key switching.  A set is a SHAPE with a prime MIX, "shape-mix":
    shapes  k7a2  k = 7, alpha = 2: digits {0,1},{2,3},{4}; L = 5, 4, 3, 1 -- full digits, a partial last digit, one one-prime digit
            k8a3  k = 8, alpha = 3: L = 5, 2
            k7a4  k = 7, alpha = 4: one digit, alpha > D = 3; L = 3
            k4a1  k = 4, alpha = 1: the scheme of hefx.h; L = 3, 1
    mixes   p50_60   data primes alternately just below 2^60 and 2^50, specials just below 2^60
            d40_s60  data primes below 2^40 (the transforms' FP64 policy), 60-bit specials
            d60_s40  60-bit data primes, specials below 2^40: Dmax / P is large, the noise with it (still below the bound)
            above60  one data prime just above 2^60, the others below 2^55, 60-bit specials
and one set at N = 32768, "big": k = 4, alpha = 2, L = 2 (p50_60).  The primes come from tests/policy_sets.py's helpers.

THE SETS AT THE SHAPES THE KERNELS ARE BUILT FOR (WIDE_SHAPES; every one keeps 4 B < Q_L at every level):
    N = 2048, mixes p50_60, above60, d40_s60
            k12a5  alpha = 5: L = 7 (digits 5 + 2), 5 (one full digit), 3 (one digit of fewer rows than alpha)
            k14a6  alpha = 6: L = 8 (6 + 2)         k16a7  alpha = 7: L = 9 (7 + 2)
            k18a8  alpha = 8, HEFX_HYBRID_ALPHA_MAX: L = 10 (8 + 2), 8 (exactly one full digit)
            k14a2  alpha = 2: L = 11, six digits, the last of one prime
            k10a1  alpha = 1: L = 9, 4, nine digits (the scheme of hefx.h again)
    N = 2048, mix top61: the k largest primes below 2^61 (the context's limit is q >> 61 == 0), the first alpha of them special
            k24a4  L = 20, 18, 17: five digits, the last one full, of two primes, of one prime
            k62a1  L = 61: the longest chain the ABI takes, the 61 products the MAC's "below 2^128" counts.  ONE case (operand
                   max, key max, element 3); in LONG_SET_NAMES, not in SET_NAMES: its key is 118 MiB on the host
    the rings between, p50_60: n4096, n8192, n16384, each k = 7, alpha = 2, L = 5, 2
    N = 32768, p50_60: big7, k = 7, alpha = 2, L = 5, 4
The key kind "max" (every word q_m - 1) with the operand "max" puts every product of the MAC at its largest.

THE NOISE BOUND.  dec(out) - pi_g(dec(in)), centred mod Q_L, has infinity norm at most
    B = ceil(L/alpha) * alpha * N * 19 * Dmax / P + alpha * (1 + N),          Dmax = the largest D_j(L).
First term: the switch adds sum_j ext_j e_j / P to the decryption, ext_j the integer the uncorrected base conversion stands for,
0 <= ext_j < alpha D_j(L), |e_j| <= 19 (the sampler's clip), a negacyclic product of N terms per coefficient, ceil(L/alpha)
digits.  Second term: the mod-down subtracts v = [acc + floor(P/2)]_P + e P with 0 <= e < alpha (the uncorrected conversion
from the special rows), so each of ks0, ks1 is round(acc / P) - e, within alpha of acc / P; ks1 meets the ternary secret:
alpha * N, ks0 alone: alpha.  Derived, not fitted."""
import numpy as np

from tests import policy_sets as PS

N = 2048
SHAPES = {"k7a2": (7, 2, (5, 4, 3, 1)), "k8a3": (8, 3, (5, 2)), "k7a4": (7, 4, (3,)), "k4a1": (4, 1, (3, 1))}
MIXES = ("p50_60", "d40_s60", "d60_s40", "above60")
ELTS = lambda N_: (1, 3, 2 * N_ - 1)
SEED = 5
# name -> (N, k, alpha, levels, mixes); a name that starts with "k" is a shape and takes "-mix", the others are whole set names
N2048_MIXES = ("p50_60", "above60", "d40_s60")
WIDE_SHAPES = {"k12a5": (N, 12, 5, (7, 5, 3), N2048_MIXES), "k14a6": (N, 14, 6, (8,), N2048_MIXES), "k16a7": (N, 16, 7, (9,), N2048_MIXES),
               "k18a8": (N, 18, 8, (10, 8), N2048_MIXES), "k14a2": (N, 14, 2, (11,), N2048_MIXES), "k10a1": (N, 10, 1, (9, 4), N2048_MIXES),
               "k24a4": (N, 24, 4, (20, 18, 17), ("top61",)), "k62a1": (N, 62, 1, (61,), ("top61",)),
               "n4096": (4096, 7, 2, (5, 2), ("p50_60",)), "n8192": (8192, 7, 2, (5, 2), ("p50_60",)),
               "n16384": (16384, 7, 2, (5, 2), ("p50_60",)), "big7": (32768, 7, 2, (5, 4), ("p50_60",))}


class HSet:
    def __init__(self, name, N_, k, alpha, levels, primes):
        self.name, self.N, self.k, self.alpha, self.levels, self.primes = name, N_, k, alpha, tuple(levels), [int(p) for p in primes]
        assert len(self.primes) == k and len(set(self.primes)) == k, name
        assert all(p % (2 * N_) == 1 and p < 1 << 61 for p in self.primes), name

    @property
    def dnum(self):
        return (self.k - self.alpha + self.alpha - 1) // self.alpha

    def __repr__(self):
        return f"HSet({self.name})"


def mix_primes(mix, N_, k, alpha):
    D = k - alpha
    if mix == "p50_60":
        p60, p50 = PS.primes_below(1 << 60, N_, (D + 1) // 2 + alpha), PS.primes_below(1 << 50, N_, D // 2)
        data = [p60[alpha + i // 2] if i % 2 == 0 else p50[i // 2] for i in range(D)]
        return data + p60[:alpha]
    if mix == "d40_s60":
        return PS.primes_below(1 << 40, N_, D) + PS.primes_below(1 << 60, N_, alpha)
    if mix == "d60_s40":
        return PS.primes_below(1 << 60, N_, D) + PS.primes_below(1 << 40, N_, alpha)
    if mix == "above60":
        return PS.primes_above(1 << 60, N_, 1) + PS.primes_below(1 << 55, N_, D - 1) + PS.primes_below(1 << 60, N_, alpha)
    if mix == "top61":
        top = PS.primes_below(1 << 61, N_, k)
        return top[alpha:] + top[:alpha]
    raise ValueError(mix)


_SETS = {}


def sets():
    if not _SETS:
        for shape, (k, alpha, levels) in SHAPES.items():
            for mix in MIXES:
                _SETS[f"{shape}-{mix}"] = HSet(f"{shape}-{mix}", N, k, alpha, levels, mix_primes(mix, N, k, alpha))
        _SETS["big"] = HSet("big", 32768, 4, 2, (2,), mix_primes("p50_60", 32768, 4, 2))
        for shape, (N_, k, alpha, levels, mixes) in WIDE_SHAPES.items():
            for mix in mixes:
                name = wide_name(shape, mix)
                _SETS[name] = HSet(name, N_, k, alpha, levels, mix_primes(mix, N_, k, alpha))
    return _SETS


def wide_name(shape, mix):
    return f"{shape}-{mix}" if shape.startswith("k") else shape


LONG_SET_NAMES = ["k62a1-top61"]
_WIDE_N = {wide_name(s, m): v[0] for s, v in WIDE_SHAPES.items() for m in v[4]}
WIDE_SET_NAMES = [n for n in _WIDE_N if n not in LONG_SET_NAMES]
SET_NAMES = sorted(f"{s}-{m}" for s in SHAPES for m in MIXES) + ["big"] + WIDE_SET_NAMES
SMALL_SET_NAMES = [n for n in SET_NAMES if n != "big" and _WIDE_N.get(n, N) == N]   # the sets at N = 2048
ALPHA_ONE_SET_NAMES = [f"k4a1-{m}" for m in MIXES] + [f"k10a1-{m}" for m in N2048_MIXES]
ALPHA_ONE_IDS = list(MIXES) + [f"k10a1-{m}" for m in N2048_MIXES]   # the k4a1 cases keep the ids they had: the mix alone


# ---------------------------------------------------------------------------------------------------------------------
# backends and operands
# ---------------------------------------------------------------------------------------------------------------------
_TWINS = {}


def twin(s):
    """the oracle backend of a set (shared: it holds only tables)"""
    from tests.oracle_backend import OracleBackend
    if s.name not in _TWINS:
        _TWINS[s.name] = OracleBackend(s.N, s.primes)
    return _TWINS[s.name]


def context(s, kind):
    from tests import encaps_cases as EC
    return EC.context(kind, s.N, s.primes)


def _fwd(be, m, row, q):
    row = (np.asarray(row, dtype=object) % q).astype(np.uint64)
    return np.asarray(be.to_host(be.ntt_forward(be.from_host(row[None, None]), 1, 1, m))).reshape(-1).astype(object)


def _inv(be, m, row):
    return np.asarray(be.to_host(be.ntt_inverse(be.from_host(np.asarray(row, dtype=np.uint64)[None, None]), 1, 1, m))).reshape(-1).astype(object)


OPERANDS = ("uniform", "max", "zeros")


def operand(s, kind, L, npoly, seed):
    """[npoly][L][N] canonical words, NTT form.  uniform: seeded; max: every word q_j - 1; zeros: the LAST polynomial (the one
    that is switched) has every seventh coefficient and the whole of row 0 zero in COEFFICIENT form, the others uniform"""
    rng = np.random.default_rng(seed)
    out = np.empty((npoly, L, s.N), dtype=np.uint64)
    for j in range(L):
        q = s.primes[j]
        out[:, j] = (q - 1) if kind == "max" else rng.integers(0, q, (npoly, s.N), dtype=np.uint64)
    if kind == "zeros":
        be = twin(s)
        for j in range(L):
            coef = rng.integers(0, s.primes[j], s.N, dtype=np.uint64)
            coef[::7] = 0
            if j == 0:
                coef[:] = 0
            out[npoly - 1, j] = _fwd(be, j, coef, s.primes[j]).astype(np.uint64)
    elif kind not in ("uniform", "max"):
        raise ValueError(kind)
    return out


def random_key(s, seed):
    """[dnum][2][k][N] uniform canonical words: any words are an input of the statement"""
    rng = np.random.default_rng(seed)
    key = np.empty((s.dnum, 2, s.k, s.N), dtype=np.uint64)
    for m, q in enumerate(s.primes):
        key[:, :, m] = rng.integers(0, q, (s.dnum, 2, s.N), dtype=np.uint64)
    return key


def max_key(s):
    """[dnum][2][k][N], every word q_m - 1: with the operand "max" every product of the MAC is the largest there is"""
    row = np.asarray([q - 1 for q in s.primes], dtype=np.uint64)
    return np.ascontiguousarray(np.broadcast_to(row[None, None, :, None], (s.dnum, 2, s.k, s.N)))


KEYS = ("uniform", "max")


def case_key(s, kind):
    """the key of a word case: the set's random key, or the max key"""
    if kind not in KEYS:
        raise ValueError(kind)
    return random_key(s, SEED) if kind == "uniform" else max_key(s)


# ---------------------------------------------------------------------------------------------------------------------
# the statement of include/hefx_hybrid.h, step by step
# ---------------------------------------------------------------------------------------------------------------------
def digits(alpha, L):
    return [list(range(j * alpha, min((j + 1) * alpha, L))) for j in range((L + alpha - 1) // alpha)]


def switch_model(be, primes, alpha, L, x, key):
    """x [L][N] NTT form, key [dnum][2][k][N] -> ks [2][L][N] as Python-integer arrays reduced to uint64"""
    q = [int(p) for p in primes]
    k = len(q)
    S = list(range(k - alpha, k))
    P = int(np.prod([q[t] for t in S], dtype=object))
    x = np.asarray(x, dtype=np.uint64).reshape(L, -1)
    n = x.shape[1]
    key = np.asarray(key, dtype=np.uint64).reshape(-1, 2, k, n)
    # 1. x~ = INTT of the L rows
    xt = [_inv(be, i, x[i]) for i in range(L)]
    rows = list(range(L)) + S
    acc = {(c, m): np.zeros(n, dtype=object) for c in range(2) for m in rows}
    for j, G in enumerate(digits(alpha, L)):
        Dj = int(np.prod([q[i] for i in G], dtype=object))
        # 2. y_i = x~_i Dhat_i^-1 mod q_i; ext_j[m] = sum_i y_i (Dhat_i mod q_m) mod q_m outside the digit
        y = {i: xt[i] * pow(Dj // q[i] % q[i], -1, q[i]) % q[i] for i in G}
        for m in rows:
            if m in G:
                ext = x[m].astype(object)                      # x's own NTT row
            else:
                conv = sum(y[i] * (Dj // q[i] % q[m]) for i in G) % q[m]
                ext = _fwd(be, m, conv, q[m])                  # 3. forward NTT of the converted rows
            for c in range(2):                                 # 4. the MAC
                acc[c, m] = (acc[c, m] + ext * key[j, c, m].astype(object)) % q[m]
    # 5. mod-down with rounding
    half = P // 2
    out = np.empty((2, L, n), dtype=np.uint64)
    for c in range(2):
        z = {}
        for t in S:
            u = (_inv(be, t, acc[c, t].astype(np.uint64)) + half % q[t]) % q[t]
            z[t] = u * pow(P // q[t] % q[t], -1, q[t]) % q[t]
        for j in range(L):
            v = sum(z[t] * (P // q[t] % q[j]) for t in S) % q[j]
            tj = (v - half % q[j]) % q[j]
            out[c, j] = ((acc[c, j] - _fwd(be, j, tj, q[j])) * pow(P % q[j], -1, q[j]) % q[j]).astype(np.uint64)
    return out


def gather(N_, elt, rows):
    """pi_g on NTT-form rows [...][N]: hefx_galois_permute's gather"""
    from seal_fyp_logistic_regression_amd import galois_tables
    return np.asarray(rows)[..., galois_tables.gather_table(N_, elt)]


def add_rows(a, b, primes):
    out = np.empty_like(np.asarray(a, dtype=np.uint64))
    for j in range(out.shape[-2]):
        out[..., j, :] = ((np.asarray(a)[..., j, :].astype(object) + np.asarray(b)[..., j, :].astype(object)) % int(primes[j])).astype(np.uint64)
    return out


def apply_galois_model(be, primes, alpha, L, ct, elt, key):
    """(pi_g(c0) + ks0(pi_g(c1)), ks1(pi_g(c1))), ct [2][L][N]"""
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, L, -1)
    p = gather(ct.shape[2], elt, ct)
    ks = switch_model(be, primes, alpha, L, p[1], key)
    ks[0] = add_rows(ks[0], p[0], primes)
    return ks


def relinearize_model(be, primes, alpha, L, ct3, key):
    """(c0 + ks0(c2), c1 + ks1(c2)), ct3 [3][L][N]"""
    ct3 = np.asarray(ct3, dtype=np.uint64).reshape(3, L, -1)
    return add_rows(switch_model(be, primes, alpha, L, ct3[2], key), ct3[:2], primes)


# ---------------------------------------------------------------------------------------------------------------------
# the word cases: per set and level three Galois items (an operand kind and an element each) and one relinearisation, on
# one random key per set; the wide sets add, at their top level, a Galois item and a relinearisation with the max operand on the
# max key; every model result is computed once per process and shared
# ---------------------------------------------------------------------------------------------------------------------
def word_cases(s):
    """[(L, form, operand kind, elt, key kind)]"""
    e1, e3, econj = ELTS(s.N)
    out, top = [], max(s.levels)
    for L in s.levels:
        if s.name in WIDE_SET_NAMES and s.N != N:   # n4096 .. n16384, big7: the model costs up to 0.7 s a call there
            out += [(L, "galois", "uniform", e3, "uniform"), (L, "galois", "max", econj, "uniform"), (L, "relin", "uniform", 0, "uniform")]
            continue
        out += [(L, "galois", "uniform", e3, "uniform"), (L, "galois", "max", econj, "uniform"), (L, "galois", "zeros", e1, "uniform"),
                (L, "relin", "uniform", 0, "uniform")]
        if L == top:
            out += [(L, "relin", "zeros", 0, "uniform"), (L, "galois", "uniform", econj, "uniform")]
    if s.name in WIDE_SET_NAMES:
        out += [(top, "galois", "max", e3, "max"), (top, "relin", "max", 0, "max")]
    if s.name == "big":
        out = [(2, "galois", "uniform", e3, "uniform"), (2, "relin", "uniform", 0, "uniform")]
    if s.name in LONG_SET_NAMES:
        out = [(top, "galois", "max", e3, "max")]
    return out


_MODEL = {}


def case_input(s, case):
    L, form, kind, elt, _ = case
    return operand(s, kind, L, 2 if form == "galois" else 3, seed=SEED + 10 * L + elt % 7)


def case_model(s, case):
    """the statement's words of a word case on the case's key, from the oracle twin's transforms"""
    key_ = (s.name, case)
    if key_ not in _MODEL:
        L, form, kind, elt, key_kind = case
        ct, key = case_input(s, case), case_key(s, key_kind)
        if form == "galois":
            _MODEL[key_] = apply_galois_model(twin(s), s.primes, s.alpha, L, ct, elt, key)
        else:
            _MODEL[key_] = relinearize_model(twin(s), s.primes, s.alpha, L, ct, key)
    return _MODEL[key_]


# ---------------------------------------------------------------------------------------------------------------------
# exact decryption and the noise bound
# ---------------------------------------------------------------------------------------------------------------------
def decrypt_rows(ct, sk_rows, primes):
    """sum_p ct[p] s^p per row, NTT form, Python integers: [L][N] object"""
    ct = np.asarray(ct)
    size, L = ct.shape[0], ct.shape[1]
    out = []
    for j in range(L):
        q, s = int(primes[j]), np.asarray(sk_rows[j]).astype(object)
        acc = ct[size - 1, j].astype(object)
        for p in range(size - 2, -1, -1):
            acc = (acc * s + ct[p, j].astype(object)) % q
        out.append(acc)
    return out


def centred_integers(be, rows, primes):
    """NTT-form rows [L][N] of one integer polynomial -> its coefficients centred mod Q_L (CRT), Python integers"""
    L = len(rows)
    q = [int(p) for p in primes[:L]]
    Q = int(np.prod(q, dtype=object))
    coef = [_inv(be, j, np.asarray(rows[j] % q[j]).astype(np.uint64)) for j in range(L)]
    x = np.zeros(len(coef[0]), dtype=object)
    for j in range(L):
        Qj = Q // q[j]
        x = (x + coef[j] * (pow(Qj % q[j], -1, q[j]) * Qj)) % Q
    return np.where((x > Q // 2).astype(bool), x - Q, x), Q


def noise_bound(s, L):
    """(B, Q_L) as exact integers (B rounded up)"""
    q = s.primes
    P = int(np.prod(q[s.k - s.alpha:], dtype=object))
    Dmax = max(int(np.prod([q[i] for i in G], dtype=object)) for G in digits(s.alpha, L))
    dn = (L + s.alpha - 1) // s.alpha
    B = -(-(dn * s.alpha * s.N * 19 * Dmax) // P) + s.alpha * (1 + s.N)
    return B, int(np.prod(q[:L], dtype=object))


def switch_noise(s, L, form, elt, ct, out, sk):
    """max |dec(out) - pi_g(dec(ct))| centred mod Q_L in exact integers (form "relin": dec(out) - dec(ct), ct of size 3), and Q_L;
    sk [k][N] the secret's NTT rows, the transforms are the oracle twin's"""
    q = s.primes
    want = decrypt_rows(ct, sk, q)
    if form == "galois":
        want = [gather(s.N, elt, r) for r in want]
    got = decrypt_rows(out, sk, q)
    diff, Q = centred_integers(twin(s), [(g - w) % int(q[j]) for j, (g, w) in enumerate(zip(got, want))], q)
    return int(np.abs(diff).max()), Q


# ---------------------------------------------------------------------------------------------------------------------
# the launch rules of the engine, restated (the idiom of tests/policy_sets.py): the GPU tests assert through them that a batch
# runs the split and the chunking it is there for, so that retuning a rule fails a test where it would silently end the coverage
# ---------------------------------------------------------------------------------------------------------------------
KS_MAX_CHUNK = 1024                    # hefx_internal.h  constexpr int KS_MAX_CHUNK
RING_SLOT_PTRS = 80 * KS_MAX_CHUNK // 8  # hefx_capi.cpp  RING_SLOT_PTRS = sizeof(KsItem) * KS_MAX_CHUNK / sizeof(void *), KsItem of 80 bytes


def split_of(N_, groups, targets):
    """how many ways a lane-loop pass splits its `targets` rows when the batch gives it `groups` row groups (hefx_hybrid.hip,
    hy_split): 256 records of two words per workgroup, doubled while below 1024 workgroups, at most 4, at most targets / 2"""
    wgs = (N_ // 2 + 255) // 256 * groups
    split = 1
    while split < 4 and wgs * split < 1024 and 2 * split <= targets:
        split *= 2
    return split


def convert_split(N_, alpha, L, n):
    """launch_hy_convert: hy_split(T, dn * n, L + alpha)"""
    return split_of(N_, (L + alpha - 1) // alpha * n, L + alpha)


def spread_split(N_, L, n):
    """launch_hy_spread: hy_split(T, 2 * n, L)"""
    return split_of(N_, 2 * n, L)


def item_rows(N_, alpha, L):
    """rows of N words one item takes in the scratch (hefx_capi.cpp, hybrid_item_rows): xn, c0p, xc | ext | accd | accs | tt, the
    blocks a transform reads (ext, accs, tt) twice at N = 32768"""
    dn, xf = (L + alpha - 1) // alpha, 2 if N_ == 32768 else 1
    return 3 * L + xf * dn * (L + alpha) + 2 * L + xf * 2 * alpha + xf * 2 * L


def table_words(alpha, L):
    """words of the (alpha, L) constants (hefx_capi.cpp, hybrid_consts: the `take` lines)"""
    return 2 * L + L * (L + alpha) + 2 * alpha + alpha + alpha * L + L + 2 * L


def chunk_of(N_, alpha, L):
    """items per chunk (hefx_capi.cpp, hybrid_run, the three `chunk` lines): scratch below 1 GiB, the table and four words an item
    within a descriptor slot, at most KS_MAX_CHUNK"""
    chunk = (1 << 30) // (item_rows(N_, alpha, L) * N_ * 8)
    chunk = max(1, min(chunk, (RING_SLOT_PTRS - table_words(alpha, L)) // 4))
    return min(chunk, KS_MAX_CHUNK)


# ---------------------------------------------------------------------------------------------------------------------
# end to end through seal.py: rotate by one and relinearise a product with HybridKeys, at k = 7, alpha = 2
# ---------------------------------------------------------------------------------------------------------------------
E2E_SET = "k7a2-p50_60"
E2E_SCALE = 2.0 ** 50
E2E_SEED = 1
E2E_FACTOR = 8   # the allowance of the engine's decode: E2E_FACTOR times the oracle twin's own decode error (see end_to_end)


def make_env(s, kind, seed=E2E_SEED):
    from seal_fyp_logistic_regression_amd import seal as S
    ctx = context(s, kind)
    kg = S.KeyGenerator(ctx, seed)
    return dict(s=s, ctx=ctx, kg=kg, enc=S.Encryptor(ctx, kg.public_key(), seed + 1), dec=S.Decryptor(ctx, kg.secret_key()),
                encoder=S.CKKSEncoder(ctx, device_encode=False), ev=S.Evaluator(ctx),
                gk=kg.hybrid_galois_keys(s.alpha, [1]), rk=kg.hybrid_relin_keys(s.alpha))


def e2e_values(N_=N):
    rng = np.random.default_rng(17)
    return rng.uniform(-1.0, 1.0, N_ // 2), rng.uniform(-1.0, 1.0, N_ // 2)


def end_to_end(e):
    """encrypt v and w at the top hybrid level k - alpha, rotate v by one slot, multiply by w, relinearise, rescale -- every key
    switch with HybridKeys -- and decode: (the result ciphertext, max |decoded - roll(v, -1) * w|).  The tolerance of the engine's
    run is E2E_FACTOR times the error of the SAME program on the oracle twin, the derivation of tests/test_gpu_lr_gradient.py:
    engine and twin compute the same words, so their decodes differ by the float decode alone, far below the twin's own error;
    tests/test_hybrid_cpu.py prints the twin's error and holds the allowance far below the values."""
    s, ev = e["s"], e["ev"]
    v, w = e2e_values(s.N)
    top = s.k - s.alpha
    cv = e["enc"].encrypt(e["encoder"].encode(v, E2E_SCALE, parms_id=top))
    cw = e["enc"].encrypt(e["encoder"].encode(w, E2E_SCALE, parms_id=top))
    prod = ev.multiply(ev.rotate_vector(cv, 1, e["gk"]), cw)
    ev.relinearize_inplace(prod, e["rk"])
    ev.rescale_to_next_inplace(prod)
    got = e["encoder"].decode(e["dec"].decrypt(prod)).real
    return prod, float(np.abs(got - np.roll(v, -1) * w).max())
