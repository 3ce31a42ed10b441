"""Exact model, crafted inputs and recorded figures for the mod-raise / refresh tests (tests/test_refresh_cpu.py,
tests/test_gpu_refresh.py).  TEST INFRASTRUCTURE: nothing here is imported by the package.

The model.  A plaintext over rows q_0 .. q_(L_in-1) is an integer polynomial whose coefficient x in [0, Q_in) stands for x
when x <= Q_in // 2 and for x - Q_in otherwise (Q_in odd: no tie).  lift() writes that polynomial over rows
q_0 .. q_(L_out-1).  It composes x by the PLAIN CRT sum  x = sum_j r_j (Q/q_j) ((Q/q_j)^-1 mod q_j) mod Q  in Python
integers -- deliberately not by mixed-radix digits, which is how both the engine's kernel and seal.lift_coefficients do it --
and moves between NTT and coefficient form with the oracle's transforms (N = 1024 and 4096 are out of reach of the O(N^2)
definitions of tests/pymodel.py)."""
import numpy as np

from oracle import oracle as O

_oracles = {}


def oracle_for(N, primes):
    key = (N, tuple(primes))
    if key not in _oracles:
        _oracles[key] = O.Oracle(N, list(primes))
    return _oracles[key]


def modulus(primes, L):
    Q = 1
    for q in primes[:L]:
        Q *= int(q)
    return Q


def compose(rows, primes, L):
    """rows [L][N] coefficient form -> list of N Python integers in [0, Q), plain CRT"""
    Q = modulus(primes, L)
    acc = np.zeros(rows.shape[1], dtype=object)
    for j in range(L):
        Qj = Q // int(primes[j])
        acc = (acc + rows[j].astype(object) * (Qj * pow(Qj, -1, int(primes[j])))) % Q
    return acc, Q


def lift_coefficients(rows, primes, L_in, L_out):
    """rows [L_in][N] coefficient form -> rows [L_out][N] of the centred integers, coefficient form"""
    x, Q = compose(rows, primes, L_in)
    x = np.array([v - Q if v > Q // 2 else v for v in x], dtype=object)
    return np.stack([(x % int(primes[j])).astype(np.uint64) for j in range(L_out)])


def lift(words, primes, L_in, L_out):
    """words [count][L_in][N] NTT form -> [count][L_out][N] NTT form: what hefx_mod_raise must give, word for word"""
    words = np.asarray(words, dtype=np.uint64)
    count, _, N = words.shape
    o = oracle_for(N, primes)
    out = np.empty((count, L_out, N), dtype=np.uint64)
    for c in range(count):
        coef = np.stack([o.ntt_inv(j, words[c, j]) for j in range(L_in)])
        full = lift_coefficients(coef, primes, L_in, L_out)
        for j in range(L_out):
            out[c, j] = o.ntt_fwd(j, full[j])
        assert np.array_equal(out[c, :L_in], words[c]), "the old rows of a lift are the input's words"
    return out


def half_digits(primes, L):
    """mixed-radix digits of Q // 2, radix (q_0, q_1, ...)"""
    h, d = modulus(primes, L) // 2, []
    for q in primes[:L]:
        d.append(h % int(q))
        h //= int(q)
    return d


def crafted_values(primes, L):
    """the coefficients every crafted polynomial carries: the ends of both sign ranges and, for L > 1, values whose
    mixed-radix digits above digit 0 are those of Q // 2, so that digit 0 alone decides the sign"""
    Q = modulus(primes, L)
    half, q0 = Q // 2, int(primes[0])
    d0 = half_digits(primes, L)[0]
    base = half - d0  # digit 0 cleared, the digits above as in Q // 2
    vals = [0, 1, Q - 1, half, half + 1, 2, Q - 2]
    vals += [base + t for t in (0, d0 - 1, d0, d0 + 1, q0 - 1) if 0 <= t < q0]
    return [v % Q for v in vals]


def crafted_coefficients(primes, L, N, count, seed):
    """[count][L][N] coefficient form, canonical: random fill, the crafted values at coefficient 0 and N - 1 (rotating
    through the list from item to item) and all of them at random positions"""
    rng = np.random.default_rng(seed)
    vals = crafted_values(primes, L)
    out = np.empty((count, L, N), dtype=np.uint64)
    for c in range(count):
        for j in range(L):
            out[c, j] = rng.integers(0, int(primes[j]), N, dtype=np.uint64)
        pos = [int(p) for p in rng.choice(np.arange(1, N - 1), size=len(vals), replace=False)]
        placed = list(zip(pos, vals)) + [(0, vals[(2 * c) % len(vals)]), (N - 1, vals[(2 * c + 1) % len(vals)])]
        if c == 0:  # the two sign boundaries at the two ends
            placed += [(0, vals[3]), (N - 1, vals[4])]
        for a, v in placed:
            for j in range(L):
                out[c, j, a] = v % int(primes[j])
    return out


def crafted_words(primes, L, N, count, seed):
    """crafted_coefficients in NTT form: an input of hefx_mod_raise"""
    o = oracle_for(N, primes)
    coef = crafted_coefficients(primes, L, N, count, seed)
    return np.stack([np.stack([o.ntt_fwd(j, coef[c, j]) for j in range(L)]) for c in range(count)])


# ---- training on the twin
# learning rate per shape (num_obs, num_weights): chosen so that the allowance below is at most a tenth of the smallest
# update |lr / n * g_j| of every iteration the tests run (tests/test_refresh_cpu.py asserts it), so a missed update cannot
# hide in the allowance
LEARNING_RATE = {(3, 4): 1.0, (8, 8): 1.0}
ITERS = 2
# Largest |decoded - w| of the ORACLE TWIN ALONE after each of the two iterations of algorithms.train_cipher at N = 4096,
# rescale division "round", against the plain recurrence w <- w - (lr / n) g(w) with g = lr_gradient_cases.expected_gradient,
# as printed by tests/test_refresh_cpu.py::test_two_iterations_of_train_cipher_on_the_twin; the GPU tests allow 8x that.
# The figure is the scale snaps' (lr_gradient_cases.TWIN_ERROR says why), times lr / n; the encryption noise under it moves
# the last printed digit with the stream ids the run happens to draw (1.183e-06 .. 1.187e-06 for (3, 4)).
# (rounded / floor division, after iteration 1 and 2:  (3, 4) 1.187e-06, 6.304e-07 / 1.065e-06, 5.756e-07;
#  (8, 8) 6.857e-07, 9.077e-07 / 7.304e-07, 9.075e-07)
TRAIN_TWIN_ERROR = {(3, 4): 1.187e-06, (8, 8): 9.077e-07}


def train_allowance(shape):
    return 8 * TRAIN_TWIN_ERROR[shape]


def plain_training(X, w, y, coeffs, lr, iters):
    """[w_1, ..., w_iters] of w <- w - (lr / n) g(w), and the gradients g(w_0) .. g(w_(iters-1))"""
    from tests import lr_gradient_cases as G
    ws, gs = [], []
    w = np.array(w, dtype=float)
    for _ in range(iters):
        g = G.expected_gradient(X, w, y, coeffs)
        w = w - (lr / X.shape[0]) * g
        ws.append(w.copy())
        gs.append(g)
    return ws, gs
