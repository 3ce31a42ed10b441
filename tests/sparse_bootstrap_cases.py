"""Shared cases of tests/test_sparse_bootstrap_cpu.py and tests/test_gpu_sparse_bootstrap.py (TEST INFRASTRUCTURE): the sparse
slot counts, the tiled inputs and the environment of the sparse bootstrap.  Ring, chain, scale, key and cap are those of
tests/bootstrap_cases.py, by import.

SPARSE_NS = 16: g = N / (2 ns) = 64, six SubSum steps, transforms of dimension 32 tiled 32 times, levels 2 + 2.
FULL_NS = 512 = N / 4: g = 2, ONE SubSum step, the period equals the slot count and nothing is tiled.
SMALL_NS = 2: one butterfly factor, the levels clip to 1 + 1 (no precision claim there)."""
import numpy as np

from tests import bootstrap_cases as BC

SPARSE_NS = 16
FULL_NS = BC.N // 4
SMALL_NS = 2


def sparse_input(ns):
    """the first ns values of the dense test's input: what the message holds; tiled() is what is encoded"""
    return BC.bootstrap_input()[:ns].copy()


def tiled(v):
    return np.tile(v, (BC.N // 2) // len(v))


def sparse_plan(ns, **kw):
    from seal_fyp_logistic_regression_amd import bootstrap as B
    from seal_fyp_logistic_regression_amd import seal as S
    return B.plan(BC.N, S.CoeffModulus.Create(BC.N, BC.CHAIN_BITS), BC.SCALE, slots=ns, **kw)


def make(kind, steps):
    """BC.make on the bootstrap chain with the sparse key and the Galois keys of `steps` and of the conjugation"""
    return BC.make(BC.N, BC.CHAIN_BITS, kind, seed=BC.KEY_SEED, hamming_weight=BC.HAMMING_WEIGHT,
                   galois_steps=tuple(sorted(set(steps))), conjugate=True)


def encrypt_tiled(e, v):
    return e["enc"].encrypt(e["encoder"].encode(tiled(v), BC.SCALE, parms_id=1))
