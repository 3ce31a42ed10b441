"""The BFV entries beyond multiply and decrypt_round without a GPU: the models of tests/bfv_front_cases.py against each
other and against brute force at N = 1024, the header's comments, and the new driver's two forms (syntax only)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bfv_cases as B
from tests import bfv_front_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = F.N
NEW_WRITERS = ("hefx_bfv_scale_plain_add", "hefx_bfv_lift_plain", "hefx_bfv_noise_budget", "hefx_bfv_batch_encode",
               "hefx_bfv_batch_decode")


def test_the_batching_moduli_are_what_the_tests_expect():
    ts = F.batching_moduli()
    assert {65537, 1032193} <= set(ts) and 2 not in ts and 1024 not in ts
    top = max(ts)
    assert top.bit_length() == 59 and all(F.allows_batching(t) for t in ts)
    # the largest one: no prime that is 1 mod 2N lies between it and 2^59
    assert not any(F.is_prime(v) for v in range(max(ts) + 2 * N, 1 << 59, 2 * N))
    for t in ts:
        psi = F.minimal_root(t)
        assert pow(psi, N, t) == t - 1
        if t < 1 << 21:  # brute force: nothing smaller has order 2N
            assert not any(pow(c, N, t) == t - 1 for c in range(2, psi))


@pytest.mark.parametrize("t", F.batching_moduli())
def test_decode_inverts_encode_and_products_are_slot_wise(t):
    rng = np.random.default_rng(t % 1000)
    for nvalues in (1, N // 2 + 1, N):
        v = [int(x) for x in rng.integers(0, t, nvalues, dtype=np.uint64)]
        v[0], v[-1] = t - 1, (0 if nvalues > 1 else t - 1)
        m = F.batch_encode_model(v, t)
        assert all(int(c) < t for c in m)
        assert [int(x) for x in F.batch_decode_model(m, t)] == v + [0] * (N - nvalues)
    a = [int(x) for x in rng.integers(0, t, N, dtype=np.uint64)]
    b = [int(x) for x in rng.integers(0, t, N, dtype=np.uint64)]
    ma, mb = F.batch_encode_model(a, t), F.batch_encode_model(b, t)
    prod = B.negacyclic_sums([[int(c) for c in ma]], [[int(c) for c in mb]], 2 * t.bit_length() + N.bit_length())[0]
    assert [int(x) for x in F.batch_decode_model([c % t for c in prod], t)] == [x * y % t for x, y in zip(a, b)]
    # slot 0 sits at psi itself, slot N/2 at its inverse: the definition, evaluated by Horner
    psi = F.minimal_root(t)
    for slot, point in ((0, psi), (N // 2, pow(psi, -1, t)), (1, pow(psi, 3, t))):
        acc = 0
        for c in reversed(ma):
            acc = (acc * point + int(c)) % t
        assert acc == a[slot]


@pytest.mark.parametrize("t", B.PLAIN_MODULI)
@pytest.mark.parametrize("name", sorted(B.prime_sets()))
def test_noise_budget_model_equals_the_closed_form(name, t):
    _, primes, L = B.prime_sets()[name]
    Q = B.modulus(primes, L)
    vals = F.noise_values(primes, L)
    picks = vals[:4] + vals[-4:] + vals[len(vals) // 2:len(vals) // 2 + 2]
    n = 8  # the model is per coefficient: a short polynomial serves
    for i, v in enumerate(picks):
        poly = [0] * n
        poly[i % n] = v
        x = F.x_for_noise(poly, primes, L, t)
        assert [B.centre(t * c % Q, Q) for c in B.compose(x, primes, L)] == poly
        assert F.noise_budget_model(x, primes, L, t) == F.budget_of(v, primes, L)
    assert F.budget_of((Q - 1) // 2, primes, L) == 0 and F.budget_of(1, primes, L) == Q.bit_length() - 2
    assert F.noise_budget_model(np.zeros((L, n), dtype=np.uint64), primes, L, t) == Q.bit_length() - 1


@pytest.mark.parametrize("t", B.PLAIN_MODULI)
def test_scale_and_lift_models_against_their_meaning(t):
    """Delta m + c0 composed over Q, and the lift as the centred message modulo every prime"""
    _, primes, L = B.prime_sets()["bfv8192_bits"]
    Q = B.modulus(primes, L)
    n = 16
    m = F.message_values(t, n, seed=3)
    c0 = B.uniform(primes, L, 1, n, 4)[0]
    got = F.scale_plain_add_model(m, n - 1, c0, primes, L, t, n=n)
    base = B.compose(c0, primes, L)
    assert B.compose(got, primes, L) == [(base[i] + (Q // t) * int(m[i]) * (i < n - 1)) % Q for i in range(n)]
    lifted = F.lift_plain_model(m, n, primes, L, t, n=n)
    for j in range(L):
        q = int(primes[j])
        for i in range(n):
            v = int(m[i])
            assert int(lifted[j, i]) % q == (v if v <= t // 2 else v - t) % q and 0 <= int(lifted[j, i]) <= q


# ---- the header
def _header():
    return open(os.path.join(ROOT, "include", "hefx_bfv.h")).read()


def test_every_new_writer_states_its_overlap_rule():
    src = _header()
    for name in NEW_WRITERS:
        at = src.index("int " + name + "(")
        comment = " ".join(src[src.rindex("/*", 0, at):at].replace("\n *", " ").split())
        assert "overlap" in comment and "HEFX_ERR_INVALID before anything is submitted" in comment, name
        assert "BYTES" in comment, name
    for name in ("hefx_bfv_batch_encode", "hefx_bfv_batch_decode"):
        at = src.index("int " + name + "(")
        assert "HEFX_ERR_UNSUPPORTED" in src[src.rindex("/*", 0, at):at], name
    assert "int hefx_bfv_batching(const hefx_bfv *b);" in src


def test_the_new_entries_are_bound():
    from seal_fyp_logistic_regression_amd import capi
    assert set(NEW_WRITERS) | {"hefx_bfv_batching"} <= set(capi.BFV_SYMBOLS)
    from seal_fyp_logistic_regression_amd import BfvPlan
    for method in ("scale_plain_add", "lift_plain", "noise_budget", "batching", "batch_encode", "batch_decode"):
        assert callable(getattr(BfvPlan, method)), method


def test_bfv_front_selftest_driver_compiles():
    """drivers/bfv_front_selftest.cpp against include/seal/seal.h, in both of its forms (syntax only: no library needed)"""
    for extra in ([], ["-DBFV_FRONT_PUBLIC_API_ONLY"]):
        r = subprocess.run(["g++", "-std=c++17", "-w", "-fsyntax-only", "-I", os.path.join(ROOT, "include")] + extra +
                           [os.path.join(ROOT, "drivers", "bfv_front_selftest.cpp")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    mk = open(os.path.join(ROOT, "drivers", "Makefile")).read()
    assert "$(OUT)/bfv_front_selftest:" in mk
    assert "$(OUT)/bfv_front_selftest " in next(line for line in mk.splitlines() if line.startswith("all:"))
    assert '"_ref/bfv_front_selftest"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_the_bfv_branches_of_the_shim_reach_the_host_functions_only_as_fall_backs():
    """include/seal/seal.h: every call of bfv_scaled_plain / bfv_lifted_plain / PlainNtt's transforms / decrypt_round_host
    outside its own definition sits on a line that says it is the fall-back"""
    src = open(os.path.join(ROOT, "include", "seal", "seal.h")).read()
    for call in (r"shim::bfv_scaled_plain\(", r"shim::bfv_lifted_plain\(", r"pntt\.inverse\(", r"pntt\.forward\(",
                 r"decrypt_round_host\("):
        lines = [ln for ln in src.splitlines() if re.search(call, ln) and not ln.lstrip().startswith("//")]
        assert lines, call
        for ln in lines:
            assert "fall-back" in ln, ln
