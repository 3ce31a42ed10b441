"""Logistic-regression training with evaluation keys only, on the GPU: algorithms.train_cipher_bootstrapped and
update_weights_bootstrapped give on the engine, word for word after EVERY iteration, the ciphertexts of the oracle-backed twin,
in both rescale divisions.

The same host code runs on both, but not the same entries: the engine takes each dot product's window sum as one
hefx_rotate_add_chain, the update's tiling and the bootstrap's SubSum as key switches with the sum in the epilogue, the packed
transforms through batched rotations and hefx_plain_combine, EvalMod through hefx_product_combine and the mod-raise through
hefx_mod_raise; the twin has none of these and runs them op by op.  The chain has 21 primes -- the key switch at k = 21, hefx_mod_raise
from one row to 20 -- which no other test of the suite reaches (tests/lr_bootstrap_cases.py: chain, shapes A and B, model).

Since the words are the twin's, the decode error is the twin's (tests/test_lr_bootstrap_cpu.py measures it); it is asserted anyway,
against the float model with the CPU test's allowance.  The twin's runs are cached in the module: a test's seconds are nearly all
the twin's, on the CPU."""
import numpy as np
import pytest

from tests import bootstrap_cases as BC
from tests import lr_bootstrap_cases as LB

pytestmark = pytest.mark.gpu

_ENV = {}


def plans():
    if "plans" not in _ENV:
        _ENV["plans"] = {ns: LB.plan(ns) for ns in sorted({s[2] for s in LB.SHAPES.values()})}
    return _ENV["plans"]


def env(kind, mode):
    """one environment per backend and rescale division (the engine reads its division when the context is made)"""
    if (kind, mode) not in _ENV:
        _ENV[(kind, mode)] = LB.make(kind, LB.galois_steps(plans()))
    return _ENV[(kind, mode)]


def twin_run(shape, mode):
    if ("twin", shape, mode) not in _ENV:
        _ENV[("twin", shape, mode)] = LB.run(env("oracle", mode), shape, plans()[LB.SHAPES[shape][2]])
    return _ENV[("twin", shape, mode)]


@pytest.mark.parametrize("shape", sorted(LB.SHAPES))
def test_every_iteration_same_words_as_the_twin(shape, rescale_mode):
    rows, weights, ns, iters = LB.SHAPES[shape]
    eg, eo = env("gpu", rescale_mode), env("oracle", rescale_mode)
    be = eg["ctx"].backend
    assert all(getattr(be, name, None) is not None for name in ("rotate_add_chain", "plain_combine", "product_combine", "mod_raise"))
    assert all(getattr(eo["ctx"].backend, name, None) is None for name in ("rotate_add_chain", "plain_combine", "mod_raise"))
    want_words, want = twin_run(shape, rescale_mode), LB.model(shape)
    got = LB.run(eg, shape, plans()[ns])
    assert len(got) == len(want_words) == iters
    for i, (g, o, w) in enumerate(zip(got, want_words, want)):
        name = (shape, rescale_mode, "iteration %d" % (i + 1))
        assert g.size() == o.size() == 2 and g.parms_id() == o.parms_id() == LB.START_LEVEL and g.scale == o.scale, name
        assert np.array_equal(LB.words(eg, g), LB.words(eo, o)), name
        first, everywhere = LB.errors(eg, g, w)
        print(f"[gpu lr bootstrap] shape {shape} ({rescale_mode}), iteration {i + 1}: words equal; decode error {first:.3e} in the "
              f"first {ns} slots, {everywhere:.3e} in all (allowance {LB.ALLOWANCE[shape]:.3e})")
        assert first <= LB.ALLOWANCE[shape] and everywhere <= LB.ALLOWANCE[shape] <= BC.CAP * LB.MAX_VALUE, name
