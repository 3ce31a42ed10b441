"""Every device arithmetic primitive, alone, on the directed operand sets of tests/arith_cases.py (MI355X).

libhefx_arith_probe.so (csrc/hefx_arith_probe.hip, built by build() with the engine's flags) runs ONE primitive per thread on
operands and per-modulus constants that come from here, from Python integers.  For every element the device's result must
  * keep the contract its source comment states (congruent to the exact integer result mod q, inside the stated range, FP64
    outputs exact integers) -- Case.check, the very function the models are held to in tests/test_arith_cases_cpu.py, and
  * equal the exact model, bit for bit.
One process, no subprocesses, no environment knobs.  The largest |mm|/q, the largest lazy result per primitive in units of q and
the largest MacL column seen ON THE DEVICE are printed (pytest -s); DESIGN.md's table quotes them."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from seal_fyp_logistic_regression_amd import _build
from tests import arith_cases as ac

pytestmark = pytest.mark.gpu

KS = ac.all_K()
_LIB = []
EXTREMES = {}   # family -> largest result in units of q (lazy ranges), over every prime run so far


def probe():
    if not _LIB:
        lib = ctypes.CDLL(_build.PROBE_SO)   # missing library: an error, there is no other path
        u64p = ctypes.POINTER(ctypes.c_uint64)
        lib.hefx_arith_probe.restype = ctypes.c_int
        lib.hefx_arith_probe.argtypes = [ctypes.c_int, ctypes.c_int, u64p, u64p, u64p, ctypes.c_int, u64p, ctypes.c_int,
                                         ctypes.c_size_t]
        _LIB.append(lib)
    return _LIB[0]


def run_case(c: ac.Case) -> np.ndarray:
    u64p = ctypes.POINTER(ctypes.c_uint64)
    k = c.k
    mc = np.asarray(k.modconst_words(), dtype=np.uint64)
    mf = np.asarray(k.modconstf_words(), dtype=np.uint64)
    tin = np.ascontiguousarray(np.asarray(c.pack(), dtype=np.uint64).reshape(len(c.tuples), c.nin))
    out = np.full((len(c.tuples), c.nout), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    rc = probe().hefx_arith_probe(c.op, c.param, mc.ctypes.data_as(u64p), mf.ctypes.data_as(u64p), tin.ctypes.data_as(u64p),
                                  c.nin, out.ctypes.data_as(u64p), c.nout, len(c.tuples))
    assert rc == 0, f"{c}: hefx_arith_probe returned {rc}"
    return out


def note(family, value):
    EXTREMES[family] = max(EXTREMES.get(family, 0.0), value)


def hold(c: ac.Case, dev: np.ndarray):
    """contract first (it says WHAT is wrong), then equality with the model"""
    m = ac.Model(c.k)
    q = c.k.q
    for t, row in zip(c.tuples, dev.tolist()):
        o = c.decode(row)
        c.check(t, o)
        if c.family.startswith("F64::mm"):
            note(c.family + " |r|/q", abs(o[0]) / q)
        elif c.family == "MacL":
            note("MacL column / 2^64", max(o[8:20]) / 2.0 ** 64)
        elif c.family == "MacF":
            note("MacF |sum|/q", max(abs(v) for v in o[4:8]) / q)
        elif c.top is not None:
            note(f"{c.family} (< {c.top}q)", max(o) / q)
    want = np.asarray(c.model_words(m), dtype=np.uint64).reshape(dev.shape)
    bad = np.argwhere(dev != want)
    assert bad.size == 0, (f"{c}: {len(bad)} words differ from the model; first: tuple {c.tuples[bad[0][0]]} word {bad[0][1]} "
                           f"device {int(dev[tuple(bad[0])]):#x} model {int(want[tuple(bad[0])]):#x}")


def test_probe_refuses_what_it_does_not_know():
    u64p = ctypes.POINTER(ctypes.c_uint64)
    z = np.zeros(8, dtype=np.uint64)
    p = z.ctypes.data_as(u64p)
    assert probe().hefx_arith_probe(999, 0, p, p, p, 1, p, 1, 1) == -1       # unknown op
    assert probe().hefx_arith_probe(ac.OP["csub"], 0, p, p, p, 3, p, 1, 1) == -1   # not the op's tuple shape
    assert probe().hefx_arith_probe(ac.OP["mac_l"], 62, p, p, p, 4 + 6 * 62, p, 20, 1) == -1


@pytest.mark.parametrize("k", KS, ids=[k.name for k in KS])
def test_every_primitive_keeps_its_contract_and_equals_the_model(k):
    cs = ac.cases(k)
    assert sum(len(c.tuples) for c in cs) <= 1 << 17 and all(len(c.tuples) <= 1 << 17 for c in cs)
    failures = []
    for c in cs:
        dev = run_case(c)
        try:
            hold(c, dev)
        except AssertionError as e:   # every primitive of the prime is reported, not only the first
            failures.append(f"{c.name}: {e}")
    assert not failures, f"{k}: {len(failures)} primitives off:\n" + "\n".join(failures[:20])


def test_report_the_extremes_the_device_reached():
    """printed for DESIGN.md's table; the bounds themselves are asserted per element above"""
    assert EXTREMES, "no primitive ran"
    for fam in sorted(EXTREMES):
        print(f"  device extreme  {fam:44s} {EXTREMES[fam]:.6f}")
    assert EXTREMES["F64::mm/2^45 |r|/q"] < 0.52 and EXTREMES["F64::mm/2^49 |r|/q"] < 0.75
    assert EXTREMES["MacL column / 2^64"] < 1.0
