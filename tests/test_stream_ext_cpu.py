"""The cases of tests/test_gpu_streams_ext.py, held to what can be held without a GPU (tests/stream_ext_cases.py): the coverage
table names every stream-taking entry of every extension header, no case can pass vacuously (the references give other words on
the decoys than on the real operands, in every checked output), and the sequence cases are sized so that they do cross the
engine's thresholds -- the scratch floor, the descriptor ring, a chunk -- by the restated launch rules."""
import os
import re

import numpy as np
import pytest

from tests import hybrid_cases as HC
from tests import stream_ext_cases as SX


def test_the_coverage_table_names_every_stream_taking_entry_of_the_extension_headers():
    """a regex over include/hefx_*.h (hefx.h is tests/test_gpu_streams.py's): a future entry that takes `void *stream` fails
    here until the table says where it is held to stream order"""
    headers = SX.extension_headers()
    assert {os.path.basename(h) for h in headers} >= {"hefx_hybrid.h", "hefx_hybrid_hoist.h", "hefx_hybrid_bsgs.h", "hefx_refresh.h", "hefx_encaps.h",
                                                       "hefx_bfv.h", "hefx_dft.h", "hefx_poly.h", "hefx_bootstrap.h"}
    assert not any(os.path.basename(h) == "hefx.h" for h in headers)
    found = [name for h in headers for name in SX.stream_entries(h)]
    assert len(found) == len(set(found))
    # the regex sees what a plain count of the parameter sees: no declaration is lost to its shape
    assert len(found) == sum(len(re.findall(r"void \*stream\)", open(h).read())) for h in headers)
    assert set(found) == set(SX.COVERAGE), (sorted(set(found) - set(SX.COVERAGE)), sorted(set(SX.COVERAGE) - set(found)))
    assert "hefx_hybrid_digits" not in found and "hefx_bfv_create" not in found        # (no stream argument)


def test_every_row_of_the_coverage_table_can_be_checked():
    """a row is a list of cases of this module whose entry is the row's, a module that holds the entry to the decoy protocol
    itself, or a stated reason"""
    kinds = {"case": 0, "module": 0, "not yet": 0}
    for entry, where in SX.COVERAGE.items():
        if isinstance(where, list):
            kinds["case"] += 1
            assert where and all(name in SX.CASES for name in where), entry
        elif where.startswith("tests/"):
            kinds["module"] += 1
            text = open(os.path.join(SX.ROOT, where)).read()
            # the entry's own gate test: decoys staged behind the gate, the entry held to `not gate.opened`
            assert re.search(entry + r" waited on the host: its stream was still shut", text) and "decoys" in text and "S.gate()" in text, entry
        else:
            kinds["not yet"] += 1
            assert where.startswith("not yet: ") and len(where) > 40, entry
    assert kinds == {"case": 12, "module": 3, "not yet": 7}
    bfv = open(os.path.join(SX.ROOT, "include", "hefx_bfv.h")).read()
    assert "belong to the hefx_bfv OBJECT" in bfv                                        # the reason, where the header gives it
    # the wide and scalar encodes are hefx.h's, and their values are host memory (the module docstring says so)
    base = open(os.path.join(SX.ROOT, "include", "hefx.h")).read()
    for name, arg in (("hefx_ckks_encode_wide", "const double *h_re"), ("hefx_ckks_encode_wide_batch", "const double *h_re"),
                      ("hefx_ckks_encode_scalar", "const double *h_values")):
        decl = re.search(r"int " + name + r"\(([^;]*)\);", base).group(1)
        assert arg in decl and name not in SX.COVERAGE


def test_every_case_of_the_table_runs_its_own_entry():
    for entry, where in SX.COVERAGE.items():
        if isinstance(where, list):
            for name in where:
                assert all(c.c_name == entry for c in SX.flat(name)), (entry, name)


@pytest.mark.parametrize("name", sorted(SX.CASES))
def test_the_decoys_give_other_words_in_every_output(name):
    """the non-vacuity condition test_gpu_streams.Op asserts for at least one output, here for every checked one, with the same
    shapes on both sides"""
    for c in SX.flat(name):
        d = c.differs()
        assert d and all(d), (c.name, d)
        for r, x in zip(c.reals, c.decoys):
            assert (r != x).any(), c.name
        for a, b in zip(c.want, c.want_decoy):
            assert (sorted(a) == sorted(b)) if isinstance(a, dict) else (a.shape == b.shape and a.dtype == np.uint64), c.name


def test_two_streams_case_is_not_vacuous():
    t = SX.two_streams()
    assert (t["want"] != t["want_decoy"]).any() and (t["A"] != t["B"]).any()


def test_the_single_cases_have_the_shapes_they_are_there_for():
    s = HC.sets()[SX.SET]
    assert (s.N, s.k, s.alpha) == (2048, 8, 3) and HC.digits(s.alpha, SX.L_TOP) == [[0, 1, 2], [3, 4]]   # two digits, the last partial
    g = SX.galois_batch()
    assert g.reals[0].shape == (3, 2, 5, 2048) and g.reals[1].shape == (2, s.dnum, 2, 8, 2048)
    assert SX.rotate_hoisted().want[0].shape == (6, 2, 5, 2048) and SX.plain_combine_hoisted().want[0].shape == (2, 2, 5, 2048)
    assert SX.bsgs_hoisted().want[0].shape == (2, 2, 5, 2048) and SX.bsgs_hoisted().reals[2].shape == (20, 8, 2048)
    b = HC.sets()[SX.BIG]
    assert b.N == 32768 and SX.flat("big_galois")[0].want[0].shape == (2, 2, 32768) and SX.flat("big_rotate_hoisted")[0].want[0].shape == (3, 2, 2, 32768)


def test_the_scratch_growth_case_crosses_the_floor():
    """by hybrid_cases.item_rows the first call fits the 64 MiB that ensure_scratch allocates at least, the second needs more --
    and is still ONE chunk, so that it is the growth, not the chunking, that the case runs"""
    s = HC.sets()[SX.SET]
    one, many = SX.scratch_growth()
    item = HC.item_rows(s.N, s.alpha, SX.L_TOP) * s.N * 8
    n = SX.grow_items(s, SX.L_TOP)
    assert item == 57 * 2048 * 8 and item <= SX.SCRATCH_FLOOR_BYTES < n * item
    assert n <= HC.chunk_of(s.N, s.alpha, SX.L_TOP)
    assert one.want[0].shape == (2, SX.L_TOP, s.N) and many.out_shapes == [(n, 2, SX.L_TOP, s.N)]
    assert {0, n - 1} <= set(many.want[0])


def test_the_ring_case_wraps_the_descriptor_ring_twice():
    src = open(os.path.join(SX.ROOT, "seal_fyp_logistic_regression_amd", "csrc", "hefx_internal.h")).read()
    assert re.search(r"constexpr int KS_RING = (\d+);", src).group(1) == str(SX.KS_RING)
    assert re.search(r"constexpr int KS_MAX_CHUNK = (\d+);", src).group(1) == str(SX.KS_MAX_CHUNK)
    ops = SX.ring_wrap()
    assert len(ops) == SX.RING_CALLS > 2 * SX.KS_RING
    assert all(c.want[0].shape == (2, 1, 2048) for c in ops) and len({c.name for c in ops}) == 3


def test_the_chunked_case_takes_two_slots():
    s = HC.sets()[SX.SET]
    c = SX.chunked()
    assert HC.chunk_of(s.N, s.alpha, 1) == 1024 < SX.CHUNKED_N == 1030
    assert {0, 1023, 1024, 1029} <= set(c.want[0]) and c.out_shapes == [(1030, 2, 1, 2048)]
    # three distinct inputs in turn: neighbours differ, so an item written from the wrong source shows
    assert all((c.want[0][i] != c.want[0][i + 1]).any() for i in (0, 1, 1023, 1024))
