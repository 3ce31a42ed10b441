"""The exact models of tests/arith_cases.py on their own directed sets (no GPU): every primitive's model satisfies the contract
its source comment states, the sets reach the edges they claim, and a table of named mutants shows that the sets are sharp --
each wrong primitive breaks a contract on the committed operands.  tests/test_gpu_arith_primitives.py then holds the device to
the same contracts and to the models, bit for bit."""
from __future__ import annotations

import pytest

from tests import arith_cases as ac

KS = ac.all_K()
IDS = [k.name for k in KS]


def _outs(k):
    """{case name: (case, model outputs)}; every output held to its contract on the way"""
    return {c.name: (c, ac.run_model(c)) for c in ac.cases(k)}


_MEMO = {}


def outs(k):
    if k.name not in _MEMO:
        _MEMO[k.name] = _outs(k)
    return _MEMO[k.name]


def test_primes_sit_where_the_policies_change():
    for N in ac.RINGS:
        t = ac.prime_table(N)
        assert all(q % (2 * N) == 1 for q in t.values())
        assert t["min"] < 1 << 20 and ac.K(t["min"], N).is_f64
        assert ac.K(t["f40"], N).c40 and not ac.K(t["f40lo"], N).c40 and t["f40lo"] < ac.C40_LO < t["f40"] < 1 << 40
        assert t["f41"] < 1 << 41 < t["i41"] and ac.K(t["f41"], N).is_f64 and not ac.K(t["i41"], N).is_f64
        assert t["i60"] < 1 << 60 < t["i60hi"] < t["i61"] < 1 << 61


@pytest.mark.parametrize("k", KS, ids=IDS)
def test_models_keep_every_stated_contract(k):
    """hefx_modarith.cuh, hefx_ntt.cuh (ArithU64T, ArithF64, InvRecentre), hefx_mac.cuh (MacW, MacL, MacF, mac_x_slack): the
    bound each comment gives, cited per case in Case.cite; run_model raises Violation on the first operand that breaks one"""
    for name, (c, o) in outs(k).items():
        assert len(o) == len(c.tuples) and c.cite


@pytest.mark.parametrize("k", KS, ids=IDS)
def test_sets_reach_the_integer_edges(k):
    q, O = k.q, outs(k)
    # mulhi64_under2: every dropped carry e in {0,1,2}; at least once per set of twiddles the full e = 2
    c, o = O["mulhi64_under2"]
    es = {((t[0] * t[1]) >> 64) - r[0] for t, r in zip(c.tuples, o)}
    assert es == {0, 1, 2}, es
    # shoup_lazy loses its one carry (result >= q), shoup_lazy4 all three (result >= 3q); both come next to their tops
    _, o2 = O["shoup_lazy"]
    _, o4 = O["shoup_lazy4"]
    assert max(r[0] for r in o2) >= q and max(r[0] for r in o4) >= 3 * q
    assert any(r[0] % q == q - 1 for r in o2) and any(r[0] % q == q - 1 for r in o4)
    # barrett128_lt2q: the short quotient estimate (result >= q) and the canonical top q - 1
    _, ob = O["barrett128_lt2q"]
    assert any(r[0] >= q for r in ob) and any(r[0] == q - 1 for r in ob) and any(r[0] == 0 for r in ob)
    for nm in ("csub", "csubn", "barrett64", "barrett128", "mulmod"):
        c, o = O[nm]
        assert any(r[0] == (q - 1 if nm not in ("csub", "csubn") else
                            (t[1] if nm == "csub" else (1 << 64) - t[1]) - 1) for t, r in zip(c.tuples, o)), nm
    if k.is_f64:
        return
    # results within one of a range's top: the canonical finishers at q - 1, the lazy operands at 2q - 1 / 4q - 1, and a
    # butterfly output within one twiddle product of its bound (the top itself needs a lazy product of exactly 4q - 1)
    pols = ("U64", "U64L") if q >> 60 == 0 else ("U64",)
    for p in pols:
        for nm, top in ((f"{p}::fwd_finish", q), (f"{p}::mac_operand/slack1", 2 * q), (f"{p}::mac_operand/slack2", 4 * q)):
            _, o = O[nm]
            assert max(r[0] for r in o) == top - 1, nm
        for st in (0, 1):
            c, o = O[f"{p}::ct/stage{st}"]
            assert max(max(r) for r in o) >= (c.top - 2) * q, (c.name, max(max(r) for r in o) / q)
        for hp in (0, 1):
            _, o = O[f"{p}::moddown/pt{hp}"]
            assert {0, q - 1} & {r[0] for r in o}
    c, o = O["U64::gs"]
    assert max(max(r) for r in o) >= 3 * q


@pytest.mark.parametrize("k", [k for k in KS if k.is_f64], ids=[k.name for k in KS if k.is_f64])
def test_sets_reach_the_fp64_edges(k):
    """an mm quotient estimate on the far side of the tie (|result| > q/2) occurs, at both operand sizes, wherever the
    estimate's error (3 |y| 2^-53 of a quotient step) can carry a residue across: q above 2^10 for |y| near 2^45"""
    q, O = k.q, outs(k)
    for nm in ("2^45", "2^49"):
        c, o = O[f"F64::mm/{nm}"]
        far = max(abs(r[0]) for r in o)
        assert 2 * far > q, (nm, far / q)
    c, o = O["F64::mm/2^49"]
    assert max(abs(r[0]) for r in o) * 100 > 51 * q   # ... and well past it where the operand is larger
    L = max(ac.MACF_LEVELS)
    c, o = O[f"MacF/L{L}/diag0"]
    assert max(abs(r[4]) for r in o) * 4 > L * q       # sums of one sign: at least half of L * 0.52q


@pytest.mark.parametrize("N", ac.RINGS)
def test_macl_columns_come_within_a_factor_two_of_2_64(N):
    """hefx_mac.cuh mac_x_slack: (2^60 + 2^62) L at L = 3, (2^60 + 2^61) L at L = 5, 2 * 2^60 L at L = 8, q just below 2^60"""
    O = outs(ac.get_K("i60", N))
    for L in (3, 5, 8):
        _, o = O[f"MacL/L{L}/lt2q0/diag0"]
        top = max(max(r[8:20]) for r in o)
        assert 1 << 63 <= top < 1 << 64, (L, top / 2 ** 64)


MUTANTS = ["under2 drops one more partial product",
           "16q butterfly without the odd-stage subtraction, q just below 2^60",
           "MacL slack 2 at L = 4",
           "MacL slack 1 at L = 6",
           "the [0,16q) form applied to a 61-bit prime",
           "reduce_wide40 outside its window (smallest 40-bit prime)",
           "mm fed 2^53",
           "moddown forming 9q"]


def test_mutant_table_is_the_one_listed():
    assert sorted(ac.mutants()) == sorted(MUTANTS)


@pytest.mark.parametrize("name", MUTANTS)
def test_every_mutant_breaks_a_contract_on_the_committed_sets(name):
    why = ac.mutant_caught(name)
    assert why, f"mutant survived: {name}"
    print(f"{name}: {why}")


def test_the_unmutated_model_passes_the_mutants_sets_inside_its_domain():
    """the sets that catch a mutated MODEL do not trip the true one (the domain mutants -- slack, 16q on 61 bits, 2^53 --
    have no true model inside the domain and are left out)"""
    for name in ("under2 drops one more partial product", "16q butterfly without the odd-stage subtraction, q just below 2^60",
                 "moddown forming 9q"):
        cs, m = ac.mutants()[name]
        for c in cs:
            ac.run_model(c, ac.Model(c.k))


def test_pack_and_decode_round_trip():
    k = ac.get_K("f41")
    for c in ac.cases(k):
        m = ac.Model(k)
        words = c.model_words(m)
        for t, wd, want in zip(c.tuples, words, ac.run_model(c, m)):
            assert c.decode(wd) == tuple(v if i in c.fout else v & ac.M64 for i, v in enumerate(want))
        assert all(0 <= v <= ac.M64 for row in c.pack() for v in row)
