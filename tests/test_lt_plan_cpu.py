"""csrc/hefx_lt_plan.h -- the rotation planner of the linear transforms -- without a GPU: drivers/lt_plan_selftest.cpp checks
its invariants (plans, flat store, forest, lane dealing) as a stand-alone program under AddressSanitizer and UBSan (nothing
loaded into Python is sanitised), and what it prints is held, element for element, to the independent Python planner:
seal.naf / seal.galois_elt_from_step / Evaluator.rotation_plan for the plans and the refusals, and the forest
algorithms._rotations_batched hands to a recording backend's apply_galois_forest."""
import os
import shutil
import subprocess
import types

import pytest

from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import seal as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """the program's output, built and run exactly like tests/test_aliasing_cpu.py runs the range check's"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build drivers/lt_plan_selftest.cpp"
    exe = str(tmp_path_factory.mktemp("lt_plan") / "lt_plan_selftest")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "drivers", "lt_plan_selftest.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "LT PLAN SELFTEST PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "FAIL" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout.splitlines()


def test_lt_plan_selftest_under_asan_and_ubsan(printed):
    """the invariants hold, and the forests the GPU tests run on two lanes are above run_forest's 96-node bound"""
    sizes = {ln.split(":")[0]: int(ln.split(":")[1].split()[0]) for ln in printed if ln.startswith("d = 160")}
    assert set(sizes) == {"d = 160, default keys, fused", "d = 160, default keys, unfused"} and min(sizes.values()) >= 96, sizes


class _Keys:
    """Galois keys by element: SEAL's default set (KeyGenerator.default_galois_elts), optionally without the key of +4"""

    def __init__(self, N, without_plus_4):
        logn = N.bit_length() - 1
        self.elts = {2 * N - 1} | {pow(3, 1 << i, 2 * N) for i in range(logn - 1)} | {pow(3, N // 2 - (1 << i), 2 * N) for i in range(logn - 1)}
        if without_plus_4:
            self.elts.remove(S.galois_elt_from_step(4, N))

    def has_key(self, elt):
        return elt in self.elts

    def key(self, elt):
        assert elt in self.elts
        return ("key", elt)


class _Recorder:
    """a backend that only records the forest it is handed"""

    def apply_galois_forest(self, L, parents, ext_ins, elts, keys, pts=None):
        assert all(k == ("key", e) for k, e in zip(keys, elts)) and all((x is not None) == (p < 0) for x, p in zip(ext_ins, parents))
        self.forest = list(zip(parents, elts, pts))
        return [("node", i) for i in range(len(parents))]


def _evaluator(N, backend=None):
    ev = types.SimpleNamespace(ctx=types.SimpleNamespace(N=N), be=backend, _check_scale=lambda scale, L: None)
    ev.rotation_plan = lambda steps, gk: S.Evaluator.rotation_plan(ev, steps, gk)
    ev._plain_product_scale = lambda *a: S.Evaluator._plain_product_scale(ev, *a)
    return ev


CASES = [(32, [s for a in range(1, 16) for s in (a, -a)], 15), (4096, [-160] + list(range(1, 161)), 160)]


@pytest.mark.parametrize("N,steps,d", CASES, ids=["N32", "N4096"])
@pytest.mark.parametrize("keyset", ["default", "no+4"])
def test_plans_and_refusals_are_the_python_planners(printed, N, steps, d, keyset):
    gk, ev = _Keys(N, keyset == "no+4"), _evaluator(N)
    got = {}
    for ln in printed:
        w = ln.split()
        if w[:3] == ["PLAN", str(N), keyset]:
            got[int(w[3])] = ln.split("! ", 1)[1] if w[4] == "!" else [int(x) for x in w[5:]]
    assert sorted(got) == sorted(steps)
    refused = 0
    for s in steps:
        try:
            want = ev.rotation_plan(s, gk)
        except ValueError as e:
            want, refused = str(e), refused + 1
        assert got[s] == want, (N, keyset, s)
        if not isinstance(want, str):   # ... and the plan is SEAL's: the direct key, else the NAF terms in order
            direct = S.galois_elt_from_step(s, N)
            assert want == ([direct] if gk.has_key(direct) else [S.galois_elt_from_step(t, N) for t in S.naf(s) if abs(t) != N // 2])
    assert (refused > 0) == (keyset == "no+4")
    for s in (N // 2, -N // 2):   # both planners refuse these with the same words (the program asserts its side itself)
        with pytest.raises(ValueError, match="step count too large"):
            ev.rotation_plan(s, gk)


@pytest.mark.parametrize("N,steps,d", CASES, ids=["N32", "N4096"])
def test_fused_forest_is_the_one_the_python_planner_builds(printed, N, steps, d):
    """node for node: parent, element and the diagonal whose product rides in the node's key switch"""
    got = [tuple(int(x) for x in ln.split()[5:]) for ln in printed if ln.split()[:4] == ["NODE", str(N), "default", str(d)]]
    rec = _Recorder()
    ct = types.SimpleNamespace(data="ct", parms_id=lambda: 2, scale=1.0)
    # plaintexts that are their own diagonal index
    diag = [types.SimpleNamespace(data=l, scale=1.0, _scale=1.0, parms_id=lambda: 2, _parms_id=2, is_zero=False) for l in range(1, d)]
    outs = alg._rotations_batched(_evaluator(N, rec), ct, list(range(1, d)), _Keys(N, False), diag)
    want = [(p, e, -1 if pt is None else pt) for p, e, pt in rec.forest]
    assert len(got) == len(want) and got == want
    assert len(outs) == d - 1
    # without the key of +4 both refuse the whole transform, with the same words
    assert f"FOREST_REFUSED {N} no+4 {d} ! Galois key not present" in printed
    with pytest.raises(ValueError, match="^Galois key not present$"):
        alg._rotations_batched(_evaluator(N, _Recorder()), ct, list(range(1, d)), _Keys(N, True), diag)
