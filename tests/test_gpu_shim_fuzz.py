"""Random evaluator programs on the real engine: drivers/_ref/shim_fuzz (drivers/shim_fuzz.cpp linked against libhefx.so) runs a
seed's program call by call (SEAL_SHIM_LAZY=0) and recorded, in SEPARATE processes -- hefx_malloc recycles blocks without
clearing them, so inside one process a buffer the recorded run never wrote could still hold the right words of the other
run -- and every observation line (size, rows, parms_id, scale, digest of the downloaded words of every live variable) and
every exception must be the same, bit for bit.  The call-by-call run also decrypts and decodes its final variables and
compares them with the slot model in doubles that the generator keeps (add, multiply, rotate, mask per slot; values are
multiples of 0.25, so a wrong operand moves a slot by 0.25 or more; thresholds of drivers/shim_selftest.cpp: 1e-5 for single
products, 1e-3 for sums of many; depth <= 2, magnitudes <= 8).

The corpus proper -- 160 seeds, eight configurations, unwritten and freed memory made detectable -- runs without a GPU in
tests/test_shim_fuzz_cpu.py; this file is the subset that says the real engine's fused and batched entries give the words of
the single ones under the same plans.  Replay: drivers/_ref/shim_fuzz --seed S [options] --dump [--ops K].

Whole file on an MI355X: %s."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
__doc__ = __doc__ % "NOT YET MEASURED (no device was free when the file was written); 10 tests, 26 driver processes of ~150 calls each"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "drivers", "_ref", "shim_fuzz")
# programs of the CPU corpus in which every fusion fires and a relinearize and a rescale are drawn
SEEDS = [21, 91]
CONFIGS = {
    "default": ({}, []),
    "small_budget": ({}, ["--pend-mb", "3"]),
    "ndev2": ({}, ["--ndev", "2"]),
    "fuse_add_off": ({"SEAL_SHIM_FUSE_ADD": "0"}, []),
    "chains_off": ({"SEAL_SHIM_CHAINS": "0"}, []),
    "merge_rot_off": ({"SEAL_SHIM_MERGE_ROT": "0"}, []),
}
_reference = {}  # (seed, rescale division) -> compared lines of the call-by-call run
_halted = []     # a run that died or hung: nothing more is started on the device by this file


def _run(seed, env, opts):
    if _halted:
        pytest.fail("not started: an earlier run of this file ended abnormally: " + _halted[0])
    if not os.path.exists(EXE):
        pytest.skip("drivers/_ref/shim_fuzz is not built (make -C drivers _ref/shim_fuzz)")
    cmd = [EXE, "--seed", str(seed)] + opts
    what = " ".join(f"{k}={v}" for k, v in env.items()) + " " + " ".join(cmd)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env={**os.environ, **env})
    except subprocess.TimeoutExpired:
        _halted.append(what + ": no end after 120 s")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _halted.append(f"{what}: exit {r.returncode}")
    assert r.returncode == 0, f"{what} -> exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return [l for l in r.stdout.split("\n") if l.startswith(("obs ", "throw ", "end "))], r.stdout


def _call_by_call(seed):
    key = (seed, os.environ.get("SEAL_SHIM_RESCALE", ""))
    if key not in _reference:
        lines, out = _run(seed, {"SEAL_SHIM_LAZY": "0"}, ["--decode"])  # exit code 4 if the slot model disagrees
        models = [l for l in out.split("\n") if l.startswith("model ")]
        assert models and all(l.endswith(" ok") for l in models), "\n".join(models)
        assert len(lines) > 20 and lines[-1].startswith("end ")
        _reference[key] = lines
    return _reference[key]


def _compare(seed, env, opts):
    ref = _call_by_call(seed)
    got, _ = _run(seed, env, opts)
    for i, (a, b) in enumerate(zip(ref + ["<nothing>"], got + ["<nothing>"])):
        assert a == b, (f"seed {seed} {env} {opts}: first difference at compared line {i}:\n  call by call: {a}\n  recorded:     {b}\n"
                        f"replay: drivers/_ref/shim_fuzz --seed {seed} {' '.join(opts)} --dump (shrink with --ops K)")
    assert len(got) == len(ref)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_recorded_program_leaves_the_words_of_the_call_by_call_run(config):
    env, opts = CONFIGS[config]
    for seed in SEEDS:  # one after the other; the first failure ends the test
        _compare(seed, env, opts)


@pytest.mark.parametrize("config", ["default", "small_budget"])
def test_recorded_program_in_both_rescale_divisions(config, rescale_mode):
    """(the driver's shim reads SEAL_SHIM_RESCALE; the programs rescale)"""
    env, opts = CONFIGS[config]
    _compare(SEEDS[0], env, opts)
