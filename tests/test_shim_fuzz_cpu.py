"""Random evaluator programs through include/seal/seal.h's recorder and fusion planner, WITHOUT a GPU: drivers/shim_fuzz.cpp
linked against the symbolic engine of drivers/hefx_symbolic.cpp (tools/make_symbolic_libhefx.py builds both with g++ into
build/symbolic/; removed afterwards -- the stand-in library is named like the real one).

For every seed the program runs call by call (SEAL_SHIM_LAZY=0, one device, default budget: the reference) and then recorded
under eight configurations, every run a process of its own; every observation line -- size, rows, parms_id, scale and a digest
of the downloaded words of every live variable -- and every exception (type and text) must be the same.  The symbolic engine
makes a buffer that was never written, or freed and recycled, detectable (poison), which a comparison on a real device is
not: hefx_malloc recycles blocks without clearing them.  It proves dataflow, liveness and ordering of the shim's calls; it
proves nothing about the kernels' arithmetic (the oracle tests judge that).

A failure names the seed, the configuration and the first differing variable; replay and shrink it with
    python tools/make_symbolic_libhefx.py && build/symbolic/shim_fuzz --seed S [the configuration's options] --dump --ops K

Measured here (8 cores, 8 worker threads): %(seeds)d seeds x 9 runs + 3 chain programs of 2000 rotate+add pairs x 3 runs in
about %(seconds)s s, build included; a program is 24 top-level draws, ~150 calls.  The sanitizer test: 8 seeds x 4 runs, 23 s
with its build (-O0); the whole file about a minute."""
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
__doc__ = __doc__ % {"seeds": len(range(1, 161)), "seconds": "36"}

# programs that once failed come first, each with what went wrong: (seed, extra options)
FIXED = [
]
SEEDS = list(range(1, 161))
CHAIN_SEEDS = [9001, 9002, 9003]
# name -> (environment, options); options may use {seed}
CONFIGS = {
    "default": ({}, []),
    "small_budget": ({}, ["--pend-mb", "{budget}"]),
    "ndev2": ({}, ["--ndev", "2"]),
    "ndev3": ({}, ["--ndev", "3"]),
    "fuse_add_off": ({"SEAL_SHIM_FUSE_ADD": "0"}, []),
    "chains_off": ({"SEAL_SHIM_CHAINS": "0"}, []),
    "merge_rot_off": ({"SEAL_SHIM_MERGE_ROT": "0"}, []),
    "sync": ({"SEAL_SHIM_SYNC": "1"}, []),
}
BOOKKEEPING = {"hefx_malloc", "hefx_free", "hefx_upload", "hefx_download", "hefx_stream_sync", "hefx_context_create", "hefx_context_destroy"}
CLEAN_ENV = {k: v for k, v in os.environ.items() if not k.startswith(("SEAL_SHIM_", "HEFX_"))}


class Run:
    def __init__(self, exe, seed, env, opts, timeout=120):
        self.cmd = [exe, "--seed", str(seed)] + opts
        self.env = env
        r = subprocess.run(self.cmd, capture_output=True, text=True, timeout=timeout, env={**CLEAN_ENV, "HEFX_SYMBOLIC_LOG": "1", **env})
        self.rc, self.out, self.err = r.returncode, r.stdout, r.stderr
        self.lines = [l for l in r.stdout.split("\n") if l.startswith(("obs ", "throw ", "end "))]
        self.log = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"hefx-symbolic-log (hefx_\w+) calls=(\d+) items=(\d+)", r.stderr)}
        m = re.search(r"with_plaintext=(\d+) without_plaintext=(\d+)", r.stderr)
        self.fused_products, self.plain_in_fused_batch = (int(m.group(1)), int(m.group(2))) if m else (0, 0)
        m = re.search(r"copied_home_for_nobody=(\d+)", r.stderr)
        self.copied_home_for_nobody = int(m.group(1)) if m else 0
        m = re.search(r"^motifs (.*)$", r.stdout, flags=re.M)
        self.motifs = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in m.group(1).split()} if m else {}
        stats = re.findall(r"^stat \d+ calls=(\d+) flushes=(\d+) nodes=(\d+)", r.stdout, flags=re.M)
        self.stats = tuple(int(x) for x in stats[-1]) if stats else (0, 0, 0)
        self.throws = [l.split(" ", 2)[2] for l in self.lines if l.startswith("throw ")]

    def calls(self, name):
        return self.log.get(name, (0, 0))[0]

    def engine_calls(self):
        return sum(c for n, (c, _) in self.log.items() if n not in BOOKKEEPING)

    def describe(self):
        env = " ".join(f"{k}={v}" for k, v in self.env.items())
        return (env + " " if env else "") + " ".join(["build/symbolic/shim_fuzz"] + self.cmd[1:])


def _sound(run):
    assert run.rc == 0 and "hefx-symbolic-error" not in run.err and "FATAL" not in run.out, \
        f"{run.describe()} -> exit {run.rc}\n{run.out[-1500:]}\n{run.err[-3000:]}"


def _same(ref, run):
    _sound(run)
    if run.lines == ref.lines:
        return
    for i, (a, b) in enumerate(zip(ref.lines + ["<nothing>"], run.lines + ["<nothing>"])):
        if a != b:
            raise AssertionError(f"first difference at compared line {i}:\n  call by call: {a}\n  recorded:     {b}\n"
                                 f"replay: {run.describe()} --dump   (shrink with --ops K)\nreference: {ref.describe()}")
    raise AssertionError(f"{run.describe()}: {len(run.lines)} compared lines, the reference has {len(ref.lines)}")


def _opts(opts, seed):
    return [o.format(budget=1 + seed % 8) for o in opts]


def _one_seed(exe, seed, extra, configs):
    ref = Run(exe, seed, {"SEAL_SHIM_LAZY": "0"}, list(extra))
    _sound(ref)
    runs = {}
    for name in configs:
        env, opts = CONFIGS[name]
        runs[name] = Run(exe, seed, env, list(extra) + _opts(opts, seed))
        _same(ref, runs[name])
    return ref, runs


def _build(sanitize):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_symbolic_libhefx.py")] + (["--sanitize"] if sanitize else []),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(ROOT, "build", "symbolic_san" if sanitize else "symbolic", "shim_fuzz")


@pytest.fixture(scope="module")
def corpus():
    """every seed under every configuration, compared; -> {seed: (reference run, {configuration: run})}"""
    try:
        exe = _build(False)
        jobs = [(s, o) for s, o in FIXED] + [(s, []) for s in SEEDS]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            results = list(pool.map(lambda j: _one_seed(exe, j[0], j[1], list(CONFIGS)), jobs))
        chains = []
        for s in CHAIN_SEEDS:  # 2000 pairs: the recorded results (1.5 GB) pass any small budget, the plan says what would be stored
            ref = Run(exe, s, {"SEAL_SHIM_LAZY": "0"}, ["--chain", "2000", "--steps", "6"])
            _sound(ref)
            runs = [Run(exe, s, {}, ["--chain", "2000", "--steps", "6", "--pend-mb", mb]) for mb in ("8", "64")]
            for r in runs:
                _same(ref, r)
            chains.append((ref, runs))
        yield {"seeds": results, "chains": chains}
    finally:  # the stand-in library never outlives the test (it is named like the real one)
        shutil.rmtree(os.path.join(ROOT, "build", "symbolic"), ignore_errors=True)


def test_recorded_runs_equal_call_by_call_runs_in_every_configuration(corpus):
    """(the comparison itself happens while the corpus runs: a difference fails here with seed, configuration and line)"""
    assert len(corpus["seeds"]) == len(FIXED) + len(SEEDS) and len(corpus["chains"]) == len(CHAIN_SEEDS)
    for ref, runs in corpus["seeds"]:
        assert set(runs) == set(CONFIGS) and ref.lines and ref.lines[-1].startswith("end ")


def test_every_motif_occurs_in_at_least_20_programs(corpus):
    for m in "abcdefghijkl":
        n = sum(1 for ref, _ in corpus["seeds"] if ref.motifs.get(m, 0) > 0)
        assert n >= 20, f"motif ({m}) occurs in {n} programs"


def test_every_fusion_fires_in_at_least_20_programs_and_never_when_switched_off(corpus):
    fired = {"product in the key switch": 0, "hefx_apply_galois_add_batch": 0, "hefx_rotate_add_chain": 0}
    for ref, runs in corpus["seeds"]:
        d = runs["default"]
        fired["product in the key switch"] += d.fused_products > 0
        fired["hefx_apply_galois_add_batch"] += d.calls("hefx_apply_galois_add_batch") > 0
        fired["hefx_rotate_add_chain"] += d.calls("hefx_rotate_add_chain") > 0
        # the reference makes no fused or batched call at all
        assert ref.calls("hefx_rotate_multiply_plain_batch") == ref.calls("hefx_apply_galois_add_batch") == ref.calls("hefx_rotate_add_chain") == 0
        off = runs["fuse_add_off"]
        assert off.calls("hefx_apply_galois_add_batch") == 0 and off.calls("hefx_rotate_add_chain") == 0, off.describe()
        assert runs["chains_off"].calls("hefx_rotate_add_chain") == 0, runs["chains_off"].describe()
        assert runs["merge_rot_off"].plain_in_fused_batch == 0, runs["merge_rot_off"].describe()
    for what, n in fired.items():
        assert n >= 20, f"{what}: reached in {n} programs of the default configuration"
    # the plain rotations do ride in the fused batch when the merge is on, somewhere
    assert sum(runs["default"].plain_in_fused_batch for _, runs in corpus["seeds"]) > 0


def test_recording_saves_engine_calls(corpus):
    ref_calls = sum(ref.engine_calls() for ref, _ in corpus["seeds"])
    rec_calls = sum(runs["default"].engine_calls() for _, runs in corpus["seeds"])
    assert 0 < rec_calls < ref_calls, (rec_calls, ref_calls)
    # and the shim's own counter counts the recorded runs' batched calls (the reference records nothing)
    assert all(ref.stats == (0, 0, 0) for ref, _ in corpus["seeds"])
    assert sum(runs["default"].stats[0] for _, runs in corpus["seeds"]) > 0


def test_a_second_device_copies_home_only_what_somebody_holds(corpus):
    """flush_multi copies a result home when somebody outside the graph holds it (use_count() - 1 - inner[i], inner counted per
    OPERAND: add(x, x) and square(x) hold x twice).  A count that is off copies a result nobody will read -- the words stay
    right, so the symbolic engine counts it instead: a block written by hefx_copy_peer_to and freed before any engine call
    could read it.  (Default budget only: see drivers/hefx_symbolic.cpp.)"""
    copies = 0
    for _, runs in corpus["seeds"]:
        for name in ("ndev2", "ndev3"):
            assert runs[name].copied_home_for_nobody == 0, runs[name].describe()
            copies += runs[name].calls("hefx_copy_peer_to")
        assert runs["default"].calls("hefx_copy_peer_to") == 0
    assert copies >= 1000, copies  # (4431 when this was written: the second device does get work)


def test_illegal_calls_throw_the_same_text_in_both_modes(corpus):
    """(the throw lines are part of the compared output; here: that there were any, of every kind)"""
    texts = {}
    for ref, runs in corpus["seeds"]:
        for name, run in runs.items():
            assert run.throws == ref.throws, run.describe()
        for t in set(ref.throws):
            texts[t] = texts.get(t, 0) + 1
    for needle in ("encrypted1 and encrypted2 parameter mismatch", "scale mismatch", "step count too large", "Galois key not present",
                   "result ciphertext is transparent", "scale out of bounds", "encrypted size must be 2", "end of modulus switching chain reached"):
        n = sum(c for t, c in texts.items() if needle in t)
        assert n >= 5, f"'{needle}' thrown in {n} programs: {sorted(texts)}"


def test_2000_pair_chains_are_estimated_by_the_plan_not_flushed(corpus):
    for ref, runs in corpus["chains"]:
        for run in runs:
            calls, flushes, nodes = run.stats
            # 4000 recorded results of 384 KB pass the budget (8 or 64 MB) every few calls; the fusion plan finds that the chain
            # stores two of them, so the recording goes on: a handful of submissions, one hefx_rotate_add_chain of 2000 steps
            assert nodes >= 4000 and flushes <= 30, (run.describe(), run.stats)
            assert run.calls("hefx_rotate_add_chain") >= 1, run.describe()
        assert ref.calls("hefx_apply_galois") >= 2000


def test_fuzz_driver_and_symbolic_engine_are_clean_under_asan_and_ubsan():
    """the same driver and library built with -fsanitize=address,undefined, as the stand-alone program it is (nothing is preloaded,
    nothing is loaded into Python): recorder, planner, multi-device submission and the symbolic engine touch no freed or foreign
    memory on a smaller corpus"""
    try:
        exe = _build(True)
        env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
        def one(seed):
            ref = Run(exe, seed, {"SEAL_SHIM_LAZY": "0", **env}, [], timeout=300)
            _sound(ref)
            for name in ("default", "small_budget", "ndev3"):
                e, opts = CONFIGS[name]
                run = Run(exe, seed, {**e, **env}, _opts(opts, seed), timeout=300)
                _same(ref, run)
                for r in (ref, run):
                    assert "runtime error" not in r.err and "AddressSanitizer" not in r.err and "LeakSanitizer" not in r.err, r.err[-4000:]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            list(pool.map(one, range(1, 9)))
    finally:
        shutil.rmtree(os.path.join(ROOT, "build", "symbolic_san"), ignore_errors=True)
