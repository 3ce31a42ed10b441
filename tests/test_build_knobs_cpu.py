"""Every compile-time knob the tree still documents must keep compiling: the front end of hipcc
(-fsyntax-only, device pass, every template instantiated; no code generation, so seconds per knob instead of minutes)
over hefx_keyswitch.hip with each -DHEFX_* define.  The knobs whose experiments are closed were deleted in round 4
(HEFX_EPI*, HEFX_MAC_WAVES, HEFX_MAC_GROUP, HEFX_NB_FWD, HEFX_EO_LANE_MIN, HEFX_INV_NAT) and after round 6 (the A/B
knobs of round 3's adopted changes, and the runtime switches of closed experiments): profiles/EXPERIMENTS.md.
The environment variables the library reads are pinned the same way (RUNTIME_KNOBS)."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seal_fyp_logistic_regression_amd", "csrc")
# knob -> what it is for (the documentation the test keeps honest)
KNOBS = {
    "-DHEFX_ONLY_LOGN=14": "development builds that instantiate one ring size (tools/build_variant.sh, tools/probe_ks.sh)",
    "-DHEFX_ONLY_LOGN=13": "... any ring size",
    "-DHEFX_STAMP=1": "clock stamps inside the small-batch kernels (tools/stamp_timeline.py)",
    "-DHEFX_SMALL_MAX=8": "how many descriptors travel in the first launch's kernel arguments",
}
# environment variable -> what it is for.  Test levers force a path that the automatic rules also take, so the tests can
# reach it at any size; none selects a path of its own.
RUNTIME_KNOBS = {
    "HEFX_CHUNK": "test lever: items per launch sequence (default: sized from the scratch budget)",
    "HEFX_STREAMS": "test lever: =0 runs the chunks serially on the caller's stream (no internal streams)",
    "HEFX_NO_FP64": "test lever: the integer arithmetic policy for every prime (no FP64 policy below 2^41)",
    "HEFX_QUARTER": "test lever: =0/1 quarter-row workgroups for none / all launches of a small batch",
    "HEFX_QMASK": "test lever: any mask of quarter-row launches and the pair path for a small batch",
    "HEFX_PAIR": "test lever: =0/1 the small-batch pair path off / on",
    "HEFX_SHARE_SRC": "test lever: =0 switches exact hoisting of shared sources off",
    "HEFX_FLIPW_MB": "test lever: memory budget of exact hoisting's flip-mask tables",
    "HEFX_POOL_MB": "test lever: how much freed device memory the hefx_malloc pool keeps parked",
    "HEFX_LT_LANES": "test lever: =0 runs a rotation forest on one lane",
    "HEFX_RESCALE": "semantics: =floor presets floor division for rescale_to_next (the default rounds)",
    "HEFX_DEBUG": "diagnostics: host-side timings and occupancy on stderr",
}


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_documented_build_knobs_are_exactly_the_ones_in_the_sources():
    """a knob in the sources that this file does not list (or the other way round) fails: no silent growth"""
    found = set()
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".cuh", ".h", ".cpp")):
            for m in re.finditer(r"#\s*if(?:n?def|)\s+(?:!?\s*defined\s*\(\s*)?(HEFX_[A-Z0-9_]+)", open(os.path.join(CSRC, f)).read()):
                found.add(m.group(1))
    internal = {"HEFX_STAGE_FENCE", "HEFX_H", "HEFX_GLOBAL_AS"}  # macros, not knobs
    listed = {re.match(r"-D(HEFX_[A-Z0-9_]+)", k).group(1) for k in KNOBS}
    assert found - internal == listed, (sorted(found - internal - listed), sorted(listed - found))


def test_documented_runtime_knobs_are_exactly_the_ones_the_library_reads():
    """an environment variable the library reads that this file does not list (or the other way round) fails"""
    found = set()
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".cuh", ".h", ".cpp")):
            found.update(re.findall(r'getenv\("(HEFX_[A-Z0-9_]+)"\)', open(os.path.join(CSRC, f)).read()))
    assert found == set(RUNTIME_KNOBS), (sorted(found - set(RUNTIME_KNOBS)), sorted(set(RUNTIME_KNOBS) - found))


def test_every_documented_knob_still_compiles():
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc in this environment")
    src = os.path.join(CSRC, "hefx_keyswitch.hip")

    def one(flag):
        extra = [] if "ONLY_LOGN" in flag else ["-DHEFX_ONLY_LOGN=14"]  # one ring size is enough for a syntax pass
        cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", "-std=c++17", "-x", "hip", flag, *extra, src]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        return flag, r.returncode, r.stderr[-1500:]

    with ThreadPoolExecutor(max_workers=4) as ex:
        results = list(ex.map(one, KNOBS))
    bad = [(f, err) for f, rc, err in results if rc != 0]
    assert not bad, bad
