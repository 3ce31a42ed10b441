"""The aliasing rule of the C-ABI, the parts that need no GPU: every entry of include/hefx.h that reads device inputs and
writes a device output has a row in tests/aliasing_cases.py (a new entry cannot be added without a rule), the rows name
tests that exist, INTEGRATION.md prints the table, and csrc/hefx_ranges.h -- the one check behind the rule -- agrees with a
plain O(n^2) interval comparison on a few thousand random layouts, under AddressSanitizer and UBSan, as a stand-alone
program (nothing loaded into Python is sanitised)."""
import os
import re
import shutil
import subprocess

import pytest

from tests import aliasing_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declarations():
    """{entry: [parameter declarations]} of include/hefx.h, parsed like tests/test_capi_cpu.py (comments stripped)"""
    src = open(os.path.join(ROOT, "include", "hefx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")]
            for m in re.finditer(r"\b(hefx_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src)}


def _entries_with_device_inputs_and_outputs():
    names = []
    for name, params in _declarations().items():
        reads = any(re.match(r"const uint64_t \*(const \*)?\s*d_\w+$", p) for p in params)
        writes = any(re.match(r"uint64_t \*(const \*)?\s*d_\w+$", p) for p in params)
        if reads and writes:
            names.append(name)
    return sorted(names)


def test_the_parser_sees_the_entries_it_is_about():
    got = _entries_with_device_inputs_and_outputs()
    assert len(got) >= 40, got
    for known in ("hefx_add", "hefx_add_many", "hefx_add_batch", "hefx_rescale_to_next_batch", "hefx_mod_drop", "hefx_decrypt",
                  "hefx_encrypt_batch", "hefx_linear_transform_plain_hoisted2_sparse", "hefx_rotate_hoisted_batch",
                  "hefx_apply_galois_forest"):
        assert known in got, known
    # host pointers, in-place-only entries and entries without a device input are not its business
    for other in ("hefx_context_create", "hefx_ntt_forward", "hefx_reduce_canonical", "hefx_ckks_encode", "hefx_ckks_decode",
                  "hefx_sample_uniform", "hefx_ks_stats"):
        assert other not in got, other


def test_every_entry_with_device_inputs_and_a_device_output_has_a_rule():
    want = _entries_with_device_inputs_and_outputs()
    missing = [n for n in want if n not in A.RULES]
    assert not missing, f"no aliasing rule in tests/aliasing_cases.py for {missing}"
    stale = [n for n in A.RULES if n not in want]
    assert not stale, f"tests/aliasing_cases.py has rows for entries the header does not declare: {stale}"


def test_every_row_is_whole_and_names_a_test_that_exists():
    for name, row in A.RULES.items():
        assert row["kind"] in (A.IN_PLACE, A.IN_PLACE_SUM, A.NO_OVERLAP, A.UNCHANGED), name
        assert row["serves"] or row["refuses"], name
        if row["kind"] in (A.IN_PLACE, A.IN_PLACE_SUM):
            assert row["serves"] and row["refuses"], name
        if row["kind"] == A.NO_OVERLAP:
            assert not row["serves"] and row["refuses"], name
        path, test = row["test"].split("::")
        text = open(os.path.join(ROOT, path)).read()
        assert re.search(rf"^def {re.escape(test)}\(", text, flags=re.M), (name, row["test"])
        if path == A.G:  # the new GPU tests are driven by name: the entry must occur in the file that claims it
            assert re.search(rf"\b{name}\b", text), (name, path)


def test_integration_md_prints_the_table():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## Aliasing" in text
    section = text.split("## Aliasing", 1)[1]
    for name, row in A.RULES.items():
        line = next((ln for ln in section.splitlines() if ln.startswith(f"| `{name}`")), None)
        assert line is not None, f"INTEGRATION.md's aliasing table has no row for {name}"
        assert row["kind"] in line, (name, line)
        assert row["test"].split("::")[1] in line, (name, line)


def test_the_header_states_the_rule_per_entry():
    """every entry the table gives a rule has the words in the comment in front of its declaration (or of the group of
    declarations it belongs to): 'alias', 'overlap' or 'in place'"""
    src = open(os.path.join(ROOT, "include", "hefx.h")).read()
    for name in A.RULES:
        at = re.search(rf"\bint {name}\(", src).start()
        before = src[:at]
        comment = before[before.rfind("/*"):]
        assert re.search(r"alias|overlap|in place|in-place", comment), f"include/hefx.h states no aliasing rule in front of {name}"


def test_ranges_selftest_under_asan_and_ubsan(tmp_path):
    """drivers/ranges_selftest.cpp: hefx_ranges.h against the slow interval comparison, 6000 seeded layouts"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build drivers/ranges_selftest.cpp"
    exe = str(tmp_path / "ranges_selftest")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "drivers", "ranges_selftest.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "RANGES SELFTEST PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "FAIL" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
