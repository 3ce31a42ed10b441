"""The BFV calls that moved to the device after multiply and decrypt -- encrypt, add_plain, multiply_plain, the noise budget,
BatchEncoder::encode / decode -- through the C++ shim on the MI355X, against the parent commit's shim, on one machine in
one session.

  cases       N = 8192, BFVDefault, t = 1032193 (vector_ops.cpp's BFV half; batching) and N = 4096, BFVDefault, t = 1024
              (1_bfv.cpp; no batching: the two BatchEncoder columns are absent there)
  quantities  median, min and max wall time of one call each, device idle before and after
              (drivers/bfv_front_selftest --time N t reps)
  paths       "device": this tree; "parent": the same source built with -DBFV_FRONT_PUBLIC_API_ONLY against the parent
              commit's include/ (--parent-exe, timed FIRST)
  metadata    VGPRs, SGPRs and private_segment_fixed_size (scratch bytes per lane) of every kernel instance this change
              added to csrc/hefx_bfv.hip, read from the code object metadata hipcc emits with the library's flags

Rules (the issue's):
  1  invariant_noise_budget on the device is faster than the parent's on both shapes ("noise_budget_faster_than_parent")
  2  each of the other five calls keeps the device path unless its median exceeds the parent's median by more than the
     parent's own max - min ("keeps_device_path" per call and case)
  3  "scratch_free": every new kernel instance has private_segment_fixed_size 0 -- checkable anywhere (--metadata-only)

Without --parent-exe (or with --metadata-only) the timing part is absent and the file says "status": "NOT MEASURED" with
what is owed.

Usage: bfv_front_bench.py [--out profiles/bfv_front.json] [--reps 9] [--parent-exe PATH] [--metadata-only]"""
import json, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seal_fyp_logistic_regression_amd import _build

CASES = [(8192, 1032193, "vector_ops.cpp"), (4096, 1024, "1_bfv.cpp")]
CALLS = ("encrypt", "add_plain", "multiply_plain", "noise_budget", "batch_encode", "batch_decode")
NEW_KERNELS = ("bfv_scale_add_kernel", "bfv_lift_plain_kernel", "bfv_noise_bits_kernel", "bfv_budget_finish_kernel",
               "bfv_slot_scatter_kernel", "bfv_slot_reduce_kernel", "bfv_slot_gather_kernel")


def kernel_metadata():
    """[{kernel, instance, vgprs, sgprs, scratch_bytes}] from the amdhsa.kernels metadata of the device assembly"""
    cmd = [_build.hipcc()] + _build.DEVICE_FLAGS + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, "hefx_bfv.hip"), "-o", "-"]
    asm = subprocess.check_output(cmd, text=True)
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = []
    for block in re.split(r"\n  - ", meta)[1:]:
        field = lambda key: re.search(r"\n    \." + key + r":\s+(\S+)", "\n    " + block)  # kernel-level keys, not an argument's
        name = field("name") and field("name").group(1)
        m = name and re.search(r"(" + "|".join(NEW_KERNELS) + r")(?:ILi(\d+)E)?", name)
        if m:
            get = lambda key: int(field(key).group(1))
            out.append({"kernel": m.group(1), "instance": int(m.group(2)) if m.group(2) else None, "vgprs": get("vgpr_count"),
                        "sgprs": get("sgpr_count"), "scratch_bytes": get("private_segment_fixed_size")})
    return sorted(out, key=lambda r: (r["kernel"], r["instance"] or 0))


def timed(exe, n, t, reps):
    r = subprocess.run([exe, "--time", str(n), str(t), str(reps)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{exe} --time {n} {t}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    args = sys.argv[1:]
    opt = lambda name, default=None: args[args.index(name) + 1] if name in args else default
    out_path, reps, parent = opt("--out"), int(opt("--reps", "9")), opt("--parent-exe")
    out = {"tool": "tools/bfv_front_bench.py", "box_clock": time.strftime("%Y-%m-%dT%H:%M:%S%z"), "library_sha16": _build.library_sha16(),
           "source_sha16": _build.source_sha16(), "reps": reps, "kernels": kernel_metadata(), "cases": []}
    out["scratch_free"] = bool(out["kernels"]) and all(k["scratch_bytes"] == 0 for k in out["kernels"])
    if "--metadata-only" in args or not parent:
        out["status"] = "NOT MEASURED"
        out["owed"] = ("on one MI355X, one session: drivers/bfv_front_selftest built with -DBFV_FRONT_PUBLIC_API_ONLY against the "
                       "parent commit's include/ and passed as --parent-exe (timed first), then this tree; 9 repetitions at "
                       "(8192, 1032193) and (4096, 1024).  Until then rule 2 is undecided and every device path is on.")
    else:
        exe = os.path.join(ROOT, "drivers", "_ref", "bfv_front_selftest")
        if not os.path.exists(exe):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "drivers"), "_ref/bfv_front_selftest"])
        out["status"] = "MEASURED"
        out["parent"] = "the parent commit's include/seal/seal.h, timed first in the same session"
        for n, t, where in CASES:
            old = timed(parent, n, t, reps)
            new = timed(exe, n, t, reps)
            row = {"N": n, "t": t, "driver": where, "on_device": new["on_device"], "batching": new["batching"], "calls": {}}
            for call in CALLS:
                if call not in new or call not in old:
                    continue
                d, p = new[call], old[call]  # {median_ms, min_ms, max_ms}
                entry = {"device": d, "parent": p, "parent_over_device": p["median_ms"] / d["median_ms"]}
                if call == "noise_budget":
                    entry["faster_than_parent"] = bool(new["on_device"] and d["median_ms"] < p["median_ms"])
                else:
                    entry["keeps_device_path"] = bool(d["median_ms"] - p["median_ms"] <= p["max_ms"] - p["min_ms"])
                row["calls"][call] = entry
            out["cases"].append(row)
            print(row, flush=True)
        out["noise_budget_faster_than_parent"] = all(r["calls"]["noise_budget"]["faster_than_parent"] for r in out["cases"])
        out["calls_that_fall_back_to_the_host_by_rule_2"] = sorted(
            {c for r in out["cases"] for c, e in r["calls"].items() if e.get("keeps_device_path") is False})
    print(json.dumps(out))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
