"""BFV square and decrypt through the C++ shim on the MI355X: the device path (include/hefx_bfv.h) against the host path it
replaced, and against the parent commit's shim, on one machine in one session.

  cases       N = 8192, BFVDefault, t = 1032193 (vector_ops.cpp's BFV half) and N = 4096, BFVDefault, t = 1024 (1_bfv.cpp)
  quantities  median wall time of one Evaluator::square and one Decryptor::decrypt, device idle before and after
              (drivers/bfv_selftest --time N t reps)
  paths       "device": what the shim does now; "host": shim_bfv.h multiply_host / decrypt_round_host, alternating with the
              device path in the same process; "parent": the same source built with -DBFV_SELFTEST_PUBLIC_API_ONLY against
              the parent commit's include/ (--parent-exe, timed first) -- without it the host path stands in and the file
              says so
  metadata    VGPRs, SGPRs and private_segment_fixed_size (scratch bytes per lane) of every bfv_round_kernel instance, read
              from the code object metadata hipcc emits for csrc/hefx_bfv.hip with the library's flags

The only condition: the device path is faster than the parent's on both shapes ("device_faster_than_parent").

Usage: bfv_bench.py [--out profiles/bfv_multiply.json] [--reps 9] [--parent-exe PATH] [--metadata-only]"""
import json, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seal_fyp_logistic_regression_amd import _build

CASES = [(8192, 1032193, "vector_ops.cpp"), (4096, 1024, "1_bfv.cpp")]


def kernel_metadata():
    """[{kernel, rows, plain, vgprs, sgprs, scratch_bytes}] from the amdhsa.kernels metadata of the device assembly"""
    cmd = [_build.hipcc()] + _build.DEVICE_FLAGS + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, "hefx_bfv.hip"), "-o", "-"]
    asm = subprocess.check_output(cmd, text=True)
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = []
    for block in re.split(r"\n  - ", meta)[1:]:
        field = lambda key: re.search(r"\n    \." + key + r":\s+(\S+)", "\n    " + block)  # kernel-level keys, not an argument's
        m = field("name") and re.search(r"bfv_round_kernelILi(\d+)ELb([01])E", field("name").group(1))
        if m:
            get = lambda key: int(field(key).group(1))
            out.append({"kernel": f"bfv_round_kernel<{m.group(1)}, {'true' if m.group(2) == '1' else 'false'}>", "rows": int(m.group(1)),
                        "plain": m.group(2) == "1", "vgprs": get("vgpr_count"), "sgprs": get("sgpr_count"),
                        "scratch_bytes": get("private_segment_fixed_size")})
    return sorted(out, key=lambda r: (r["plain"], r["rows"]))


def timed(exe, n, t, reps):
    r = subprocess.run([exe, "--time", str(n), str(t), str(reps)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{exe} --time {n} {t}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    args = sys.argv[1:]
    opt = lambda name, default=None: args[args.index(name) + 1] if name in args else default
    out_path, reps, parent = opt("--out"), int(opt("--reps", "9")), opt("--parent-exe")
    out = {"tool": "tools/bfv_bench.py", "box_clock": time.strftime("%Y-%m-%dT%H:%M:%S%z"), "library_sha16": _build.library_sha16(),
           "source_sha16": _build.source_sha16(), "reps": reps, "kernels": kernel_metadata(), "cases": []}
    out["scratch_free"] = all(k["scratch_bytes"] == 0 for k in out["kernels"])
    if "--metadata-only" not in args:
        exe = os.path.join(ROOT, "drivers", "_ref", "bfv_selftest")
        if not os.path.exists(exe):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "drivers"), "_ref/bfv_selftest"])
        out["parent"] = ("the parent commit's include/seal/seal.h, timed first in the same session" if parent else
                         "not given: the host path of this commit (the parent's code, moved to shim_bfv.h) stands in")
        for n, t, where in CASES:
            old = timed(parent, n, t, reps) if parent else None
            new = timed(exe, n, t, reps)
            p_sq = old["square_ms"] if old else new["square_host_ms"]
            p_dec = old["decrypt_ms"] if old else new["decrypt_host_ms"]
            row = {"N": n, "t": t, "driver": where, "on_device": new["on_device"],
                   "square_ms": {"device": new["square_ms"], "host": new["square_host_ms"], "parent": p_sq},
                   "decrypt_ms": {"device": new["decrypt_ms"], "host": new["decrypt_host_ms"], "parent": p_dec},
                   "square_parent_over_device": p_sq / new["square_ms"], "decrypt_parent_over_device": p_dec / new["decrypt_ms"]}
            row["device_faster_than_parent"] = bool(new["on_device"] and new["square_ms"] < p_sq and new["decrypt_ms"] < p_dec)
            out["cases"].append(row)
            print(row, flush=True)
        out["device_faster_than_parent"] = all(r["device_faster_than_parent"] for r in out["cases"])
    print(json.dumps(out))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
