"""What the aliasing rule costs the element-wise entries on the MI355X: two builds of libhefx.so, alternating, each run in a
process of its own (capi.py loads the library HEFX_LIB names, once per process).

  device   hefx_add (out of place and with d_out == d_a), hefx_multiply_plain at N = 16384, L = 5, size 2, count = 256 and a
           64-input hefx_add_many (N = 16384, L = 5, size 2): device events around a window of back-to-back calls sized to
           about 0.4 s, WINDOWS windows after a warm-up, microseconds per call.
  host     the range check in front of a linear transform's first launch, d = 512: host clock around calls of
           hefx_linear_transform_plain that are refused (a) by the null-pointer scan, with the last diagonal NULL -- every
           check in front of the range check has run -- and (b) by the range check, with d_out one row into the last
           diagonal -- the check has sorted the outputs and looked up all 513 inputs.  (b) - (a) is the check (and its
           message).  Nothing is submitted by either.  A library without the check is not refused in (b); the line says so.

Usage: aliasing_ew_timing.py --lib LABEL=PATH [--lib LABEL=PATH ...] [--rounds 3] [--out profiles/aliasing_ew_timing.jsonl]
One JSON line per library and round: the label, the sha256[:16] of that library file, the figures.  No paths."""
import hashlib, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOWS = 5


def child(label):
    import ctypes as C
    from seal_fyp_logistic_regression_amd import Engine, capi
    from seal_fyp_logistic_regression_amd import seal as S
    N, size, count, d = 16384, 2, 256, 512
    primes = S.CoeffModulus.Create(N, [60, 40, 40, 40, 40, 60])
    e, L = Engine(N, primes), len(primes) - 1
    lib, h, key32 = capi.lib(), e._h, bytes(range(32))
    a = e.sample("uniform", key32, 1, count * size, L)
    b = e.sample("uniform", key32, 2, count * size, L)
    pt = e.sample("uniform", key32, 3, 1, L)
    out = e.empty(count, size, L, N)
    ins = [e.sample("uniform", key32, 10 + i, size, L) for i in range(64)]
    arr = capi.ptr_array([x.ptr for x in ins])
    out1 = e.empty(size, L, N)
    ev0, ev1 = e.event(), e.event()

    def timed(f, reps):
        for _ in range(20):
            f()
        e.sync()
        res = []
        for _ in range(WINDOWS):
            e.event_record(ev0)
            for _ in range(reps):
                f()
            e.event_record(ev1)
            e.sync()
            res.append(e.event_elapsed_ms(ev0, ev1) * 1000.0 / reps)
        return {"median_us": round(statistics.median(res), 2), "min_us": round(min(res), 2), "max_us": round(max(res), 2),
                "window_ms": round(statistics.median(res) * reps / 1000.0, 1)}

    r = {"lib": label, "library_sha16": hashlib.sha256(open(capi.library_path(), "rb").read()).hexdigest()[:16],
         "add": timed(lambda: capi.check(lib.hefx_add(h, L, size, count, a.ptr, b.ptr, out.ptr, None)), 2000),
         "add_in_place": timed(lambda: capi.check(lib.hefx_add(h, L, size, count, a.ptr, b.ptr, a.ptr, None)), 2000),
         "multiply_plain": timed(lambda: capi.check(lib.hefx_multiply_plain(h, L, size, count, a.ptr, pt.ptr, out.ptr, None)), 2500),
         "add_many_64": timed(lambda: capi.check(lib.hefx_add_many(h, L, size, 64, arr, out1.ptr, None)), 12000)}
    # ---- host time of the linear transform's range check, d = 512: refused calls, nothing submitted
    slab = e.empty((d + 2) * L * N)
    diags = [slab.ptr + 8 * i * L * N for i in range(d)]
    inside = capi.ptr_array(diags)
    holed = capi.ptr_array(diags[:-1] + [None])
    lt_out = diags[-1] + 8 * (L - 1) * N  # one row into the last diagonal; ends inside the slab
    ct = ins[0].ptr

    def host_us(darr, calls=3000):
        rcs = set()
        for _ in range(100):
            lib.hefx_linear_transform_plain(h, L, ct, d, darr, 0, None, None, lt_out, None)
        t0 = time.perf_counter()
        for _ in range(calls):
            rcs.add(lib.hefx_linear_transform_plain(h, L, ct, d, darr, 0, None, None, lt_out, None))
        us = (time.perf_counter() - t0) * 1e6 / calls
        return round(us, 2), sorted(rcs), lib.hefx_last_error().decode()

    t_null, rc_null, _ = host_us(holed)
    t_chk, rc_chk, msg = host_us(inside)
    r["lt_d512_host"] = {"refused_by_null_scan_us": t_null, "refused_after_range_check_us": t_chk, "rc": rc_null + rc_chk,
                         "range_check_refused": "overlap" in msg, "last_message": msg}
    e.sync()
    print(json.dumps(r), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1])
    libs, rounds, out_path = [], 3, None
    while args:
        k = args.pop(0)
        if k == "--lib":
            label, path = args.pop(0).split("=", 1)
            libs.append((label, os.path.abspath(path)))
        elif k == "--rounds":
            rounds = int(args.pop(0))
        elif k == "--out":
            out_path = args.pop(0)
        else:
            sys.exit(__doc__)
    if not libs:
        sys.exit(__doc__)
    lines = []
    for _ in range(rounds):
        for label, path in libs:  # alternating: every round visits every library
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", label], env=dict(os.environ, HEFX_LIB=path),
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"{label}: exit {p.returncode}\n{p.stderr[-3000:]}")
            lines.append(p.stdout.strip().splitlines()[-1])
            print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
