"""The general-size ciphertext product and relinearisation on the MI355X (hefx_multiply_sizes[_batch],
hefx_relinearize_sizes) at C3 (N=16384, L=5) and C2 (N=8192, L=3), against the size-2 x size-2 entries (hefx_multiply,
hefx_multiply_batch: the <2, 2> instances of the same kernel family, reached through their own entries).

  product     device-event time per call and achieved bytes/s on the algorithmic bytes 8 N L (2 (sa + sb) - 1) at the shapes
              (2,2), (3,2), (3,3), (4,4), (8,9): one product (latency; operands cache-resident) and a batch of BATCH distinct
              products through the pointer table (bandwidth).  The yardstick is hefx_multiply / hefx_multiply_batch at 2 x 2,
              timed five times interleaved with the shapes in the same session: their run-to-run spread is what a general
              kernel's bytes/s is held against.  A shape slower per byte than the 2 x 2 kernel by more than that spread is
              listed with its registers and waves per SIMD (DESIGN.md kernel table).
  relinearise hefx_relinearize_sizes 4 -> 2 and 5 -> 2 against two / three calls of hefx_relinearize (what the parent
              commit runs for the same number of key switches), and the share of the staging copies: the same copies alone.

Usage: ct_sizes_bench.py [--out profiles/ct_sizes.json] [--quick]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seal_fyp_logistic_regression_amd import Engine, _build
from seal_fyp_logistic_regression_amd import seal as S

args = sys.argv[1:]
out_path = args.pop(args.index("--out") + 1) if "--out" in args else None
quick = "--quick" in args
SHAPES = [(2, 2), (3, 2), (3, 3), (4, 4), (8, 9)]
BATCH, CALLS, REPEATS, HBM_PEAK = (8, 3, 2, 8e12) if quick else (256, 20, 5, 8e12)
# registers / waves per SIMD of the kernels behind each shape (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)
RESOURCES = {(2, 2): ("multiply_sizes_kernel<2, 2>", 53, 8), (3, 2): ("multiply_sizes_kernel<3, 2>", 57, 8),
             (3, 3): ("multiply_sizes_kernel<3, 3>", 70, 7), (4, 4): ("multiply_sizes_kernel<4, 4>", 90, 5),
             (8, 9): ("multiply_sizes_kernel<0, 0>", 54, 8)}


def event_us(e, run, calls=CALLS):
    """device time per call over `calls` back-to-back submissions (one untimed first)"""
    run()
    e.sync()
    e0, e1 = e.event(), e.event()
    e.event_record(e0)
    for _ in range(calls):
        run()
    e.event_record(e1)
    e.sync()
    us = e.event_elapsed_ms(e0, e1) * 1e3 / calls
    e.event_destroy(e0), e.event_destroy(e1)
    return us


def spread(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs), "samples_us": [round(x, 2) for x in xs]}


out = {"tool": "tools/ct_sizes_bench.py", "box_clock": time.strftime("%Y-%m-%dT%H:%M:%S%z"),
       "library_sha16": _build.library_sha16(), "source_sha16": _build.source_sha16(), "batch": BATCH, "calls_per_sample": CALLS,
       "repeats": REPEATS, "product": [], "relinearize": []}
key32 = bytes(range(32))
for name, N, bits in (("C3", 16384, [60, 40, 40, 40, 40, 60]), ("C2", 8192, [60, 40, 40, 60])):
    primes = S.CoeffModulus.Create(N, bits)
    e, L = Engine(N, primes), len(primes) - 1
    pw = L * N
    sizes = sorted({s for sh in SHAPES for s in sh})
    # ---- product: one call, and BATCH distinct items
    one = {s: (e.sample("uniform", key32, 10 + s, s, L), e.sample("uniform", key32, 30 + s, s, L)) for s in sizes}
    many = {s: ([e.sample("uniform", key32, 1000 * s + 2 * i, s, L) for i in range(BATCH)],
                [e.sample("uniform", key32, 1000 * s + 2 * i + 1, s, L) for i in range(BATCH)]) for s in sizes}
    res = {}
    for rep in range(REPEATS):  # every repeat visits every shape: the shapes and the yardstick are interleaved
        for sa, sb in SHAPES:
            o1, on = e.empty(sa + sb - 1, L, N), e.empty_many(BATCH, (sa + sb - 1, L, N))
            a, b, As, Bs = one[sa][0], one[sb][1], many[sa][0], many[sb][1]
            if (sa, sb) == (2, 2):
                legs = {"single": lambda: e.multiply(L, a, b, out=o1), "batch": lambda: e.multiply_batch(L, As, Bs, outs=on)}
            else:
                legs = {"single": lambda: e.multiply_sizes(L, sa, a, sb, b, out=o1),
                        "batch": lambda: e.multiply_sizes_batch(L, sa, As, sb, Bs, outs=on)}
            for leg, run in legs.items():
                res.setdefault((sa, sb, leg), []).append(event_us(e, run))
            del o1, on
    yard = {leg: spread(res[(2, 2, leg)]) for leg in ("single", "batch")}
    for (sa, sb, leg), xs in res.items():
        items = BATCH if leg == "batch" else 1
        algo = 8 * N * L * (2 * (sa + sb) - 1) * items
        st = spread(xs)
        bps = algo / (st["median_us"] * 1e-6)
        y = yard[leg]
        y_bps_lo = 8 * N * L * 7 * items / (y["max_us"] * 1e-6)  # the yardstick's slowest repeat, in bytes/s
        kern, vgpr, waves = RESOURCES[(sa, sb)]
        row = {"set": name, "N": N, "L": L, "shape": [sa, sb], "leg": leg, "items": items, "algorithmic_bytes": algo,
               "bytes_per_s": bps, "share_of_8TBps": bps / HBM_PEAK, "kernel": kern, "vgprs": vgpr, "waves_per_simd": waves,
               "slower_per_byte_than_2x2_beyond_its_spread": bool(bps < y_bps_lo), **st}
        out["product"].append(row)
        print({k: v for k, v in row.items() if k != "samples_us"}, flush=True)
    del one, many
    # ---- relinearise
    keys = [e.sample("uniform", key32, 500 + p, 2 * (len(primes) - 1), len(primes)) for p in (2, 3, 4)]
    ct3 = [e.sample("uniform", key32, 600 + i, 3, L) for i in range(3)]
    out2 = e.empty(2, L, N)
    stage = e.empty(2, 3, L, N)
    for size_in in (4, 5):
        ct = e.sample("uniform", key32, 700 + size_in, size_in, L)
        steps = size_in - 2

        def parent():
            for t in range(steps):
                e.relinearize(L, ct3[t], keys[0], out=out2)

        def copies():  # what hefx_relinearize_sizes stages: (c0, c1) once, then one polynomial per step
            e.copy_raw(stage.ptr, ct.ptr, 2 * pw * 8)
            for t in range(steps):
                e.copy_raw(stage.ptr + (t & 1) * 3 * pw * 8 + 2 * pw * 8, ct.ptr + (size_in - 1 - t) * pw * 8, pw * 8)

        legs = {"relinearize_sizes": lambda: e.relinearize_sizes(L, size_in, 2, ct, keys[:steps], out=out2),
                f"{steps} x hefx_relinearize": parent, "staging copies alone": copies}
        rr = {leg: [] for leg in legs}
        for rep in range(REPEATS):
            for leg, run in legs.items():
                rr[leg].append(event_us(e, run))
        row = {"set": name, "N": N, "L": L, "size_in": size_in, "size_out": 2, "key_switches": steps,
               **{leg: spread(xs) for leg, xs in rr.items()}}
        row["staging_share"] = row["staging copies alone"]["median_us"] / row["relinearize_sizes"]["median_us"]
        row["over_parent_calls"] = row["relinearize_sizes"]["median_us"] / row[f"{steps} x hefx_relinearize"]["median_us"]
        out["relinearize"].append(row)
        print({k: (v if not isinstance(v, dict) else round(v["median_us"], 1)) for k, v in row.items()}, flush=True)
    e.close()

print(json.dumps(out))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
