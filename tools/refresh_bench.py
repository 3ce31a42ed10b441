"""Refresh on the MI355X: hefx_refresh / hefx_refresh_batch against the path they replace -- hefx_decrypt, hefx_ckks_decode
(blocks, the slot values go to the host), hefx_ckks_encode, hefx_encrypt per ciphertext -- one item and a batch of 64, at
N = 4096 and N = 16384 on the LR chain {60, 40 x 7, 60}, L 1 -> 8, scale 2^40.

Both paths run in this process on the same context and the same ciphertexts, alternating repetition by repetition, each
repetition a host clock around work that ends in a device synchronise (the old path synchronises by itself in decode).
Every shape is warmed before its window.  The old path re-encodes at the first level, so its result is the same
plaintext up to the two floating-point transforms; the tool records how far the two results' slots differ, and that
refresh_batch's words are those of the single calls.  No threshold: both figures and both hashes go into the file.

Usage: refresh_bench.py [--out profiles/refresh.json] [--reps R]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from seal_fyp_logistic_regression_amd import Engine, _build
from seal_fyp_logistic_regression_amd import seal as S

args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else None
REPS = int(args[args.index("--reps") + 1]) if "--reps" in args else 20
BITS, SCALE, KEY = [60, 40, 40, 40, 40, 40, 40, 40, 60], 2.0 ** 40, bytes(range(32))
L_IN, L_OUT, SIZE, BATCH = 1, 8, 2, 64


def stats(walls):
    us = sorted(w * 1e6 for w in walls)
    q = statistics.quantiles(us, n=4)
    return {"median_us": statistics.median(us), "min_us": us[0], "max_us": us[-1], "iqr_us": q[2] - q[0],
            "samples_us": [round(x, 1) for x in us]}


out = {"tool": "tools/refresh_bench.py", "box_clock": time.strftime("%Y-%m-%dT%H:%M:%S%z"),
       "library_sha16": _build.library_sha16(), "source_sha16": _build.source_sha16(), "reps": REPS,
       "params": f"LR chain {BITS}, L {L_IN} -> {L_OUT}, size {SIZE}, scale 2^40", "rows": []}

for N in (4096, 16384):
    primes = S.CoeffModulus.Create(N, BITS)
    e = Engine(N, primes)
    k = len(primes)
    # real keys and real ciphertexts of small values: the old path decodes them, so they must decode
    sk = e.sample("ternary", KEY, 1, 1, k)
    e.ntt_forward(sk, 1, k)
    a = e.sample("uniform", KEY, 2, 1, k)
    err = e.sample("noise", KEY, 3, 1, k)
    e.ntt_forward(err, 1, k)
    pk0 = e.negate(k, 1, e.add(k, 1, e.multiply_plain(k, 1, a, sk), err))
    pk = e.to_device(np.stack([pk0.download().reshape(k, N), a.download().reshape(k, N)]))
    rng = np.random.default_rng(N)
    vals = rng.uniform(-1, 1, (BATCH, N // 2))
    pts = e.ckks_encode(L_IN, vals, SCALE)
    cts = e.encrypt_batch(L_IN, pk, [pts.view(i * L_IN * N, (L_IN, N)) for i in range(BATCH)], KEY, 100)
    for n in (1, BATCH):
        sub = cts[:n]
        new_outs, old_outs = e.empty_many(n, (2, L_OUT, N)), e.empty_many(n, (2, L_OUT, N))
        old_pts = e.empty_many(n, (L_IN, N))

        def new_path():
            if n == 1:
                e.refresh(L_IN, SIZE, L_OUT, sub[0], sk, pk, KEY, 500, out=new_outs[0])
            else:
                e.refresh_batch(L_IN, SIZE, L_OUT, sub, sk, pk, KEY, 500, outs=new_outs)
            e.sync()

        def old_path():  # per ciphertext, as the reference's loop does it (logistic_regression_ckks.cpp:362-381)
            for i in range(n):
                pt = e.decrypt(L_IN, SIZE, sub[i], sk, out=old_pts[i])
                v = e.ckks_decode(L_IN, pt, SCALE, complex_out=False)
                fresh = e.ckks_encode(L_OUT, v, SCALE)
                e.encrypt(L_OUT, pk, fresh, KEY, 500 + i, out=old_outs[i])
            e.sync()

        for _ in range(3):
            new_path(); old_path()
        walls = {"refresh": [], "decrypt+decode+encode+encrypt": []}
        for _ in range(REPS):  # alternating: drift of the box hits both alike
            for name, run in (("refresh", new_path), ("decrypt+decode+encode+encrypt", old_path)):
                t = time.perf_counter(); run(); walls[name].append(time.perf_counter() - t)
        # what the two paths hold: slot values of both results, and the batch against the single calls
        dec = lambda ct: e.ckks_decode(L_OUT, e.decrypt(L_OUT, 2, ct, sk), SCALE, complex_out=False)[0]
        slot_diff = max(float(np.abs(dec(new_outs[i]) - dec(old_outs[i])).max()) for i in range(n))
        value_err = max(float(np.abs(dec(new_outs[i]) - vals[i]).max()) for i in range(n))
        same = all(np.array_equal(new_outs[i].download(), e.refresh(L_IN, SIZE, L_OUT, sub[i], sk, pk, KEY, 500 + i).download())
                   for i in range(min(n, 4)))
        row = {"N": N, "items": n, "batch_words_equal_single_calls": bool(same), "max_slot_difference_between_paths": slot_diff,
               "max_slot_error_of_refresh": value_err,
               "old_over_new_median": statistics.median(walls["decrypt+decode+encode+encrypt"]) / statistics.median(walls["refresh"]),
               **{name: stats(w) for name, w in walls.items()}}
        out["rows"].append(row)
        print({kk: (vv if not isinstance(vv, dict) else {x: round(y, 1) for x, y in vv.items() if x != "samples_us"})
               for kk, vv in row.items()}, flush=True)
    del e

print(json.dumps(out))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
