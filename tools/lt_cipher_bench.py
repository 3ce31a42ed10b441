"""Linear_Transform_Cipher (helper.h:212-234, "C_vec . C_mat" of linear_transformation.cpp / FYP slide 27) wall time on
the MI355X at the reference's chart points -- N=8192 {60,40,40,60}, scale 2^40, d = 10 / 100 / 1000 -- compute phase only,
with the default power-of-two Galois keys (NAF chains) and with a direct key per step; and the primitive underneath,
the sum of ciphertext products, alone: Engine.multiply_sum against multiply_batch + add_many at C2 and C3.

The transform is timed through algorithms.linear_transform_cipher, so the same file runs on a tree that has no native
entry (there it times the op-by-op composition) and on one that has; the primitive's fused leg is skipped where the
engine has no multiply_sum.  Usage: lt_cipher_bench.py [--out FILE] [--label TEXT] [--skip-primitive] [d ...]; then
lt_cipher_bench.py --merge PARENT.json[,PARENT_AGAIN.json] BRANCH.json --out profiles/lt_cipher.json joins the two sides
into the one record with the comparison per dimension."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
from seal_fyp_logistic_regression_amd import _build, capi
from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import seal as S

REPS, HBM_PEAK = 12, 8e12
args = sys.argv[1:]


def merge(parent_files, branch_file, out_file):
    """one record from the files of both sides (the parent's may be several runs of one session: their medians and
    extremes give its run-to-run spread), with the acceptance comparison per (d, key mode) spelled out"""
    parents, branch = [json.load(open(f)) for f in parent_files], json.load(open(branch_file))
    rows = []
    for b in branch["transform"]:
        ps = [p for side in parents for p in side["transform"] if (p["d"], p["mode"]) == (b["d"], b["mode"])]
        spread = max(p["max_us"] for p in ps) - min(p["min_us"] for p in ps)
        best = min(p["median_us"] for p in ps)
        rows.append({"d": b["d"], "mode": b["mode"], "parent_median_us": [round(p["median_us"], 1) for p in ps],
                     "parent_min_us": round(min(p["min_us"] for p in ps), 1), "parent_max_us": round(max(p["max_us"] for p in ps), 1),
                     "parent_spread_us": round(spread, 1), "branch_median_us": round(b["median_us"], 1),
                     "branch_min_us": round(b["min_us"], 1), "branch_max_us": round(b["max_us"], 1),
                     "parent_over_branch": round(best / b["median_us"], 3),
                     "branch_median_within_parent_median_plus_spread": bool(b["median_us"] <= best + spread),
                     "parent_peak_device_bytes": ps[0]["peak_device_bytes"], "branch_peak_device_bytes": b["peak_device_bytes"]})
        print(rows[-1])
    rec = {"tool": "tools/lt_cipher_bench.py", "comparison": rows, "parent": parents, "branch": branch}
    with open(out_file, "w") as f:
        json.dump(rec, f, indent=1)


if "--merge" in args:  # lt_cipher_bench.py --merge PARENT.json[,PARENT2.json] BRANCH.json --out profiles/lt_cipher.json
    i = args.index("--merge")
    merge(args[i + 1].split(","), args[i + 2], args[args.index("--out") + 1])
    sys.exit(0)
out_path = args.pop(args.index("--out") + 1) if "--out" in args else None
label = args.pop(args.index("--label") + 1) if "--label" in args else ""
skip_primitive = "--skip-primitive" in args
dims = [int(x) for x in args if not x.startswith("--")] or [10, 100, 1000]


def free_bytes(eng):
    f, t = C.c_size_t(0), C.c_size_t(0)
    capi.check(capi.lib().hefx_device_memory(eng._h, C.byref(f), C.byref(t)))
    return int(f.value)


def timed(eng, run, reps=REPS, warm=2):
    """per-call wall times (call + device synchronise), after `warm` untimed calls"""
    for _ in range(warm):
        r = run()
        eng.sync()
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        r = run()
        eng.sync()
        walls.append(time.perf_counter() - t)
    return r, walls


def stats(walls):
    us = sorted(w * 1e6 for w in walls)
    q = statistics.quantiles(us, n=4)
    return {"median_us": statistics.median(us), "min_us": us[0], "max_us": us[-1], "iqr_us": q[2] - q[0],
            "samples_us": [round(x, 1) for x in us]}


out = {"label": label, "box_clock": time.strftime("%Y-%m-%dT%H:%M:%S%z"), "library_sha16": _build.library_sha16(),
       "source_sha16": _build.source_sha16(), "reps": REPS, "transform": [], "primitive": []}

# ---- the transform ---------------------------------------------------------------------------------------------------
# A fresh context per (d, key mode): the memory figure below then belongs to that run alone.
N, bits, scale = 8192, [60, 40, 40, 60], 2.0 ** 40
out["params"] = f"N={N} {bits} scale 2^40"
for d in dims:
    for mode in ("default_keys", "direct_keys"):
        parms = S.EncryptionParameters("ckks"); parms.set_poly_modulus_degree(N); parms.set_coeff_modulus(S.CoeffModulus.Create(N, bits))
        ctx = S.SEALContext.Create(parms)
        eng = ctx.backend.engine
        kg = S.KeyGenerator(ctx, 1); enc = S.Encryptor(ctx, kg.public_key(), 2); dec = S.Decryptor(ctx, kg.secret_key())
        encoder, ev = S.CKKSEncoder(ctx), S.Evaluator(ctx)
        out["native_entry"] = hasattr(ctx.backend, "linear_transform_cipher")
        rng = np.random.default_rng(d)
        M, v = rng.standard_normal((d, d)), rng.standard_normal(d)
        cdiags = [enc.encrypt(p) for p in encoder.encode_many(list(alg.get_all_diagonals(M)), scale)]
        ct = enc.encrypt(encoder.encode(v, scale))
        steps = [-d] + list(range(1, d))
        gk = kg.galois_keys() if mode == "default_keys" else kg.galois_keys(steps)
        eng.sync()
        free0 = free_bytes(eng)
        r, walls = timed(eng, lambda: alg.linear_transform_cipher(ev, ct, cdiags, gk))
        # free memory before the first call minus after the last.  hipMemGetInfo counts what the context's pool has parked
        # and what its workspaces hold as used, and neither shrinks: blocks freed between the calls (the op-by-op path's d
        # products) still count, so this is the high-water mark of the transform's device memory, result included
        peak = free0 - free_bytes(eng)
        err = float(np.abs(encoder.decode(dec.decrypt(r))[:d].real - M @ v).max())
        row = {"d": d, "mode": mode, "key_switches_in_SEAL_order": sum(len(ev.rotation_plan(s, gk)) for s in steps),
               "galois_keys": len(gk.keys), "peak_device_bytes": peak, "max_abs_err": err, **stats(walls)}
        out["transform"].append(row)
        print({k: v for k, v in row.items() if k != "samples_us"}, flush=True)
        del r, gk, cdiags, ct, ev, encoder, dec, enc, kg, eng, ctx

# ---- the primitive: sum of n ciphertext products ------------------------------------------------------------------------
if not skip_primitive:
    from seal_fyp_logistic_regression_amd import Engine
    for name, Np, bp in (("C2", 8192, [60, 40, 40, 60]), ("C3", 16384, [60, 40, 40, 40, 40, 60])):
        primes = S.CoeffModulus.Create(Np, bp)
        e = Engine(Np, primes)
        L = len(primes) - 1
        key = bytes(range(32))
        for n in (16, 100, 1000):
            As = [e.sample("uniform", key, 2 * i, 2, L) for i in range(n)]      # distinct operands: the traffic is real
            Bs = [e.sample("uniform", key, 2 * i + 1, 2, L) for i in range(n)]
            need = 4 * L * Np * 8 * n                                           # the operand bytes a fused sum has to read
            # outputs allocated once, outside the timed window, for both legs: kernels and their submission only
            prods, total = e.empty_many(n, (3, L, Np)), e.empty(3, L, Np)
            legs = {"multiply_batch+add_many": lambda: e.add_many(L, 3, e.multiply_batch(L, As, Bs, outs=prods), out=total)}
            if hasattr(e, "multiply_sum"):
                legs["multiply_sum"] = lambda: e.multiply_sum(L, As, Bs, outs=[total])[0]
            res = {}
            for leg, run in legs.items():
                r, walls = timed(e, run)
                res[leg] = r.download()
                st = stats(walls)
                row = {"set": name, "N": Np, "L": L, "n": n, "leg": leg, "operand_bytes": need,
                       "bytes_per_s_on_operand_bytes": need / (st["median_us"] * 1e-6),
                       "share_of_8TBps": need / (st["median_us"] * 1e-6) / HBM_PEAK, **st}
                out["primitive"].append(row)
                print({k: v for k, v in row.items() if k != "samples_us"}, flush=True)
            if len(res) == 2:
                assert (res["multiply_sum"] == res["multiply_batch+add_many"]).all(), (name, n)
            del As, Bs, res, prods, total
        del e

print(json.dumps(out))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
