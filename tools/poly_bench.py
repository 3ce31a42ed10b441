"""hefx_scalar_combine and algorithms.evaluate_polynomial on the MI355X against what they replace, both sides alternating in
one process (same clocks, same neighbours), at N = 16384, L = 5 and N = 8192, L = 3 (size-2 ciphertexts).

  primitive   Engine.scalar_combine with m = 8 inputs and G = 1, 4, 8 outputs against the call-by-call composition per output:
              one hefx_ckks_encode_scalar of the m weights (m plaintexts of L * N words), m hefx_multiply_plain, one
              hefx_add_many, one encode of the constant and one hefx_add_plain -- every buffer of both legs allocated outside
              the timed window.  Bytes: (m + G) ciphertext volumes, the least the fused call can move; achieved bytes/s on
              those.  Beside it hefx_multiply_plain_sum (mulplain_sum_kernel, the nearest relative) on ITS least bytes: m
              ciphertexts, m plaintexts, one output.  The legs' words are compared.
  evaluator   evaluate_polynomial on SIGMOID_COEFFS[7] against tree_cipher and horner_cipher where the chain has their levels
              (Horner needs 7, the tree 4, the plan 3): N = 16384 {60, 40 x 4, 60}; at N = 8192 {60, 40, 40, 60} only degree 3
              through evaluate_polynomial fits, and the record says so.

A window is INNER calls and one device synchronise (host clock); REPS windows per leg, alternating; medians and extremes.
Usage: poly_bench.py [--out FILE]   (writes the "timing" section; the precision section of profiles/poly_eval.json comes from
tests/test_poly_eval_cpu.py with POLY_EVAL_RECORD=1)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from seal_fyp_logistic_regression_amd import Engine, _build, poly
from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import seal as S

REPS, INNER, HBM_PEAK = 9, 200, 8e12
args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else None


def stats(walls, inner):
    us = sorted(w * 1e6 / inner for w in walls)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}


def alternate(eng, legs, inner=INNER, reps=REPS):
    """{name: per-call stats}; every leg warmed twice, then windows of `inner` calls + one synchronise, legs in turn"""
    for run in legs.values():
        for _ in range(2):
            run()
        eng.sync()
    walls = {name: [] for name in legs}
    for _ in range(reps):
        for name, run in legs.items():
            t = time.perf_counter()
            for _ in range(inner):
                run()
            eng.sync()
            walls[name].append(time.perf_counter() - t)
    return {name: stats(w, inner) for name, w in walls.items()}


out = {"tool": "tools/poly_bench.py", "box_clock": time.strftime("%Y-%m-%dT%H:%M:%S%z"), "library_sha16": _build.library_sha16(),
       "source_sha16": _build.source_sha16(), "reps": REPS, "calls_per_window": INNER, "primitive": [], "evaluator": []}

# ---- the primitive -----------------------------------------------------------------------------------------------------
for N, bits in ((16384, [60, 40, 40, 40, 40, 60]), (8192, [60, 40, 40, 60])):
    primes = S.CoeffModulus.Create(N, bits)
    L, size, m = len(primes) - 1, 2, 8
    e = Engine(N, primes)
    key = bytes(range(32))
    ins = [e.sample("uniform", key, i, size, L) for i in range(m)]
    vol = size * L * N * 8
    rng = np.random.default_rng(N)
    wscale = S_ = 2.0 ** 40
    for G in (1, 4, 8):
        wv, cv = rng.uniform(-2, 2, (G, m)), rng.uniform(-1, 1, G)
        wres = np.array([[[poly.weight_residue(wv[g, k], wscale, q) for q in primes[:L]] for k in range(m)] for g in range(G)], dtype=np.uint64)
        cres = np.array([[poly.weight_residue(cv[g], S_, q) for q in primes[:L]] for g in range(G)], dtype=np.uint64)
        fused_out, comp_out = e.empty_many(G, (size, L, N)), e.empty_many(G, (size, L, N))
        pts, cpt = e.empty(m, L, N), e.empty(1, L, N)
        prods, acc = e.empty_many(m, (size, L, N)), e.empty(size, L, N)

        def fused():
            e.scalar_combine(L, size, ins, [L] * m, wres, cres, outs=fused_out)

        def composed():
            for g in range(G):
                e.ckks_encode_scalar(L, wv[g], wscale, out=pts)
                for k in range(m):
                    e.multiply_plain(L, size, ins[k], pts.view(k * L * N, (L, N)), out=prods[k])
                e.add_many(L, size, prods, out=acc)
                e.ckks_encode_scalar(L, [cv[g]], S_, out=cpt)
                e.add_plain(L, size, acc, cpt.view(0, (L, N)), out=comp_out[g])

        res = alternate(e, {"scalar_combine": fused, "composition": composed})
        for a, b in zip(fused_out, comp_out):
            assert (a.download() == b.download()).all(), (N, G)
        need = (m + G) * vol
        row = {"N": N, "L": L, "m": m, "G": G, "least_bytes": need, **{k: v for k, v in res.items()},
               "scalar_combine_bytes_per_s": round(need / (res["scalar_combine"]["median_us"] * 1e-6)),
               "scalar_combine_share_of_8TBps": round(need / (res["scalar_combine"]["median_us"] * 1e-6) / HBM_PEAK, 4),
               "composition_over_scalar_combine": round(res["composition"]["median_us"] / res["scalar_combine"]["median_us"], 2),
               "fused_is_slower": bool(res["scalar_combine"]["median_us"] > res["composition"]["median_us"])}
        out["primitive"].append(row)
        print(row, flush=True)
    # the nearest relative on its own least bytes: m ciphertexts, m full plaintexts, one output
    full = [e.sample("uniform", key, 100 + i, 1, L).view(0, (L, N)) for i in range(m)]
    one = e.empty_many(1, (size, L, N))
    res = alternate(e, {"multiply_plain_sum": lambda: e.multiply_plain_sum(L, size, ins, full, outs=one)})
    need = m * vol + m * L * N * 8 + vol
    row = {"N": N, "L": L, "m": m, "least_bytes": need, **res,
           "multiply_plain_sum_bytes_per_s": round(need / (res["multiply_plain_sum"]["median_us"] * 1e-6))}
    out["primitive"].append(row)
    print(row, flush=True)
    del e

# a shape at which the fused call lost would have to go back to the composition in Evaluator.scalar_combine: none may be listed
out["shapes_where_the_fused_call_is_slower"] = [(r["N"], r["L"], r["m"], r["G"]) for r in out["primitive"] if r.get("fused_is_slower")]

# ---- the evaluator -----------------------------------------------------------------------------------------------------
for N, bits, d in ((16384, [60, 40, 40, 40, 40, 60], 7), (8192, [60, 40, 40, 60], 3)):
    parms = S.EncryptionParameters("ckks"); parms.set_poly_modulus_degree(N); parms.set_coeff_modulus(S.CoeffModulus.Create(N, bits))
    ctx = S.SEALContext.Create(parms)
    eng = ctx.backend.engine
    kg = S.KeyGenerator(ctx, 1); enc = S.Encryptor(ctx, kg.public_key(), 2); dec = S.Decryptor(ctx, kg.secret_key())
    encoder, ev, rk = S.CKKSEncoder(ctx), S.Evaluator(ctx), kg.relin_keys()
    x = np.linspace(-1, 1, N // 2)
    ct = enc.encrypt(encoder.encode(x, 2.0 ** 40))
    coeffs = alg.SIGMOID_COEFFS[d]
    want = sum(c * x ** k for k, c in enumerate(coeffs))
    legs = {"evaluate_polynomial": lambda: alg.evaluate_polynomial(ev, ct, coeffs, rk)}
    skipped = {}
    for name, run in (("tree_cipher", lambda: alg.tree_cipher(ev, encoder, enc, ct, d, 2.0 ** 40, coeffs, rk)),
                      ("horner_cipher", lambda: alg.horner_cipher(ev, encoder, enc, ct, d, coeffs, 2.0 ** 40, rk))):
        try:
            run()
            legs[name] = run
        except ValueError as err:
            skipped[name] = f"not run: the chain lacks its levels ({err})"
    res = alternate(eng, legs, inner=20)
    errs = {name: float(np.abs(encoder.decode(dec.decrypt(run())).real - want).max()) for name, run in legs.items()}
    row = {"N": N, "L": len(bits) - 1, "degree": d, **res, **skipped, "max_slot_error": errs}
    if "tree_cipher" in res:
        row["tree_over_evaluate_polynomial"] = round(res["tree_cipher"]["median_us"] / res["evaluate_polynomial"]["median_us"], 2)
    out["evaluator"].append(row)
    print(row, flush=True)
    del eng, ctx

if out_path:
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["timing"] = out
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
