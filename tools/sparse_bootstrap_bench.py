"""Sparse-slot bootstrapping (bootstrap.plan(..., slots=ns), algorithms.bootstrap) on the MI355X against the dense bootstrap of
the same chain, in one process: N = 16384, {60, 50 x 13, 60}, scale 2^50, Hamming weight 32.

  dense            algorithms.bootstrap with the dense plan, timed FIRST: the baseline of this session.
  sparse           ns = 16, 256 and 4096 = N / 4: the whole bootstrap and its phases mod_raise, subsum, c2s, eval_mod, s2c, with
                   the key switches of the plan and the decode error over the first ns slots.
  baby_rotations   the baby rotations of a packed stage (the nonzero babies of ONE ciphertext) at L = 14 and L = 4, two ways:
                   apply_galois_batch (what dense stages use: it hoists only above 32 items) and rotate_hoisted_batch (one
                   shared digit decomposition at any count).  Same words, compared here; algorithms._dft_stage uses the
                   first for every mode, since the two measured alike.

Two clocks per leg.  device: K calls in a row between two events on the stream, queued behind a 0.5 GiB copy; a phase is many
launches issued from Python, so where the host is the slower side the figure contains the device's waits for it.  host: a window
of calls and one synchronise.  Legs of one comparison alternate; medians and extremes over REPS windows.
Usage: sparse_bootstrap_bench.py [--out FILE] [--n 2048]   (--n 2048: a rehearsal size, not a measurement; writes the "timing"
section, the precision section of profiles/sparse_bootstrap.json comes from tests/test_sparse_bootstrap_cpu.py with
BOOTSTRAP_RECORD=1)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from seal_fyp_logistic_regression_amd import _build, bootstrap
from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import seal as S

REPS, INNER, K = 7, 3, 3
BITS, SCALE, HAMMING_WEIGHT = [60] + [50] * 13 + [60], 2.0 ** 50, 32
args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else None
N = int(args[args.index("--n") + 1]) if "--n" in args else 16384
SLOTS = [16, 256, N // 4]


def spread(us):
    us = sorted(us)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}


def measure(eng, legs, inner=INNER, k=K, reps=REPS):
    """{name: {"device": ..., "host": ...}}; every leg warmed twice, then the legs in turn, REPS times on either clock"""
    a, b = measure.delay
    for run in legs.values():
        for _ in range(2):
            run()
        eng.sync()
    host, dev = {name: [] for name in legs}, {name: [] for name in legs}
    for _ in range(reps):
        for name, run in legs.items():
            t = time.perf_counter()
            for _ in range(inner):
                run()
            eng.sync()
            host[name].append((time.perf_counter() - t) * 1e6 / inner)
        for name, run in legs.items():
            ev0, ev1 = eng.event(), eng.event()
            eng.copy_raw(a.ptr, b.ptr, a.nbytes)
            eng.event_record(ev0)
            for _ in range(k):
                run()
            eng.event_record(ev1)
            eng.sync()
            dev[name].append(eng.event_elapsed_ms(ev0, ev1) * 1e3 / k)
            eng.event_destroy(ev0), eng.event_destroy(ev1)
    return {name: {"device": spread(dev[name]), "host": spread(host[name])} for name in legs}


parms = S.EncryptionParameters("ckks")
parms.set_poly_modulus_degree(N)
parms.set_coeff_modulus(S.CoeffModulus.Create(N, BITS))
ctx = S.SEALContext.Create(parms)
kg = S.KeyGenerator(ctx, 1, hamming_weight=HAMMING_WEIGHT)
eng, ev, encoder = ctx.backend.engine, S.Evaluator(ctx), S.CKKSEncoder(ctx)
enc, dec, rk = S.Encryptor(ctx, kg.public_key(), 2), S.Decryptor(ctx, kg.secret_key()), kg.relin_keys()
measure.delay = (eng.empty(1 << 26), eng.empty(1 << 26))   # 0.5 GiB each
values = np.random.default_rng(5).uniform(-1.0, 1.0, N // 2)

out = {"tool": "tools/sparse_bootstrap_bench.py", "box_clock": time.strftime("%Y-%m-%dT%H:%M:%S%z"), "N": N, "chain_bits": BITS,
       "scale": "2^50", "hamming_weight": HAMMING_WEIGHT, "library_sha16": _build.library_sha16(), "source_sha16": _build.source_sha16(),
       "reps": REPS, "calls_per_host_window": INNER, "calls_between_events": K,
       "unit": "us per call; device: between two events around K calls in a row (contains the device's waits for the host); "
               "host: a window of calls and one synchronise", "sparse": {}}

# ---- the dense baseline, first ------------------------------------------------------------------------------------------------
bp = bootstrap.plan(N, ctx.primes, SCALE)
gk = kg.galois_keys(bp.galois_steps(), conjugate=True)
encoded = bp.encode(encoder)
ct = enc.encrypt(encoder.encode(values, SCALE, parms_id=1))
res = alg.bootstrap(ev, ct, bp, gk, rk, encoded)
err = float(np.abs(encoder.decode(dec.decrypt(res)).real - values).max() / np.abs(values).max())
out["dense"] = {"key_switches": bp.key_switches(True), "levels": bp.levels(), "result_level": bp.result_level, "decode_error": err,
                **measure(eng, {"bootstrap": lambda: alg.bootstrap(ev, ct, bp, gk, rk, encoded)})}
print(json.dumps({"dense": out["dense"]}), flush=True)
del gk, encoded, res

# ---- the sparse plans: the whole bootstrap and its phases -----------------------------------------------------------------------
for ns in SLOTS:
    sp = bootstrap.plan(N, ctx.primes, SCALE, slots=ns)
    gk = kg.galois_keys(sp.galois_steps(), conjugate=True)
    encoded = sp.encode(encoder)
    v = values[:ns]
    ct = enc.encrypt(encoder.encode(np.tile(v, N // 2 // ns), SCALE, parms_id=1))
    raised = ev.mod_raise(ct, sp.top_level)
    summed = alg.subsum(ev, raised, ns, gk)
    x = alg.coeffs_to_slots_packed(ev, summed, sp.c2s, gk, encoded[0])
    (y,) = alg.eval_mod(ev, [x], sp, rk)
    res = alg.bootstrap(ev, ct, sp, gk, rk, encoded)
    got = encoder.decode(dec.decrypt(res)).real
    legs = {"mod_raise": lambda: ev.mod_raise(ct, sp.top_level),
            "subsum": lambda: alg.subsum(ev, raised, ns, gk),
            "c2s": lambda: alg.coeffs_to_slots_packed(ev, summed, sp.c2s, gk, encoded[0]),
            "eval_mod": lambda: alg.eval_mod(ev, [x], sp, rk),
            "s2c": lambda: alg.slots_to_coeffs_packed(ev, y, sp.s2c, gk, encoded[1]),
            "bootstrap": lambda: alg.bootstrap(ev, ct, sp, gk, rk, encoded)}
    row = {"slots": ns, "key_switches": sp.key_switches(True),
           "key_switches_by_phase": {"subsum": len(sp.subsum_steps()), "c2s": sp.c2s.key_switches(), "s2c": sp.s2c.key_switches(),
                                     "eval_mod": sp.key_switches(True) - len(sp.subsum_steps()) - sp.c2s.key_switches() - sp.s2c.key_switches()},
           "galois_keys": len(sp.galois_steps()) + 1, "levels": sp.levels(), "c2s_levels": sp.c2s.levels, "s2c_levels": sp.s2c.levels,
           "result_level": sp.result_level,
           "stages_babies_giants": [[len(st.babies), len(st.giants)] for st in sp.c2s.stages + sp.s2c.stages],
           "decode_error": float(np.abs(got[:ns] - v).max() / np.abs(v).max()),
           "decode_error_all_slots": float(np.abs(got - np.tile(v, N // 2 // ns)).max() / np.abs(v).max()),
           **measure(eng, legs)}
    row["dense_over_sparse_device"] = round(out["dense"]["bootstrap"]["device"]["median_us"] / row["bootstrap"]["device"]["median_us"], 2)
    out["sparse"][str(ns)] = row
    print(json.dumps({"sparse": row}), flush=True)
    if ns == SLOTS[0]:
        # ---- a packed stage's baby rotations, both ways, at the top of the chain and at SlotToCoeff's level ------------------------
        from seal_fyp_logistic_regression_amd.seal import galois_elt_from_step
        out["baby_rotations"] = []
        for L, stage, src in ((sp.top_level, sp.c2s.stages[0], summed), (sp.s2c_level, sp.s2c.stages[0], y)):
            assert src.parms_id() == L
            steps = [b for b in stage.babies if b]
            wide = sorted({s for st in sp.c2s.stages + sp.s2c.stages for s in st.babies + st.giants if s})[:7]   # a stage of eight babies
            for name, ss in (("the stage's own babies", steps), ("seven rotations of the plan", wide)):
                elts = [galois_elt_from_step(s, N) for s in ss]
                keys = [gk.key(e) for e in elts]
                batch = eng.apply_galois_batch(L, [src.data] * len(ss), elts, keys)
                hoist = eng.rotate_hoisted_batch(L, src.data, elts, keys)
                eng.sync()
                same = all(np.array_equal(a.download(), b.download()) for a, b in zip(batch, hoist))
                m = measure(eng, {"apply_galois_batch": lambda: eng.apply_galois_batch(L, [src.data] * len(ss), elts, keys, outs=batch),
                                  "rotate_hoisted_batch": lambda: eng.rotate_hoisted_batch(L, src.data, elts, keys, outs=hoist)}, inner=20, k=8)
                ab = {"L": L, "rotations": len(ss), "what": name, "words_equal": same, **m,
                      "batch_over_hoisted_device": round(m["apply_galois_batch"]["device"]["median_us"]
                                                         / m["rotate_hoisted_batch"]["device"]["median_us"], 3)}
                out["baby_rotations"].append(ab)
                print(json.dumps({"baby_rotations": ab}), flush=True)
    del gk, encoded, raised, summed, x, y, res

slow = [ns for ns in SLOTS if ns <= N // 8 and out["sparse"][str(ns)]["bootstrap"]["device"]["median_us"] >= out["dense"]["bootstrap"]["device"]["median_us"]]
out["sparse_not_faster_than_dense_at"] = slow
if out_path:
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["timing"] = out
    json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
    open(out_path, "a").write("\n")
