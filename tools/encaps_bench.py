"""Sparse-secret encapsulation on the MI355X (include/hefx_encaps.h), three measurements in one process:

  raise_switch     N = 16384, {60, 50 x 19, 60}, L = 20: hefx_raise_switch against the composition it replaces,
                   hefx_mod_raise(count = 2) + hefx_switch_key at L = 20, on random canonical operands (the time does not depend
                   on the words), legs alternating.  The condition: the fused call is faster, in this run.
  bootstrap        N = 16384, {60, 50 x 13, 60}, one sparse bootstrap (ns = 8) without encapsulation (sparse main secret,
                   Hamming weight 32) and with it (DENSE main secret, encapsulation keys of weight 32), legs alternating, and
                   both decode errors.  Expected overhead: one key switch at L = 1 plus the difference above at L = 14.
  n32768           the first bootstrap this engine runs at N = 32768: ns = 8, dense main secret, encapsulation keys; the chain's
                   bit count is printed, the time and the decode error against the input recorded.  No parent to compare with.

Device time between two events around K calls in a row (queued behind a 0.5 GiB copy), medians of REPS windows.  A bootstrap is
many launches issued from Python: where the host is the slower side its figure contains the device's waits for it, so the host
clock (a window of calls and one synchronise) is recorded beside it.
Usage: encaps_bench.py [--out FILE] [--only raise_switch|bootstrap|n32768]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from seal_fyp_logistic_regression_amd import _build, bootstrap
from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import seal as S

REPS, SCALE, HAMMING_WEIGHT, NS = 5, 2.0 ** 50, 32, 8
args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else None
only = args[args.index("--only") + 1] if "--only" in args else None


def spread(us):
    us = sorted(us)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}


def measure(eng, legs, k, inner=3, reps=REPS):
    """{name: {"device": ..., "host": ...}}; every leg warmed twice, then the legs in turn, REPS times on either clock"""
    a, b = eng.empty(1 << 26), eng.empty(1 << 26)   # 0.5 GiB each: the delay the event windows queue behind
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


def context(N, bits):
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(S.CoeffModulus.Create(N, bits))
    return S.SEALContext.Create(parms)


def save(section, row):
    print(json.dumps({section: row}), flush=True)
    if out_path:
        doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
        doc.setdefault("tool", "tools/encaps_bench.py")
        doc.update(library_sha16=_build.library_sha16(), source_sha16=_build.source_sha16(), reps=REPS,
                   unit="us per call; device: between two events around K calls in a row; host: a window of calls and one synchronise")
        doc[section] = row
        json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
        open(out_path, "a").write("\n")


def raise_switch_section():
    N, bits = 16384, [60] + [50] * 19 + [60]
    ctx = context(N, bits)
    eng, primes, k = ctx.backend.engine, ctx.primes, ctx.k
    L = k - 1
    rng = np.random.default_rng(1)
    ct = eng.to_device(rng.integers(0, int(primes[0]), (2, 1, N), dtype=np.uint64))
    key_h = np.empty((k - 1, 2, k, N), dtype=np.uint64)
    for m, q in enumerate(primes):
        key_h[:, :, m] = rng.integers(0, int(q), (k - 1, 2, N), dtype=np.uint64)
    key = eng.to_device(key_h)
    ckey = eng.collapse_key(L, key)
    fused, raised, switched = eng.empty(2, L, N), eng.empty(2, L, N), eng.empty(2, L, N)
    # the fused call gives the words of its reference form (the ordinary key switch on the synthetic two-digit operand)
    ev = S.Evaluator(ctx)
    c, keys = S.Ciphertext()._set(ct, 2, 1, 1.0), S.EncapsKeys(None, key, HAMMING_WEIGHT)
    same = bool(np.array_equal(eng.raise_switch(L, ct, ckey, out=fused).download(), ev._raise_switch_composed(c, keys, L).download()))

    def composition():
        eng.mod_raise(1, L, ct, count=2, out=raised)
        eng.switch_key(L, raised, key, out=switched)

    m = measure(eng, {"raise_switch": lambda: eng.raise_switch(L, ct, ckey, out=fused), "mod_raise_then_switch_key": composition,
                      "mod_raise": lambda: eng.mod_raise(1, L, ct, count=2, out=raised),
                      "switch_key": lambda: eng.switch_key(L, raised, key, out=switched),
                      "collapse_key": lambda: eng.collapse_key(L, key, out=ckey)}, k=20, inner=20)
    ratio = round(m["mod_raise_then_switch_key"]["device"]["median_us"] / m["raise_switch"]["device"]["median_us"], 2)
    save("raise_switch", {"N": N, "chain_bits": bits, "L": L, "row_transforms": {"raise_switch": 4 * L + 3, "switch_key_about": L * L + 5 * L},
                          "words_equal_reference": same, "calls_between_events": 20, **m, "composition_over_fused_device": ratio,
                          "fused_is_faster": ratio > 1.0})


def bootstrap_run(ctx, kg, keys, values):
    """one sparse bootstrap (ns = NS) under kg's secret, with encapsulation keys or None: (plan, decode error, the call to time, engine,
    what the call needs kept alive)"""
    N = ctx.N
    eng, ev, encoder = ctx.backend.engine, S.Evaluator(ctx), S.CKKSEncoder(ctx)
    enc, dec, rk = S.Encryptor(ctx, kg.public_key(), 2), S.Decryptor(ctx, kg.secret_key()), kg.relin_keys()
    sp = bootstrap.plan(N, ctx.primes, SCALE, slots=NS)
    gk = kg.galois_keys(sp.galois_steps(), conjugate=True)
    encoded = sp.encode(encoder)
    v = values[:NS]
    ct = enc.encrypt(encoder.encode(np.tile(v, N // 2 // NS), SCALE, parms_id=1))
    res = alg.bootstrap(ev, ct, sp, gk, rk, encoded, encaps=keys)
    got = encoder.decode(dec.decrypt(res)).real
    err = float(np.abs(got - np.tile(v, N // 2 // NS)).max() / np.abs(v).max())
    run = lambda: alg.bootstrap(ev, ct, sp, gk, rk, encoded, encaps=keys)
    return sp, err, run, eng, (gk, encoded, rk, ct)


def bootstrap_section():
    N, bits = 16384, [60] + [50] * 13 + [60]
    ctx = context(N, bits)
    values = np.random.default_rng(5).uniform(-1.0, 1.0, N // 2)
    kg_sparse = S.KeyGenerator(ctx, 1, hamming_weight=HAMMING_WEIGHT)
    kg_dense = S.KeyGenerator(ctx, 1)
    keys = kg_dense.encapsulation_keys(HAMMING_WEIGHT, seed=7)
    sp, err_plain, run_plain, eng, hold_a = bootstrap_run(ctx, kg_sparse, None, values)
    _, err_encaps, run_encaps, _, hold_b = bootstrap_run(ctx, kg_dense, keys, values)
    m = measure(eng, {"sparse_secret": run_plain, "dense_secret_encaps": run_encaps}, k=3)
    save("bootstrap", {"N": N, "chain_bits": bits, "slots": NS, "hamming_weight": HAMMING_WEIGHT, "key_switches": sp.key_switches(True),
                       "result_level": sp.result_level, "decode_error_sparse_secret": err_plain, "decode_error_dense_secret_encaps": err_encaps,
                       "unit_of_error": "max error over all slots / max|expected|", "calls_between_events": 3, **m,
                       "encaps_overhead_device_us": round(m["dense_secret_encaps"]["device"]["median_us"] - m["sparse_secret"]["device"]["median_us"], 1)})


def n32768_section():
    N, bits = 32768, [60] + [50] * 13 + [60]
    ctx = context(N, bits)
    total_bits = sum(int(q).bit_length() for q in ctx.primes)
    print(f"N = {N}: chain of {len(bits)} primes, {total_bits} bits in all (HE-standard table, 128 bits, uniform ternary secret: 881)", flush=True)
    values = np.random.default_rng(5).uniform(-1.0, 1.0, N // 2)
    kg = S.KeyGenerator(ctx, 1)
    keys = kg.encapsulation_keys(HAMMING_WEIGHT, seed=7)
    sp, err, run, eng, hold = bootstrap_run(ctx, kg, keys, values)
    m = measure(eng, {"dense_secret_encaps": run}, k=3)
    save("n32768", {"N": N, "chain_bits": bits, "chain_total_bits": total_bits, "table_bits_128_ternary": 881, "slots": NS,
                    "hamming_weight_of_the_auxiliary_secret": HAMMING_WEIGHT, "key_switches": sp.key_switches(True), "result_level": sp.result_level,
                    "decode_error": err, "unit_of_error": "max error over all slots / max|expected|", "calls_between_events": 3, **m})


for name, section in (("raise_switch", raise_switch_section), ("bootstrap", bootstrap_section), ("n32768", n32768_section)):
    if only in (None, name):
        section()
