"""Sparse-secret encapsulation on hybrid keys on the MI355X (include/ext/hefx_hybrid_encaps.h): (a) the raise and the switch back,
shape by shape, and (b) one sparse bootstrap on hybrid keys under a dense secret, in one process.

(a) N in {16384, 32768}, L in {14, 20} data primes {60, 50 x (L-1)}, alpha in {3, 4} special primes of 60 bits.  A ciphertext at
    q_0, a random hybrid key.  Two legs that end in the same place, a ciphertext at level L under the key's target secret:
      fused     hefx_hybrid_raise_switch with the collapsed key (made once, outside the window: it is cached per key and level)
      composed  hefx_mod_raise (both polynomials) + hefx_hybrid_apply_galois_batch of one item with the element 1: what
                Evaluator.mod_raise + Evaluator.switch_key(high) run
    hefx_mod_raise serves poly_degree <= 16384, so at N = 32768 the composed leg cannot run: the row records the fused leg alone
    and says so under "owed".  Random canonical operands.  Device time between two events around K calls in a row (queued behind a
    0.5 GiB copy), every leg warmed twice, legs alternating, medians of REPS windows with min and max -- the method of
    tools/hybrid_bsgs_bench.py.  The row transforms of both legs are recorded: counts, not times.
(b) One sparse bootstrap (ns = 16) at N = 16384, scale 2^50, data primes {60, 50 x 13}, alpha = 4: bootstrap_hybrid with
    encaps= under a DENSE main secret, and without it under a main secret of Hamming weight 32.  Wall time of the call and the
    device sync behind it, legs alternating, medians of REPS runs; the decode error of both legs is recorded.
No ratio is expected or asserted.
Usage: hybrid_encaps_bench.py [--out FILE] [--only N] [--no-bootstrap] [--no-raise]"""
import gc, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from seal_fyp_logistic_regression_amd import _build
from seal_fyp_logistic_regression_amd import seal as S

REPS, KCALLS = 5, 10
RINGS, LEVELS, ALPHAS = (16384, 32768), (14, 20), (3, 4)
MOD_RAISE_MAX_N = 16384   # the range of hefx_mod_raise (include/hefx_refresh.h)
BOOT_N, BOOT_NS, BOOT_ALPHA, BOOT_DATA_BITS, BOOT_SCALE, BOOT_HAMMING, AUX_SEED = 16384, 16, 4, [60] + [50] * 13, 2.0 ** 50, 32, 7
args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else None
only = int(args[args.index("--only") + 1]) if "--only" in args else None


def spread(us):
    us = sorted(us)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}


def measure(eng, delay, legs, k, reps=REPS):
    """legs: {name: run} on one engine -> {name: spread of device us per call}"""
    for run in legs.values():
        for _ in range(2):
            run()
        eng.sync()
    dev = {name: [] for name in legs}
    for _ in range(reps):
        for name, run in legs.items():
            ev0, ev1 = eng.event(), eng.event()
            eng.copy_raw(delay[0].ptr, delay[1].ptr, delay[0].nbytes)
            eng.event_record(ev0)
            for _ in range(k):
                run()
            eng.event_record(ev1)
            eng.sync()
            dev[name].append(eng.event_elapsed_ms(ev0, ev1) * 1e3 / k)
            eng.event_destroy(ev0), eng.event_destroy(ev1)
    return {name: spread(dev[name]) for name in legs}


def context(N, primes):
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus([int(p) for p in primes])
    return S.SEALContext.Create(parms)


def random_words(rng, primes, rows, lead, N):
    """lead + [len(rows)][N] uniform canonical words, row r mod primes[rows[r]]"""
    out = np.empty(tuple(lead) + (len(rows), N), dtype=np.uint64)
    for r, m in enumerate(rows):
        out[..., r, :] = rng.integers(0, int(primes[m]), tuple(lead) + (N,), dtype=np.uint64)
    return out


doc = {"tool": "tools/hybrid_encaps_bench.py", "library_sha16": _build.library_sha16(), "source_sha16": _build.source_sha16(), "reps": REPS,
       "raise": {"unit": "us per call, device time between two events around K calls in a row, median of reps windows",
                 "row_transforms_are": "counts of rows transformed, not times", "rows": []}}


def save():
    if out_path:
        json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
        open(out_path, "a").write("\n")


for N in RINGS if "--no-raise" not in args else ():
    if only not in (None, N):
        continue
    for L in LEVELS:
        chain = S.CoeffModulus.Create(N, [60] + [50] * (L - 1) + [60] * max(ALPHAS))
        data, special = chain[:L], chain[L:]
        rng = np.random.default_rng(N + L)
        ct_h = random_words(rng, data, range(1), (2,), N)
        for alpha in ALPHAS:
            primes = data + special[:alpha]
            he = context(N, primes).backend.engine
            delay = (he.empty(1 << 26), he.empty(1 << 26))
            k, dn = L + alpha, he.hybrid_digits(alpha)
            key = he.to_device(random_words(rng, primes, range(k), (dn, 2), N))
            ct = he.to_device(ct_h)
            ckey = he.hybrid_collapse_key(alpha, L, key)
            out_f, out_c, raised = he.empty(2, L, N), he.empty(2, L, N), he.empty(2, L, N)
            legs = {"fused": lambda: he.hybrid_raise_switch(alpha, L, ct, ckey, out=out_f)}
            owed = None
            if N <= MOD_RAISE_MAX_N:
                def composed():
                    he.mod_raise(1, L, ct, 2, out=raised)
                    he.hybrid_apply_galois_batch(alpha, L, [raised], [1], [key], outs=[out_c])
                legs["composed"] = composed
            else:
                owed = f"the composed leg: hefx_mod_raise serves poly_degree <= {MOD_RAISE_MAX_N}, nothing composes the raise at N = {N}"
            m = measure(he, delay, legs, KCALLS)
            dnL = (L + alpha - 1) // alpha
            row = {"N": N, "L": L, "alpha": alpha, "digits": dnL, "calls_between_events": KCALLS, **m,
                   "row_transforms": {"fused": 4 * L + 3 * alpha, "composed": 2 * L + L + dnL * (L + alpha) + 2 * alpha + 2 * L}}
            if owed:
                row["owed"] = owed
            else:
                noise = max(m[leg]["max_us"] - m[leg]["min_us"] for leg in m)
                gain = m["composed"]["median_us"] - m["fused"]["median_us"]
                row.update(composed_over_fused=round(m["composed"]["median_us"] / m["fused"]["median_us"], 3),
                           larger_max_minus_min_us=round(noise, 2), fused_wins_by_more_than_the_spread=bool(gain > noise))
            print(json.dumps(row), flush=True)
            doc["raise"]["rows"].append(row)
            save()
            del delay, key, ct, ckey, out_f, out_c, raised, legs, he
            gc.collect()

if "--no-bootstrap" not in args:
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import bootstrap as B
    N, alpha = BOOT_N, BOOT_ALPHA
    ctx = context(N, S.CoeffModulus.Create(N, BOOT_DATA_BITS + [60] * alpha))
    eng = ctx.backend.engine
    plan = B.plan(N, ctx.primes, BOOT_SCALE, slots=BOOT_NS, special=alpha)
    encoder, ev = S.CKKSEncoder(ctx, device_encode=False), S.Evaluator(ctx)
    encoded = plan.encode(encoder, extended=True)
    v = np.random.default_rng(5).uniform(-1.0, 1.0, BOOT_NS)
    sides = {}
    for name, hamming in (("encaps_dense_secret", None), ("sparse_main_secret", BOOT_HAMMING)):
        kg = S.KeyGenerator(ctx, 1, hamming_weight=hamming)
        gk, rk = kg.hybrid_galois_keys(alpha, plan.galois_steps(), conjugate=True), kg.hybrid_relin_keys(alpha)
        keys = kg.hybrid_encapsulation_keys(alpha, BOOT_HAMMING, seed=AUX_SEED) if hamming is None else None
        ct = S.Encryptor(ctx, kg.public_key(), 2).encrypt(encoder.encode(np.tile(v, (N // 2) // BOOT_NS), BOOT_SCALE, parms_id=1))
        sides[name] = dict(gk=gk, rk=rk, keys=keys, ct=ct, dec=S.Decryptor(ctx, kg.secret_key()))
    legs = {name: (lambda s=s: alg.bootstrap_hybrid(ev, s["ct"], plan, s["gk"], s["rk"], encoded, encaps=s["keys"])) for name, s in sides.items()}
    errors, wall = {}, {name: [] for name in legs}
    for name, run in legs.items():       # warm, and the decode error of the leg
        out = run()
        eng.sync()
        got = encoder.decode(sides[name]["dec"].decrypt(out))
        errors[name] = float(np.abs(got[:BOOT_NS] - v).max() / np.abs(v).max())
    for _ in range(REPS):
        for name, run in legs.items():
            eng.sync()
            t0 = time.perf_counter()
            run()
            eng.sync()
            wall[name].append((time.perf_counter() - t0) * 1e6)
    m = {name: spread(wall[name]) for name in legs}
    noise = max(m[leg]["max_us"] - m[leg]["min_us"] for leg in m)
    boot = {"N": N, "slots": BOOT_NS, "alpha": alpha, "data_primes": len(BOOT_DATA_BITS), "scale_bits": 50, "hamming_weight": BOOT_HAMMING,
            "unit": "us per bootstrap, wall time of the call and the device sync behind it, median of reps runs", **m,
            "encaps_minus_sparse_median_us": round(m["encaps_dense_secret"]["median_us"] - m["sparse_main_secret"]["median_us"], 2),
            "larger_max_minus_min_us": round(noise, 2), "decode_error_of_largest_value": errors,
            "encapsulation_key_bytes": {"low": int(sides["encaps_dense_secret"]["keys"].low.nbytes),
                                        "high": int(sides["encaps_dense_secret"]["keys"].high.hybrid_key(1).nbytes)}}
    print(json.dumps(boot), flush=True)
    doc["bootstrap"] = boot
    save()
