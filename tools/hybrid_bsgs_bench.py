"""The hoisted giant steps on the MI355X (include/hefx_hybrid_bsgs.h): (a) one stage of the homomorphic DFT, shape by shape, and
(b) one sparse bootstrap on hybrid keys, in one process.

(a) The stage of tools/hybrid_hoist_bench.py: N in {16384, 32768}, L in {14, 20} data primes {60, 50 x (L-1)}, alpha in {3, 4}
    special primes of 60 bits; n = 2 inputs, m = 8 baby steps (the first is the step 0), G = 8 inner sums (2 outputs x 4 giant
    steps) over all 16 terms, 6 giant rotations (the giant step 0 of each output is none), the sums and the rescale.  Two legs:
      hoisted   hefx_hybrid_bsgs_hoisted (one call) + the batched rescale
      present   hefx_hybrid_plain_combine_hoisted + hefx_hybrid_apply_galois_batch (6 items) + hefx_add_many per output + the
                batched rescale: algorithms._dft_stage_hybrid as it runs by default
    Random canonical operands, keys and plaintexts; every key and plaintext is a device buffer of its own.  Device time between
    two events around K stages in a row (queued behind a 0.5 GiB copy), every leg warmed twice, legs alternating, medians of
    REPS windows with min and max -- the method of tools/hybrid_hoist_bench.py.  The row transforms of both legs are recorded.
(b) One sparse bootstrap (ns = 16) at N = 16384, scale 2^50, data primes {60, 50 x 13}: bootstrap_hybrid on alpha = 4 special
    primes with the giants hoisted and not, and bootstrap on the same data primes with one special prime.  Wall time of the
    call and the device sync behind it, legs alternating, medians of REPS runs; the decode error of every leg and the bytes of
    all evaluation keys of both sides are recorded.
No ratio is expected or asserted.
Usage: hybrid_bsgs_bench.py [--out FILE] [--only N] [--no-bootstrap] [--no-stage]"""
import gc, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from seal_fyp_logistic_regression_amd import _build
from seal_fyp_logistic_regression_amd import seal as S

REPS, KCALLS = 5, 3
RINGS, LEVELS, ALPHAS = (16384, 32768), (14, 20), (3, 4)
SOURCES, BABIES, OUTPUTS, GIANTS = 2, 8, 2, 4
BOOT_N, BOOT_NS, BOOT_ALPHA, BOOT_DATA_BITS, BOOT_SCALE, BOOT_HAMMING = 16384, 16, 4, [60] + [50] * 13, 2.0 ** 50, 32
args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else None
only = int(args[args.index("--only") + 1]) if "--only" in args else None


def spread(us):
    us = sorted(us)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}


def measure(legs, k, reps=REPS):
    """legs: {name: (engine, run)} -> {name: spread of device us per call}"""
    for eng, run in legs.values():
        for _ in range(2):
            run()
        eng.sync()
    dev = {name: [] for name in legs}
    for _ in range(reps):
        for name, (eng, run) in legs.items():
            a, b = delay[eng]
            ev0, ev1 = eng.event(), eng.event()
            eng.copy_raw(a.ptr, b.ptr, a.nbytes)
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


doc = {"tool": "tools/hybrid_bsgs_bench.py", "library_sha16": _build.library_sha16(), "source_sha16": _build.source_sha16(), "reps": REPS,
       "stage": {"inputs": SOURCES, "baby_steps": BABIES, "inner_sums": OUTPUTS * GIANTS, "giant_rotations": OUTPUTS * (GIANTS - 1),
                 "unit": "us per stage, device time between two events around K stages in a row, median of reps windows", "rows": []}}


def save():
    if out_path:
        json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
        open(out_path, "a").write("\n")


delay = {}
T, G, MOVED = SOURCES * BABIES, OUTPUTS * GIANTS, OUTPUTS * (GIANTS - 1)
for N in RINGS if "--no-stage" not in args else ():
    if only not in (None, N):
        continue
    baby_elts = [pow(3, i, 2 * N) for i in range(BABIES)]                      # the first is 1: the step 0
    giant_elts = [pow(3, BABIES * g, 2 * N) for g in range(1, GIANTS)] * OUTPUTS
    for L in LEVELS:
        chain = S.CoeffModulus.Create(N, [60] + [50] * (L - 1) + [60] * max(ALPHAS))
        data, special = chain[:L], chain[L:]
        rng = np.random.default_rng(N + L)
        ct_h = random_words(rng, data, range(L), (SOURCES, 2), N)
        for alpha in ALPHAS:
            hyb = context(N, data + special[:alpha])
            he = hyb.backend.engine
            delay[he] = (he.empty(1 << 26), he.empty(1 << 26))
            k, dn = L + alpha, he.hybrid_digits(alpha)
            key_h = random_words(rng, data + special[:alpha], range(k), (dn, 2), N)
            keys = [he.to_device(key_h) for _ in range(BABIES - 1)]
            del key_h
            src = [he.to_device(ct_h[i]) for i in range(SOURCES)]
            ptk_h = random_words(rng, data + special[:alpha], range(k), (), N)
            pts_k = [[he.to_device(ptk_h) for _ in range(T)] for _ in range(G)]
            inner, moved = [he.empty(2, L, N) for _ in range(G)], [he.empty(2, L, N) for _ in range(MOVED)]
            outs_p, outs_h = he.empty_many(OUTPUTS, (2, L, N)), he.empty_many(OUTPUTS, (2, L, N))
            giant_in = [inner[o * GIANTS + g] for o in range(OUTPUTS) for g in range(1, GIANTS)]
            giant_keys = (keys * 2)[:MOVED]
            # the hoisted entry's view of the same stage: inner sum (o, g) gets giant step g (0: none) and dest = o
            g_elts = [1 if g == 0 else giant_elts[g - 1] for o in range(OUTPUTS) for g in range(GIANTS)]
            g_keys = [None if g == 0 else giant_keys[o * (GIANTS - 1) + g - 1] for o in range(OUTPUTS) for g in range(GIANTS)]
            dest = [o for o in range(OUTPUTS) for _ in range(GIANTS)]

            def run_present():
                he.hybrid_plain_combine_hoisted(alpha, L, src, baby_elts, [None] + keys, pts_k, outs=inner)
                he.hybrid_apply_galois_batch(alpha, L, giant_in, giant_elts, giant_keys, outs=moved)
                for o in range(OUTPUTS):
                    he.add_many(L, 2, [inner[o * GIANTS]] + moved[o * (GIANTS - 1):(o + 1) * (GIANTS - 1)], out=outs_p[o])
                he.rescale_batch(L, 2, outs_p)

            def run_hoisted():
                he.hybrid_bsgs_hoisted(alpha, L, src, baby_elts, [None] + keys, pts_k, g_elts, g_keys, dest, outs=outs_h)
                he.rescale_batch(L, 2, outs_h)

            m = measure({"hoisted": (he, run_hoisted), "present": (he, run_present)}, KCALLS)
            full = L + dn * (L + alpha) + 2 * alpha + 2 * L          # one hybrid switch as launched (hefx_hybrid.h)
            decomp, down = L + dn * (L + alpha), 2 * alpha + 2 * L
            noise = max(m[leg]["max_us"] - m[leg]["min_us"] for leg in m)
            gain = m["present"]["median_us"] - m["hoisted"]["median_us"]
            row = {"N": N, "L": L, "alpha": alpha, "digits": dn, "calls_between_events": KCALLS, **m,
                   "present_over_hoisted": round(m["present"]["median_us"] / m["hoisted"]["median_us"], 3),
                   "larger_max_minus_min_us": round(noise, 2), "hoisted_wins_by_more_than_the_spread": bool(gain > noise),
                   "row_transforms": {"present": SOURCES * decomp + G * down + MOVED * full,
                                      "hoisted": SOURCES * decomp + MOVED * (alpha + L + L + dn * (L + alpha)) + OUTPUTS * down}}
            print(json.dumps(row), flush=True)
            doc["stage"]["rows"].append(row)
            save()
            del delay[he], keys, src, pts_k, inner, moved, outs_p, outs_h, giant_in, giant_keys, g_keys, he, hyb
            gc.collect()

if doc["stage"]["rows"]:
    doc["stage"]["hoisted_wins_at_every_shape"] = all(r["hoisted_wins_by_more_than_the_spread"] for r in doc["stage"]["rows"])
    save()

if "--no-bootstrap" not in args:
    from seal_fyp_logistic_regression_amd import algorithms as alg
    from seal_fyp_logistic_regression_amd import bootstrap as B
    N = BOOT_N
    chain = S.CoeffModulus.Create(N, BOOT_DATA_BITS + [60] * BOOT_ALPHA)
    data, special = chain[:len(BOOT_DATA_BITS)], chain[len(BOOT_DATA_BITS):]
    v = np.random.default_rng(5).uniform(-1.0, 1.0, BOOT_NS)
    sides = {}
    for name, primes, alpha in (("hybrid", data + special, BOOT_ALPHA), ("reference", data + special[:1], 1)):
        ctx = context(N, primes)
        kg = S.KeyGenerator(ctx, 1, hamming_weight=BOOT_HAMMING)
        plan = B.plan(N, ctx.primes, BOOT_SCALE, slots=BOOT_NS, special=alpha)
        encoder = S.CKKSEncoder(ctx, device_encode=False)
        if name == "hybrid":
            gk, rk = kg.hybrid_galois_keys(alpha, plan.galois_steps(), conjugate=True), kg.hybrid_relin_keys(alpha)
            encoded = plan.encode(encoder, extended=True)
        else:
            gk, rk = kg.galois_keys(plan.galois_steps(), conjugate=True), kg.relin_keys()
            encoded = plan.encode(encoder)
        ct = S.Encryptor(ctx, kg.public_key(), 2).encrypt(encoder.encode(np.tile(v, (N // 2) // BOOT_NS), BOOT_SCALE, parms_id=1))
        sides[name] = dict(ctx=ctx, ev=S.Evaluator(ctx), plan=plan, gk=gk, rk=rk, encoded=encoded, ct=ct, encoder=encoder,
                           dec=S.Decryptor(ctx, kg.secret_key()),
                           key_bytes=sum(int(k.nbytes) for keys in (gk, rk) for k in keys.keys.values()), key_count=len(gk.keys) + len(rk.keys))
    h, r = sides["hybrid"], sides["reference"]
    legs = {"hybrid_hoisted": (h, lambda: alg.bootstrap_hybrid(h["ev"], h["ct"], h["plan"], h["gk"], h["rk"], h["encoded"], hoist_giants=True)),
            "hybrid_unhoisted": (h, lambda: alg.bootstrap_hybrid(h["ev"], h["ct"], h["plan"], h["gk"], h["rk"], h["encoded"], hoist_giants=False)),
            "reference": (r, lambda: alg.bootstrap(r["ev"], r["ct"], r["plan"], r["gk"], r["rk"], r["encoded"]))}
    errors, wall = {}, {name: [] for name in legs}
    for name, (e, run) in legs.items():       # warm, and the decode error of the leg
        out = run()
        e["ctx"].backend.engine.sync()
        got = e["encoder"].decode(e["dec"].decrypt(out))
        errors[name] = float(np.abs(got[:BOOT_NS] - v).max() / np.abs(v).max())
    for _ in range(REPS):
        for name, (e, run) in legs.items():
            eng = e["ctx"].backend.engine
            eng.sync()
            t0 = time.perf_counter()
            run()
            eng.sync()
            wall[name].append((time.perf_counter() - t0) * 1e6)
    boot = {"N": N, "slots": BOOT_NS, "alpha": BOOT_ALPHA, "data_primes": len(data), "scale_bits": 50, "hamming_weight": BOOT_HAMMING,
            "unit": "us per bootstrap, wall time of the call and the device sync behind it, median of reps runs",
            **{name: spread(wall[name]) for name in legs}, "decode_error_of_largest_value": errors,
            "evaluation_key_bytes": {"hybrid": h["key_bytes"], "reference": r["key_bytes"]},
            "evaluation_keys": {"hybrid": h["key_count"], "reference": r["key_count"]},
            "result_level": {"hybrid": h["plan"].result_level, "reference": r["plan"].result_level}}
    print(json.dumps(boot), flush=True)
    doc["bootstrap"] = boot
    save()
