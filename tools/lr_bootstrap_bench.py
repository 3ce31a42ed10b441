"""One iteration of encrypted logistic-regression training with evaluation keys only (algorithms.update_weights_bootstrapped) on
the MI355X, against update_weights_refreshed -- the only other way a step ends, and it needs the secret key -- on the same
inputs and chain, in one process: N = 16384, {60, 50 x (12 + lr_step_levels(3, "ps")), 60}, scale 2^50, Hamming weight 32, ns = 8,
8 weights, degree 3, poly "ps".

  refreshed        update_weights_refreshed(poly="ps") from first-level operands, timed FIRST: the baseline of this session.
  bootstrapped     the whole step from operands at level s = 1 + lr_step_levels, and its three phases with the key switches of each:
                   gradient        lr_gradient(level=s): rows (weights + 1) + the sigmoid's products + weights (rows + 1)
                   update_tile     the product with learning_rate / rows, its rescale, subsum as the tiling, sub and negate:
                                   log2(N / 2 ns) key switches at one prime
                   bootstrap       algorithms.bootstrap and the mod-switch to s: plan.key_switches()
                   and the decode error of the new weights against the float model, for both ways.

Two clocks per leg, as tools/sparse_bootstrap_bench.py: device (K calls between two events, queued behind a 0.5 GiB copy; contains
the device's waits for the host) and host (a window of calls and one synchronise); medians and extremes over REPS windows.
Usage: lr_bootstrap_bench.py [--out FILE] [--n 2048] [--rows 64,256]   (--n 2048: a rehearsal size, not a measurement)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from seal_fyp_logistic_regression_amd import _build, bootstrap, poly
from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import seal as S

REPS, INNER, K = 5, 2, 2
DEGREE, POLY, NS, WEIGHTS, LEARNING_RATE, HAMMING_WEIGHT, SCALE = 3, "ps", 8, 8, 0.5, 32, 2.0 ** 50
STEP = alg.lr_step_levels(DEGREE, POLY)
BITS = [60] + [50] * (12 + STEP) + [60]
args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else None
N = int(args[args.index("--n") + 1]) if "--n" in args else 16384
ROWS = [int(r) for r in args[args.index("--rows") + 1].split(",")] if "--rows" in args else [64]


def spread(us):
    us = sorted(us)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}


def measure(eng, legs, inner=INNER, k=K, reps=REPS):
    """{name: {"device": ..., "host": ...}}; every leg warmed once, then the legs in turn, REPS times on either clock"""
    a, b = measure.delay
    for run in legs.values():
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


def model_step(X, w, y):
    """one step in float64 where the reference's window sums are whole (rows >= weights is NOT that: see
    tests/lr_gradient_cases.py; here the operation sequence itself, on plain vectors)"""
    coeffs = alg.SIGMOID_COEFFS[DEGREE]

    def dot(a, b, size):
        m = np.zeros(N // 2)
        m[:len(a)] = np.asarray(a) * np.asarray(b)[:len(a)]
        dup, acc = m + np.roll(m, size), m.copy()
        for _ in range(1, size):
            dup = np.roll(dup, -1)
            acc += dup
        return acc

    rows, nw = X.shape
    z = np.array([dot(X[i], w, nw)[i] for i in range(rows)])
    pl = sum(c * z ** k for k, c in enumerate(coeffs)) - y
    g = np.array([dot(X[:, j], pl, rows)[j] for j in range(nw)])
    return w - (LEARNING_RATE / rows) * g


parms = S.EncryptionParameters("ckks")
parms.set_poly_modulus_degree(N)
parms.set_coeff_modulus(S.CoeffModulus.Create(N, BITS))
ctx = S.SEALContext.Create(parms)
kg = S.KeyGenerator(ctx, 1, hamming_weight=HAMMING_WEIGHT)
eng, ev, encoder = ctx.backend.engine, S.Evaluator(ctx), S.CKKSEncoder(ctx)
enc, dec, rk = S.Encryptor(ctx, kg.public_key(), 2), S.Decryptor(ctx, kg.secret_key()), kg.relin_keys()
measure.delay = (eng.empty(1 << 26), eng.empty(1 << 26))   # 0.5 GiB each
bp = bootstrap.plan(N, ctx.primes, SCALE, slots=NS, max_value=1.0)
s = 1 + STEP
assert bp.result_level == s
encoded = bp.encode(encoder)
sigmoid_muls = poly.plan(alg.SIGMOID_COEFFS[DEGREE], "power", ctx.primes[:s - 2], SCALE, SCALE).muls

out = {"tool": "tools/lr_bootstrap_bench.py", "box_clock": time.strftime("%Y-%m-%dT%H:%M:%S%z"), "N": N, "chain_bits": BITS,
       "scale": "2^50", "hamming_weight": HAMMING_WEIGHT, "slots": NS, "weights": WEIGHTS, "degree": DEGREE, "poly": POLY,
       "start_level": s, "learning_rate": LEARNING_RATE, "library_sha16": _build.library_sha16(), "source_sha16": _build.source_sha16(),
       "reps": REPS, "calls_per_host_window": INNER, "calls_between_events": K,
       "unit": "us per call; device: between two events around K calls in a row (contains the device's waits for the host); "
               "host: a window of calls and one synchronise", "rows": {}}

for rows in ROWS:
    rng = np.random.default_rng(rows)
    X, w, y = rng.uniform(-1, 1, (rows, WEIGHTS)) / np.sqrt(rows), rng.uniform(-0.5, 0.5, WEIGHTS), rng.integers(0, 2, rows).astype(float)
    want = model_step(X, w, y)
    gk = kg.galois_keys(alg.lr_bootstrap_galois_steps(bp, rows, WEIGHTS), conjugate=True)
    e = lambda v, level=None: enc.encrypt(encoder.encode(np.asarray(v, dtype=float), SCALE, parms_id=level))
    tiled = np.tile(w, N // 2 // NS)
    # ---- the baseline, first: the step the holder of the secret key can finish ---------------------------------------------------
    top = [e(r) for r in X], [e(c) for c in X.T], e(y), e(tiled)
    refreshed = lambda: alg.update_weights_refreshed(ev, encoder, enc, dec, *top, LEARNING_RATE, gk, rk, SCALE, DEGREE, POLY)
    try:
        err_ref = float(np.abs(encoder.decode(dec.decrypt(refreshed())).real[:WEIGHTS] - want).max())
        row = {"rows": rows, "refreshed": {"decode_error": err_ref, "level_of_the_step": ctx.first_parms_id(),
                                           **measure(eng, {"step": refreshed})["step"]}}
    except ValueError as refusal:   # hefx_refresh lifts from at most HEFX_LIFT_MAX_LIN = 16 primes; the second refresh is at 19
        row = {"rows": rows, "refreshed": {"refused": str(refusal), "level_of_the_step": ctx.first_parms_id()}}
    print(json.dumps({"refreshed": row["refreshed"]}), flush=True)
    del top
    # ---- the bootstrapped step and its phases --------------------------------------------------------------------------------------
    feats, featsT, cy, cw = [e(r, s) for r in X], [e(c, s) for c in X.T], e(y, s), e(tiled, s)
    grad, _ = alg.lr_gradient(ev, encoder, enc, feats, featsT, cy, cw, gk, rk, SCALE, DEGREE, POLY, level=s)
    low = alg._update_and_tile(ev, encoder, grad, cw, LEARNING_RATE / rows, SCALE, NS, gk)
    legs = {"gradient": lambda: alg.lr_gradient(ev, encoder, enc, feats, featsT, cy, cw, gk, rk, SCALE, DEGREE, POLY, level=s),
            "update_tile": lambda: alg._update_and_tile(ev, encoder, grad, cw, LEARNING_RATE / rows, SCALE, NS, gk),
            "bootstrap": lambda: ev.mod_switch_to_inplace(alg.bootstrap(ev, low, bp, gk, rk, encoded), s),
            "step": lambda: alg.update_weights_bootstrapped(ev, encoder, enc, feats, featsT, cy, cw, LEARNING_RATE, gk, rk, SCALE, bp,
                                                            DEGREE, POLY, encoded)}
    got = encoder.decode(dec.decrypt(legs["step"]())).real
    row["bootstrapped"] = {"decode_error": float(np.abs(got[:WEIGHTS] - want).max()),
                           "decode_error_all_slots": float(np.abs(got - np.tile(want, N // 2 // NS)).max()),
                           "key_switches": {"gradient": rows * (WEIGHTS + 1) + sigmoid_muls + WEIGHTS * (rows + 1),
                                            "update_tile": (N // (2 * NS)).bit_length() - 1, "bootstrap": bp.key_switches(True)},
                           "galois_keys": len(gk.keys), **measure(eng, legs)}
    b = row["bootstrapped"]
    b["bootstrap_share_of_step_device"] = round(b["bootstrap"]["device"]["median_us"] / b["step"]["device"]["median_us"], 3)
    if "device" in row["refreshed"]:
        b["bootstrapped_over_refreshed_device"] = round(b["step"]["device"]["median_us"] / row["refreshed"]["device"]["median_us"], 3)
    out["rows"][str(rows)] = row
    print(json.dumps({"bootstrapped": b}), flush=True)
    del gk, feats, featsT, cy, cw, grad, low

if out_path:
    json.dump(out, open(out_path, "w"), indent=1, sort_keys=True)
    open(out_path, "a").write("\n")
