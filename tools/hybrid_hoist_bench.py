"""Hoisted hybrid key switching on the MI355X (include/hefx_hybrid_hoist.h): one stage of the homomorphic DFT, shape by shape in
one process.

  N in {16384, 32768}, L in {14, 20} data primes {60, 50 x (L-1)}, alpha in {3, 4} special primes of 60 bits.  The stage: n = 2
  inputs, m = 8 baby steps (the first is the step 0: no key switch), G = 8 inner sums (2 outputs x 4 giant steps) over all 16
  terms, then the 6 giant rotations (the giant step 0 of each output is none).  The final add_many and rescale are the same
  kernels in every leg and are left out.  Four legs:
    op_by_op    hefx_hybrid_apply_galois_batch (14 items) + hefx_plain_combine + hefx_hybrid_apply_galois_batch (6 items)
    rotate      hefx_hybrid_rotate_hoisted_batch (2 x 7) + hefx_plain_combine + hefx_hybrid_apply_galois_batch (6)
    combine     hefx_hybrid_plain_combine_hoisted (2 x 8, key-level plaintexts) + hefx_hybrid_apply_galois_batch (6)
    reference   the one-special-prime stage on the same data primes: hefx_apply_galois_batch (14) + hefx_plain_combine +
                hefx_apply_galois_batch (6)

Random canonical operands, keys and plaintexts (the time does not depend on the words); every key and plaintext is a device
buffer of its own, so no leg is flattered by a cache hit that a real stage would not have.  Device time between two events around
K stages in a row (queued behind a 0.5 GiB copy, so that the host is ahead of the device when the window opens), every leg warmed
twice, legs alternating, medians of REPS windows -- the method of tools/hybrid_bench.py.  Recorded per shape: the times and the
row transforms each leg launches.  No ratio is expected or asserted.
Usage: hybrid_hoist_bench.py [--out FILE] [--only N]"""
import gc, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from seal_fyp_logistic_regression_amd import _build
from seal_fyp_logistic_regression_amd import seal as S

REPS, KCALLS = 5, 3
RINGS, LEVELS, ALPHAS = (16384, 32768), (14, 20), (3, 4)
SOURCES, BABIES, OUTPUTS, GIANTS = 2, 8, 2, 4
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


def random_words(rng, primes, rows, lead):
    """lead + [len(rows)][N] uniform canonical words, row r mod primes[rows[r]]"""
    out = np.empty(tuple(lead) + (len(rows), N), dtype=np.uint64)
    for r, m in enumerate(rows):
        out[..., r, :] = rng.integers(0, int(primes[m]), tuple(lead) + (N,), dtype=np.uint64)
    return out


def save(row):
    print(json.dumps(row), flush=True)
    rows.append(row)
    if out_path:
        doc = {"tool": "tools/hybrid_hoist_bench.py", "library_sha16": _build.library_sha16(), "source_sha16": _build.source_sha16(),
               "reps": REPS, "unit": "us per stage, device time between two events around K stages in a row, median of reps windows",
               "stage": {"inputs": SOURCES, "baby_steps": BABIES, "inner_sums": OUTPUTS * GIANTS, "giant_rotations": OUTPUTS * (GIANTS - 1)},
               "rows": rows}
        json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
        open(out_path, "a").write("\n")


rows, delay = [], {}
T, G, MOVED = SOURCES * BABIES, OUTPUTS * GIANTS, OUTPUTS * (GIANTS - 1)
for N in RINGS:
    if only not in (None, N):
        continue
    baby_elts = [pow(3, i, 2 * N) for i in range(BABIES)]                      # the first is 1: the step 0
    giant_elts = [pow(3, BABIES * g, 2 * N) for g in range(1, GIANTS)] * OUTPUTS
    for L in LEVELS:
        chain = S.CoeffModulus.Create(N, [60] + [50] * (L - 1) + [60] * max(ALPHAS))
        data, special = chain[:L], chain[L:]
        rng = np.random.default_rng(N + L)
        ct_h = random_words(rng, data, range(L), (SOURCES, 2))
        pt_h = random_words(rng, data, range(L), ())
        # ---- the reference: one special prime
        ref = context(N, data + special[:1])
        re_ = ref.backend.engine
        delay[re_] = (re_.empty(1 << 26), re_.empty(1 << 26))
        key_ref_h = random_words(rng, data + special[:1], range(L + 1), (L, 2))
        keys_r = [re_.to_device(key_ref_h) for _ in range(BABIES - 1)]
        del key_ref_h
        src_r = [re_.to_device(ct_h[i]) for i in range(SOURCES)]
        pts_r = [[re_.to_device(pt_h) for _ in range(T)] for _ in range(G)]
        rot_r, inner_r, moved_r = [re_.empty(2, L, N) for _ in range(T - SOURCES)], [re_.empty(2, L, N) for _ in range(G)], [re_.empty(2, L, N) for _ in range(MOVED)]
        terms_r = [src_r[i] if b == 0 else rot_r[i * (BABIES - 1) + b - 1] for i in range(SOURCES) for b in range(BABIES)]
        giant_in_r = [inner_r[o * GIANTS + g] for o in range(OUTPUTS) for g in range(1, GIANTS)]

        def run_r():
            re_.apply_galois_batch(L, [s for s in src_r for _ in range(BABIES - 1)], baby_elts[1:] * SOURCES, keys_r * SOURCES, outs=rot_r)
            re_.plain_combine(L, terms_r, pts_r, outs=inner_r)
            re_.apply_galois_batch(L, giant_in_r, giant_elts, (keys_r * 2)[:MOVED], outs=moved_r)

        for alpha in ALPHAS:
            hyb = context(N, data + special[:alpha])
            he = hyb.backend.engine
            delay[he] = (he.empty(1 << 26), he.empty(1 << 26))
            k, dn = L + alpha, he.hybrid_digits(alpha)
            key_h = random_words(rng, data + special[:alpha], range(k), (dn, 2))
            keys = [he.to_device(key_h) for _ in range(BABIES - 1)]
            del key_h
            src = [he.to_device(ct_h[i]) for i in range(SOURCES)]
            pts_L = [[he.to_device(pt_h) for _ in range(T)] for _ in range(G)]
            ptk_h = random_words(rng, data + special[:alpha], range(k), ())
            pts_k = [[he.to_device(ptk_h) for _ in range(T)] for _ in range(G)]
            rot, inner, moved = [he.empty(2, L, N) for _ in range(T - SOURCES)], [he.empty(2, L, N) for _ in range(G)], [he.empty(2, L, N) for _ in range(MOVED)]
            terms = [src[i] if b == 0 else rot[i * (BABIES - 1) + b - 1] for i in range(SOURCES) for b in range(BABIES)]
            giant_in = [inner[o * GIANTS + g] for o in range(OUTPUTS) for g in range(1, GIANTS)]
            giant_keys = (keys * 2)[:MOVED]

            def giants():
                he.hybrid_apply_galois_batch(alpha, L, giant_in, giant_elts, giant_keys, outs=moved)

            def run_op():
                he.hybrid_apply_galois_batch(alpha, L, [s for s in src for _ in range(BABIES - 1)], baby_elts[1:] * SOURCES, keys * SOURCES, outs=rot)
                he.plain_combine(L, terms, pts_L, outs=inner)
                giants()

            def run_rot():
                he.hybrid_rotate_hoisted_batch(alpha, L, src, baby_elts[1:], keys, outs=rot)
                he.plain_combine(L, terms, pts_L, outs=inner)
                giants()

            def run_comb():
                he.hybrid_plain_combine_hoisted(alpha, L, src, baby_elts, [None] + keys, pts_k, outs=inner)
                giants()

            m = measure({"op_by_op": (he, run_op), "rotate": (he, run_rot), "combine": (he, run_comb), "reference": (re_, run_r)}, KCALLS)
            full = L + dn * (L + alpha) + 2 * alpha + 2 * L          # one hybrid switch as launched (hefx_hybrid.h)
            decomp, down = L + dn * (L + alpha), 2 * alpha + 2 * L
            save({"N": N, "L": L, "alpha": alpha, "digits": dn, "calls_between_events": KCALLS, **m,
                  "op_by_op_over_combine": round(m["op_by_op"]["median_us"] / m["combine"]["median_us"], 3),
                  "op_by_op_over_rotate": round(m["op_by_op"]["median_us"] / m["rotate"]["median_us"], 3),
                  "reference_over_combine": round(m["reference"]["median_us"] / m["combine"]["median_us"], 3),
                  "row_transforms": {"op_by_op": (T - SOURCES + MOVED) * full, "rotate": SOURCES * decomp + (T - SOURCES) * down + MOVED * full,
                                     "combine": SOURCES * decomp + G * down + MOVED * full,
                                     "reference_about": (T - SOURCES + MOVED) * (L * L + 5 * L)},
                  "key_bytes_hybrid": dn * 2 * k * N * 8, "key_bytes_reference": L * 2 * (L + 1) * N * 8})
            del delay[he], keys, src, pts_L, pts_k, rot, inner, moved, terms, giant_in, giant_keys, he, hyb
            gc.collect()
        del delay[re_], keys_r, src_r, pts_r, rot_r, inner_r, moved_r, terms_r, giant_in_r, re_, ref
        gc.collect()
