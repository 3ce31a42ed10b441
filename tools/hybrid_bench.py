"""Hybrid key switching on the MI355X (include/hefx_hybrid.h) against the key switch of hefx.h, shape by shape in one process:

  N in {16384, 32768}, L in {5, 8, 14, 20} data primes {60, 50 x (L-1)}, alpha in {1, 2, 3, 4} special primes of 60 bits,
  one item (hefx_hybrid_apply_galois_batch with the element 1 against hefx_switch_key) and 64 items (the element 3 against
  hefx_apply_galois_batch), every ciphertext at level L = k - alpha.  The reference context has the SAME data primes and ONE
  special prime (the first of the four), so at alpha = 1 the two chains and key layouts coincide and the words are compared.

Random canonical operands and keys (the time does not depend on the words).  Device time between two events around K calls in a
row (queued behind a 0.5 GiB copy, so that the host is ahead of the device when the window opens), both legs warmed twice, legs
alternating, medians of REPS windows.  Recorded per shape: both times, reference / hybrid, the key bytes of both, and the row
transforms the hybrid entry launches.  No ratio is expected or asserted: this tool is where the first figures come from.
Usage: hybrid_bench.py [--out FILE] [--only N]"""
import gc, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from seal_fyp_logistic_regression_amd import _build
from seal_fyp_logistic_regression_amd import seal as S

REPS = 5
RINGS, LEVELS, ALPHAS, BATCHES = (16384, 32768), (5, 8, 14, 20), (1, 2, 3, 4), (1, 64)
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
        doc = {"tool": "tools/hybrid_bench.py", "library_sha16": _build.library_sha16(), "source_sha16": _build.source_sha16(), "reps": REPS,
               "unit": "us per call, device time between two events around K calls in a row, median of reps windows",
               "reference": "hefx_switch_key (1 item) / hefx_apply_galois_batch (64 items) on the same data primes with one special prime",
               "rows": rows}
        json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
        open(out_path, "a").write("\n")


rows, delay = [], {}
for N in RINGS:
    if only not in (None, N):
        continue
    for L in LEVELS:
        chain = S.CoeffModulus.Create(N, [60] + [50] * (L - 1) + [60] * max(ALPHAS))
        data, special = chain[:L], chain[L:]
        rng = np.random.default_rng(N + L)
        ct_h = random_words(rng, data, range(L), (max(BATCHES), 2))
        ref = context(N, data + special[:1])
        re_ = ref.backend.engine
        delay[re_] = (re_.empty(1 << 26), re_.empty(1 << 26))
        kr = L + 1
        key_ref_h = random_words(rng, data + special[:1], range(kr), (L, 2))
        key_ref = re_.to_device(key_ref_h)
        ins_r = [re_.to_device(ct_h[i]) for i in range(max(BATCHES))]
        outs_r = [re_.empty(2, L, N) for _ in range(max(BATCHES))]
        for alpha in ALPHAS:
            hyb = context(N, data + special[:alpha])
            he = hyb.backend.engine
            delay[he] = (he.empty(1 << 26), he.empty(1 << 26))
            k, dnum = L + alpha, he.hybrid_digits(alpha)
            assert dnum == -(-L // alpha)
            key_h = key_ref_h if alpha == 1 else random_words(rng, data + special[:alpha], range(k), (dnum, 2))
            key = he.to_device(key_h)
            ins_h = [he.to_device(ct_h[i]) for i in range(max(BATCHES))]
            outs_h = [he.empty(2, L, N) for _ in range(max(BATCHES))]
            for n in BATCHES:
                elt = 1 if n == 1 else 3
                run_h = lambda: he.hybrid_apply_galois_batch(alpha, L, ins_h[:n], [elt] * n, [key] * n, outs=outs_h[:n])
                if n == 1:
                    run_r = lambda: re_.switch_key(L, ins_r[0], key_ref, out=outs_r[0])
                else:
                    run_r = lambda: re_.apply_galois_batch(L, ins_r[:n], [elt] * n, [key_ref] * n, outs=outs_r[:n])
                equal = None
                if alpha == 1:
                    run_h(), run_r()
                    equal = all(bool(np.array_equal(outs_h[i].download(), outs_r[i].download())) for i in range(n))
                kcalls = 20 if n == 1 else 3
                m = measure({"hybrid": (he, run_h), "reference": (re_, run_r)}, kcalls)
                dn = -(-L // alpha)
                save({"N": N, "L": L, "alpha": alpha, "items": n, "digits": dn, "calls_between_events": kcalls,
                      "hybrid": m["hybrid"], "reference": m["reference"],
                      "reference_over_hybrid": round(m["reference"]["median_us"] / m["hybrid"]["median_us"], 3),
                      "key_bytes_hybrid": dnum * 2 * k * N * 8, "key_bytes_reference": L * 2 * kr * N * 8,
                      "row_transforms_hybrid": L + dn * (L + alpha) + 2 * alpha + 2 * L,
                      "row_transforms_statement": L + dn * (L + alpha) - L + 2 * alpha + 2 * L,
                      "words_equal_reference": equal})
            del delay[he], key, ins_h, outs_h, he, hyb
            gc.collect()
        del delay[re_], key_ref, ins_r, outs_r, re_, ref
        gc.collect()
