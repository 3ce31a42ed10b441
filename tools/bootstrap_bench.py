"""hefx_product_combine, algorithms.eval_mod and algorithms.bootstrap on the MI355X; both sides of every comparison alternate in
one process (same clocks, same neighbours).

  node        the nodes of the degree-31 plan of EvalMod's interpolant (every COMBINE that takes deferred products: its level,
              P products, m linear terms, the operands' own levels) at N = 16384 on {60, 50 x 8, 60}, n = 2 items in lockstep
              (the two chains of the DFT), two ways:
                fused     Engine.product_combine, then ONE relinearize_batch of the n sums
                composed  the parent commit's path: multiply_batch of the n P products, relinearize_batch of all of them, one
                          scalar_combine per item over its P + m size-2 inputs
              and the kernel alone (fused_kernel) against what forms the same size-3 sum call by call (unfused_sum):
              multiply_batch of the n P products and one size-3 scalar_combine per item -- the products written, read back and
              summed.  Every buffer is allocated outside the timed window; where the node has no linear term the two size-3
              results are compared word for word.
              Two clocks per leg.  host: a window of INNER calls and one device synchronise.  device: K calls queued while the
              device is busy with a 0.5 GiB copy, between two events.
  eval_mod    algorithms.eval_mod lazy against eager on the two outputs of coeffs_to_slots, N = 16384, {60, 50 x 13, 60}, scale
              2^50, Hamming weight 32, with the key switches of either.
  bootstrap   one whole algorithms.bootstrap on the same ring, and its four phases (mod_raise, coeffs_to_slots, eval_mod,
              slots_to_coeffs) each between synchronises.

REPS windows per leg, alternating; medians and extremes.  A node shape at which the fused leg loses (with the key switches) is
listed under "fused_loses": Evaluator.product_combine would have to send it to the composition.
Usage: bootstrap_bench.py [--out FILE] [--no-bootstrap]   (writes the "timing" section; the precision section of
profiles/bootstrap.json comes from tests/test_bootstrap_cpu.py with BOOTSTRAP_RECORD=1)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from seal_fyp_logistic_regression_amd import _build, bootstrap, capi, poly
from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import seal as S

REPS, INNER = 9, 50
args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else None
N = int(args[args.index("--n") + 1]) if "--n" in args else 16384   # (--n 2048: a rehearsal size, not a measurement)


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


_delay = {}


def device_us(eng, run, reps=5, K=8):
    """device time per run: K runs queued behind a long copy (the host is done submitting before the copy ends), between events"""
    if id(eng) not in _delay:
        _delay.clear()
        _delay[id(eng)] = (eng.empty(1 << 26), eng.empty(1 << 26))   # 0.5 GiB each
    a, b = _delay[id(eng)]
    res = []
    for _ in range(reps):
        ev0, ev1 = eng.event(), eng.event()
        eng.copy_raw(a.ptr, b.ptr, a.nbytes)
        eng.event_record(ev0)
        for _ in range(K):
            run()
        eng.event_record(ev1)
        eng.sync()
        res.append(eng.event_elapsed_ms(ev0, ev1) * 1e3 / K)
        eng.event_destroy(ev0), eng.event_destroy(ev1)
    return {"median_us": round(statistics.median(res), 2), "min_us": round(min(res), 2), "runs_per_window": K}


def make(bits, hamming_weight=None, seed=1):
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(S.CoeffModulus.Create(N, bits))
    ctx = S.SEALContext.Create(parms)
    kg = S.KeyGenerator(ctx, seed, hamming_weight=hamming_weight)
    return dict(ctx=ctx, kg=kg, eng=ctx.backend.engine, enc=S.Encryptor(ctx, kg.public_key(), seed + 1),
                dec=S.Decryptor(ctx, kg.secret_key()), encoder=S.CKKSEncoder(ctx), ev=S.Evaluator(ctx),
                rk=kg.relin_keys())


def interpolant(degree=31, r=3, K=12):
    return bootstrap.chebyshev_interpolant(lambda u: np.cos((2.0 * np.pi * (K + 0.25) * u - 0.5 * np.pi) / 2.0 ** r), degree)


out = {"tool": "tools/bootstrap_bench.py", "box_clock": time.strftime("%Y-%m-%dT%H:%M:%S%z"), "library_sha16": _build.library_sha16(),
       "source_sha16": _build.source_sha16(), "reps": REPS, "calls_per_window": INNER, "N": N, "node": [], "fused_loses": []}

# ---- node ------------------------------------------------------------------------------------------------------------------
e = make([60] + [50] * 8 + [60])
eng, primes, top = e["eng"], e["ctx"].primes, e["ctx"].first_parms_id()
plan = poly.plan(interpolant(), "chebyshev", primes[:top], 2.0 ** 50)
deferred = plan.deferred()
level_of = {0: top}
for st in plan.steps:
    level_of[st.dst] = st.level - 1 if st.op == capi.POLY_COMBINE else st.level
rng = np.random.default_rng(1)
n_items = 2
rk = e["rk"].key(0)


def device_ct(rows):
    return eng.to_device(np.stack([np.stack([rng.integers(0, primes[j], N, dtype=np.uint64) for j in range(rows)]) for _ in range(2)]))


seen = set()
for ci, st in enumerate(plan.steps):
    muls = [plan.steps[i] for i, c in deferred.items() if c == ci]
    if not muls:
        continue
    lin_src = [t.src for t in st.terms if t.src not in {m_.dst for m_ in muls}]
    L, P, m = st.level, len(muls), len(lin_src)
    a_rows, b_rows, lin_rows = [level_of[x.a] for x in muls], [level_of[x.b] for x in muls], [level_of[s] for s in lin_src]
    shape = (L, P, m, tuple(a_rows), tuple(b_rows), tuple(lin_rows))
    if shape in seen:
        continue
    seen.add(shape)
    A = [[device_ct(r) for r in a_rows] for _ in range(n_items)]
    B = [[A[i][p] if muls[p].a == muls[p].b else device_ct(b_rows[p]) for p in range(P)] for i in range(n_items)]
    Lin = [[device_ct(r) for r in lin_rows] for _ in range(n_items)]
    u = np.array([[rng.integers(1, primes[j], dtype=np.uint64) for j in range(L)] for _ in range(P)], dtype=np.uint64).reshape(P, L)
    w = np.array([[rng.integers(1, primes[j], dtype=np.uint64) for j in range(L)] for _ in range(m)], dtype=np.uint64).reshape(m, L)
    c = np.array([rng.integers(0, primes[j], dtype=np.uint64) for j in range(L)], dtype=np.uint64)
    low = lambda d, r: d if r == L else eng.mod_drop(r, L, 2, d)
    lowA = [[low(A[i][p], a_rows[p]) for p in range(P)] for i in range(n_items)]
    lowB = [[lowA[i][p] if muls[p].a == muls[p].b else low(B[i][p], b_rows[p]) for p in range(P)] for i in range(n_items)]
    lowL = [[low(Lin[i][k], lin_rows[k]) for k in range(m)] for i in range(n_items)]
    flatA, flatB = [x for r in lowA for x in r], [x for r in lowB for x in r]
    sums3, sums2 = eng.empty_many(n_items, (3, L, N)), eng.empty_many(n_items, (2, L, N))
    prod3, prod2 = eng.empty_many(n_items * P, (3, L, N)), eng.empty_many(n_items * P, (2, L, N))
    outs2, outs3 = eng.empty_many(n_items, (2, L, N)), eng.empty_many(n_items, (3, L, N))
    w_all = np.concatenate([u, w])[None] if m else u[None]          # [1][P + m][L]
    u_only = u[None]

    def fused(relin=True):
        eng.product_combine(L, A, a_rows, B, b_rows, u, Lin, lin_rows, w if m else None, c, outs=sums3)
        if relin:
            eng.relinearize_batch(L, sums3, rk, outs=sums2)

    def composed():
        eng.multiply_batch(L, flatA, flatB, outs=prod3)
        eng.relinearize_batch(L, prod3, rk, outs=prod2)
        for i in range(n_items):
            eng.scalar_combine(L, 2, prod2[i * P:(i + 1) * P] + lowL[i], [L] * (P + m), w_all, c[None], outs=[outs2[i]])

    def unfused_sum():   # the same size-3 words as the fused kernel, call by call: products written, read back, summed
        eng.multiply_batch(L, flatA, flatB, outs=prod3)
        for i in range(n_items):
            eng.scalar_combine(L, 3, prod3[i * P:(i + 1) * P], [L] * P, u_only, c[None], outs=[outs3[i]])

    fused(False), unfused_sum()
    eng.sync()
    same = m == 0 and all(np.array_equal(a_.download(), b_.download()) for a_, b_ in zip(sums3, outs3))
    host = alternate(eng, {"fused": fused, "composed": composed, "fused_kernel": lambda: fused(False), "unfused_sum": unfused_sum})
    dev = {name: device_us(eng, run) for name, run in (("fused", fused), ("composed", composed), ("fused_kernel", lambda: fused(False)),
                                                        ("unfused_sum", unfused_sum))}
    row = {"L": L, "P": P, "m": m, "n": n_items, "a_rows": a_rows, "b_rows": b_rows, "lin_rows": lin_rows,
           "key_switches": {"fused": n_items, "composed": n_items * P}, "host": host, "device": dev,
           "words_equal_kernel_pair": same if m == 0 else "not comparable (linear terms are size 2)",
           "speedup_device_with_key_switches": round(dev["composed"]["median_us"] / dev["fused"]["median_us"], 2),
           "speedup_device_kernel_only": round(dev["unfused_sum"]["median_us"] / dev["fused_kernel"]["median_us"], 2)}
    out["node"].append(row)
    if dev["fused"]["median_us"] > dev["composed"]["median_us"]:
        out["fused_loses"].append({"L": L, "P": P, "m": m})
    print(json.dumps(row), flush=True)
del e, eng, A, B, Lin

# ---- eval_mod and the whole bootstrap -------------------------------------------------------------------------------------------
if "--no-bootstrap" not in args:
    e = make([60] + [50] * 13 + [60], hamming_weight=32)
    eng, ev = e["eng"], e["ev"]
    bp = bootstrap.plan(N, e["ctx"].primes, 2.0 ** 50)
    gk = e["kg"].galois_keys(bp.galois_steps(), conjugate=True)
    encoded = bp.encode(e["encoder"])
    v = np.random.default_rng(5).uniform(-1.0, 1.0, N // 2)
    ct = e["enc"].encrypt(e["encoder"].encode(v, 2.0 ** 50, parms_id=1))
    raised = ev.mod_raise(ct, bp.top_level)
    ca, cb = alg.coeffs_to_slots(ev, raised, bp.c2s, gk, encoded[0])
    ya, yb = alg.eval_mod(ev, [ca, cb], bp, e["rk"])
    eng.sync()
    p31 = poly.plan(bp.coeffs, "chebyshev", e["ctx"].primes[:bp.evalmod_level], 2.0 ** 50, bp.poly_target_scale)
    em = alternate(eng, {"lazy": lambda: alg.eval_mod(ev, [ca, cb], bp, e["rk"], lazy=True),
                         "eager": lambda: alg.eval_mod(ev, [ca, cb], bp, e["rk"], lazy=False)}, inner=5)
    out["eval_mod"] = {"chain_bits": [60] + [50] * 13 + [60], "scale": "2^50", "items": 2, "unit": "us per eval_mod of both chains",
                       "key_switches_per_chain": {"lazy": p31.relinearizations(True) + bp.r, "eager": p31.muls + bp.r},
                       **em, "speedup": round(em["eager"]["median_us"] / em["lazy"]["median_us"], 3)}
    print(json.dumps(out["eval_mod"]), flush=True)
    phases = {"mod_raise": lambda: ev.mod_raise(ct, bp.top_level),
              "coeffs_to_slots": lambda: alg.coeffs_to_slots(ev, raised, bp.c2s, gk, encoded[0]),
              "eval_mod": lambda: alg.eval_mod(ev, [ca, cb], bp, e["rk"]),
              "slots_to_coeffs": lambda: alg.slots_to_coeffs(ev, ya, yb, bp.s2c, gk, encoded[1]),
              "bootstrap": lambda: alg.bootstrap(ev, ct, bp, gk, e["rk"], encoded)}
    ph = alternate(eng, phases, inner=3)
    res = alg.bootstrap(ev, ct, bp, gk, e["rk"], encoded)
    err = float(np.abs(e["encoder"].decode(e["dec"].decrypt(res)).real - v).max())
    out["bootstrap"] = {"unit": "us per call, host clock around the call and a synchronise", "key_switches": bp.key_switches(True),
                        "levels": bp.levels(), "result_level": bp.result_level, "decode_error": err, **ph}
    print(json.dumps(out["bootstrap"]), flush=True)

if out_path:
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["timing"] = out
    json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
    open(out_path, "a").write("\n")
