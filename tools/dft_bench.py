"""hefx_plain_combine and algorithms.coeffs_to_slots on the MI355X, the fused call against what it replaces, both sides
alternating in one process (same clocks, same neighbours), at N = 16384, L = 5 and N = 32768, L = 8.

  primitive   Engine.plain_combine against hefx_multiply_plain_sum (mulplain_sum_kernel, the parent commit's path for the
              inner sums of a baby-step/giant-step transform) on IDENTICAL pointer lists: one grouped call where every output
              has the same number of terms, else one call per output.  Patterns: m = G = 8 dense, m = G = 4 dense, and the
              stage shapes of the levels = 3 plans of dft.py at that N (the block-sparse matrices algorithms._dft_stage hands
              over: both chains, every giant step).  Every buffer of both legs is allocated outside the timed window and the
              legs' words are compared.
              Bytes by DESIGN.md's count, in L * N words: unfused 4 d reads (d non-null terms), fused d + 2 * (inputs a tile
              uses, summed over the tiles; the tile width by the rule of hefx_capi.cpp, restated below) reads, 2 G written by
              both; achieved bytes/s on each leg's own count and device time.
              Two clocks per leg.  host: a window of INNER calls and one device synchronise -- what a caller pays, the host's
              submission included (a small call is bound by it).  device: K calls queued while the device is busy with a
              0.5 GiB copy, between two events -- the device's own time per call, table copy and launch gaps included.
  transform   coeffs_to_slots at N = 32768, levels = 3 on {60, 40 x 7, 60}, its key-switch count beside the time, with the
              fused inner sums and with Evaluator.plain_combine sent down its fallback (multiply_plain_sum per output).

REPS windows per leg, alternating; medians and extremes.
Usage: dft_bench.py [--out FILE] [--no-transform]   (writes the "timing" section; the precision section of profiles/dft.json
comes from tests/test_dft_cpu.py with DFT_RECORD=1)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from seal_fyp_logistic_regression_amd import Engine, _build, capi, dft
from seal_fyp_logistic_regression_amd import algorithms as alg
from seal_fyp_logistic_regression_amd import seal as S

REPS, INNER, HBM_PEAK, TARGET_WAVES, RING_SLOT = 9, 100, 8e12, 4096, 10240
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


def tile_width(G, m, L, N):
    """plain_combine_tile of hefx_capi.cpp"""
    words = lambda gt: m + -(-G // gt) * (gt + m * gt)
    gt = 8
    while gt > 1 and gt // 2 >= G:
        gt //= 2
    while gt > 1 and L * (N // 128) * -(-G // gt) < TARGET_WAVES:
        gt //= 2
    while gt > 1 and words(gt) > RING_SLOT:
        gt //= 2
    return gt


_delay = {}


def device_us(eng, run, calls_per_run, reps=5):
    """device time per run: K runs queued behind a long copy (the host is done submitting before the copy ends), between events"""
    if id(eng) not in _delay:
        _delay.clear()
        _delay[id(eng)] = (eng.empty(1 << 26), eng.empty(1 << 26))   # 0.5 GiB each
    a, b = _delay[id(eng)]
    K = max(1, min(12, 24 // calls_per_run))
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


def stage_pattern(stage):
    """the boolean [G][m] matrix algorithms._dft_stage hands to plain_combine for this stage"""
    nb = len(stage.babies)
    rows = []
    for c in range(stage.outputs):
        feeds = [(0, c)] if stage.mode == "split" else [(c, 0)] if stage.mode == "lockstep" else [(0, 0), (1, 1)]
        for g in stage.giants:
            row = [False] * (stage.inputs * nb)
            for src, mat in feeds:
                for bi, b in enumerate(stage.babies):
                    row[src * nb + bi] = stage.rotated(mat, g, b) is not None
            rows.append(row)
    return rows


def word_counts(pattern, gt):
    """(unfused reads, fused reads, writes) in units of L * N words, for tiles of gt outputs"""
    d = sum(sum(r) for r in pattern)
    used = 0
    for g0 in range(0, len(pattern), gt):
        tile = pattern[g0:g0 + gt]
        used += sum(1 for k in range(len(pattern[0])) if any(r[k] for r in tile))
    return 4 * d, d + 2 * used, 2 * len(pattern)


out = {"tool": "tools/dft_bench.py", "box_clock": time.strftime("%Y-%m-%dT%H:%M:%S%z"), "library_sha16": _build.library_sha16(),
       "source_sha16": _build.source_sha16(), "reps": REPS, "calls_per_window": INNER, "target_waves": TARGET_WAVES, "primitive": [], "transform": []}

# ---- the primitive -----------------------------------------------------------------------------------------------------
for N, bits in ((16384, [60, 40, 40, 40, 40, 60]), (32768, [60] + [40] * 7 + [60])):
    primes = S.CoeffModulus.Create(N, bits)
    L = len(primes) - 1
    e = Engine(N, primes)
    key = bytes(range(32))
    patterns = [(f"dense m={m_} G={g_}", [[True] * m_ for _ in range(g_)])   # (the last four: what the dispatch rule was fitted on)
                for m_, g_ in ((8, 8), (4, 4), (4, 16), (16, 4), (8, 1), (16, 16))]
    for direction in (dft.C2S, dft.S2C):
        plan = dft.plan(N, 3, direction, [primes[L - 1 - i] for i in range(3)])
        for i, st in enumerate(plan.stages):
            patterns.append((f"{direction} levels=3 stage {i} ({st.mode}, {len(st.babies)} babies x {len(st.giants)} giants)", stage_pattern(st)))
    row_words = L * N
    for name, pat in patterns:
        G, m = len(pat), len(pat[0])
        ins = [e.sample("uniform", key, i, 2, L) for i in range(m)]
        # as in a stage, every term has a plaintext of its own
        pts = [[e.sample("uniform", key, 1000 + g * m + k, 1, L).view(0, (L, N)) if pat[g][k] else None for k in range(m)] for g in range(G)]
        fused_out, old_out = e.empty_many(G, (2, L, N)), e.empty_many(G, (2, L, N))
        counts = [sum(r) for r in pat]
        terms_ct = [[ins[k] for k in range(m) if pat[g][k]] for g in range(G)]
        terms_pt = [[pts[g][k] for k in range(m) if pat[g][k]] for g in range(G)]

        def fused():
            e.plain_combine(L, ins, pts, outs=fused_out)

        if len(set(counts)) == 1:
            flat_ct, flat_pt = [c for t in terms_ct for c in t], [p for t in terms_pt for p in t]

            def old():
                e.multiply_plain_sum(L, 2, flat_ct, flat_pt, group=counts[0], outs=old_out)
        else:
            def old():
                for g in range(G):
                    e.multiply_plain_sum(L, 2, terms_ct[g], terms_pt[g], outs=[old_out[g]])

        res = alternate(e, {"plain_combine": fused, "multiply_plain_sum": old})
        for a, b in zip(fused_out, old_out):
            assert (a.download() == b.download()).all(), (N, name)
        ncalls = 1 if len(set(counts)) == 1 else G
        dev = {"plain_combine": device_us(e, fused, 1), "multiply_plain_sum": device_us(e, old, ncalls)}
        gt = tile_width(G, m, L, N)
        unfused_r, fused_r, wr = word_counts(pat, gt)
        t_f, t_o = dev["plain_combine"]["median_us"] * 1e-6, dev["multiply_plain_sum"]["median_us"] * 1e-6
        row = {"N": N, "L": L, "pattern": name, "m": m, "G": G, "terms": sum(counts), "tile": gt,
               "multiply_plain_sum_calls": ncalls, "host": res, "device": dev,
               "evaluator_takes": "multiply_plain_sum" if capi.plain_combine_route(True, m, counts, L * N) == "grouped" else "plain_combine",
               "reads_LN_words": {"multiply_plain_sum": unfused_r, "plain_combine": fused_r}, "writes_LN_words": wr,
               "plain_combine_bytes_per_s": round((fused_r + wr) * row_words * 8 / t_f),
               "plain_combine_share_of_8TBps": round((fused_r + wr) * row_words * 8 / t_f / HBM_PEAK, 4),
               "multiply_plain_sum_bytes_per_s": round((unfused_r + wr) * row_words * 8 / t_o),
               "old_over_fused": round(t_o / t_f, 2), "fused_is_slower": bool(t_f > t_o)}
        out["primitive"].append(row)
        print(row, flush=True)
        del ins, pts, fused_out, old_out, terms_ct, terms_pt
    del e

# a shape at which the fused call loses goes back to multiply_plain_sum in Evaluator.plain_combine (its rule answers in
# "evaluator_takes") and is listed here; a shape listed here that the evaluator still sends to the fused call is a misdispatch
out["shapes_where_the_fused_call_is_slower"] = [(r["N"], r["L"], r["pattern"]) for r in out["primitive"] if r["fused_is_slower"]]
out["misdispatched"] = [(r["N"], r["L"], r["pattern"], r["old_over_fused"]) for r in out["primitive"]
                        if r["fused_is_slower"] != (r["evaluator_takes"] == "multiply_plain_sum")]

# ---- the transform -----------------------------------------------------------------------------------------------------
if "--no-transform" not in args:
    N, bits, levels = 32768, [60] + [40] * 7 + [60], 3
    parms = S.EncryptionParameters("ckks"); parms.set_poly_modulus_degree(N); parms.set_coeff_modulus(S.CoeffModulus.Create(N, bits))
    ctx = S.SEALContext.Create(parms)
    eng = ctx.backend.engine
    top, q = ctx.first_parms_id(), ctx.primes
    plan = dft.plan(N, levels, dft.C2S, [q[top - 1 - i] for i in range(levels)])
    kg = S.KeyGenerator(ctx, 1); enc = S.Encryptor(ctx, kg.public_key(), 2); dec = S.Decryptor(ctx, kg.secret_key())
    encoder, ev = S.CKKSEncoder(ctx), S.Evaluator(ctx)
    gk = kg.galois_keys(plan.galois_steps(), conjugate=True)
    tables = plan.encode(encoder, top)
    rng = np.random.default_rng(1)
    z = np.sqrt(rng.uniform(0, 1, N // 2)) * np.exp(2j * np.pi * rng.uniform(0, 1, N // 2))
    ct = enc.encrypt(encoder.encode(z, 2.0 ** 40))

    class NoFusedSums:
        """the evaluator with Evaluator.plain_combine on its fallback: multiply_plain_sum per output"""
        def __init__(self, ev):
            self._ev = ev
        def __getattr__(self, name):
            return getattr(self._ev, name)
        def plain_combine(self, cts, rows):
            scale = cts[0].scale * next(p for p in rows[0] if p is not None).scale
            L = cts[0].parms_id()
            datas = [self._ev.be.multiply_plain_sum(L, 2, [c.data for c, p in zip(cts, r) if p is not None],
                                                    [p.data for p in r if p is not None])[0] for r in rows]
            return [S.Ciphertext()._set(d, 2, L, scale) for d in datas]

    class AlwaysFused(NoFusedSums):
        """... and with every stage on hefx_plain_combine, whatever the evaluator's dispatch rule says"""
        def plain_combine(self, cts, rows):
            scale = cts[0].scale * next(p for p in rows[0] if p is not None).scale
            L = cts[0].parms_id()
            datas = self._ev.be.plain_combine(L, [c.data for c in cts], [[None if p is None else p.data for p in r] for r in rows])
            return [S.Ciphertext()._set(d, 2, L, scale) for d in datas]

    legs = {"coeffs_to_slots": lambda: alg.coeffs_to_slots(ev, ct, plan, gk, encoded=tables),
            "coeffs_to_slots_always_fused": lambda: alg.coeffs_to_slots(AlwaysFused(ev), ct, plan, gk, encoded=tables),
            "coeffs_to_slots_unfused_sums": lambda: alg.coeffs_to_slots(NoFusedSums(ev), ct, plan, gk, encoded=tables)}
    res = alternate(eng, legs, inner=5, reps=7)
    a, b = legs["coeffs_to_slots"](), legs["coeffs_to_slots_unfused_sums"]()
    same = all((x.data.download() == y.data.download()).all() for x, y in zip(a, b))
    # the real coefficients of z's encoding as CKKSEncoder.encode forms them (an FFT: no dense matrix at this size)
    A = np.zeros(N, dtype=np.complex128)
    A[encoder._r1], A[encoder._r2] = z, np.conj(z)
    coeffs = np.real(np.fft.fft(A) / N * np.conj(encoder._zeta))
    R = dft.bit_reversal(N // 2)
    want = np.concatenate([coeffs[:N // 2][R], coeffs[N // 2:][R]])
    got = np.concatenate([encoder.decode(dec.decrypt(x)) for x in a])
    row = {"N": N, "L": top, "levels": levels, "key_switches": plan.key_switches(), "galois_keys": len(gk.keys),
           "stages": [{"mode": st.mode, "diagonals": len(st.indices), "babies": len(st.babies), "giants": len(st.giants)} for st in plan.stages],
           **res, "same_words_with_and_without_the_fused_sums": bool(same),
           "max_error_over_max_expected": float(np.abs(got - want).max() / np.abs(want).max())}
    out["transform"].append(row)
    print(row, flush=True)

if out_path:
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["timing"] = out
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
