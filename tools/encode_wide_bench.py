#!/usr/bin/env python3
"""CKKS encode throughput at any scale (a sibling of tools/encode_bench.py).  Prints one JSON object.

    python tools/encode_wide_bench.py --narrow            hefx_ckks_encode at scale 2^40, count 1 / 64 / 512, on
                                                          N = 8192, L = 3 and N = 16384, L = 5 -- nothing but the narrow
                                                          entry, so the same file measures an older commit's tree
    python tools/encode_wide_bench.py --wide              hefx_ckks_encode_wide at scale 2^80 on the same shapes, the host
                                                          path it replaces (CKKSEncoder(device_encode=False)) in the same
                                                          run, hefx_ckks_encode_scalar against the host scalar path
How profiles/encode_wide.json was made: --narrow on this commit and on its parent on one machine, runs alternating,
three each; --wide once."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((8192, [60, 40, 40, 60]), (16384, [60, 40, 40, 40, 40, 60]))
COUNTS = (1, 64, 512)


def context(N, bits):
    from seal_fyp_logistic_regression_amd import seal as S
    parms = S.EncryptionParameters("ckks")
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(S.CoeffModulus.Create(N, bits))
    return S, S.SEALContext.Create(parms)


def rate(e, fn, count, reps=None):
    """vectors per second of fn() (which encodes `count` vectors): two warm-up calls, then three windows of at least a
    quarter of a second each, every one closed by a device synchronise; the median"""
    for _ in range(2):
        fn()
    e.sync()
    reps, rates = reps or 4, []
    while len(rates) < 3:
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        e.sync()
        dt = time.perf_counter() - t0
        if dt < 0.25:  # too short a window measures the clock: lengthen it and start over
            reps, rates = int(reps * max(2.0, 0.3 / max(dt, 1e-6))), []
            continue
        rates.append(reps * count / dt)
    return sorted(rates)[1]


def batch_rates(e, entry, N, L, scale):
    rng = np.random.default_rng(1)
    row = {}
    for count in COUNTS:
        v = rng.uniform(-1, 1, (count, N // 2))
        out = e.empty(count, L, N)
        row[f"batch{count}_vectors_per_s"] = rate(e, lambda: entry(L, v, scale, out=out), count)
    return row


def main():
    res = {}
    for N, bits in SHAPES:
        S, ctx = context(N, bits)
        e, L = ctx.backend.engine, len(bits) - 1
        key = f"N={N},L={L}"
        if "--narrow" in sys.argv[1:]:
            res[key] = {"narrow_2^40": batch_rates(e, e.ckks_encode, N, L, 2.0 ** 40)}
        if "--wide" in sys.argv[1:]:
            dev, host = S.CKKSEncoder(ctx), S.CKKSEncoder(ctx, device_encode=False)
            scale = 2.0 ** 80
            row = {"wide_2^80": batch_rates(e, e.ckks_encode_wide, N, L, scale),
                   "narrow_2^40": batch_rates(e, e.ckks_encode, N, L, 2.0 ** 40)}
            v = np.random.default_rng(2).uniform(-1, 1, N // 2)
            row["CKKSEncoder_2^80_device_vectors_per_s"] = rate(e, lambda: dev.encode(v, scale), 1)
            row["CKKSEncoder_2^80_host_path_vectors_per_s"] = rate(e, lambda: host.encode(v, scale), 1, reps=2)
            row["CKKSEncoder_scalar_2^80_device_per_s"] = rate(e, lambda: dev.encode(0.37, scale), 1)
            row["CKKSEncoder_scalar_2^80_host_path_per_s"] = rate(e, lambda: host.encode(0.37, scale), 1)
            res[key] = row
    from seal_fyp_logistic_regression_amd import _build
    res["source_sha16"] = _build.source_sha16()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
