"""bench.py's plain run on the MI355X: one JSON line with the headline only, --steps really sets the timed steps, and
--dump-outputs writes the same words on every run -- the words the CPU oracle computes for the dumped items."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_is_the_headline_and_its_dumped_outputs_match_the_oracle(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    B = 64
    lines = []
    for d, steps in (("a", 3), ("b", 2)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                            "1", "--batch", str(B), "--dump-outputs", str(tmp_path / d)], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    a, b = lines
    assert a["steps"] == 3 and b["steps"] == 2 and a["warmup"] == 1 and a["full"] is False
    assert a["value"] > 0 and a["ms_per_step"] > 0 and a["higher_is_better"] is True and a["dtype"] == "u64"
    assert a["unit"] == "rotate+multiply_plain ops/s" and a["metric"].startswith("CKKS ciphertext rotate+plain-mult")
    assert 0 < a["roofline"]["frac"] < 1
    for k in ("verified", "sustained", "batch_ladder", "secondary", "variants", "lt_sharded", "composites", "cpu_baseline"):
        assert k not in a, k

    got = np.load(tmp_path / "a" / "rotate_multiply_plain_out.npy")
    items = [int(i) for i in np.load(tmp_path / "a" / "rotate_multiply_plain_items.npy")]
    assert (got == np.load(tmp_path / "b" / "rotate_multiply_plain_out.npy")).all()
    assert items[0] == 0 and items[-1] == B - 1 and len(items) == 16
    words = got[..., 0].astype(np.uint64) + (got[..., 1].astype(np.uint64) << np.uint64(32))

    # the bench's inputs, drawn again from its seeds on the device, through the oracle
    sys.path.insert(0, ROOT)
    import bench
    from oracle import oracle as O
    from seal_fyp_logistic_regression_amd import Engine
    N, primes = bench.SETS["C3"]
    k, L = len(primes), len(primes) - 1
    e = Engine(N, primes, device=0)
    seed = lambda tag: hashlib.sha256(tag).digest()
    ct = e.sample("uniform", seed(b"hefx-bench:ct:0"), 1, 2 * B, L, 0).download().reshape(B, 2, L, N)
    pt = e.sample("uniform", seed(b"hefx-bench:pt:0"), 2, B, L, 0).download().reshape(B, L, N)
    key = e.sample("uniform", seed(b"hefx-bench:key"), 3, 2 * L, k, 0).download().reshape(L, 2, k, N)
    o = O.Oracle(N, primes)
    for j, i in enumerate(items):
        assert (words[j] == o.rotate_mulplain(ct[i], 3, key, pt[i])).all(), i
