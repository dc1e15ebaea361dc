"""bench.py --dump-outputs: the last timed step's rows, written as .npy.

Both tests run the benchmark itself (that is what they are about) at the
smallest shapes that still cross a step boundary, and compare every dumped
row with a host oracle of the same seeded stream.
"""
import json
import os
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest

from windflow_amd.synth import gen_batch, bf16_to_f32_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(out_dir, *args):
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--dump-outputs", str(out_dir), *args],
        cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    arrs = {f[:-4]: np.load(os.path.join(out_dir, f))
            for f in sorted(os.listdir(out_dir)) if f.endswith(".npy")}
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    for name, a in arrs.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
    return json.loads(lines[0]), arrs


def test_dump_outputs_cpu_config(tmp_path):
    """cpu config (source -> 3v+1 -> drop multiples of 5 -> sink), 4 steps
    of 1000: the dump holds exactly the 4th step's surviving rows."""
    K, B = 4, 1000
    res, arrs = _run_bench(tmp_path, "--config", "cpu", "--steps", str(K),
                           "--warmup", "1", "--batch", str(B))
    assert res["steps"] == K and res["ms_per_step"] > 0
    v = np.arange((K - 1) * B + 1, K * B + 1, dtype=np.int64)
    x = 3 * v + 1
    keep = x % 5 != 0
    # rows are sorted by (key, ts); key = v % 1000, ts = v
    order = np.lexsort((v[keep], v[keep] % 1000))
    assert sorted(arrs) == ["c0", "key", "ts"]
    assert np.array_equal(arrs["ts"], v[keep][order].astype(np.float64))
    assert np.array_equal(arrs["key"], (v[keep] % 1000)[order].astype(np.float64))
    assert np.array_equal(arrs["c0"], x[keep][order].astype(np.float64))


@pytest.mark.gpu
def test_dump_outputs_flagship_vs_oracle(tmp_path):
    """Flagship keyed FFAT pipeline at 4 steps x 100k tuples, 2100 keys
    (max_keys > 4096 and pane >= 32, the kernel selection of the default
    run), win=128 slide=32: every row of the last step — windows completed
    by a tuple of the 4th batch, plus the end-of-stream flush of every open
    window — against a float64 oracle of the seeded stream."""
    K, B, n_keys, win, slide = 4, 100_000, 2100, 128, 32
    res, arrs = _run_bench(tmp_path, "--steps", str(K), "--warmup", "1",
                           "--batch", str(B), "--keys", str(n_keys),
                           "--win", str(win), "--slide", str(slide))
    assert res["steps"] == K and res["ms_per_step"] > 0
    assert res["dtype"] == "bf16" and res["metric"] == "tuples_per_sec"

    ts, key, val = gen_batch(K * B, 0, 42, n_keys, 5)
    val = bf16_to_f32_np(val).astype(np.float64)
    per = defaultdict(list)
    for i, k in enumerate(key.tolist()):
        per[k].append(i)
    exp = []
    max_windows = 0
    for k, idx in per.items():
        vs = val[idx]
        w = 0
        while w * slide + win <= len(idx):      # full windows
            t = idx[w * slide + win - 1]        # ts of the completing tuple
            if t >= (K - 1) * B:
                exp.append((k, t, vs[w * slide: w * slide + win].sum()))
            w += 1
        while w * slide < len(idx):             # EOS flush: partial tails
            exp.append((k, idx[-1], vs[w * slide:].sum()))
            w += 1
        max_windows = max(max_windows, w)
    exp.sort()
    exp_key = np.array([e[0] for e in exp], dtype=np.float64)
    exp_ts = np.array([e[1] for e in exp], dtype=np.float64)
    exp_val = np.array([e[2] for e in exp], dtype=np.float64)

    assert sorted(arrs) == ["c0", "key", "ts"]
    assert arrs["c0"].dtype == np.float32
    assert len(arrs["key"]) == len(exp)
    assert np.array_equal(arrs["key"], exp_key)
    assert np.array_equal(arrs["ts"], exp_ts)
    # fp32 error bound: values lie in [0, 1), so every intermediate is
    # <= win and each fp32 add/subtract errs by at most 2^-24 * win.  A
    # result takes at most `win` adds for its pane partials plus, on the
    # running-total path, 2 * (win / slide) pane updates per earlier window
    # of its key.
    n_ops = win + 2 * (win // slide) * max_windows
    tol = n_ops * 2.0 ** -24 * win
    err = np.abs(arrs["c0"].astype(np.float64) - exp_val)
    print(f"max |err| {err.max():.3e}, bound {tol:.3e}, rows {len(exp)}")
    assert err.max() <= tol
