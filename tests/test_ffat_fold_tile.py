"""LDS-tiled CB window fold (k_ffat_cb_tile) through the public pipeline.

gpu_source -> Ffat_Windows_GPU -> Python sink, with max_keys=5000 (> 4096,
so the wave-per-segment fold is the one selected and, by default, its tiled
kernel).  Every row is compared with a float64 host oracle of the seeded
stream; the old kernel (WFA_CB_FOLD=wave) serves as a second reference.

Sum tolerance (as in test_bench_outputs.py): values lie in [0, 1], so every
intermediate is <= win and each fp32 add/subtract errs by at most
2^-24 * win.  A result takes at most `win` adds for its pane partials plus
2 * (win / pane) running-total updates per earlier window of its key:
    tol = (win + 2 * (win / pane) * max_windows_per_key) * 2^-24 * win
Min, max and count are exact.
"""
import functools
import math
from collections import defaultdict

import numpy as np
import pytest

import windflow_amd as wf
from windflow_amd import native_gpu
from windflow_amd.builders_gpu import (Source_GPU_Builder,
                                       Ffat_Windows_GPU_Builder)
from windflow_amd.synth import gen_batch, bf16_to_f32_np

pytestmark = pytest.mark.gpu

N = 60_000
BATCH = 11_003   # no multiple of any pane: st_fill / st_acc carry over
MAX_KEYS = 5000  # > 4096: not the pane2 path
TILE = 1024      # tuples per LDS tile of the production kernel
SEED = 42
COMBS = {"sum": native_gpu.COMB_SUM, "min": native_gpu.COMB_MIN,
         "max": native_gpu.COMB_MAX, "count": native_gpu.COMB_COUNT}


def _pipeline(n, n_keys, batch, win, slide, comb, vdt, dense,
              max_keys=MAX_KEYS):
    """Rows (key, ts, val) of one run, in arrival order."""
    src = (Source_GPU_Builder(native_gpu.gpu_source(n, n_keys, batch, vdt=vdt,
                                                    seed=SEED))
           .withOutputSchema([vdt]).withOutputBatchSize(batch).build())
    ff = (Ffat_Windows_GPU_Builder(
        native_gpu.gpu_ffat_windows(COMBS[comb], 0, win, slide,
                                    max_keys=max_keys, dense_keys=dense))
          .withOutputSchema([2]).withOutputBatchSize(batch).build())
    rows = []

    def pysink(cols):
        rows.append((cols['key'].astype(np.int64), cols['ts'].astype(np.int64),
                     cols['c0'].astype(np.float32)))

    g = wf.PipeGraph("foldtile")
    p = g.add_source(src)
    p.chain(ff)
    snk = wf.Sink_Builder(pysink).withParallelism(1).build()
    snk.out_schema = [2]
    p.add_sink(snk)
    g.run()
    return tuple(np.concatenate([r[c] for r in rows]) for c in range(3))


@functools.lru_cache(maxsize=None)
def _run(variant, n, n_keys, batch, win, slide, comb, vdt, dense,
         max_keys=MAX_KEYS):
    """Cached run with WFA_CB_FOLD = variant ('' = default).  The operator
    reads the variable when it is constructed."""
    mp = pytest.MonkeyPatch()
    try:
        if variant:
            mp.setenv("WFA_CB_FOLD", variant)
        else:
            mp.delenv("WFA_CB_FOLD", raising=False)
        out = _pipeline(n, n_keys, batch, win, slide, comb, vdt, dense,
                        max_keys)
    finally:
        mp.undo()
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(n, n_keys, win, slide, comb, vdt):
    """float64 oracle: {(key, ts): sorted values}, max windows per key."""
    ts, key, val = gen_batch(n, 0, SEED, n_keys, vdt)
    val = (bf16_to_f32_np(val) if vdt == 5 else val).astype(np.float64)
    f = {"sum": np.sum, "min": np.min, "max": np.max,
         "count": lambda a: float(len(a))}[comb]
    exp = defaultdict(list)
    max_windows = 0
    order = np.argsort(key, kind="stable")
    bounds = np.flatnonzero(np.diff(key[order])) + 1
    for idx in np.split(order, bounds):
        k = int(key[idx[0]])
        vs = val[idx]
        w = 0
        while w * slide + win <= len(idx):      # full windows
            t = int(ts[idx[w * slide + win - 1]])
            exp[(k, t)].append(float(f(vs[w * slide: w * slide + win])))
            w += 1
        while w * slide < len(idx):             # EOS flush: partial tails
            exp[(k, int(ts[idx[-1]]))].append(float(f(vs[w * slide:])))
            w += 1
        max_windows = max(max_windows, w)
    return {kt: sorted(v) for kt, v in exp.items()}, max_windows


def _group(rows):
    key, ts, val = rows
    got = defaultdict(list)
    for k, t, v in zip(key.tolist(), ts.tolist(), val.tolist()):
        got[(k, t)].append(v)
    return {kt: sorted(v) for kt, v in got.items()}


def _tol(win, slide, max_windows):
    pane = math.gcd(win, slide)
    return (win + 2 * (win // pane) * max_windows) * 2.0 ** -24 * win


def _check_vs_oracle(n, n_keys, batch, win, slide, comb="sum", vdt=5,
                     dense=False, variant="", max_keys=MAX_KEYS):
    exp, max_windows = _oracle(n, n_keys, win, slide, comb, vdt)
    got = _group(_run(variant, n, n_keys, batch, win, slide, comb, vdt, dense,
                      max_keys))
    # row count, key and ts: exact (EOS-flush rows share a ts per key, so
    # values are compared as sorted multisets per (key, ts))
    assert sorted(got) == sorted(exp)
    assert {kt: len(v) for kt, v in got.items()} == \
        {kt: len(v) for kt, v in exp.items()}
    tol = _tol(win, slide, max_windows) if comb == "sum" else 0.0
    worst = 0.0
    for kt, ref in exp.items():
        for a, b in zip(got[kt], ref):
            worst = max(worst, abs(a - b))
    print(f"{comb} win={win} slide={slide} keys={n_keys} batch={batch} "
          f"vdt={vdt}: rows {sum(map(len, exp.values()))}, max |err| "
          f"{worst:.3e}, bound {tol:.3e}")
    assert worst <= tol


SHAPES = [(128, 32),    # P=4, S=1, R=8
          (96, 64),     # pane 32, P=3, S=2: every second pane fires
          (100, 100),   # tumbling, P=1
          (1000, 100)]  # the flagship's


@pytest.mark.parametrize("n_keys", [1, 3, 2100])
@pytest.mark.parametrize("win,slide", SHAPES)
def test_tile_fold_vs_oracle(win, slide, n_keys):
    """1 key: one giant segment over many tiles ((96, 64): 343 panes per
    batch against R=8, the ring wraps inside a batch).  3 keys: several
    tiles per segment, tile and pane boundaries drift.  2100 keys: segments
    of ~5 tuples, most batches complete no pane."""
    _check_vs_oracle(N, n_keys, BATCH, win, slide)


@pytest.mark.parametrize("batch", [TILE, TILE + 1])
def test_tile_boundary(batch):
    """One key, segment length == T and == T + 1."""
    _check_vs_oracle(12 * batch + 7, 1, batch, 96, 64)


@pytest.mark.parametrize("vdt", [5, 2])
@pytest.mark.parametrize("comb", ["sum", "min", "max", "count"])
def test_combiners_both_value_paths(comb, vdt):
    """bf16 rides the sort key (vdt 6 in the fold); f32 is gathered through
    idx_sorted (vdt 2)."""
    _check_vs_oracle(N, 3, BATCH, 128, 32, comb=comb, vdt=vdt)


@pytest.mark.parametrize("vdt,dense", [(2, True), (2, False), (5, True)])
def test_flagship_shape_value_paths_dense_and_hashed(vdt, dense):
    _check_vs_oracle(N, 3, BATCH, 1000, 100, vdt=vdt, dense=dense)


@pytest.mark.parametrize("n_keys,win,slide,comb,vdt", [
    (3, 1000, 100, "sum", 5),
    (1, 96, 64, "sum", 5),
    (2100, 128, 32, "sum", 5),
    (3, 128, 32, "sum", 2),
    (3, 128, 32, "min", 5),
    (3, 128, 32, "max", 2),
    (3, 128, 32, "count", 5),
])
def test_tile_matches_wave(n_keys, win, slide, comb, vdt):
    """Old kernel (WFA_CB_FOLD=wave) against the default: same keys and ts;
    min/max/count identical; sums within twice the oracle bound (each side
    may err by the bound)."""
    old = _group(_run("wave", N, n_keys, BATCH, win, slide, comb, vdt, False))
    new = _group(_run("", N, n_keys, BATCH, win, slide, comb, vdt, False))
    assert sorted(old) == sorted(new)
    _, max_windows = _oracle(N, n_keys, win, slide, comb, vdt)
    tol = 2 * _tol(win, slide, max_windows) if comb == "sum" else 0.0
    worst = 0.0
    for kt, ref in old.items():
        assert len(new[kt]) == len(ref), kt
        for a, b in zip(new[kt], ref):
            worst = max(worst, abs(a - b))
    print(f"wave vs tile {comb} win={win} slide={slide} keys={n_keys}: "
          f"max |diff| {worst:.3e}, bound {tol:.3e}")
    assert worst <= tol


@pytest.mark.parametrize("comb", ["sum", "min"])
def test_ring_in_global_memory(comb):
    """win=2048 slide=32: P=64, so R=128 > 64 lanes and the ring stays in
    global memory; min recombines 64 panes per fire."""
    _check_vs_oracle(N, 3, BATCH, 2048, 32, comb=comb)


@pytest.mark.parametrize("variant", [pytest.param("", id="default"), "wave"])
@pytest.mark.parametrize("n_keys,win,slide", [(3, 1000, 100), (700, 128, 32)])
def test_small_max_keys_vs_oracle(variant, n_keys, win, slide):
    """max_keys <= 4096: the default is still the tiled fold; with
    WFA_CB_FOLD=wave the operator selects as it did before the tiled fold
    existed, i.e. the fused two-stage (pane2) fold, which stays covered
    here."""
    _check_vs_oracle(N, n_keys, BATCH, win, slide, variant=variant,
                     max_keys=1024)


@pytest.mark.parametrize("n_keys,win,slide,vdt", [(3, 1000, 100, 5),
                                                  (2100, 128, 32, 2)])
def test_tile_deterministic(n_keys, win, slide, vdt, monkeypatch):
    """Two runs of the default give bit-identical rows.  Hashed slots are
    handed out by atomics, so rows are put in (key, ts, value bits) order
    first; the values themselves must not differ in any bit."""
    monkeypatch.delenv("WFA_CB_FOLD", raising=False)

    def canon(rows):
        key, ts, val = rows
        bits = val.view(np.uint32)
        o = np.lexsort((bits, ts, key))
        return key[o], ts[o], bits[o]

    a = canon(_pipeline(N, n_keys, BATCH, win, slide, "sum", vdt, False))
    b = canon(_pipeline(N, n_keys, BATCH, win, slide, "sum", vdt, False))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
