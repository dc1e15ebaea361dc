#!/usr/bin/env python3
"""windflow_amd flagship benchmark — driver contract.

Headline metric (BASELINE.json): tuples/sec (whole node) on a keyed FFAT
sliding window, count-based win=1000 slide=100, bf16 tuple values with
random keys, synthetic GPU-resident stream.  One rank per GPU; for N>1
the driver launches via torch.distributed.run (RCCL backend).

A "step" = one micro-batch of --batch tuples through the pipeline
(device source -> keyed FFAT window -> sink).  W warmup steps run first
(untimed), then exactly K steps are timed, bracketed by barrier +
torch.cuda.synchronize on both sides; value = whole-job aggregate
tuples/sec (max step time over ranks).

A plain run does only that: set up, warm up, time the K steps, print the
result line.  --full is where secondary measurements belong (none at
present: every other pipeline is a separate, explicit --config run).

--dump-outputs DIR delivers the timed pipeline's results to a host sink
(the rows a caller of the pipeline receives) instead of counting them on
the device, and after the timed steps writes the rows of the LAST step —
those completed by a tuple of the last micro-batch, end-of-stream window
flush included — to DIR/ts.npy, DIR/key.npy and DIR/c<i>.npy (one per
payload column), sorted by (key, ts); a fixed seeded sample of the rows
when they would exceed 64 MB.  The stream is
seeded, so the same arguments give the same rows on every run.  The host
delivery (D2H copy + Python sink) is inside the timed region of such a
run, so its headline value reads lower than a plain run's.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DUMP_MAX_BYTES = 64 << 20   # --dump-outputs budget over all arrays
DUMP_SAMPLE_SEED = 20240229


class OutputCapture:
    """Host sink for --dump-outputs: keeps a copy of the last step's rows
    and drops earlier steps' rows on arrival.  A result row carries the ts
    of the tuple that completed it, so the last step's rows are those with
    ts >= `ts_lo` (the first ts of the last micro-batch), plus every row
    delivered once the watermark has reached `last_wm` (the end-of-stream
    flush of windows whose key saw no tuple in the last step)."""

    def __init__(self, ts_lo, last_wm):
        self.ts_lo = ts_lo
        self.last_wm = last_wm
        self.parts = []

    def __call__(self, cols):
        import numpy as np
        ts = cols["ts"]
        if len(ts) == 0:
            return
        names = ["ts", "key"] + sorted(
            k for k in cols if k[0] == "c" and k[1:].isdigit())
        # the views alias the engine's batch: copy before it is recycled
        if int(cols["watermark"]) >= self.last_wm:
            self.parts.append({k: np.array(cols[k]) for k in names})
            return
        keep = ts >= self.ts_lo
        if keep.any():
            self.parts.append({k: np.asarray(cols[k])[keep] for k in names})

    def write(self, out_dir, suffix=""):
        """Rows sorted by (key, ts) — arrival order across keys is not part
        of a keyed stream's contract — as float64 (ts, key, integer
        columns) / float32 (f32 and bf16 columns); a seeded sample of the
        sorted rows when they exceed DUMP_MAX_BYTES.  Returns
        (rows written, rows captured)."""
        import numpy as np
        from windflow_amd.synth import bf16_to_f32_np
        os.makedirs(out_dir, exist_ok=True)
        names = list(self.parts[0]) if self.parts else ["ts", "key", "c0"]
        arrs = {}
        for k in names:
            a = (np.concatenate([p[k] for p in self.parts]) if self.parts
                 else np.zeros(0))
            if a.dtype == np.uint16:
                a = bf16_to_f32_np(a)
            elif a.dtype != np.float32:
                a = a.astype(np.float64)
            arrs[k] = a
        total = len(arrs["ts"])
        # payload columns break (key, ts) ties, so the order is canonical
        order = np.lexsort([arrs[k] for k in reversed(names)][:-2]
                           + [arrs["ts"], arrs["key"]])
        row_bytes = sum(a.dtype.itemsize for a in arrs.values())
        keep = DUMP_MAX_BYTES // row_bytes
        if total > keep:
            rng = np.random.default_rng(DUMP_SAMPLE_SEED)
            order = order[np.sort(rng.choice(total, keep, replace=False))]
        for k, a in arrs.items():
            np.save(os.path.join(out_dir, f"{k}{suffix}.npy"), a[order])
        return len(order), total


def attach_sink(mp, device, schema, capture):
    """Terminate a GPU pipeline: the device-side count sink of a plain run,
    or the host capture sink (behind the engine's D2H stage) when dumping."""
    import windflow_amd as wf
    from windflow_amd import native_gpu
    from windflow_amd.builders_gpu import Sink_GPU_Builder
    if capture is None:
        snk = (Sink_GPU_Builder(native_gpu.gpu_count_sink())
               .withDevice(device).build())
        mp.chain_sink(snk)
    else:
        snk = wf.Sink_Builder(capture).withParallelism(1).build()
        snk.out_schema = schema
        mp.add_sink(snk)
    return snk


def build_ffat_graph(n_tuples, batch, n_keys, win, slide, rank, world, device,
                     dense=True, capture=None):
    import windflow_amd as wf
    from windflow_amd import native_gpu
    from windflow_amd.builders_gpu import (Source_GPU_Builder,
                                           Ffat_Windows_GPU_Builder)
    src = (Source_GPU_Builder(
        native_gpu.gpu_source(n_tuples, n_keys, batch, vdt=5, seed=42 + rank))
        .withOutputSchema([5]).withOutputBatchSize(batch)
        .withDevice(device).build())
    # keys are random-ORDER but dense-VALUED integers in [0, n_keys): the
    # withDenseKeys declaration (slot = key, no hash probe) is the honest
    # MI355X-first choice for this stream; --no-dense-keys measures the
    # general hashed path (both recorded in BASELINE.md)
    ff = (Ffat_Windows_GPU_Builder(
        native_gpu.gpu_ffat_windows(native_gpu.COMB_SUM, 0, win, slide,
                                    max_keys=2 * n_keys, dense_keys=dense))
        .withOutputSchema([2]).withOutputBatchSize(batch)
        .withDevice(device).build())
    g = wf.PipeGraph("bench_ffat")
    mp = g.add_source(src)
    mp.chain(ff)
    snk = attach_sink(mp, device, [2], capture)
    return g, snk


def build_a2a_graph(n_tuples, batch, n_keys, rank, world, device, dist_cfg,
                    dense=True, capture=None):
    """Driver config #4: Map_GPU -> RCCL keyby all-to-all -> Reduce_GPU,
    one rank per GPU."""
    import windflow_amd as wf
    from windflow_amd import native_gpu
    from windflow_amd.builders_gpu import (Source_GPU_Builder, Map_GPU_Builder,
                                           KeyBy_Exchange_GPU_Builder,
                                           Reduce_GPU_Builder)
    src = (Source_GPU_Builder(
        native_gpu.gpu_source(n_tuples, n_keys, batch, vdt=2, seed=42 + rank))
        .withOutputSchema([2]).withOutputBatchSize(batch)
        .withDevice(device).build())
    mp_ = (Map_GPU_Builder(native_gpu.gpu_affine_map(0, 2.0, 0.5, dtype=2))
           .withOutputSchema([2]).withOutputBatchSize(batch)
           .withDevice(device).build())
    ex = (KeyBy_Exchange_GPU_Builder(native_gpu.gpu_keyby_exchange())
          .withOutputSchema([2]).withOutputBatchSize(3 * batch)
          .withDevice(device).build())
    rd = (Reduce_GPU_Builder(
        native_gpu.gpu_keyed_reduce(native_gpu.COMB_SUM, 0, 4 * n_keys,
                                    dense_keys=dense))
        .withOutputSchema([2]).withOutputBatchSize(3 * batch)
        .withDevice(device).build())
    g = wf.PipeGraph("bench_a2a")
    g.set_dist(*dist_cfg)
    mp = g.add_source(src)
    mp.chain(mp_)
    mp.chain(ex)
    mp.chain(rd)
    snk = attach_sink(mp, device, [2], capture)
    return g, snk


def build_ffat_x_graph(n_tuples, batch, n_keys, win, slide, rank, world, device,
                       dist_cfg, dense=True, capture=None):
    """Keyed FFAT with a true cross-GPU keyby: source -> RCCL all-to-allv
    exchange -> FFAT window.  Every key's window state lives on exactly one
    rank (hash(key) % world)."""
    import windflow_amd as wf
    from windflow_amd import native_gpu
    from windflow_amd.builders_gpu import (Source_GPU_Builder,
                                           KeyBy_Exchange_GPU_Builder,
                                           Ffat_Windows_GPU_Builder)
    src = (Source_GPU_Builder(
        native_gpu.gpu_source(n_tuples, n_keys, batch, vdt=5, seed=42 + rank))
        .withOutputSchema([5]).withOutputBatchSize(batch)
        .withDevice(device).build())
    ex = (KeyBy_Exchange_GPU_Builder(native_gpu.gpu_keyby_exchange())
          .withOutputSchema([5]).withOutputBatchSize(3 * batch)
          .withDevice(device).build())
    ff = (Ffat_Windows_GPU_Builder(
        native_gpu.gpu_ffat_windows(native_gpu.COMB_SUM, 0, win, slide,
                                    max_keys=2 * n_keys, dense_keys=dense))
        .withOutputSchema([2]).withOutputBatchSize(3 * batch)
        .withDevice(device).build())
    g = wf.PipeGraph("bench_ffat_x")
    g.set_dist(*dist_cfg)
    mp = g.add_source(src)
    mp.chain(ex)
    mp.chain(ff)
    snk = attach_sink(mp, device, [2], capture)
    return g, snk


def build_mapfilter_graph(n_tuples, batch, n_keys, rank, world, device,
                          capture=None):
    """Driver config #2: Map_GPU + Filter_GPU chained, bf16 tuples."""
    import windflow_amd as wf
    from windflow_amd import native_gpu
    from windflow_amd.builders_gpu import (Source_GPU_Builder, Map_GPU_Builder,
                                           Filter_GPU_Builder)
    src = (Source_GPU_Builder(
        native_gpu.gpu_source(n_tuples, n_keys, batch, vdt=5, seed=42 + rank))
        .withOutputSchema([5]).withOutputBatchSize(batch)
        .withDevice(device).build())
    mp_ = (Map_GPU_Builder(native_gpu.gpu_affine_map(0, 1.5, 0.25, dtype=5))
           .withOutputSchema([5]).withOutputBatchSize(batch)
           .withDevice(device).build())
    fl = (Filter_GPU_Builder(native_gpu.gpu_gt_filter(0, 0.5, dtype=5))
          .withOutputSchema([5]).withOutputBatchSize(batch)
          .withDevice(device).build())
    g = wf.PipeGraph("bench_mapfilter")
    mp = g.add_source(src)
    mp.chain(mp_)
    mp.chain(fl)
    snk = attach_sink(mp, device, [5], capture)
    return g, snk


def cpu_sink(capture, schema):
    """native count sink, or the host capture sink when dumping"""
    import windflow_amd as wf
    from windflow_amd import native
    if capture is None:
        return wf.Sink_Builder(native.count_sink()).withParallelism(1).build()
    snk = wf.Sink_Builder(capture).withParallelism(1).build()
    snk.out_schema = schema
    return snk


def build_join_graph(n_tuples, batch, n_keys, par, capture=None):
    """Driver config #5 shape (CPU side): two keyed sources -> interval
    join (KP) -> paned windows -> sink, watermark collectors throughout."""
    import windflow_amd as wf
    from windflow_amd import native
    from windflow_amd.builders import (Interval_Join_Builder,
                                       Paned_Windows_Builder)
    g = wf.PipeGraph("bench_join")
    sa = (wf.Source_Builder(native.seq_source(n_tuples, n_keys, batch))
          .withParallelism(1).withOutputSchema([0])
          .withOutputBatchSize(batch).build())
    # B's offset must be a multiple of n_keys: key = v % n_keys, so a
    # misaligned offset shifts every B key off A's and the join matches
    # NOTHING (round-2 validity fix — the join was running empty)
    off_b = (1_000_000_000 // n_keys) * n_keys
    sb = (wf.Source_Builder(native.seq_source(n_tuples, n_keys, batch,
                                              value_offset=off_b))
          .withParallelism(1).withOutputSchema([0])
          .withOutputBatchSize(batch).build())
    mpA = g.add_source(sa)
    mpB = g.add_source(sb)
    mp = mpA.merge(mpB)
    mp.add(Interval_Join_Builder().withBoundaries(-2, 2).withKPMode()
           .withValueCols(0).withParallelism(par)
           .withOutputSchema([0, 0]).withOutputBatchSize(batch).build())
    mp.add(Paned_Windows_Builder(plq_func=("sum", 0))
           .withTBWindows(1000, 100).withParallelism(par)
           .withOutputSchema([0]).withOutputBatchSize(batch).build())
    snk = cpu_sink(capture, [0])
    mp.add_sink(snk)
    return g, snk


def build_cpu_graph(n_tuples, batch, par=1, capture=None):
    """Config #1: Source -> Map -> Filter -> Sink.  par=1 chains all four
    into ONE thread (round-1 shape); par>1 runs `par` source replicas
    each chained with its own map+filter+sink replica (rebalanced
    stream shards, zero cross-thread shuffles — operator replication,
    SURVEY §2.10)."""
    import windflow_amd as wf
    from windflow_amd import native
    g = wf.PipeGraph("bench_cpu")
    per = n_tuples // par
    pipes = []
    snks = []
    for r in range(par):
        src = (wf.Source_Builder(native.seq_source(per, 1000, batch,
                                                   value_offset=r * per))
               .withParallelism(1).withOutputSchema([0])
               .withOutputBatchSize(batch).build())
        mp = g.add_source(src)
        mp.chain(wf.Map_Builder(native.affine_map(0, 3, 1)).withParallelism(1)
                 .withOutputSchema([0]).withOutputBatchSize(batch).build())
        mp.chain(wf.Filter_Builder(native.mod_filter(0, 5, 0)).withParallelism(1)
                 .withOutputSchema([0]).withOutputBatchSize(batch).build())
        snk = cpu_sink(capture, [0])
        mp.chain_sink(snk)
        snks.append(snk)
        pipes.append(mp)
    return g, snks[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults sized so the driver's own record carries a sustained claim
    # (~1.7 B tuples, ~100 ms timed region) while finishing in seconds
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    # default micro-batch = measured throughput plateau (BASELINE.md sweep:
    # 16.2 B t/s @4M, 19.8 @8M, 19.8 @16M; p99 2.2 ms at 8M)
    ap.add_argument("--batch", type=int, default=16_777_216)
    ap.add_argument("--keys", type=int, default=8192,
                    help="distinct keys per rank")
    ap.add_argument("--par", type=int, default=1,
                    help="CPU configs: operator parallelism")
    ap.add_argument("--no-dense-keys", action="store_true",
                    help="ffat config: use the hashed key->slot path even "
                         "though the synthetic keys are dense integers")
    ap.add_argument("--win", type=int, default=1000)
    ap.add_argument("--slide", type=int, default=100)
    ap.add_argument("--config", choices=["ffat", "ffat_x", "a2a", "mapfilter", "cpu", "join"], default="ffat")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements and checks "
                         "(none at present: a plain run already measures "
                         "only the headline figure, and every other "
                         "pipeline is its own --config run)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="deliver the timed pipeline's results to a host "
                         "sink and write the last step's rows to "
                         "DIR/<ts|key|c0...>.npy (float32/float64, at most "
                         "64 MB, sorted by key then ts); the host delivery "
                         "is inside the timed region of such a run")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    dist = None
    torch = None
    dist_cfg = None
    if args.config not in ("cpu", "join"):
        import torch  # noqa: F811
        if world > 1:
            import torch.distributed as dist  # noqa: F811
            # gloo for the out-of-band bootstrap (rccl id broadcast +
            # barriers): torch's own nccl group would refuse multiple ranks
            # per device, but the ENGINE's RCCL communicator is the thing
            # under test; device collectives all run through it.
            backend = os.environ.get("WFA_DIST_BACKEND", "gloo")
            dist.init_process_group(backend, rank=rank, world_size=world)
            torch.cuda.set_device(local_rank)
        if args.config in ("a2a", "ffat_x"):
            if world > 1:
                from windflow_amd.dist import init_from_torch
                dist_cfg = init_from_torch()
            else:
                from windflow_amd import _core
                dist_cfg = (0, 1, _core.rccl_unique_id())

    def sync():
        if torch is not None and torch.cuda.is_available():
            torch.cuda.synchronize()

    def barrier():
        if dist is not None:
            dist.barrier()

    K, W, B = args.steps, args.warmup, args.batch
    p99_us = None
    capture = None

    if args.config in ("cpu", "join"):
        B = min(B, 65536)
        build = ((lambda n, b, c=None: build_cpu_graph(n, b, args.par, c))
                 if args.config == "cpu"
                 else lambda n, b, c=None: build_join_graph(
                     n, b, args.keys, args.par if args.par > 1 else 4, c))
        gw, _ = build(W * B, B)
        gw.run()
        if args.dump_outputs:
            # sequence sources stamp ts = 1..n; the cpu config splits the
            # stream over --par source shards.  Rows are picked by ts alone:
            # how far the watermark has got when a row arrives depends on
            # thread timing in these multi-threaded graphs.
            shards = args.par if args.config == "cpu" else 1
            capture = OutputCapture(K * B // shards - B + 1, float("inf"))
        g, snk = build(K * B, B, capture)
        t0 = time.time()
        g.run()
        dt = time.time() - t0
        n_gpus = 0
        lat = sorted(g.engine.sink_latencies(g._sink_map[id(snk)]))
        p99_us = lat[min(len(lat) - 1, int(0.99 * len(lat)))] if lat else None
    else:
        def builder(steps, capture=None):
            if args.config == "mapfilter":
                return build_mapfilter_graph(steps * B, B, args.keys, rank,
                                             world, local_rank,
                                             capture=capture)
            if args.config == "a2a":
                return build_a2a_graph(steps * B, B, args.keys, rank, world,
                                       local_rank, dist_cfg,
                                       dense=not args.no_dense_keys,
                                       capture=capture)
            if args.config == "ffat_x":
                return build_ffat_x_graph(steps * B, B, args.keys, args.win,
                                          args.slide, rank, world, local_rank,
                                          dist_cfg,
                                          dense=not args.no_dense_keys,
                                          capture=capture)
            return build_ffat_graph(steps * B, B, args.keys, args.win,
                                    args.slide, rank, world, local_rank,
                                    dense=not args.no_dense_keys,
                                    capture=capture)
        # warmup engine (also JIT-warms pools/streams/arena)
        if W > 0:
            gw, _ = builder(W)
            gw.run()
        if args.dump_outputs:
            # the device source stamps ts = 0..n-1 and watermark = last ts
            capture = OutputCapture((K - 1) * B, K * B - 1)
        g, snk = builder(K, capture)
        g.prepare()   # threads spawned + streams/pools warm, gated
        sync()
        barrier()
        t0 = time.time()
        g.run_gated()
        sync()
        t1 = time.time()
        barrier()
        dt = t1 - t0
        n_gpus = world
        lat = sorted(g.engine.sink_latencies(g._sink_map[id(snk)]))
        p99_us = lat[min(len(lat) - 1, int(0.99 * len(lat)))] if lat else None

    # max step time over ranks (tensor device must match the backend)
    if dist is not None:
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())

    if capture is not None:
        # one set of files per rank (each rank owns its keys' results)
        wrote, got = capture.write(args.dump_outputs,
                                   f".rank{rank}" if rank else "")
        print(f"[bench] rank {rank}: wrote {wrote} of the last step's {got} "
              f"rows to {args.dump_outputs}", file=sys.stderr)

    total_tuples = K * B * max(world, 1)
    value = total_tuples / dt
    if rank == 0:
        out = {
            "metric": "tuples_per_sec",
            "value": value,
            "unit": "tuples/s",
            "n_gpus": 0 if args.config in ("cpu", "join") else n_gpus,
            "steps": K,
            "warmup": W,
            "ms_per_step": dt / K * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": {"ffat": "bf16", "ffat_x": "bf16", "a2a": "f32",
                      "mapfilter": "bf16", "cpu": "int64",
                      "join": "int64"}[args.config],
            "data": "synthetic",
            "config": {
                "model": {"ffat": "keyed_ffat_cb_window",
                          "ffat_x": "rccl_keyby_ffat_cb_window",
                          "a2a": "map_gpu_rccl_keyby_reduce_gpu",
                          "mapfilter": "map_gpu_filter_gpu_chained",
                          "cpu": "cpu_source_map_filter_sink",
                          "join": "interval_join_paned_windows_cpu"}[args.config],
                "global_batch": B * max(world, 1),
                "win": args.win,
                "slide": args.slide,
                "keys_per_rank": args.keys,
                "parallelism": f"keyed-dp{max(world,1)}",
                "p99_batch_latency_us": p99_us,
                "dense_keys": (args.config in ("ffat", "ffat_x", "a2a")
                               and not args.no_dense_keys),
            },
        }
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
