"""Tuple-granular DETERMINISTIC / PROBABILISTIC collector semantics.

Round 1 ordered whole batches by head timestamp, which is only correct for
ts-contiguous batches.  These tests inject ADVERSARIAL per-tuple
interleavings across source replicas (reference ordering_collector.hpp:51
releases per-tuple total order; kslack_collector.hpp:52 buffers/drops per
tuple) and assert exact order / accounting at the sink.
"""
import random
import threading

import numpy as np
import pytest

import windflow_amd as wf
from windflow_amd import native


def _striped_source(ts_list, batch):
    """Connector-style source emitting fixed (ts, value=ts) rows in batches
    of `batch` — batches are NOT ts-contiguous across sources."""
    state = dict(pos=0)

    def src(replica, par):
        p = state['pos']
        if p >= len(ts_list):
            return None
        chunk = ts_list[p:p + batch]
        state['pos'] += len(chunk)
        t = np.array(chunk, dtype=np.int64)
        return dict(ts=t, key=np.zeros(len(chunk), dtype=np.uint64), c0=t,
                    watermark=int(t.max()))

    return src


def test_ordering_merges_interleaved_tuples_exactly():
    """Two sources stripe even/odd timestamps in 50-row batches; whole-batch
    ordering would emit 0,2,..,98,1,3,..  The tuple-granular merge must
    deliver 0,1,2,3,... exactly."""
    n = 4000
    evens = list(range(0, 2 * n, 2))
    odds = list(range(1, 2 * n, 2))
    seen = []

    def sink(cols):
        seen.extend(cols['ts'].tolist())

    g = wf.PipeGraph("ord", wf.ExecutionMode.DETERMINISTIC,
                     wf.TimePolicy.EVENT_TIME)
    p1 = g.add_source(wf.Source_Builder(_striped_source(evens, 50))
                      .withParallelism(1).withOutputSchema([0])
                      .withOutputBatchSize(50).build())
    p2 = g.add_source(wf.Source_Builder(_striped_source(odds, 50))
                      .withParallelism(1).withOutputSchema([0])
                      .withOutputBatchSize(50).build())
    mp = p1.merge(p2)
    snk = wf.Sink_Builder(sink).withParallelism(1).build()
    snk.out_schema = [0]
    mp.add_sink(snk)
    g.run()
    assert seen == list(range(2 * n))


@pytest.mark.parametrize("seed", [7, 21, 63])
def test_ordering_fuzz_random_interleavings(seed):
    """K sources with random disjoint ts subsets in random batch sizes:
    the DETERMINISTIC sink must observe a globally sorted sequence with the
    exact multiset of rows."""
    rng = random.Random(seed)
    n_src = rng.randint(2, 4)
    n = 3000
    all_ts = list(range(n))
    rng.shuffle(all_ts)
    shards = [sorted(all_ts[i::n_src]) for i in range(n_src)]
    # each shard ts-sorted (per-channel order is the channel sequence), but
    # batch boundaries interleave adversarially across shards
    seen = []

    def sink(cols):
        seen.extend(cols['ts'].tolist())

    g = wf.PipeGraph("ordf", wf.ExecutionMode.DETERMINISTIC,
                     wf.TimePolicy.EVENT_TIME)
    pipes = []
    for s in shards:
        b = rng.choice([1, 13, 50, 200])
        pipes.append(g.add_source(
            wf.Source_Builder(_striped_source(s, b)).withParallelism(1)
            .withOutputSchema([0]).withOutputBatchSize(b).build()))
    mp = pipes[0].merge(*pipes[1:]) if len(pipes) > 1 else pipes[0]
    snk = wf.Sink_Builder(sink).withParallelism(1).build()
    snk.out_schema = [0]
    mp.add_sink(snk)
    g.run()
    assert seen == list(range(n))


def test_ordering_after_keyby_shuffle():
    """DETERMINISTIC order downstream of a keyby shuffle: rows of one source
    scatter across 3 map replicas, then a par=1 sink's ordering collector
    must reassemble the exact global ts order."""
    n, batch = 6000, 64
    seen = []

    def sink(cols):
        seen.extend(cols['ts'].tolist())

    g = wf.PipeGraph("ordk", wf.ExecutionMode.DETERMINISTIC,
                     wf.TimePolicy.EVENT_TIME)
    src = (wf.Source_Builder(native.seq_source(n, 31, batch))
           .withParallelism(1).withOutputSchema([0])
           .withOutputBatchSize(batch).build())
    mp = g.add_source(src)
    mp.add(wf.Map_Builder(native.affine_map(0, 1, 0)).withParallelism(3)
           .withOutputSchema([0]).withOutputBatchSize(batch)
           .withKeyBy(0).build())
    snk = wf.Sink_Builder(sink).withParallelism(1).build()
    snk.out_schema = [0]
    mp.add_sink(snk)
    g.run()
    assert len(seen) == n
    assert seen == sorted(seen)


def test_kslack_tuple_order_and_accounting():
    """PROBABILISTIC mode with bounded per-tuple disorder INSIDE batches:
    the released stream must be globally nondecreasing and every input row
    either delivered or counted dropped (per tuple, not per batch)."""
    rng = random.Random(5)
    n, batch, D = 20000, 100, 40
    ts = list(range(n))
    # bounded shuffle: swap within windows of D
    for i in range(0, n - D, D):
        w = ts[i:i + D]
        rng.shuffle(w)
        ts[i:i + D] = w
    seen = []

    def sink(cols):
        seen.extend(cols['ts'].tolist())

    g = wf.PipeGraph("ks", wf.ExecutionMode.PROBABILISTIC,
                     wf.TimePolicy.EVENT_TIME)
    mp = g.add_source(wf.Source_Builder(_striped_source(ts, batch))
                      .withParallelism(1).withOutputSchema([0])
                      .withOutputBatchSize(batch).build())
    snk = wf.Sink_Builder(sink).withParallelism(1).build()
    snk.out_schema = [0]
    mp.add_sink(snk)
    g.run()
    assert seen == sorted(seen), "released rows must be ts-sorted"
    assert len(seen) + g.getNumDroppedTuples() == n
    # bounded disorder: the adapted slack keeps losses tiny (2D margin:
    # adaptation may lag by one window under scheduler jitter)
    assert g.getNumDroppedTuples() <= 2 * D


def test_kslack_drops_are_per_tuple():
    """One ancient row inside an otherwise-ordered batch: only THAT row is
    dropped (round 1 dropped whole batches)."""
    n, batch = 5000, 100
    late_at = 4000
    ts = list(range(n))
    ts[late_at] = 7  # one ancient timestamp mid-stream
    seen = []
    caught_up = threading.Event()

    def sink(cols):
        seen.extend(cols['ts'].tolist())
        if len(seen) >= late_at:
            caught_up.set()

    # "Ancient" means behind what the collector has already released, so the
    # source holds the batch carrying the late row until the sink has taken
    # every earlier row; a source that outruns the sink thread would
    # otherwise park the whole stream in the slack heap, where ts=7 is
    # simply in order.
    inner = _striped_source(ts, batch)
    emitted = dict(rows=0)

    def paced_source(replica, par):
        if emitted['rows'] == late_at:
            assert caught_up.wait(60), "sink never received the earlier rows"
        out = inner(replica, par)
        if out is not None:
            emitted['rows'] += len(out['ts'])
        return out

    g = wf.PipeGraph("ks1", wf.ExecutionMode.PROBABILISTIC,
                     wf.TimePolicy.EVENT_TIME)
    mp = g.add_source(wf.Source_Builder(paced_source)
                      .withParallelism(1).withOutputSchema([0])
                      .withOutputBatchSize(batch).build())
    snk = wf.Sink_Builder(sink).withParallelism(1).build()
    snk.out_schema = [0]
    mp.add_sink(snk)
    g.run()
    assert g.getNumDroppedTuples() == 1
    assert len(seen) == n - 1
    assert seen == sorted(seen)
