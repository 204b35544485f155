"""The stream contract for the two device entries of include/sea_current_hip_update.h, which the
chains of tests/stream_cases.py do not cover: sc_cost_field_update_batch and sc_cost_field_weighted_update_batch run on the
caller's stream, in order, and only enqueue.

The gate is that of tests/test_gpu_stream_order.py (its Gate, controls and gate length are imported): on a stream S on
which the gate has power, a bounded stretch of GPU work, then copies that bring the inputs of set B (both maps, the
costmaps, the old field, the roots) and fills that poison status and stats, then the call.  The call has to return while
the gate is still running, and g, status and stats have to be the C statement's for B: an operation that left S ran before
B arrived and gives set A's values, poison or garbage."""
import time

import numpy as np
import pytest

from sea_current_amd import synth
from field_twin import Twin, d2_of
from field_w_twin import TwinW
from field_update_twin import TwinU
from test_gpu_stream_order import GATE_MIN_MS, Gate, _control, _dev, _poison, gate_ms

pytestmark = pytest.mark.gpu

W, H = 130, 70


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gate(ctx):
    return Gate()


@pytest.fixture(scope="module")
def stream(ctx, gate, oracle):
    """A stream on which the gate has power (both controls stale); the context is left on it."""
    import torch
    seen = []
    for _ in range(4):
        S = torch.cuda.Stream()
        own, null = _control("own", S, gate, oracle), _control("null", S, gate, oracle)
        seen.append((own, null))
        if own and null:
            ctx.set_stream(S.cuda_stream)
            return S
    pytest.fail(f"the gate has no power on this machine: {seen}")


def _inputs(which, weighted, t0, tw, tu):
    """One frame of set `which`: the maps, the costmaps, the old field, the root; and what the C statement returns."""
    seed = dict(A=71, B=72)[which]
    rects = synth.block_rects(W, H, 0.15, seed=seed, smin=3, smax=12)
    occ0 = synth.raster_rects(rects, W, H)
    occ1 = synth.raster_rects(synth.move_rects(rects, 0, W, H, K=6, step=2, seed=seed), W, H)
    d0, d1 = d2_of(occ0), d2_of(occ1)
    root = int(np.flatnonzero((d0.ravel() >= 1) & (d1.ravel() >= 1))[seed])
    p0 = p1 = None
    if weighted:
        rng = np.random.default_rng(seed)
        p0 = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
        p1 = p0.copy()
        p1[10:40, 30:90] = rng.integers(0, 256, size=(30, 60), dtype=np.uint8)
    g0 = (tw.field(d0, p0, root) if weighted else t0.field(d0, root))[0]
    want = tu.update(d0, d1, g0, root, 0, p0, p1)
    ins = dict(d2_old=d0, d2_new=d1, g=g0[None], roots=np.array([root], np.int32))
    if weighted:
        ins.update(pen_old=p0, pen_new=p1)
    return ins, want


@pytest.mark.parametrize("weighted", [False, True], ids=["sc_cost_field_update_batch", "sc_cost_field_weighted_update_batch"])
def test_update_behind_the_gate(ctx, stream, gate, tmp_path_factory, weighted):
    import torch
    d = tmp_path_factory.mktemp("stream_order_field_update")
    t0, tw, tu = Twin(d), TwinW(d), TwinU(d)
    (a, _), (b, (want_g, want_st, want_stats)) = _inputs("A", weighted, t0, tw, tu), _inputs("B", weighted, t0, tw, tu)
    S = stream
    with torch.cuda.stream(S):
        dev = {k: _dev(v) for k, v in a.items()}
        new = {k: _dev(v) for k, v in b.items()}
        S.synchronize()

        def call():
            return ctx.cost_fields_update(dev["d2_old"], dev["d2_new"], dev["g"], dev["roots"], pen_old=dev.get("pen_old"),
                                          pen_new=dev.get("pen_new"))
        call()                                                # warm: scratch growth; leaves A's results
        S.synchronize()
        dev["g"].copy_(_dev(a["g"]))
        S.synchronize()
        t = time.perf_counter()
        prev = call()                                         # the host time of the call
        t_host = (time.perf_counter() - t) * 1e3
        S.synchronize()
        ctx.synchronize()
        end = gate.enqueue(S, gate_ms(t_host))
        for k in dev:
            dev[k].copy_(new[k])
        _poison(prev["status"])                               # status and stats are the call's own allocations: torch's cache
        _poison(prev["stats"])                                # hands the poisoned blocks back to the next call
        del prev
        out = call()
        pending = not end.query()                             # the moment the call returns
        status, stats = out["status"], out["stats"]
        S.synchronize()
        ctx.synchronize()
        got_g, got_st, got_stats = dev["g"].cpu().numpy()[0], int(status.cpu()[0]), stats.cpu().numpy()[0].tolist()
    assert pending, "the gate had ended when the call returned: the call waited for the stream"
    assert gate_ms(t_host) >= GATE_MIN_MS
    np.testing.assert_array_equal(got_g, want_g)
    assert got_st == want_st and got_stats == want_stats and want_stats[0] > 0
