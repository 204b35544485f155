"""The stream contract for the three device entries of include/sea_current_hip_car.h, which the chains of
tests/stream_cases.py do not cover: sc_arc_mask_u16, sc_car_field_batch and sc_car_paths_batch run on the caller's stream, in
order, and only enqueue.

The gate is that of tests/test_gpu_stream_order.py (its Gate, controls and gate length are imported): on a stream S on which
the gate has power, a bounded stretch of GPU work, then copies that bring the inputs of set B (the map, the footprint mask, the
root, the targets), then the three calls as a chain at 130 x 70.  The last call has to return while the gate is still running,
and the mask, the field and the read-outs have to be the C statement's for B: an operation that left S ran before B arrived
and gives set A's values or garbage."""
import time

import numpy as np
import pytest

import car_twin as ct
import pose_twin as pt
from test_gpu_stream_order import GATE_MIN_MS, Gate, _control, _dev, _poison, gate_ms

pytestmark = pytest.mark.gpu

W, H = 130, 70
N, AC, REV = 2, 3, 5


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


def _inputs(which, ref):
    """One frame of set `which`: the map, the footprint mask, the root pose and the targets; and what the C statement returns."""
    seed = dict(A=81, B=82)[which]
    d2 = pt.d2_of(pt.blocks(W, H, seed=seed))
    hm = pt.footprint_mask(d2, 2, 1, 1, 0)
    fit = np.flatnonzero(hm.ravel() == 0xFF)
    root = int(fit[len(fit) // 2])
    targets = pt.free_cells(d2, 24, seed)
    thead = (np.arange(24) % 9 - 1).astype(np.int32)
    am = ref.arc_mask(d2, N, 0, hm)
    gp, st = ref.car_field(d2, root, 0, N, AC, REV, True, 0, hm)
    paths = ref.car_paths(d2, am, gp, root, 0, targets, thead, N, AC, REV, True, 0, hm, 256, True)
    ins = dict(d2=d2, hmask=hm, roots=np.array([root], np.int32), rhead=np.zeros(1, np.int32), qfield=np.zeros(24, np.int32), targets=targets,
               thead=thead)
    return ins, (am, gp, st, paths)


def test_car_chain_behind_the_gate(ctx, stream, gate, tmp_path_factory):
    import torch
    ref = ct.Ref(tmp_path_factory.mktemp("stream_order_car"))
    (a, _), (b, (want_am, want_gp, want_st, want_paths)) = _inputs("A", ref), _inputs("B", ref)
    S = stream
    with torch.cuda.stream(S):
        dev = {k: _dev(v) for k, v in a.items()}
        new = {k: _dev(v) for k, v in b.items()}
        S.synchronize()

        def call():
            am = ctx.arc_mask(dev["d2"], N, hmask=dev["hmask"])
            fld = ctx.car_fields(dev["d2"], am, dev["roots"], dev["rhead"], N, AC, REV, True, hmask=dev["hmask"])
            res = ctx.car_paths(dev["d2"], am, fld["gp"], dev["roots"], dev["rhead"], dev["qfield"], dev["targets"], dev["thead"], N, AC, REV,
                                True, hmask=dev["hmask"], Lmax=256, to_root=True)
            return am, fld, res
        call()                                                # warm: scratch growth; leaves A's results
        S.synchronize()
        t = time.perf_counter()
        prev = call()                                         # the host time of the chain
        t_host = (time.perf_counter() - t) * 1e3
        S.synchronize()
        ctx.synchronize()
        end = gate.enqueue(S, gate_ms(t_host))
        for k in dev:
            dev[k].copy_(new[k])
        for t_ in (prev[0], prev[1]["gp"], prev[1]["status"], *prev[2].values()):   # the outputs are the calls' own allocations:
            _poison(t_)                                                              # torch's cache hands the poisoned blocks back
        del prev
        am, fld, res = call()
        pending = not end.query()                             # the moment the last call returns
        S.synchronize()
        ctx.synchronize()
        got_am, got_gp, got_st = am.cpu().numpy().view(np.uint16), fld["gp"].cpu().numpy()[0], int(fld["status"].cpu()[0])
        got_paths = {k: v.cpu().numpy() for k, v in res.items()}
    assert pending, "the gate had ended when the last call returned: a call waited for the stream"
    assert gate_ms(t_host) >= GATE_MIN_MS
    np.testing.assert_array_equal(got_am, want_am)
    np.testing.assert_array_equal(got_gp, want_gp)
    assert got_st == want_st == 0
    assert ct.same_readout(want_paths, got_paths) and (want_paths["status"] == 0).sum() >= 5
    assert not np.array_equal(want_am, _inputs("A", ref)[1][0])            # the two sets differ, so stale inputs would show
