"""Every device entry runs on the caller's stream, in order, and only enqueues (include/sea_current_hip.h, Conventions).

The suite's other tests leave the context on torch's current stream, which is HIP's null stream: there everything in the
process is serialised against everything else, and a launch on the wrong stream, a synchronous copy or a hidden wait
changes nothing.  Here every chain of tests/stream_cases.py runs on a torch.cuda.Stream() S behind a gate: a bounded
stretch of GPU work on S, then copies that bring the inputs (set B) and fills that poison the outputs, then the library
calls.  The last call has to return while the gate is still running (nothing inside waited), and every result has to be
the CPU oracle's / the twins' for B: an operation that left S ran before B arrived and gives the values of the warm run
on set A, poison or garbage.  Two controls that misuse the API on purpose (a context left on its own stream, and on the
null stream) have to come out stale, or the gate sees nothing on this machine and the module fails.
SC_STREAM_ORDER_TIMES=<file> writes the host times and gate lengths of the run (profiles/stream_order_time.json)."""
import json
import os
import time

import numpy as np
import pytest

import stream_cases as cases

pytestmark = pytest.mark.gpu

GATE_MIN_MS, GATE_FACTOR, GATE_CAP_MS = 30.0, 20.0, 1000.0
TIMES = {}


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    return cases.Twins(tmp_path_factory.mktemp("stream_order"))


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()
    if os.environ.get("SC_STREAM_ORDER_TIMES"):
        with open(os.environ["SC_STREAM_ORDER_TIMES"], "w") as f:
            json.dump(TIMES, f, indent=1, sort_keys=True)


class Gate:
    """torch.cuda._sleep for a number of milliseconds, calibrated once with two events."""

    def __init__(self):
        import torch
        torch.cuda._sleep(1_000_000)                         # the first launch loads the kernel
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(20_000_000)
        e1.record()
        torch.cuda.synchronize()
        self.cycles_per_ms = 20_000_000 / e0.elapsed_time(e1)
        TIMES["gate"] = dict(cycles_per_ms=self.cycles_per_ms)

    def enqueue(self, S, ms):
        """The gate on S (the current stream) and the event that marks its end."""
        import torch
        assert torch.cuda.current_stream() == S and ms <= GATE_CAP_MS
        torch.cuda._sleep(int(ms * self.cycles_per_ms))
        end = torch.cuda.Event()
        end.record(S)
        return end


@pytest.fixture(scope="module")
def gate(ctx):
    return Gate()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _control(kind, S, gate, oracle):
    """An EDT on a context that is NOT on S, of a grid whose new content arrives behind the gate on S: True when the result
    is the EDT of the old content (the gate shows an operation off the stream)."""
    import torch
    import sea_current_amd as sc
    occ_a, occ_b = cases._salt_occ(64, 48, 0.1, "A", 90), cases._salt_occ(64, 48, 0.1, "B", 90)
    other = sc.Context(0, use_torch_stream=False)
    try:
        if kind == "null":
            other.set_stream(None)
        with torch.cuda.stream(S):
            occ, new = _dev(occ_a), _dev(occ_b)
            out = torch.full((48, 64), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            end = gate.enqueue(S, GATE_MIN_MS)
            occ.copy_(new)
            other.edt(occ, out=out)                         # misuse on purpose: not ordered behind S
            other.synchronize()
            pending = not end.query()
            S.synchronize()
            got = out.cpu().numpy()
        stale, fresh = np.array_equal(got, oracle.edt(occ_a)), np.array_equal(got, oracle.edt(occ_b))
        return pending and stale and not fresh
    finally:
        other.close()


@pytest.fixture(scope="module")
def stream(ctx, gate, twins):
    """A stream on which the gate has power: the first of four candidates for which both controls come out stale.  The
    context is left on it."""
    import torch
    seen = []
    for _ in range(4):
        S = torch.cuda.Stream()
        own, null = _control("own", S, gate, twins.oracle), _control("null", S, gate, twins.oracle)
        seen.append((own, null))
        if own and null:
            ctx.set_stream(S.cuda_stream)
            TIMES["controls"] = dict(candidates_tried=len(seen), own_stale=True, null_stale=True)
            return S
    pytest.fail(f"the gate has no power on this machine: an EDT off the stream did not come out stale on any of four streams "
                f"(own stream, null stream): {seen}")


def gate_ms(t_host_ms):
    ms = max(GATE_MIN_MS, GATE_FACTOR * t_host_ms)
    assert ms <= GATE_CAP_MS, f"20 x t_host = {GATE_FACTOR * t_host_ms:.0f} ms exceeds the cap: split the chain"
    return ms


def _poison(t):
    t.fill_(float("nan") if t.dtype.is_floating_point else (249 if t.dtype.itemsize == 1 else -7))


def run_gated(ctx, S, gate, chain, tw, sets=("A", "B"), record=None, min_ms=0.0, during=None):
    """The chain on S: warm on sets[0], then behind the gate on sets[1]; returns (pending at return, the results' view, the
    expected view).  during(end): called once the chain is enqueued, while the gate is meant to be still running."""
    import torch
    a, b = chain.inputs(sets[0]), chain.inputs(sets[1])
    if not chain.staged:
        want = chain.expected_view(sets[1], tw)
    with torch.cuda.stream(S):
        d = {k: _dev(v) for k, v in a.items()}
        new = {k: _dev(v) for k, v in b.items()}
        S.synchronize()
        prev = chain.run(ctx, d)                             # warm: scratch growth, one-time uploads; leaves A's results everywhere
        S.synchronize()
        t0 = time.perf_counter()
        again = chain.run(ctx, d, prev)                      # the host time of the calls, with the outputs of the warm run reused
        t_host = (time.perf_counter() - t0) * 1e3
        S.synchronize()
        ctx.synchronize()
        del again                                            # the outputs a call allocates itself come back from torch's cache
        ms = max(gate_ms(t_host), min_ms)
        end = gate.enqueue(S, ms)
        for k in d:
            d[k].copy_(new[k])
        for t in prev.values():
            if t is not None:
                _poison(t)
        out = chain.run(ctx, d, prev)
        pending = not end.query()                            # the moment the last call returns
        got = {k: (None if v is None else v.clone()) for k, v in out.items()}
        if during is not None:
            during(end)
        S.synchronize()
        ctx.synchronize()                                    # SC_OK, and the status block's copy runs on S
        got = {k: (None if v is None else v.cpu().numpy()) for k, v in got.items()}
    if chain.staged:
        want = chain.expected_view(sets[1], tw, up=got)
    if record is not None:
        TIMES[record] = dict(t_host_ms=round(t_host, 3), gate_ms=round(ms, 1))
    return pending, chain.view(got), want


@pytest.mark.parametrize("chain", cases.CHAINS, ids=lambda c: c.name)
def test_chain_behind_the_gate(ctx, stream, gate, twins, chain):
    pending, got, want = run_gated(ctx, stream, gate, chain, twins, record=chain.name)
    assert pending, f"{chain.name}: the gate had ended when the last call returned: a call waited for the stream"
    chain.compare(got, want)


def run_plain(ctx, S, chain, tw, which):
    """The chain on set `which` with no gate, on S (None: the caller has synchronised everything and the context is on a stream
    of its own); compares."""
    import torch
    with torch.cuda.stream(S if S is not None else torch.cuda.current_stream()):
        wait = torch.cuda.synchronize if S is None else S.synchronize      # never the whole device while another stream is gated
        d = {k: _dev(v) for k, v in chain.inputs(which).items()}
        wait()
        out = chain.run(ctx, d)
        ctx.synchronize()
        wait()
        got = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    chain.compare(chain.view(got), chain.expected_view(which, tw, up=got if chain.staged else None))


def _chain(name):
    return next(c for c in cases.CHAINS if c.name.startswith(name))


def test_documented_exceptions_wait_on_the_callers_stream(ctx, stream, gate, twins):
    """sc_astar_last_expansions, sc_astar_debug_stats and sc_astar_gfield say that they synchronise: behind the gate they return
    only once the gate has ended, and with the values of the inputs that arrived behind it -- they wait on the context's
    stream, not on another one."""
    import torch
    o, W, H, Q, Lmax = twins.oracle, 130, 70, 10, 256
    case = _chain("10d")
    a, b = case.inputs("A"), case.inputs("B")
    d2_b = o.edt(b["occ"])
    ref = o.astar_batch(d2_b, b["start"], b["goal"], Lmax=Lmax)
    q0 = int(np.flatnonzero(ref["status"] == 0)[0])
    one = o.astar(d2_b, b["start"][q0], b["goal"][q0], want_g=True)
    with torch.cuda.stream(stream):
        d = {k: _dev(v) for k, v in a.items()}
        new = {k: _dev(v) for k, v in b.items()}
        g, cs = torch.empty((H, W), dtype=torch.int32, device="cuda"), torch.empty(2, dtype=torch.int32, device="cuda")

        def gfield():
            st = ctx._l.sc_astar_gfield(ctx._h, d2.data_ptr(), W, H, 0, int(b["start"][q0]), int(b["goal"][q0]), g.data_ptr(), cs.data_ptr(),
                                        cs.data_ptr() + 4)
            assert st == 0
        reads = dict(last_expansions=ctx.astar_last_expansions, debug_stats=lambda: ctx.astar_debug_stats(Q)[0], gfield=gfield)
        d2 = ctx.edt(d["occ"])
        ctx.astar_batch(d2, d["start"], d["goal"], Lmax=Lmax)
        gfield()
        ctx.synchronize()                                     # warm
        for name, read in reads.items():
            for k in d:
                d[k].copy_(_dev(a[k]))
            ctx.edt(d["occ"], out=d2)                         # what a read that did not wait would find: the values of set A
            ctx.astar_batch(d2, d["start"], d["goal"], Lmax=Lmax)
            gfield()
            ctx.synchronize()
            end = gate.enqueue(stream, GATE_MIN_MS)
            for k in d:
                d[k].copy_(new[k])
            ctx.edt(d["occ"], out=d2)
            ctx.astar_batch(d2, d["start"], d["goal"], Lmax=Lmax)
            value = read()
            assert end.query(), f"{name} returned while the gate was still running: it did not wait for the context's stream"
            if name == "last_expansions":
                assert value == int(ref["expanded"].sum())
            elif name == "debug_stats":
                assert np.array_equal(value, ref["expanded"])
            else:
                stream.synchronize()
                gf, (cost, status) = g.cpu().numpy().view(np.uint32), cs.cpu().tolist()
                assert cost == one["cost"] and status in (0, 3)          # the path itself is not asked for (Lmax = 1): Q_TRUNCATED
                yy, xx = np.divmod(np.arange(W * H), W)
                gx, gy = int(b["goal"][q0]) % W, int(b["goal"][q0]) // W
                dx, dy = np.abs(xx - gx), np.abs(yy - gy)
                h = (10 * np.maximum(dx, dy) + 4 * np.minimum(dx, dy)).reshape(H, W)
                inE = (one["g"] != 0xFFFFFFFF) & (one["g"].astype(np.int64) + h <= one["cost"])   # tests/test_gpu_astar.py: bit-exact on E
                assert np.array_equal(gf[inE], one["g"][inE]) and np.all(gf[~inE] >= one["g"][~inE])
        ctx.synchronize()


def test_host_forms_behind_the_gate(ctx, stream, gate, twins):
    """The _host forms copy in, run, copy back and synchronise on the context's stream: behind the gate they return after it has
    ended, with complete and correct host arrays and nothing further to wait for."""
    import torch
    import scan_twin
    o = twins.oracle
    occ = cases._salt_occ(130, 70, 0.1, "B", 91)
    d2 = o.edt(occ)
    roots = np.flatnonzero(occ.ravel() == 0)[[5, 900]].astype(np.int32)
    rays = scan_twin.square_fan(40, 30, 15)
    hit = twins.scan.cast(occ, rays)
    par = (2, 1, 8, 2, 1)
    forms = dict(
        edt_host=(lambda: ctx.edt_host(occ), lambda got: np.array_equal(got, d2)),
        cost_fields_host=(lambda: ctx.cost_fields_host(d2, roots),
                          lambda got: all(np.array_equal(got["g"][f], twins.field.field(d2, int(r))[0]) for f, r in enumerate(roots))),
        logodds_update_host=(lambda: ctx.logodds_update_host(rays, hit, 130, 70, occ_est=True, known=True),
                             lambda got: all(np.array_equal(x, y) for x, y in zip(got, twins.scan.update(None, rays, hit, 130, 70, *par)))))
    with torch.cuda.stream(stream):
        for name, (call, right) in forms.items():
            call()                                            # warm: the staging buffer grows once
            end = gate.enqueue(stream, GATE_MIN_MS)
            got = call()
            assert end.query(), f"{name} returned while the gate was still running"
            assert right(got), name
        ctx.synchronize()


def test_two_contexts_on_one_host_thread(ctx, stream, gate, twins):
    """Contexts are independent: while context X's chain 5 waits behind a gate on its stream, context Y runs chain 8 on another
    stream to completion with the right results, and X's gate is still pending then; X's results then arrive and are right."""
    import torch
    import sea_current_amd as sc
    x_chain, y_chain = _chain("5"), _chain("8")
    y_chain.expected_view("B", twins)                          # the CPU side first: nothing slow between the gate and the check
    other = sc.Context(0)
    try:
        done, S2 = {}, None
        for _ in range(4):                                    # a stream that does not share the hardware queue of X's stream
            cand = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                end = gate.enqueue(stream, GATE_MIN_MS)
            with torch.cuda.stream(cand):
                probe = torch.zeros(16, device="cuda") + 1
                cand.synchronize()
            free = not end.query()
            stream.synchronize()
            if free:
                S2 = cand
                break
        assert S2 is not None, "no second stream runs beside the gated one on this machine: the test has no power here"

        def during(end):
            other.set_stream(S2.cuda_stream)
            run_plain(other, S2, y_chain, twins, "B")
            done["pending"] = not end.query()

        # warm Y first, so that its scratch exists; its stream is set inside `during`
        other.set_stream(stream.cuda_stream)
        run_plain(other, stream, y_chain, twins, "A")
        pending, got, want = run_gated(ctx, stream, gate, x_chain, twins, min_ms=600.0, during=during)
        assert pending and done["pending"], "context X's gate had ended before context Y finished: the contexts are not independent"
        x_chain.compare(got, want)
    finally:
        other.close()


def test_switching_streams_after_a_synchronise(ctx, stream, twins):
    """set_stream(S1), a chain, synchronize, set_stream(S2), the chain on other inputs, use_own_stream, the chain again: right
    every time, and the scratch of the first run serves the others (the header's rule: synchronise before the switch)."""
    import torch
    chain = _chain("4")
    S2 = torch.cuda.Stream()
    try:
        ctx.set_stream(stream.cuda_stream)
        run_plain(ctx, stream, chain, twins, "A")
        ctx.synchronize()
        scratch = ctx.scratch_bytes()
        ctx.set_stream(S2.cuda_stream)
        run_plain(ctx, S2, chain, twins, "B")
        ctx.synchronize()
        assert ctx.scratch_bytes() == scratch
        ctx.use_own_stream()
        run_plain(ctx, None, chain, twins, "C")
        ctx.synchronize()
        assert ctx.scratch_bytes() == scratch
    finally:
        ctx.synchronize()
        ctx.set_stream(stream.cuda_stream)
