"""Every grid entry at the dimension limit of the header (W, H <= SC_MAX_DIM = 8192) against the CPU oracle and the twins: the
chains of tests/limit_cases.py on strips of 8192 x 72, 72 x 8192 and 4100 x 70 cells, A* rounds on the same strips through the
three A* builds, and the space-time planner on strips three cells wide.  A* packs a queue entry as y << 19 | flags | d << 13 | x
(bit 31 is set from y = 4096 on), its duplicate table keeps 13 + 13 bits of a node, the wide matcher 13-bit offsets, and the tile
engines reach their largest tables at 8192 cells: a signed shift, a 12-bit mask or a 16-bit table index passes every other test
of the suite.  tests/test_limit_cases.py holds the conditions under which these comparisons say something."""
import numpy as np
import pytest

import limit_cases as lc
import stream_cases as sc_cases
from test_gpu_stream_order import run_plain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    return sc_cases.Twins(tmp_path_factory.mktemp("limit"))


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_chain_at_the_limit(ctx, twins, case):
    """The chain as test_gpu_stream_order.run_plain runs it: inputs to the device, the calls, one synchronise, the comparison."""
    import torch
    family, shape = case
    chain = lc.chain(family, shape)
    for which in ("A", "B") if shape == lc.SHAPES[0] else ("A",):
        torch.cuda.synchronize()
        run_plain(ctx, None, chain, twins, which)


ASTAR_BUILDS = {"default": {}, "one-wavefront": {"SC_ASTAR_DUAL": "0"}, "throughput": {"SC_ASTAR_LATENCY": "0"}}


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("build", list(ASTAR_BUILDS))
def test_astar_rounds_at_the_limit(oracle, monkeypatch, build, shape):
    import sea_current_amd as sc
    for k, v in ASTAR_BUILDS[build].items():
        monkeypatch.setenv(k, v)                        # read when the context runs its first A*
    c = sc.Context(0)
    try:
        rng = lc.astar_rng(*shape)
        for fam in (0, 1):                              # salt, then walls with gaps
            lc.astar_limit_round(c, oracle, rng, *shape, fam=fam)
    finally:
        c.close()


@pytest.mark.parametrize("shape", lc.TPLAN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tplan_strips(ctx, shape):
    """Reservations and the space-time search on 8192 x 3 and 3 x 8192: sc_fleet_replan_batch (the builder's call), then
    sc_traj_reserve_batch and sc_tplan_batch on their own, word for word."""
    import tplan_twin as tw
    from test_gpu_tplan import _np, _t, _words, gpu, same, same_plan, twin
    c = lc.tplan_case(*shape)
    ref = twin(c)
    same(gpu(ctx, c), ref, c)
    assert ref["res"].any() and (ref["status"] == tw.TP_OK).any()
    res = ctx.traj_reserve(_t(c["knots"]), None, _t(c["radius"]), c["W"], c["H"], c["frame"], c["pad"])
    o = ctx.tplan(_t(c["d2"]), _t(c["start"]), _t(c["goal"]), res=res, t_start=_t(c["t_start"]), hold=True, frame=c["frame"], want_reach=True)
    ctx.synchronize()
    assert np.array_equal(_words(res.cpu().numpy()), tw.pack(ref["res"]))
    same_plan(_np(o), ref, c)


def test_host_forms_on_a_strip(ctx, oracle, twins):
    """The staging helper takes its sizes from W and H: sc_astar_batch_host, sc_cost_field_batch_host and sc_tplan_batch_host on
    8192-long strips."""
    import tplan_twin as tw
    from test_gpu_tplan import same_plan, twin
    W, H = lc.SHAPES[0]
    c = lc.astar_limit_case(oracle, lc.astar_rng(W, H), W, H, fam=0, nthreads=16)
    got, ref = ctx.astar_batch_host(c["d2"], c["start"], c["goal"], r2=c["r2"], Lmax=lc.ASTAR_LMAX), c["ref"]
    for k in ("status", "cost", "len"):
        assert np.array_equal(got[k], ref[k]), k
    for q in np.flatnonzero(ref["status"] == lc.Q_OK):
        assert np.array_equal(got["path"][q, :ref["len"][q]], ref["path"][q, :ref["len"][q]]), q
    fields = lc.chain(lc.Fields, lc.SHAPES[1])
    inp, want = fields.inputs("A"), fields.expected_view("A", twins)
    f = ctx.cost_fields_host(want["d2"], inp["roots"])
    assert np.array_equal(f["g"], want["f_g"]) and np.array_equal(f["status"], want["f_status"])
    t = lc.tplan_case(*lc.TPLAN_SHAPES[0])
    ref = twin(t)
    o = ctx.tplan_host(t["d2"], t["start"], t["goal"], res=tw.pack(ref["res"]), t_start=t["t_start"], hold=True, frame=t["frame"], want_reach=True)
    same_plan(o, ref, t)
