"""sc_field_cost_matrix / sc_assign_batch / sc_fleet_assign_batch (Context.field_cost_matrix, assign, fleet_assign) on the GPU:
every output, steps included, equal to the NumPy twin (tests/assign_twin.py) on shapes that straddle the three kernel builds and
the transpose; the certificate on the GPU's own output; batches with more problems than compute units and a bad problem in the
middle; buffers, the _host forms and argument errors; the matrix against NumPy indexing of the fields; and the chain
cost_fields -> fleet_assign -> field_paths against astar_batch."""
import ctypes

import numpy as np
import pytest

import assign_twin as tw

pytestmark = pytest.mark.gpu

KEYS = ("col_of", "row_of", "u", "v", "info")
SHAPES = [(1, 1), (1, 5), (5, 1), (3, 3), (17, 64), (64, 17), (63, 63), (64, 64), (64, 65), (65, 64), (65, 65), (255, 256), (256, 256),
          (256, 300), (300, 256), (257, 257), (7, 1024), (1024, 7), (1023, 1024), (1024, 1000), (1024, 1024)]


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _gpu(ctx, cost):
    o = ctx.assign(_t(cost))
    ctx.synchronize()
    return _np(o)


def _same(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if not np.array_equal(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError(f"{k}: {len(bad)} differ, first at {bad[0].tolist()}: gpu {got[k][tuple(bad[0])]} twin {want[k][tuple(bad[0])]}")


def _check(ctx, cost):
    """cost [B][R][C]: equal to the twin, and the certificate on what the GPU returned."""
    got = _gpu(ctx, cost)
    _same(got, tw.assign(cost))
    for b in range(cost.shape[0]):
        if got["info"][b, 3] == tw.OK:
            tw.certificate(cost[b], {k: got[k][b] for k in KEYS})
    return got


@pytest.mark.parametrize("kind", ["full", "octile"])
@pytest.mark.parametrize("R,C", SHAPES)
def test_every_shape(ctx, R, C, kind):
    _check(ctx, tw.random_cost(np.random.default_rng(R * 2048 + C), R, C, kind)[None])


@pytest.mark.parametrize("R,C", [s for s in SHAPES if max(s) <= 257])
def test_every_step_a_tie(ctx, R, C):
    _check(ctx, tw.random_cost(np.random.default_rng(R * 2048 + C + 1), R, C, "tie")[None])


@pytest.mark.parametrize("fb", [0.0, 0.1, 0.5, 0.9, 1.0])
@pytest.mark.parametrize("R,C", [(5, 1), (17, 64), (65, 64), (256, 300), (300, 256)])
def test_forbidden_fractions(ctx, R, C, fb):
    rng = np.random.default_rng(int(fb * 10) + R)
    got = _check(ctx, np.stack([tw.random_cost(rng, R, C, kind, fb) for kind in ("small", "octile", "full")]))
    if fb == 1.0:
        assert not got["info"][:, :2].any() and (got["col_of"] == -1).all()


@pytest.mark.parametrize("R,C", [(64, 64), (64, 65), (300, 256)])
def test_forbidden_row_and_column(ctx, R, C):
    cost = tw.random_cost(np.random.default_rng(R + C), R, C, "octile")[None].repeat(2, 0)
    cost[0, R // 3, :] = tw.INF
    cost[1, :, C // 3] = tw.INF
    got = _check(ctx, cost)
    assert got["col_of"][0, R // 3] == -1 and got["row_of"][1, C // 3] == -1


def test_batch_of_two_across_builds(ctx):
    for R, C in ((40, 64), (200, 100), (300, 700)):
        _check(ctx, np.stack([tw.random_cost(np.random.default_rng(k), R, C, "small", 0.05 * k) for k in range(2)]))


@pytest.mark.parametrize("n", [16, 64])
def test_more_problems_than_compute_units(ctx, n):
    rng = np.random.default_rng(n)
    cost = np.stack([tw.random_cost(rng, n, n, ("tie", "small", "octile", "full")[b % 4], (0.0, 0.3)[b % 2]) for b in range(300)])
    _check(ctx, cost)


@pytest.mark.parametrize("R,C", [(16, 16), (100, 80), (300, 300)])
def test_bad_problem_in_the_middle(ctx, R, C):
    cost = tw.random_cost(np.random.default_rng(9), R, C, "small")[None].repeat(3, 0)
    cost[1, R - 1, C - 1] = -1
    got = _check(ctx, cost)
    assert got["info"][:, 3].tolist() == [tw.OK, tw.BAD, tw.OK] and got["info"][1].tolist() == [0, 0, 0, tw.BAD]
    assert (got["col_of"][1] == -1).all() and (got["row_of"][1] == -1).all() and not got["u"][1].any() and not got["v"][1].any()
    for k in KEYS:
        assert np.array_equal(got[k][0], got[k][2])


def test_ij_1024_by_certificate(ctx):
    """The longest kernel of the suite: i * j at 1024 x 1024 takes the full n (n + 1) / 2 steps."""
    i, j = np.mgrid[0:1024, 0:1024]
    cost = (i * j).astype(np.int32)
    got = _gpu(ctx, cost)
    assert got["info"].tolist() == [1024, 178433024, 524800, tw.OK]
    tw.certificate(cost, got)


def _raw(ctx, name, cost, B, R, C, col_of, row_of, u, v, info):
    p = lambda a: None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    return getattr(ctx._l, name)(ctx._h, p(cost), B, R, C, p(col_of), p(row_of), p(u), p(v), p(info))


def test_prefilled_buffers_null_outputs_and_the_empty_batch(ctx):
    import torch
    cost = tw.random_cost(np.random.default_rng(1), 70, 33, "octile", 0.3)[None].repeat(2, 0)
    cost[1] = cost[1, ::-1]
    want = tw.assign(cost)
    d = _t(cost)
    full = lambda shape, dt: torch.full(shape, 0x5a5a5a5a, dtype=dt, device="cuda")
    o = dict(col_of=full((2, 70), torch.int32), row_of=full((2, 33), torch.int32), u=full((2, 70), torch.int64), v=full((2, 33), torch.int64),
             info=full((2, 4), torch.int64))
    assert _raw(ctx, "sc_assign_batch", d, 2, 70, 33, *(o[k] for k in KEYS)) == 0
    ctx.synchronize()
    _same(_np(o), want)
    o2 = dict(col_of=full((2, 70), torch.int32), info=full((2, 4), torch.int64))
    assert _raw(ctx, "sc_assign_batch", d, 2, 70, 33, o2["col_of"], None, None, None, o2["info"]) == 0
    ctx.synchronize()
    assert np.array_equal(o2["col_of"].cpu().numpy(), want["col_of"]) and np.array_equal(o2["info"].cpu().numpy(), want["info"])
    assert _raw(ctx, "sc_assign_batch", d, 0, 70, 33, o2["col_of"], None, None, None, o2["info"]) == 0      # B == 0: a no-op
    ctx.synchronize()
    assert np.array_equal(o2["info"].cpu().numpy(), want["info"])


def test_argument_errors(ctx):
    import torch
    d = _t(np.zeros((1, 4, 4), np.int32))
    co, info = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    for name in ("sc_assign_batch", "sc_assign_batch_host"):
        assert _raw(ctx, name, None, 1, 4, 4, co, None, None, None, info) == 1
        assert _raw(ctx, name, d, 1, 4, 4, None, None, None, None, info) == 1
        assert _raw(ctx, name, d, 1, 4, 4, co, None, None, None, None) == 1
        for R, C in ((0, 4), (4, 0), (1025, 4), (4, 1025), (-1, 4)):
            assert _raw(ctx, name, d, 1, R, C, co, None, None, None, info) == 1
        assert _raw(ctx, name, d, -1, 4, 4, co, None, None, None, info) == 1
    g = torch.zeros((2, 3, 4), dtype=torch.int32, device="cuda")
    cells = torch.zeros(5, dtype=torch.int32, device="cuda")
    out = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    L, h = ctx._l, ctx._h
    assert L.sc_field_cost_matrix(h, None, 2, 4, 3, cells.data_ptr(), 5, None, out.data_ptr()) == 1
    assert L.sc_field_cost_matrix(h, g.data_ptr(), 2, 4, 3, None, 5, None, out.data_ptr()) == 1
    assert L.sc_field_cost_matrix(h, g.data_ptr(), 2, 4, 3, cells.data_ptr(), 5, None, None) == 1
    assert L.sc_field_cost_matrix(h, g.data_ptr(), 0, 4, 3, cells.data_ptr(), 5, None, out.data_ptr()) == 1
    assert L.sc_field_cost_matrix(h, g.data_ptr(), 2, 0, 3, cells.data_ptr(), 5, None, out.data_ptr()) == 1
    assert L.sc_field_cost_matrix(h, g.data_ptr(), 2, 4, 3, cells.data_ptr(), 0, None, out.data_ptr()) == 1
    fleet = lambda F, R, col_of, info_: L.sc_fleet_assign_batch(h, g.data_ptr(), F, 4, 3, cells.data_ptr(), R, None, None, col_of, None, None, None, info_)
    assert fleet(2, 5, None, info.data_ptr()) == 1 and fleet(2, 5, co.data_ptr(), None) == 1
    assert fleet(1025, 5, co.data_ptr(), info.data_ptr()) == 1 and fleet(2, 1025, co.data_ptr(), info.data_ptr()) == 1


def test_host_forms(ctx):
    import sea_current_amd as sc
    rng = np.random.default_rng(6)
    for shape in ((3, 20, 64), (2, 300, 90)):
        cost = np.stack([tw.random_cost(rng, shape[1], shape[2], "octile", 0.2) for _ in range(shape[0])])
        cost[0, 0, 0] = -3
        _same(ctx.assign_host(cost), tw.assign(cost))
    one = ctx.assign_host(cost[1])
    assert one["col_of"].shape == (300,) and np.array_equal(one["col_of"], tw.assign_one(cost[1])["col_of"])
    g = rng.integers(0, 10**6, (6, 9, 13)).astype(np.int32)
    g[rng.random(g.shape) < 0.3] = tw.INF
    cells = rng.integers(-2, 9 * 13 + 2, 11).astype(np.int32)
    cc = rng.integers(0, tw.SEED_COST_MAX + 1, 6).astype(np.int32)
    for col_cost in (None, cc):
        m = tw.field_cost_matrix(g, cells, col_cost)
        assert np.array_equal(ctx.field_cost_matrix_host(g, cells, col_cost), m)
        o = ctx.fleet_assign_host(g, cells, col_cost, want_cost=True)
        assert np.array_equal(o.pop("cost"), m)
        _same({k: v[None] for k, v in o.items()}, tw.assign(m))
        _same({k: v[None] for k, v in ctx.fleet_assign_host(g, cells, col_cost).items()}, tw.assign(m))
    # refusals: a field value below 0, a column cost outside its range
    neg = g.copy()
    neg[5, 8, 12] = -1
    for bad_g, bad_cc in ((neg, cc), (g, np.where(np.arange(6) == 2, -1, cc)), (g, np.where(np.arange(6) == 5, tw.SEED_COST_MAX + 1, cc))):
        with pytest.raises(sc.SeaCurrentError):
            ctx.field_cost_matrix_host(bad_g, cells, bad_cc)
        with pytest.raises(sc.SeaCurrentError):
            ctx.fleet_assign_host(bad_g, cells, bad_cc)


def _map():
    occ = np.zeros((48, 64), np.uint8)
    occ[4:9, 6:12] = 1
    occ[30:40, 22:30] = 1
    occ[10:14, 50:64] = 1
    occ[44:48, 0:64:3] = 1
    return occ


def test_field_cost_matrix(ctx):
    """Against NumPy indexing of cost_fields' output: plain, weighted and multi-source g, with col_cost, a cell out of range and
    a robot in another free-space component (a walled room)."""
    import torch
    occ = _map()
    occ[18:27, 36:45] = 1
    occ[20:25, 38:43] = 0                                            # a room behind a wall two cells thick
    cell = lambda x, y: y * 64 + x
    d2 = ctx.edt(_t(occ))
    roots = np.array([cell(2, 2), cell(60, 40), cell(33, 20), cell(40, 22)], np.int32)      # the last one inside the room
    robots = np.array([cell(1, 20), cell(40, 21), 64 * 48, cell(62, 2), -1, cell(8, 6), cell(20, 43)], np.int32)   # 8,6: an obstacle
    cc = np.array([0, 5, 1 << 24, 77], np.int32)
    pen = ctx.clearance_penalty(d2, r2=1, r2_soft=25, pen_max=30)
    seeds, seed_off = _t(np.array([cell(2, 2), cell(60, 40), cell(33, 20)], np.int32)), _t(np.array([0, 2, 3], np.int32))
    fields = {
        "plain": ctx.cost_fields(d2, _t(roots), r2=1)["g"],
        "weighted": ctx.cost_fields(d2, _t(roots), r2=1, pen=pen)["g"],
        "multi": ctx.cost_fields_multi(d2, seeds, seed_off, r2=1)["g"],
    }
    for name, g in fields.items():
        F = g.shape[0]
        plain = ctx.field_cost_matrix(g, _t(robots))
        priced = ctx.field_cost_matrix(g, _t(robots), _t(cc[:F]), out=torch.full((7, F), -9, dtype=torch.int32, device="cuda"))
        ctx.synchronize()
        gh = g.cpu().numpy()
        want = np.full((7, F), tw.INF, np.int64)
        for r, c in enumerate(robots):
            if 0 <= c < 64 * 48:
                want[r] = gh.reshape(F, -1)[:, c]
        assert np.array_equal(plain.cpu().numpy(), want), name
        assert np.array_equal(plain.cpu().numpy(), tw.field_cost_matrix(gh, robots)), name
        assert np.array_equal(priced.cpu().numpy(), np.where(want == tw.INF, tw.INF, want + cc[:F])), name
        assert (want[[2, 4, 5]] == tw.INF).all()
        if name != "multi":
            assert (want[1, :3] == tw.INF).all() and want[1, 3] < tw.INF and (want[[0, 3, 6], 3] == tw.INF).all()   # the room
            assert (want[[0, 3, 6], :3] < tw.INF).all()


@pytest.mark.parametrize("n_goal,n_robot", [(5, 7), (7, 5)])
def test_chain_fields_assign_paths(ctx, n_goal, n_robot):
    """cost_fields -> fleet_assign -> field_paths(qfield=col_of, to_root=True) on one stream.  Every assigned robot's path, cost
    and status are what astar_batch returns for that pair (the fields' stated equality: A* from the goal to the robot, the
    cells in the robot..goal order of to_root); unassigned robots get Q_BAD_ENDPOINT; the costs add up to total; the combined
    call equals the separate ones and does not depend on whose buffer holds the matrix."""
    import sea_current_amd as sc
    d2 = ctx.edt(_t(_map()))
    cell = lambda x, y: y * 64 + x
    goals = np.array([cell(60, 20), cell(60, 24), cell(58, 30), cell(40, 4), cell(3, 40), cell(30, 20), cell(50, 42)][:n_goal], np.int32)
    robots = np.array([cell(2, 16), cell(2, 20), cell(2, 24), cell(20, 2), cell(35, 43), cell(15, 30), cell(45, 20)][:n_robot], np.int32)
    fl = ctx.cost_fields(d2, _t(goals), r2=1)
    o = ctx.fleet_assign(fl["g"], _t(robots), want_cost=True)
    paths = ctx.field_paths(d2, fl["g"], _t(goals), o["col_of"], _t(robots), r2=1, Lmax=256, to_root=True)
    m = ctx.field_cost_matrix(fl["g"], _t(robots))
    sep = ctx.assign(m)
    scratch = ctx.fleet_assign(fl["g"], _t(robots))
    ctx.synchronize()
    a, paths, sep, scratch = _np(o), _np(paths), _np(sep), _np(scratch)
    cost = a.pop("cost")
    assert np.array_equal(cost, m.cpu().numpy()) and np.array_equal(cost, tw.field_cost_matrix(fl["g"].cpu().numpy(), robots))
    _same({k: v[None] for k, v in a.items()}, tw.assign(cost))
    _same(a, sep)
    _same(a, scratch)
    tw.certificate(cost, a)
    k = min(n_goal, n_robot)
    assert a["info"].tolist()[0] == k and (a["col_of"] >= 0).sum() == k
    on = np.flatnonzero(a["col_of"] >= 0)
    ref = ctx.astar_batch(d2, _t(goals[a["col_of"][on]]), _t(robots[on]), r2=1, Lmax=256)
    ctx.synchronize()
    ref = _np(ref)
    assert (ref["status"] == sc.Q_OK).all()
    for i, q in enumerate(on):
        assert paths["status"][q] == ref["status"][i] and paths["len"][q] == ref["len"][i] and paths["cost"][q] == ref["cost"][i], q
        n = ref["len"][i]
        assert np.array_equal(paths["path"][q, :n], ref["path"][i, :n][::-1]), q
        assert paths["path"][q, 0] == robots[q] and paths["path"][q, n - 1] == goals[a["col_of"][q]]
    off = np.flatnonzero(a["col_of"] < 0)
    assert len(off) == n_robot - k and (paths["status"][off] == sc.Q_BAD_ENDPOINT).all()
    assert int(paths["cost"][on].sum()) == int(a["info"][1])
