"""sc_known_from_discs / sc_d2_known_i32 / sc_frontier_batch / sc_frontier_cost_matrix / sc_fleet_explore_batch on the GPU:
every output bit-equal to the NumPy twin (tests/frontier_twin.py) on shapes at which the tile logic can fail -- 64 x 64,
65 x 63, 130 x 70, 1 x 200, 200 x 1, 256 x 256 and one 1000 x 700 -- with the corner diagonals, a staircase and a band that cross
tile edges at every offset, three grids in one launch, r2_clear 4 on a block map, the Cmax cut, min_size, optional outputs
NULL; the matrix and the goals for 1, 5 and 40 robots with the paths to the goals against astar_batch; host forms and
argument errors; the whole chain on one stream; the exploration loop against the twin's."""

import numpy as np
import pytest

import frontier_twin as ft
from field_twin import d2_of

pytestmark = pytest.mark.gpu

Q_OK, Q_BAD_ENDPOINT = 0, 2


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fields(tmp_path_factory):
    from field_twin import Twin
    return Twin(tmp_path_factory.mktemp("field_ref"))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(o):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _same(got, want, keys):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        if not np.array_equal(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError(f"{k}: {len(bad)} differ, first at {bad[0].tolist()}: gpu {got[k][tuple(bad[0])]} twin {want[k][tuple(bad[0])]}")


def _check(ctx, d2, known, r2=0, min_size=1, Cmax=128, **kw):
    got = ctx.frontiers(_t(d2), _t(known), r2, min_size, Cmax, **kw)
    ctx.synchronize()
    got = _np(got)
    want = ft.frontiers(d2, known, r2, min_size, Cmax)
    _same(got, want, [k for k in ft.KEYS if got[k] is not None])
    return got, want


def _free(known):
    return np.full(known.shape, 9, np.int32)


def _salt(W, H, p=0.2, seed=2):
    from sea_current_amd import synth
    return d2_of(synth.salt_grid(W, H, p, seed=seed)), ft.known_from_discs(None, ft.three_discs(W, H), W, H)


def _consistent(o, W):
    """slot / rep / csize / cbox / csum of one grid against its label."""
    L = min(int(o["ncl"][0]), len(o["rep"]))
    for k in range(L):
        cells = np.flatnonzero(o["label"].ravel() == o["rep"][k])
        x, y = cells % W, cells // W
        assert o["csize"][k] == len(cells) and (o["slot"].ravel()[cells] == k).all()
        assert o["cbox"][k].tolist() == [x.min(), y.min(), x.max(), y.max()] and o["csum"][k].tolist() == [x.sum(), y.sum()]
    assert int((o["slot"] >= 0).sum()) == int(o["csize"].sum())


SALT_SHAPES = [(64, 64), (65, 63), (130, 70), (256, 256), (1000, 700)]


@pytest.mark.parametrize("W,H", SALT_SHAPES)
def test_salt_maps_equal_the_twin(ctx, W, H):
    d2, known = _salt(W, H)
    got, want = _check(ctx, d2, known, Cmax=512)
    assert 1 <= want["ncl"][0, 1] <= 512 and (got["label"] >= 0).any()
    _consistent({k: (v if k in ("label", "slot") else v[0]) for k, v in got.items()}, W)
    if (W, H) == (130, 70):
        assert want["ncl"].tolist() == [[43, 43]]
        got8, _ = _check(ctx, d2, known, Cmax=8)                      # the cut: the first eight by representative, L in full
        assert got8["ncl"].tolist() == [[43, 43]] and np.array_equal(got8["rep"][0], got["rep"][0, :8])
        got3, _ = _check(ctx, d2, known, min_size=3, Cmax=64)
        assert got3["ncl"].tolist() == [[23, 43]]
        _check(ctx, d2, known, Cmax=1)


@pytest.mark.parametrize("W,H", [(200, 1), (1, 200)])
def test_lines(ctx, W, H):
    discs = [(50, 0, 100), (120, 0, 25)] if H == 1 else [(0, 50, 100), (0, 120, 25)]
    rng = np.random.default_rng(7)
    d2 = (rng.random((H, W)) >= 0.1).astype(np.int32)
    _, want = _check(ctx, d2, ft.known_from_discs(None, discs, W, H))
    assert 2 <= want["ncl"][0, 1] <= 4


def test_corner_diagonals(ctx):
    """One cluster through (63,63)-(64,64), and one through (64,63)-(63,64): links that exist only across a four-tile corner."""
    for known in (ft.corner_diagonal(130, 130), ft.corner_antidiagonal(130, 130), ft.corner_antidiagonal(256, 256, 255),
                  ft.corner_diagonal(65, 65)):
        _, want = _check(ctx, _free(known), known)
        assert want["ncl"].tolist() == [[1, 1]]
    # two cells only, one on each side of the corner, both ways
    for a, b in (((63, 63), (64, 64)), ((64, 63), (63, 64))):
        known = np.zeros((128, 128), np.uint8)
        known[a[1], a[0]] = known[b[1], b[0]] = 1
        _, want = _check(ctx, _free(known), known)
        assert want["ncl"].tolist() == [[1, 1]] and want["csize"][0, 0] == 2


def test_staircases_and_bands_cross_tile_edges_at_every_offset(ctx):
    for step in (1, 2, 3, 5):
        for shift in (0, 61, 62, 63, 64):
            known = ft.staircase(200, 140, step, shift)
            _, want = _check(ctx, _free(known), known)
            assert want["ncl"][0, 1] == 1
    for a, b, off in ((3, 2, 0), (3, 2, 17), (1, 1, 5), (2, 3, 130), (1, 4, 300), (5, 1, -200)):
        known = ft.band(256, 256, a, b, off)
        _, want = _check(ctx, _free(known), known)
        assert 1 <= want["ncl"][0, 1] <= 2
    known = ft.two_discs()
    _, want = _check(ctx, _free(known), known)
    assert want["ncl"].tolist() == [[1, 1]] and want["csize"][0, 0] == 268
    known = ft.ring(200, 150, 100, 75, 60, 30)
    _, want = _check(ctx, _free(known), known)
    assert want["ncl"].tolist() == [[2, 2]]


def test_three_grids_in_one_launch(ctx):
    d2a, ka = _salt(130, 70)
    d2b, kb = _free(ka), ft.staircase(130, 70)
    d2 = np.stack([d2a, d2b, d2a])
    known = np.stack([ka, kb, np.ones_like(ka)])                      # the last grid: all known, no frontier
    got, want = _check(ctx, d2, known, Cmax=64)
    assert want["ncl"].tolist() == [[43, 43], [1, 1], [0, 0]]
    # fields on two of the grids, and on one that does not exist
    free = np.flatnonzero(ft.d2_known(d2a, ka).ravel() >= 1)
    roots = np.array([free[0], free[len(free) // 2], 0, free[-1]], np.int32)
    fgrid = np.array([0, 2, 1, 5], np.int32)
    d2k = ft.d2_known(d2, known)
    g = ctx.cost_fields(_t(d2k), _t(roots), fgrid=_t(fgrid))["g"]
    fr = ctx.frontiers(_t(d2k), _t(known), Cmax=64)
    m = _np(ctx.frontier_cost_matrix(g, fr, gain=2, size_cap=6, fgrid=_t(fgrid)))
    ctx.synchronize()
    cost, cell = ft.cost_matrix(g.cpu().numpy(), want["slot"], want["csize"], 64, 2, 6, fgrid)
    _same(m, dict(cost=cost, cell=cell), ("cost", "cell"))
    assert (cost[0] != ft.INF).any() and (cost[1] == ft.INF).all() and (cost[2] != ft.INF).any() and (cost[3] == ft.INF).all()


def test_clearance_on_a_block_map(ctx, oracle):
    from sea_current_amd import synth
    occ = synth.block_grid(256, 192, 0.3, seed=10, smin=3, smax=24)
    d2 = oracle.edt(occ)
    known = ft.known_from_discs(None, ft.three_discs(256, 192), 256, 192)
    _, w4 = _check(ctx, d2, known, r2=4)
    _, w0 = _check(ctx, d2, known)
    assert (w4["label"] >= 0).sum() < (w0["label"] >= 0).sum() and w4["ncl"][0, 1] >= 2


def test_optional_outputs_may_be_left_out(ctx):
    d2, known = _salt(130, 70)
    full = ft.frontiers(d2, known)
    for kw in (dict(want_label=False), dict(want_slot=False), dict(want_stats=False), dict(want_label=False, want_slot=False, want_stats=False)):
        got, _ = _check(ctx, d2, known, **kw)
        assert all((got[k] is None) == (not kw.get(w, True)) for k, w in (("label", "want_label"), ("slot", "want_slot"), ("cbox", "want_stats")))
        assert np.array_equal(got["rep"], full["rep"])
    # an `out` dict reused on another map of the same shape: every row is rewritten
    out = ctx.frontiers(_t(d2), _t(known))
    k2 = ft.staircase(130, 70)
    got = _np(ctx.frontiers(_t(_free(k2)), _t(k2), out=out))
    _same(got, ft.frontiers(_free(k2), k2), ft.KEYS)


def test_known_and_d2_known(ctx):
    rng = np.random.default_rng(1)
    base = (rng.random((70, 130)) < 0.1).astype(np.uint8) * 7
    discs = np.array([(10, 10, 30), (64, 35, 0), (129, 69, 100), (-5, 20, 64), (40, 40, -1)], np.int32)
    for b in (None, base):
        k = ctx.known_from_discs(_t(discs), 130, 70, base=None if b is None else _t(b))
        assert np.array_equal(k.cpu().numpy(), ft.known_from_discs(b, discs, 130, 70))
    kb = _t(base)
    assert ctx.known_from_discs(_t(discs), 130, 70, base=kb, out=kb) is kb            # in place
    assert np.array_equal(kb.cpu().numpy(), ft.known_from_discs(base, discs, 130, 70))
    assert np.array_equal(ctx.known_from_discs(_t(discs[:0]), 130, 70, base=_t(base)).cpu().numpy(), (base != 0).astype(np.uint8))
    big = np.array([(2000, 3000, 2**31 - 1), (-2**31, 5, 2**31 - 1)], np.int32)      # the squares need 64 bits
    assert np.array_equal(ctx.known_from_discs(_t(big), 130, 70).cpu().numpy(), ft.known_from_discs(None, big, 130, 70))
    d2 = rng.integers(0, 50, (3, 70, 130)).astype(np.int32)
    k3 = np.stack([ft.known_from_discs(None, discs[i:i + 2], 130, 70) for i in range(3)])
    t = _t(d2)
    assert np.array_equal(ctx.d2_known(t, _t(k3)).cpu().numpy(), ft.d2_known(d2, k3))
    assert ctx.d2_known(t, _t(k3), out=t) is t and np.array_equal(t.cpu().numpy(), ft.d2_known(d2, k3))


@pytest.mark.parametrize("R", [1, 5, 40])
def test_goals_for_a_fleet(ctx, R):
    import torch
    W, H = 130, 70
    d2, known = _salt(W, H)
    d2k = ft.d2_known(d2, known)
    free = np.flatnonzero(d2k.ravel() >= 1)
    robots = free[np.random.default_rng(R).choice(len(free), R, replace=False)].astype(np.int32)
    td2k, tk = _t(d2k), _t(known)
    g = ctx.cost_fields(td2k, _t(robots))["g"]
    for gain, cap, Cmax in ((0, 0, 64), (5, 8, 64), (0, 0, 8)):
        fr = ctx.frontiers(td2k, tk, Cmax=Cmax)
        m = _np(ctx.frontier_cost_matrix(g, fr, gain, cap))
        got = _np(ctx.fleet_explore(td2k, tk, g, Cmax=Cmax, gain=gain, size_cap=cap, want_all=True))
        lean = _np(ctx.fleet_explore(td2k, tk, g, Cmax=Cmax, gain=gain, size_cap=cap))          # everything else in scratch
        ctx.synchronize()
        want = ft.fleet_explore(d2k, known, g.cpu().numpy(), Cmax=Cmax, gain=gain, size_cap=cap)
        _same(m, want, ("cost", "cell"))
        _same(got, want, ft.KEYS + ("cost", "cell", "col_of", "row_of", "info", "goal", "gcost"))
        _same(lean, want, ("goal", "gcost"))
        matched = np.flatnonzero(got["goal"] >= 0)
        assert 1 <= len(matched) == got["info"][0] <= min(R, Cmax)
        labels = got["label"].ravel()[got["goal"][matched]]
        assert (labels >= 0).all() and len(set(labels.tolist())) == len(matched)                  # pairwise different clusters
    # the paths to the goals: field read-out == A* on d2k
    goal = _t(got["goal"])
    qf = torch.arange(R, dtype=torch.int32, device="cuda")
    p = _np(ctx.field_paths(td2k, g, _t(robots), qf, goal, Lmax=512))
    a = _np(ctx.astar_batch(td2k, _t(robots), _t(np.where(got["goal"] >= 0, got["goal"], robots).astype(np.int32)), Lmax=512))
    ctx.synchronize()
    for r in range(R):
        if got["goal"][r] < 0:
            assert p["status"][r] == Q_BAD_ENDPOINT and got["gcost"][r] == -1
            continue
        assert p["status"][r] == Q_OK == a["status"][r] and p["cost"][r] == got["gcost"][r] == a["cost"][r] and p["len"][r] == a["len"][r]
        assert np.array_equal(p["path"][r, :p["len"][r]], a["path"][r, :a["len"][r]])


def test_host_forms(ctx):
    d2, known = _salt(130, 70)
    discs = ft.three_discs(130, 70)
    assert np.array_equal(ctx.known_from_discs_host(discs, 130, 70), known)
    d2k = ctx.d2_known_host(d2, known)
    assert np.array_equal(d2k, ft.d2_known(d2, known))
    want = ft.frontiers(d2k, known, Cmax=64)
    got = ctx.frontiers_host(d2k, known, Cmax=64)
    _same(got, want, ft.KEYS)
    lean = ctx.frontiers_host(d2k, known, Cmax=64, want_label=False, want_slot=False, want_stats=False)
    assert lean["label"] is None and np.array_equal(lean["csize"], want["csize"])
    free = np.flatnonzero(d2k.ravel() >= 1)
    robots = free[::len(free) // 5][:5].astype(np.int32)
    g = ctx.cost_fields_host(d2k, robots)["g"]
    m = ctx.frontier_cost_matrix_host(g, got, gain=3, size_cap=4)
    cost, cell = ft.cost_matrix(g, want["slot"], want["csize"], 64, 3, 4)
    _same(m, dict(cost=cost, cell=cell), ("cost", "cell"))
    w = ft.fleet_explore(d2k, known, g, Cmax=64, gain=3, size_cap=4)
    _same(ctx.fleet_explore_host(d2k, known, g, Cmax=64, gain=3, size_cap=4, want_all=True), w,
          ft.KEYS + ("cost", "cell", "col_of", "row_of", "info", "goal", "gcost"))
    _same(ctx.fleet_explore_host(d2k, known, g, Cmax=64, gain=3, size_cap=4), w, ("goal", "gcost"))
    # a field value below 0 is refused before any launch
    import sea_current_amd as sc
    bad = g.copy()
    bad[2, 5, 5] = -1
    with pytest.raises(sc.SeaCurrentError):
        ctx.frontier_cost_matrix_host(bad, got)
    with pytest.raises(sc.SeaCurrentError):
        ctx.fleet_explore_host(d2k, known, bad)


def test_argument_errors(ctx):
    import sea_current_amd as sc
    l, h, p = ctx._l, ctx._h, sc._ptr
    d2, known = _t(np.ones((8, 8), np.int32)), _t(np.ones((8, 8), np.uint8))
    i32 = lambda *s: _t(np.zeros(s, np.int32))
    label, slot, ncl, rep, csize, g, cost, cell, one, discs = i32(8, 8), i32(8, 8), i32(2), i32(4), i32(4), i32(1, 8, 8), i32(4), i32(4), i32(1), i32(1, 3)
    info = _t(np.zeros(4, np.int64))
    INV = 1
    for W, H in ((0, 8), (8, 0), (8193, 8), (8, 8193)):
        assert l.sc_known_from_discs(h, None, p(discs), 1, W, H, p(known)) == INV
        assert l.sc_d2_known_i32(h, p(d2), p(known), 1, W, H, p(label)) == INV
        assert l.sc_frontier_batch(h, p(d2), p(known), 1, W, H, 0, 1, 4, None, None, p(ncl), p(rep), p(csize), None, None) == INV
        assert l.sc_frontier_cost_matrix(h, p(g), 1, None, p(slot), p(csize), 1, W, H, 4, 0, 0, p(cost), p(cell)) == INV
    assert l.sc_known_from_discs(h, None, None, 1, 8, 8, p(known)) == INV and l.sc_known_from_discs(h, None, p(discs), -1, 8, 8, p(known)) == INV
    assert l.sc_known_from_discs(h, None, p(discs), 1, 8, 8, None) == INV and l.sc_d2_known_i32(h, p(d2), p(known), 0, 8, 8, p(label)) == INV
    fr = lambda G=1, ms=1, C=4, d=d2, k=known, n=ncl, r=rep, c=csize: l.sc_frontier_batch(h, p(d), p(k), G, 8, 8, 0, ms, C, None, None, p(n), p(r), p(c),
                                                                                           None, None)
    assert fr() == 0
    assert [fr(G=0), fr(ms=0), fr(C=0), fr(C=65537), fr(d=None), fr(k=None), fr(n=None), fr(r=None), fr(c=None)] == [INV] * 9
    mat = lambda F=1, G=1, C=4, gain=0, cap=0, gg=g, s=slot, cs=csize, co=cost, ce=cell: l.sc_frontier_cost_matrix(
        h, p(gg), F, None, p(s), p(cs), G, 8, 8, C, gain, cap, p(co), p(ce))
    assert mat() == 0
    assert [mat(F=0), mat(G=0), mat(G=2), mat(C=0), mat(C=65537), mat(gain=-1), mat(cap=-1), mat(gain=2**15 + 1, cap=2**15), mat(gg=None),
            mat(s=None), mat(cs=None), mat(co=None), mat(ce=None)] == [INV] * 13
    assert mat(gain=2**15, cap=2**15) == 0
    ex = lambda F=1, C=4, ms=1, gain=0, go=one, gc=one, gg=g: l.sc_fleet_explore_batch(h, p(d2), p(known), 8, 8, 0, ms, C, p(gg), F, gain, 0, None,
                                                                                       None, None, None, None, None, None, None, None, None, None,
                                                                                       p(info), p(go), p(gc))
    assert ex() == 0
    assert [ex(F=0), ex(F=1025), ex(C=0), ex(C=1025), ex(ms=0), ex(gain=-1), ex(go=None), ex(gc=None), ex(gg=None)] == [INV] * 9
    ctx.synchronize()


def test_the_chain_on_one_stream(ctx, oracle):
    """known_from_discs -> edt -> d2_known -> cost_fields -> fleet_explore -> field_paths, one synchronise at the end."""
    import torch
    from sea_current_amd import synth
    W, H = 130, 70
    occ = synth.salt_grid(W, H, 0.2, seed=2)
    discs = ft.three_discs(W, H)
    robots = np.array([35 * W + 30, 35 * W + 65, 35 * W + 100, 30 * W + 60], np.int32)
    occ[robots // W, robots % W] = 0
    known = ctx.known_from_discs(_t(discs), W, H)
    seen = _t(occ) * known                                             # the obstacles the robots have observed
    d2k = ctx.d2_known(ctx.edt(seen), known)
    g = ctx.cost_fields(d2k, _t(robots))["g"]
    ex = ctx.fleet_explore(d2k, known, g, Cmax=64)
    paths = ctx.field_paths(d2k, g, _t(robots), torch.arange(4, dtype=torch.int32, device="cuda"), ex["goal"], Lmax=512)
    ctx.synchronize()
    kn = ft.known_from_discs(None, discs, W, H)
    wd2k = ft.d2_known(oracle.edt(np.where(kn != 0, occ, 0).astype(np.uint8)), kn)
    assert np.array_equal(d2k.cpu().numpy(), wd2k)
    want = ft.fleet_explore(wd2k, kn, g.cpu().numpy(), Cmax=64)
    _same(_np(ex), want, ("goal", "gcost"))
    assert (want["goal"] >= 0).all()
    paths = _np(paths)
    assert (paths["status"] == Q_OK).all() and np.array_equal(paths["cost"], want["gcost"])
    for r in range(4):
        assert paths["path"][r, 0] == robots[r] and paths["path"][r, paths["len"][r] - 1] == want["goal"][r]


@pytest.mark.parametrize("name", ["salt96x80", "blocks96x80", "salt130x70"])
def test_exploration_loop_visits_the_twins_goals(ctx, oracle, fields, name):
    occ = ft.loop_maps()[name]
    start = ft.loop_start(occ)

    def gpu_step(occ_seen, known, pos):
        tk = _t(known)
        d2k = ctx.d2_known(ctx.edt(_t(occ_seen)), tk)
        g = ctx.cost_fields(d2k, _t(np.array([pos], np.int32)))["g"]
        goal = ctx.fleet_explore(d2k, tk, g, Cmax=256)["goal"]
        ctx.synchronize()
        return int(goal.cpu().numpy()[0])

    goals, known = ft.explore_loop(occ, start, gpu_step)
    want_goals, want_known = ft.explore_loop(occ, start, ft.twin_step(oracle, fields))
    assert goals == want_goals and np.array_equal(known, want_known)
    assert (known[ft.true_component(occ, start)] != 0).all()
