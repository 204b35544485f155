"""sc_known_from_views / sc_view_gain_batch on the GPU: known, occ_seen and gain bit-equal to the NumPy twin
(tests/views_twin.py) on 64 x 64, 65 x 63 and 130 x 70, blocks and salt, with 1, 3 and 17 views -- every ignored kind, r2 = 0,
a view covering the whole grid; centres on the tile edges (x or y = 63, 64), in the four grid corners, boxes clipped on two
sides; the corner rule and the door map; 1 x 200 and 200 x 1; base in place, occ_seen NULL and given, a reused out; the gain
identity and 1, 64 and 300 candidates; host forms; argument errors; the whole chain on one stream; the exploration loop against
the twin's; one view covering 1000 x 700, where a workgroup takes more than one tile in both ray kernels, against the C
reference.  The kernels have one path."""

import numpy as np
import pytest

import frontier_twin as ft
import views_twin as vt

pytestmark = pytest.mark.gpu

Q_OK = 0


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return vt.Ref(tmp_path_factory.mktemp("views_ref"))


@pytest.fixture(scope="module")
def fields(tmp_path_factory):
    from field_twin import Twin
    return Twin(tmp_path_factory.mktemp("field_ref"))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _eq(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{name}: {len(bad)} differ, first at {bad[0].tolist()}: gpu {got[tuple(bad[0])]} twin {want[tuple(bad[0])]}")


def _check(ctx, occ, views, base=None):
    """known, occ_seen and gain (against base, or nothing known) of the GPU == the twin's; returns the twin's."""
    views = np.ascontiguousarray(views, dtype=np.int32).reshape(-1, 3)
    tocc, tviews = _t(occ), _t(views)
    known, occ_seen = ctx.known_from_views(tviews, tocc, base=None if base is None else _t(base), occ_seen=True)
    before = np.zeros_like(occ) if base is None else base
    gain = ctx.view_gain(tviews, tocc, _t(before))
    ctx.synchronize()
    want_known, want_seen = vt.known_from_views(base, occ, views)
    want_gain = vt.view_gain(occ, before, views)
    _eq("known", known.cpu().numpy(), want_known)
    _eq("occ_seen", occ_seen.cpu().numpy(), want_seen)
    _eq("gain", gain.cpu().numpy(), want_gain)
    return want_known, want_seen, want_gain


def _map(kind, W, H):
    from sea_current_amd import synth
    return synth.block_grid(W, H, 0.3, seed=10, smin=3, smax=24) if kind == "blocks" else synth.salt_grid(W, H, 0.05, seed=2)


def _views(occ, n):
    """1: one view covering the whole grid; 3: r2 = 0 on a free cell, a centre on an obstacle, a mid-range view; 17: those,
    every ignored kind and random views."""
    H, W = occ.shape
    free = np.flatnonzero(occ.ravel() == 0)
    mid = int(free[np.argmin((free % W - W // 2) ** 2 + (free // W - H // 2) ** 2)])
    cover = (mid % W, mid // W, W * W + H * H)
    if n == 1:
        return np.array([cover], np.int32)
    blocked = int(np.flatnonzero(occ.ravel() != 0)[7])
    three = [(int(free[5]) % W, int(free[5]) // W, 0), (blocked % W, blocked // W, 400), (mid % W, mid // W, 300)]
    if n == 3:
        return np.array(three, np.int32)
    rng = np.random.default_rng(W * H)
    cells = free[rng.choice(len(free), 6, replace=False)]
    more = [(int(c) % W, int(c) // W, int(r2)) for c, r2 in zip(cells, rng.integers(1, 900, 6))]
    ignored = [(mid % W, mid // W, -1), (-1, H // 2, 400), (W, H // 2, 400), (W // 2, -1, 400), (W // 2, H, 400), (-2**31, 0, 2**31 - 1)]
    return np.array(three + ignored[:3] + more + ignored[3:] + [(int(free[-1]) % W, int(free[-1]) // W, 64), cover][:2], np.int32)


@pytest.mark.parametrize("kind", ["blocks", "salt"])
@pytest.mark.parametrize("W,H", [(64, 64), (65, 63), (130, 70)])
def test_maps_equal_the_twin(ctx, W, H, kind):
    occ = _map(kind, W, H)
    rng = np.random.default_rng(1)
    base = (rng.random((H, W)) < 0.1).astype(np.uint8) * 7
    for n in (1, 3, 17):
        views = _views(occ, n)
        assert len(views) == n
        known, occ_seen, gain = _check(ctx, occ, views)
        _check(ctx, occ, views, base)
        assert known.any() and gain.max() > 0 and (n == 1 or (gain == 0).any())
        if n == 3:
            assert gain.tolist()[:2] == [1, 0]                         # r2 = 0 sees its own free cell; the blocked centre nothing
    assert occ_seen.any() and not known.all()


def test_tile_and_box_edges(ctx):
    """Centres on the 16-cell tile edges of a view's box and the 64-cell edges of the grid, in the grid's corners, and boxes
    clipped on two sides."""
    W, H = 130, 70
    for kind in ("blocks", "salt"):
        occ = _map(kind, W, H).copy()
        centres = [(63, 35), (64, 35), (63, 63), (64, 64), (30, 63), (30, 64), (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (2, 3), (W - 3, H - 2)]
        for x, y in centres:
            occ[y, x] = 0
        for r2 in (15 * 15, 16 * 16, 17 * 17 + 3, 33 * 33):
            _, _, gain = _check(ctx, occ, [(x, y, r2) for x, y in centres])
            assert (gain > 0).all()
        for x, y in centres:                                           # one at a time: its box alone
            _check(ctx, occ, [(x, y, 40 * 40)])


def test_corner_rule_and_door_map(ctx):
    for block, seen in (([(5, 4)], False), ([(4, 5)], False), ([], True)):
        occ = vt.corner_map(block)
        known, _, _ = _check(ctx, occ, [(4, 4, 8)])
        assert bool(known[5, 5]) == seen
    occ = vt.door_map()
    known, occ_seen, gain = _check(ctx, occ, [vt.DOOR_VIEW])
    assert int(known.sum()) == 3276 and gain.tolist() == [3215] and known[:, 48].all() and int(known[:, 49:].sum()) == 140
    assert int(occ_seen.sum()) == 61


def test_more_tiles_than_workgroups(ctx, ref):
    """One view covering 1000 x 700: its box has 63 x 44 = 2 772 tiles of 16 x 16, more than the 2 048 workgroups a view gets,
    so workgroups of the view kernel take a second tile (the gain kernel, with 64 workgroups per candidate at most, does so
    from 65 tiles on).  Against the C reference: the twin walks column by column in NumPy, slow at this size.  A second view
    of 30 cells' radius shares the launch."""
    from sea_current_amd import synth
    W, H = 1000, 700
    occ = synth.block_grid(W, H, 0.15, seed=3, smin=3, smax=24)
    occ[H // 2, W // 2] = occ[40, 900] = 0
    views = np.array([(W // 2, H // 2, W * W + H * H), (900, 40, 900)], np.int32)
    tocc, tviews = _t(occ), _t(views)
    known, occ_seen = ctx.known_from_views(tviews, tocc, occ_seen=True)
    gain = ctx.view_gain(tviews, tocc, _t(np.zeros_like(occ)))
    ctx.synchronize()
    want_known, want_seen = ref.known_from_views(None, occ, views)
    _eq("known", known.cpu().numpy(), want_known)
    _eq("occ_seen", occ_seen.cpu().numpy(), want_seen)
    _eq("gain", gain.cpu().numpy(), ref.view_gain(occ, np.zeros_like(occ), views))
    assert 10000 < want_known.sum() < W * H and want_known[528:].any()                 # rows of the tiles past the first 2 048


@pytest.mark.parametrize("W,H", [(200, 1), (1, 200)])
def test_lines(ctx, W, H):
    occ = np.zeros((H, W), np.uint8)
    occ.ravel()[[80, 150]] = 1
    views = [(50, 0, 10000), (120, 0, 25), (199, 0, 9)] if H == 1 else [(0, 50, 10000), (0, 120, 25), (0, 199, 9)]
    known, _, gain = _check(ctx, occ, views)
    assert known.ravel()[:81].all() and not known.ravel()[81:115].any() and gain.tolist() == [80, 11, 4]


def test_aliasing_and_optional_outputs(ctx):
    occ = _map("blocks", 130, 70)
    views = _views(occ, 17)
    rng = np.random.default_rng(4)
    base = (rng.random(occ.shape) < 0.1).astype(np.uint8) * 3
    want, want_seen = vt.known_from_views(base, occ, views)
    tocc, tviews = _t(occ), _t(views)
    kb = _t(base)
    assert ctx.known_from_views(tviews, tocc, base=kb, out=kb) is kb                       # in place, occ_seen NULL
    _eq("in place", kb.cpu().numpy(), want)
    seen = _t(np.full(occ.shape, 9, np.uint8))
    kb = _t(base)
    k, s = ctx.known_from_views(tviews, tocc, base=kb, out=kb, occ_seen=seen)             # in place, occ_seen given
    assert k is kb and s is seen
    _eq("in place", kb.cpu().numpy(), want)
    _eq("occ_seen", seen.cpu().numpy(), want_seen)
    # a reused out on other views: every cell is rewritten
    v2 = _views(occ, 3)
    k2 = ctx.known_from_views(_t(v2), tocc, out=k, occ_seen=seen)[0]
    assert k2 is k
    w2, s2 = vt.known_from_views(None, occ, v2)
    _eq("reused", k.cpu().numpy(), w2)
    _eq("reused occ_seen", seen.cpu().numpy(), s2)
    # R = 0 copies base, or clears
    none = _t(np.zeros((0, 3), np.int32))
    _eq("R = 0", ctx.known_from_views(none, tocc, base=_t(base)).cpu().numpy(), (base != 0).astype(np.uint8))
    assert not ctx.known_from_views(none, tocc).cpu().numpy().any()
    # a reused gain
    g = ctx.view_gain(tviews, tocc, _t(want))
    assert ctx.view_gain(tviews, tocc, _t(np.zeros_like(occ)), out=g) is g
    _eq("gain", g.cpu().numpy(), vt.view_gain(occ, np.zeros_like(occ), views))
    assert ctx.view_gain(none, tocc, _t(want)).shape == (0,)
    ctx.synchronize()


@pytest.mark.parametrize("N", [1, 64, 300])
def test_gain_for_many_candidates(ctx, N):
    """gain == the twin's, and with the true map == the free cells known_from_views newly marks for that view alone."""
    occ = _map("blocks", 130, 70)
    H, W = occ.shape
    rng = np.random.default_rng(N)
    known, occ_seen = vt.known_from_views(None, occ, _views(occ, 3))
    cells = rng.integers(0, W * H, N)                                 # free and occupied centres alike
    views = np.stack([cells % W, cells // W, rng.integers(0, 500, N)], 1).astype(np.int32)
    if N > 1:
        views[::7, 2] = -1                                             # ignored ones among them
        views[3::11, 0] = W
    tocc, tk = _t(occ), _t(known)
    gain = ctx.view_gain(_t(views), tocc, tk).cpu().numpy()
    _eq("gain", gain, vt.view_gain(occ, known, views))
    _eq("predicted", ctx.view_gain(_t(views), _t(occ_seen), tk).cpu().numpy(), vt.view_gain(occ_seen, known, views))
    assert N == 1 or (gain > 0).any()
    for i in range(0, N, max(N // 8, 1)):
        more = ctx.known_from_views(_t(views[i:i + 1]), tocc, base=tk).cpu().numpy()
        assert gain[i] == int(((more != 0) & (known == 0) & (occ == 0)).sum()), i


def test_host_forms(ctx):
    occ = _map("salt", 130, 70)
    views = _views(occ, 17)
    base = (np.random.default_rng(8).random(occ.shape) < 0.1).astype(np.uint8)
    want, want_seen = vt.known_from_views(base, occ, views)
    _eq("known", ctx.known_from_views_host(views, occ, base=base), want)
    k, s = ctx.known_from_views_host(views, occ, base=base, occ_seen=True)
    _eq("known", k, want)
    _eq("occ_seen", s, want_seen)
    _eq("lists", ctx.known_from_views_host(views.tolist(), occ), vt.known_from_views(None, occ, views)[0])
    _eq("gain", ctx.view_gain_host(views, occ, base), vt.view_gain(occ, base, views))
    assert ctx.view_gain_host(np.zeros((0, 3), np.int32), occ, base).shape == (0,)
    _eq("R = 0", ctx.known_from_views_host(np.zeros((0, 3), np.int32), occ, base=base), base)


def test_argument_errors(ctx):
    import sea_current_amd as sc
    l, h, p = ctx._l, ctx._h, sc._ptr
    occ, known, seen = (_t(np.zeros((8, 8), np.uint8)) for _ in range(3))
    views, gain = _t(np.array([[4, 4, 9]], np.int32)), _t(np.zeros(1, np.int32))
    INV = 1
    kv = lambda W=8, H=8, R=1, o=occ, v=views, k=known, s=seen, b=None: l.sc_known_from_views(h, p(b), p(o), p(v), R, W, H, p(k), p(s))
    assert kv() == 0 and kv(s=None) == 0 and kv(b=known) == 0 and kv(R=0, v=None) == 0
    assert [kv(W=0), kv(H=0), kv(W=8193), kv(H=8193), kv(R=-1), kv(o=None), kv(v=None), kv(k=None), kv(s=occ), kv(s=known)] == [INV] * 10
    vg = lambda W=8, H=8, N=1, o=occ, k=known, v=views, g=gain: l.sc_view_gain_batch(h, p(o), p(k), p(v), N, W, H, p(g))
    assert vg() == 0 and vg(N=0, v=None, g=None) == 0
    assert [vg(W=0), vg(H=0), vg(W=8193), vg(H=8193), vg(N=-1), vg(o=None), vg(k=None), vg(v=None), vg(g=None)] == [INV] * 9
    ctx.synchronize()
    o, k, s = (np.zeros((8, 8), np.uint8) for _ in range(3))
    v, g = np.array([[4, 4, 9]], np.int32), np.zeros(1, np.int32)
    assert l.sc_known_from_views_host(h, None, p(o), p(v), 1, 8, 8, p(k), p(s)) == 0
    assert l.sc_known_from_views_host(h, None, p(o), p(v), 1, 8, 8, p(k), p(o)) == INV
    assert l.sc_known_from_views_host(h, None, p(o), p(v), 1, 8, 8, p(k), p(k)) == INV
    assert l.sc_known_from_views_host(h, None, p(o), p(v), -1, 8, 8, p(k), None) == INV
    assert l.sc_view_gain_batch_host(h, p(o), p(k), p(v), 1, 8, 0, p(g)) == INV and l.sc_view_gain_batch_host(h, p(o), p(k), None, 1, 8, 8, p(g)) == INV


def test_the_chain_on_one_stream(ctx, oracle):
    """known_from_views(occ_seen=...) -> edt(occ_seen) -> d2_known -> cost_fields -> fleet_explore -> field_paths, one
    synchronise at the end."""
    import torch
    W, H = 130, 70
    occ = _map("salt", W, H).copy()
    robots = np.array([35 * W + 30, 35 * W + 65, 35 * W + 100, 30 * W + 60], np.int32)
    occ[robots // W, robots % W] = 0
    views = np.stack([robots % W, robots // W, np.full(4, 400)], 1).astype(np.int32)
    known, occ_seen = ctx.known_from_views(_t(views), _t(occ), occ_seen=True)
    d2k = ctx.d2_known(ctx.edt(occ_seen), known)
    g = ctx.cost_fields(d2k, _t(robots))["g"]
    ex = ctx.fleet_explore(d2k, known, g, Cmax=64)
    paths = ctx.field_paths(d2k, g, _t(robots), torch.arange(4, dtype=torch.int32, device="cuda"), ex["goal"], Lmax=512)
    ctx.synchronize()
    kn, seen = vt.known_from_views(None, occ, views)
    _eq("known", known.cpu().numpy(), kn)
    _eq("occ_seen", occ_seen.cpu().numpy(), seen)
    wd2k = ft.d2_known(oracle.edt(seen), kn)
    _eq("d2k", d2k.cpu().numpy(), wd2k)
    want = ft.fleet_explore(wd2k, kn, g.cpu().numpy(), Cmax=64)
    _eq("goal", ex["goal"].cpu().numpy(), want["goal"])
    _eq("gcost", ex["gcost"].cpu().numpy(), want["gcost"])
    assert (want["goal"] >= 0).all()
    p = {k: v.cpu().numpy() for k, v in paths.items()}
    assert (p["status"] == Q_OK).all() and np.array_equal(p["cost"], want["gcost"])
    for r in range(4):
        assert p["path"][r, 0] == robots[r] and p["path"][r, p["len"][r] - 1] == want["goal"][r]


@pytest.mark.parametrize("name", ["blocks96x80", "rooms96x80"])
def test_exploration_loop_visits_the_twins_goals(ctx, oracle, fields, name):
    occ = vt.loop_maps()[name]
    start = ft.loop_start(occ)
    tocc = _t(occ)

    def gpu_sense(base, occ_, views):
        known, occ_seen = ctx.known_from_views(_t(np.array(views, np.int32)), tocc, base=None if base is None else _t(base), occ_seen=True)
        return known.cpu().numpy(), occ_seen.cpu().numpy()

    def gpu_step(occ_seen, known, pos):
        tk = _t(known)
        d2k = ctx.d2_known(ctx.edt(_t(occ_seen)), tk)
        g = ctx.cost_fields(d2k, _t(np.array([pos], np.int32)))["g"]
        goal = ctx.fleet_explore(d2k, tk, g, Cmax=256)["goal"]
        ctx.synchronize()
        return int(goal.cpu().numpy()[0])

    goals, known = vt.explore_loop_views(occ, start, gpu_step, sense=gpu_sense)
    want_goals, want_known = vt.explore_loop_views(occ, start, ft.twin_step(oracle, fields))
    assert goals == want_goals and np.array_equal(known, want_known) and len(goals) >= 10
    assert (known[ft.true_component(occ, start)] != 0).all()
