"""sc_known_from_sectors / sc_sector_gain_batch / sc_view_gain_headings_batch / sc_views_from_cells on the GPU: every output
bit-equal to the NumPy twin (tests/sectors_twin.py) on 64 x 64, 65 x 63 and 130 x 70, blocks and salt, with 1, 3 and 17 sector
views -- every ignored kind among live ones; centres on the tile edges (x or y = 63, 64) and in the grid corners with radii 15,
16, 17 and 33; sector edges along the axes and the diagonals (they fall on tile borders), one bin of 64, exactly half a turn,
reflex sectors; a box clipped on two sides and a sector of which only the centre's tile survives the skip; base in place,
occ_seen NULL and given, R = 0; the gain of every heading for 1, 64 and 300 candidates, 3, 8, 16 and 64 bins, span 1, B/2,
B - 1 and B, hist / gainh NULL and given, a reused out; the identities (a), (b), (c) on the device; argument errors; host
forms; the goal-pose chain on one stream; one view covering 1000 x 700 against the C statement; the exploration loop with the
twin's goals, headings and counts."""

import numpy as np
import pytest

import frontier_twin as ft
import sectors_twin as st
import views_twin as vt

pytestmark = pytest.mark.gpu

E, NE, N_, NW, W_, SW, S_, SE = (1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)
# (a, b): along the axes and diagonals; a quarter, an eighth, half a turn, three quarters (reflex), and seven eighths
SHAPES = [(E, N_), (NE, N_), (N_, W_), (E, W_), (W_, E), (S_, NE), (NW, SW), (N_, E), (SE, S_), (NE, SW), (SW, NE), (E, SE)]
IGNORED = [((1, 0), (2, 0)), ((3, 3), (3, 3)), ((1, 0), (0, 0)), ((0, 0), (0, 1)), ((32768, 0), (0, 1)), ((1, 0), (0, -32768))]


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return st.Ref(tmp_path_factory.mktemp("sectors_ref"))


@pytest.fixture(scope="module")
def fields(tmp_path_factory):
    from field_twin import Twin
    return Twin(tmp_path_factory.mktemp("field_ref"))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _eq(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{name}: {len(bad)} differ, first at {bad[0].tolist()}: gpu {got[tuple(bad[0])]} twin {want[tuple(bad[0])]}")


def _check(ctx, occ, rows, base=None):
    """known, occ_seen and gain (against base, or nothing known) of the GPU == the twin's; returns the twin's."""
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 7)
    tocc, trows = _t(occ), _t(rows)
    known, occ_seen = ctx.known_from_sectors(trows, tocc, base=None if base is None else _t(base), occ_seen=True)
    before = np.zeros_like(occ) if base is None else base
    gain = ctx.sector_gain(trows, tocc, _t(before))
    ctx.synchronize()
    want_known, want_seen = st.known_from_sectors(base, occ, rows)
    want_gain = st.sector_gain(occ, before, rows)
    _eq("known", known.cpu().numpy(), want_known)
    _eq("occ_seen", occ_seen.cpu().numpy(), want_seen)
    _eq("gain", gain.cpu().numpy(), want_gain)
    return want_known, want_seen, want_gain


def _map(kind, W, H):
    from sea_current_amd import synth
    return synth.block_grid(W, H, 0.3, seed=10, smin=3, smax=24) if kind == "blocks" else synth.salt_grid(W, H, 0.05, seed=2)


def _row(x, y, r2, a, b):
    return (x, y, r2, a[0], a[1], b[0], b[1])


def _rows(occ, n):
    """1: a reflex sector covering the whole grid; 3: r2 = 0, a centre on an obstacle, a quarter; 17: those, every ignored kind
    and random sectors of every shape."""
    H, W = occ.shape
    free = np.flatnonzero(occ.ravel() == 0)
    mid = int(free[np.argmin((free % W - W // 2) ** 2 + (free // W - H // 2) ** 2)])
    mx, my = mid % W, mid // W
    cover = _row(mx, my, W * W + H * H, N_, E)
    if n == 1:
        return np.array([cover], np.int32)
    blocked = int(np.flatnonzero(occ.ravel() != 0)[7])
    three = [_row(int(free[5]) % W, int(free[5]) // W, 0, S_, W_), _row(blocked % W, blocked // W, 400, E, N_), _row(mx, my, 300, NE, NW)]
    if n == 3:
        return np.array(three, np.int32)
    rng = np.random.default_rng(W * H)
    cells = free[rng.choice(len(free), 5, replace=False)]
    d64 = st.heading_dirs(64, 0.123)
    more = [_row(int(c) % W, int(c) // W, int(r2), *SHAPES[k]) for k, (c, r2) in enumerate(zip(cells[:4], rng.integers(1, 900, 4)), 3)]
    more.append(_row(int(cells[4]) % W, int(cells[4]) // W, 2500, d64[5], d64[6]))                 # one bin of 64
    ignored = [_row(mx, my, 400, a, b) for a, b in IGNORED] + [_row(mx, my, -1, E, N_), _row(W, H // 2, 400, E, N_)]
    out = three + ignored[:4] + more + ignored[4:] + [cover]
    return np.array(np.clip(np.array(out, np.int64), -2**31, 2**31 - 1), np.int32)


@pytest.mark.parametrize("kind", ["blocks", "salt"])
@pytest.mark.parametrize("W,H", [(64, 64), (65, 63), (130, 70)])
def test_maps_equal_the_twin(ctx, W, H, kind):
    occ = _map(kind, W, H)
    rng = np.random.default_rng(1)
    base = (rng.random((H, W)) < 0.1).astype(np.uint8) * 7
    for n in (1, 3, 17):
        rows = _rows(occ, n)
        assert len(rows) == n
        known, occ_seen, gain = _check(ctx, occ, rows)
        _check(ctx, occ, rows, base)
        assert known.any() and gain.max() > 0 and (n == 1 or (gain == 0).any())
        if n == 3:
            assert gain.tolist()[:2] == [1, 0]                         # r2 = 0 sees its own free cell; the blocked centre nothing
        if n == 17:
            assert not gain[3:7].any() and not gain[12:16].any()       # the ignored rows
    assert not known.all()


def test_tile_borders_and_sector_shapes(ctx):
    """Centres on the 16-cell tile edges and the 64-cell edges, in the grid's corners; radii around the tile; every shape."""
    W, H = 130, 70
    for kind in ("blocks", "salt"):
        occ = _map(kind, W, H).copy()
        centres = [(63, 35), (64, 35), (63, 63), (64, 64), (30, 63), (30, 64), (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (2, 3), (W - 3, H - 2)]
        for x, y in centres:
            occ[y, x] = 0
        for k, r2 in enumerate((15 * 15, 16 * 16, 17 * 17 + 3, 33 * 33)):
            rows = [_row(x, y, r2, *SHAPES[(i + 3 * k) % len(SHAPES)]) for i, (x, y) in enumerate(centres)]
            _, _, gain = _check(ctx, occ, rows)
            assert (gain > 0).all()
        for a, b in SHAPES:                                            # every shape from a tile corner of the grid: edges on tile borders
            _check(ctx, occ, [_row(64, 32, 40 * 40, a, b), _row(63, 31, 33 * 33, a, b)])


def test_culling(ctx):
    """A box clipped on two sides; a narrow sector of a large view, where nearly every tile is skipped; a sector that points
    out of the grid from a corner, so that no tile but the centre's survives."""
    W, H = 130, 70
    occ = _map("salt", W, H).copy()
    occ[2, 3] = occ[69, 129] = occ[35, 64] = 0
    d64 = st.heading_dirs(64, 0.5)
    rows = [_row(3, 2, 40 * 40, E, N_), _row(3, 2, 40 * 40, W_, S_), _row(64, 35, W * W, d64[9], d64[10]), _row(64, 35, W * W, d64[40], d64[41]),
            _row(129, 69, 50 * 50, E, N_), _row(129, 69, 50 * 50, SE, NE)]
    _, _, gain = _check(ctx, occ, rows)
    assert gain[0] > 100 and gain[1] <= 12 and gain[4] == 1                   # (129, 69) looking out of the grid sees its own cell
    for r in rows:
        _check(ctx, occ, [r])


def test_known_from_sectors_forms(ctx):
    occ = _map("blocks", 130, 70)
    rows = _rows(occ, 17)
    rng = np.random.default_rng(4)
    base = (rng.random(occ.shape) < 0.1).astype(np.uint8) * 3
    want, want_seen = st.known_from_sectors(base, occ, rows)
    tocc, trows = _t(occ), _t(rows)
    kb = _t(base)
    assert ctx.known_from_sectors(trows, tocc, base=kb, out=kb) is kb                      # in place, occ_seen NULL
    _eq("in place", kb.cpu().numpy(), want)
    seen = _t(np.full(occ.shape, 9, np.uint8))
    kb = _t(base)
    k, s = ctx.known_from_sectors(trows, tocc, base=kb, out=kb, occ_seen=seen)            # in place, occ_seen given
    assert k is kb and s is seen
    _eq("in place", kb.cpu().numpy(), want)
    _eq("occ_seen", seen.cpu().numpy(), want_seen)
    none = _t(np.zeros((0, 7), np.int32))                                                 # R = 0 copies base, or clears
    _eq("R = 0", ctx.known_from_sectors(none, tocc, base=_t(base)).cpu().numpy(), (base != 0).astype(np.uint8))
    assert not ctx.known_from_sectors(none, tocc).cpu().numpy().any()
    g = ctx.sector_gain(trows, tocc, _t(want))
    assert ctx.sector_gain(trows, tocc, _t(np.zeros_like(occ)), out=g) is g                # a reused gain
    _eq("gain", g.cpu().numpy(), st.sector_gain(occ, np.zeros_like(occ), rows))
    assert ctx.sector_gain(none, tocc, _t(want)).shape == (0,)
    ctx.synchronize()


def _candidates(occ, N):
    H, W = occ.shape
    rng = np.random.default_rng(N)
    cells = rng.integers(0, W * H, N)                                 # free and occupied centres alike
    views = np.stack([cells % W, cells // W, rng.integers(0, 500, N)], 1).astype(np.int32)
    if N > 1:
        views[::7, 2] = -1                                             # ignored ones among them
        views[3::11, 0] = W
    else:
        free = np.flatnonzero(occ.ravel() == 0)
        views[0] = (free[len(free) // 2] % W, free[len(free) // 2] // W, 400)
    return views


@pytest.mark.parametrize("N", [1, 64, 300])
def test_gain_per_heading(ctx, N):
    """hist, gainh and best == the twin's for every B and span, with hist / gainh absent or given and a reused out; identities
    (a) and (b) on the device."""
    occ = _map("blocks", 130, 70)
    known, occ_seen = vt.known_from_views(None, occ, vt.free_centres(occ, ft.three_discs(130, 70))[:1])
    views = _candidates(occ, N)
    tocc, tk, tv = _t(occ), _t(known), _t(views)
    full = ctx.view_gain(tv, tocc, tk).cpu().numpy()
    out = None
    for B in (3, 8, 16, 64):
        dirs = st.heading_dirs(B, 0.123 if B != 16 else 0.0)
        counts = st.view_gain_headings(occ, known, views, dirs, 1)     # the rays once per table; the windows per span
        for span in sorted({1, B // 2, B - 1, B}):
            want = dict(counts, **st.headings_from_hist(counts["hist"], counts["c0"], span))
            got = ctx.view_gain_headings(tv, tocc, tk, dirs, span, hist=True, gainh=True)
            for key in ("hist", "gainh", "best"):
                _eq(f"{key} B={B} span={span}", got[key].cpu().numpy(), want[key])
            _eq("(a)", (want["hist"].sum(1) + want["c0"]).astype(np.int32), full)
            out = ctx.view_gain_headings(tv, tocc, tk, dirs, span, out=out)               # hist and gainh NULL, out reused
            _eq("best alone", out.cpu().numpy(), want["best"])
            only = ctx.view_gain_headings(tv, tocc, tk, dirs, span, gainh=got["gainh"])
            assert set(only) == {"best", "gainh"} and only["gainh"] is got["gainh"]
            _eq("gainh alone", only["gainh"].cpu().numpy(), want["gainh"])
            hs = range(B) if N <= 64 else (0, B // 2, B - 1)                               # (b): the sector gain of (u_h, u_{h+span})
            for h in hs:
                sg = ctx.sector_gain(_t(st.sector_views(views, dirs, h, span)), tocc, tk).cpu().numpy()
                _eq(f"(b) B={B} span={span} h={h}", sg, want["gainh"][:, h])
    predicted = ctx.view_gain_headings(tv, _t(occ_seen), tk, st.heading_dirs(16), 4).cpu().numpy()
    _eq("predicted", predicted, st.view_gain_headings(occ_seen, known, views, st.heading_dirs(16), 4)["best"])
    assert N == 1 or (full > 0).any()
    assert ctx.view_gain_headings(_t(np.zeros((0, 3), np.int32)), tocc, tk, st.heading_dirs(8), 2).shape == (0, 2)


def test_full_circle_rows_are_the_views(ctx):
    """(c): rows with a = b = 0 give known_from_views and view_gain bit for bit."""
    import sea_current_amd as sc
    occ = _map("salt", 130, 70)
    views = _candidates(occ, 17)
    rows = sc.sector_views(views, sc.heading_dirs(8), 0, 8)
    base = (np.random.default_rng(8).random(occ.shape) < 0.1).astype(np.uint8)
    tocc, tb = _t(occ), _t(base)
    k1, s1 = ctx.known_from_sectors(_t(rows), tocc, base=tb, occ_seen=True)
    k2, s2 = ctx.known_from_views(_t(views), tocc, base=tb, occ_seen=True)
    _eq("known", k1.cpu().numpy(), k2.cpu().numpy())
    _eq("occ_seen", s1.cpu().numpy(), s2.cpu().numpy())
    _eq("gain", ctx.sector_gain(_t(rows), tocc, tb).cpu().numpy(), ctx.view_gain(_t(views), tocc, tb).cpu().numpy())
    assert k1.cpu().numpy().sum() > base.sum()


def test_views_from_cells(ctx):
    W, H = 130, 70
    cell = np.array([0, 129, 130, W * H - 1, -1, W * H, -2**31, 2**31 - 1, 35 * W + 64], np.int32)
    want = st.views_from_cells(cell, W, H, 100)
    _eq("views", ctx.views_from_cells(_t(cell), W, H, 100).cpu().numpy(), want)
    out = _t(np.full((9, 3), 7, np.int32))
    assert ctx.views_from_cells(_t(cell), W, H, 100, out=out) is out
    _eq("out", out.cpu().numpy(), want)
    _eq("host", ctx.views_from_cells_host(cell, W, H, 100), want)
    assert ctx.views_from_cells(_t(np.zeros(0, np.int32)), W, H, 100).shape == (0, 3)
    assert ctx.views_from_cells_host([], W, H, 100).shape == (0, 3)


def test_host_forms(ctx):
    occ = _map("salt", 130, 70)
    rows = _rows(occ, 17)
    base = (np.random.default_rng(8).random(occ.shape) < 0.1).astype(np.uint8)
    want, want_seen = st.known_from_sectors(base, occ, rows)
    _eq("known", ctx.known_from_sectors_host(rows, occ, base=base), want)
    k, s = ctx.known_from_sectors_host(rows, occ, base=base, occ_seen=True)
    _eq("known", k, want)
    _eq("occ_seen", s, want_seen)
    _eq("lists", ctx.known_from_sectors_host(rows.tolist(), occ), st.known_from_sectors(None, occ, rows)[0])
    _eq("gain", ctx.sector_gain_host(rows, occ, base), st.sector_gain(occ, base, rows))
    assert ctx.sector_gain_host(np.zeros((0, 7), np.int32), occ, base).shape == (0,)
    _eq("R = 0", ctx.known_from_sectors_host(np.zeros((0, 7), np.int32), occ, base=base), base)
    views = _candidates(occ, 64)
    dirs = st.heading_dirs(16, 0.5)
    tw = st.view_gain_headings(occ, base, views, dirs, 5)
    _eq("best", ctx.view_gain_headings_host(views, occ, base, dirs, 5), tw["best"])
    got = ctx.view_gain_headings_host(views, occ, base, dirs.tolist(), 5, hist=True, gainh=True)
    for key in ("hist", "gainh", "best"):
        _eq(key, got[key], tw[key])
    assert set(ctx.view_gain_headings_host(views, occ, base, dirs, 5, hist=True)) == {"best", "hist"}


def test_argument_errors(ctx):
    import sea_current_amd as sc
    l, h, p = ctx._l, ctx._h, sc._ptr
    occ, known, seen = (_t(np.zeros((8, 8), np.uint8)) for _ in range(3))
    rows, views, gain = _t(np.array([[4, 4, 9, 1, 0, 0, 1]], np.int32)), _t(np.array([[4, 4, 9]], np.int32)), _t(np.zeros(1, np.int32))
    INV = 1
    ks = lambda W=8, H=8, R=1, o=occ, v=rows, k=known, s=seen, b=None: l.sc_known_from_sectors(h, p(b), p(o), p(v), R, W, H, p(k), p(s))
    assert ks() == 0 and ks(s=None) == 0 and ks(b=known) == 0 and ks(R=0, v=None) == 0
    assert [ks(W=0), ks(H=0), ks(W=8193), ks(H=8193), ks(R=-1), ks(o=None), ks(v=None), ks(k=None), ks(s=occ), ks(s=known)] == [INV] * 10
    sg = lambda W=8, H=8, N=1, o=occ, k=known, v=rows, g=gain: l.sc_sector_gain_batch(h, p(o), p(k), p(v), N, W, H, p(g))
    assert sg() == 0 and sg(N=0, v=None, g=None) == 0
    assert [sg(W=0), sg(H=0), sg(W=8193), sg(H=8193), sg(N=-1), sg(o=None), sg(k=None), sg(v=None), sg(g=None)] == [INV] * 9
    good = st.heading_dirs(8)
    hist, gainh, best = _t(np.zeros((1, 8), np.int32)), _t(np.zeros((1, 8), np.int32)), _t(np.zeros((1, 2), np.int32))

    def vh(W=8, H=8, N=1, o=occ, k=known, v=views, d=good, B=None, span=2, hi=hist, gh=gainh, be=best):
        d = None if d is None else np.ascontiguousarray(d, dtype=np.int32)
        return l.sc_view_gain_headings_batch(h, p(o), p(k), p(v), N, W, H, p(d), (0 if d is None else len(d)) if B is None else B, span, p(hi), p(gh), p(be))

    assert vh() == 0 and vh(hi=None, gh=None) == 0 and vh(N=0, v=None, be=None) == 0 and vh(span=8) == 0 and vh(span=1) == 0
    assert [vh(W=0), vh(H=0), vh(W=8193), vh(H=8193), vh(N=-1), vh(o=None), vh(k=None), vh(v=None), vh(be=None)] == [INV] * 9
    assert [vh(span=0), vh(span=9), vh(d=None, B=8), vh(B=2), vh(d=st.heading_dirs(64), B=65)] == [INV] * 5
    swapped, repeated, far = good.copy(), good.copy(), good.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    repeated[1] = repeated[0]
    far[0] = (32768, 0)
    two_turns = st.heading_dirs(5)[(2 * np.arange(5)) % 5]
    assert [vh(d=good[::-1]), vh(d=swapped), vh(d=repeated), vh(d=far), vh(d=np.concatenate([good, good]), span=2), vh(d=two_turns)] == [INV] * 6
    assert vh(N=(1 << 30) // 8 + 1) == INV                                                # N * B > 2^30: refused before anything is touched
    cell, rows3 = _t(np.array([5], np.int32)), _t(np.zeros((1, 3), np.int32))
    vc = lambda W=8, H=8, N=1, c=cell, v=rows3: l.sc_views_from_cells(h, p(c), N, W, H, 9, p(v))
    assert vc() == 0 and vc(N=0, c=None, v=None) == 0
    assert [vc(W=0), vc(H=8193), vc(N=-1), vc(c=None), vc(v=None)] == [INV] * 5
    ctx.synchronize()
    o, k, s = (np.zeros((8, 8), np.uint8) for _ in range(3))
    r, v, g, b2 = np.array([[4, 4, 9, 1, 0, 0, 1]], np.int32), np.array([[4, 4, 9]], np.int32), np.zeros(1, np.int32), np.zeros((1, 2), np.int32)
    assert l.sc_known_from_sectors_host(h, None, p(o), p(r), 1, 8, 8, p(k), p(s)) == 0
    assert l.sc_known_from_sectors_host(h, None, p(o), p(r), 1, 8, 8, p(k), p(o)) == INV
    assert l.sc_known_from_sectors_host(h, None, p(o), p(r), 1, 8, 8, p(k), p(k)) == INV
    assert l.sc_sector_gain_batch_host(h, p(o), p(k), p(r), 1, 8, 0, p(g)) == INV and l.sc_sector_gain_batch_host(h, p(o), p(k), None, 1, 8, 8, p(g)) == INV
    assert l.sc_view_gain_headings_batch_host(h, p(o), p(k), p(v), 1, 8, 8, p(good), 8, 2, None, None, p(b2)) == 0
    assert l.sc_view_gain_headings_batch_host(h, p(o), p(k), p(v), 1, 8, 8, p(good), 8, 2, None, None, None) == INV
    assert l.sc_view_gain_headings_batch_host(h, p(o), p(k), p(v), 1, 8, 8, p(np.ascontiguousarray(good[::-1])), 8, 2, None, None, p(b2)) == INV
    assert l.sc_views_from_cells_host(h, None, 1, 8, 8, 9, p(v)) == INV


def test_the_goal_pose_chain_on_one_stream(ctx, oracle):
    """known_from_sectors(occ_seen=...) -> edt -> d2_known -> cost_fields -> fleet_explore -> views_from_cells ->
    view_gain_headings, one synchronise at the end; a fifth robot walled in has no goal and its row is ignored."""
    W, H = 130, 70
    occ = _map("salt", W, H).copy()
    robots = np.array([35 * W + 30, 35 * W + 65, 35 * W + 100, 30 * W + 60], np.int32)
    occ[robots // W, robots % W] = 0
    dirs = st.heading_dirs(16)
    rows = st.sector_views(np.stack([robots % W, robots // W, np.full(4, 400)], 1), dirs, [0, 4, 8, 12], 6)
    known, occ_seen = ctx.known_from_sectors(_t(rows), _t(occ), occ_seen=True)
    d2k = ctx.d2_known(ctx.edt(occ_seen), known)
    g = ctx.cost_fields(d2k, _t(robots))["g"]
    ex = ctx.fleet_explore(d2k, known, g, Cmax=64)
    poses = ctx.views_from_cells(ex["goal"], W, H, 100)
    res = ctx.view_gain_headings(poses, occ_seen, known, dirs, 4, gainh=True)
    lost = ctx.view_gain_headings(ctx.views_from_cells(_t(np.array([-1, 5], np.int32)), W, H, 100), occ_seen, known, dirs, 4)
    ctx.synchronize()
    kn, seen = st.known_from_sectors(None, occ, rows)
    _eq("known", known.cpu().numpy(), kn)
    _eq("occ_seen", occ_seen.cpu().numpy(), seen)
    wd2k = ft.d2_known(oracle.edt(seen), kn)
    _eq("d2k", d2k.cpu().numpy(), wd2k)
    want = ft.fleet_explore(wd2k, kn, g.cpu().numpy(), Cmax=64)
    _eq("goal", ex["goal"].cpu().numpy(), want["goal"])
    assert (want["goal"] >= 0).all()
    wposes = st.views_from_cells(want["goal"], W, H, 100)
    _eq("poses", poses.cpu().numpy(), wposes)
    tw = st.view_gain_headings(seen, kn, wposes, dirs, 4)
    _eq("best", res["best"].cpu().numpy(), tw["best"])
    _eq("gainh", res["gainh"].cpu().numpy(), tw["gainh"])
    assert (tw["best"][:, 0] > 0).all()                               # a frontier goal always has something to see
    assert lost.cpu().numpy()[0].tolist() == [0, 0]


def test_more_tiles_than_workgroups(ctx, ref):
    """One view covering 1000 x 700: 2 772 tiles for 2 048 workgroups in the sector view kernel, and 64 workgroups per
    candidate in the two gain kernels: the strided tile loop with skipped tiles in it.  Against the C statement."""
    from sea_current_amd import synth
    W, H = 1000, 700
    occ = synth.block_grid(W, H, 0.15, seed=3, smin=3, smax=24)
    occ[H // 2, W // 2] = occ[40, 900] = 0
    dirs = st.heading_dirs(16, 0.123)
    views = np.array([(W // 2, H // 2, W * W + H * H), (900, 40, 900)], np.int32)
    rows = np.concatenate([st.sector_views(views, dirs, 3, 5), st.sector_views(views[:1], dirs, 9, 11)])
    tocc, trows = _t(occ), _t(rows)
    zero = np.zeros_like(occ)
    known, occ_seen = ctx.known_from_sectors(trows, tocc, occ_seen=True)
    gain = ctx.sector_gain(trows, tocc, _t(zero))
    got = ctx.view_gain_headings(_t(views), tocc, _t(zero), dirs, 5, hist=True, gainh=True)
    ctx.synchronize()
    want_known, want_seen = ref.known_from_sectors(None, occ, rows)
    _eq("known", known.cpu().numpy(), want_known)
    _eq("occ_seen", occ_seen.cpu().numpy(), want_seen)
    _eq("gain", gain.cpu().numpy(), ref.sector_gain(occ, zero, rows))
    want = ref.view_gain_headings(occ, zero, views, dirs, 5)
    for key in ("hist", "gainh", "best"):
        _eq(key, got[key].cpu().numpy(), want[key])
    assert want["gainh"][0, 3] == gain.cpu().numpy()[0] and 10000 < want_known.sum() < W * H


LOOP_COUNTS = {"blocks96x80": (189, 0), "rooms96x80": (229, 0)}     # the twin's (iterations, full-circle fallbacks)


@pytest.mark.parametrize("name", ["blocks96x80", "rooms96x80"])
def test_exploration_loop_visits_the_twins_goals(ctx, oracle, fields, name):
    occ = vt.loop_maps()[name]
    start = ft.loop_start(occ)
    tocc = _t(occ)
    dirs = st.heading_dirs(16)

    def gpu_sense(base, occ_, rows):
        known, occ_seen = ctx.known_from_sectors(_t(np.array(rows, np.int32)), tocc, base=_t(base), occ_seen=True)
        return known.cpu().numpy(), occ_seen.cpu().numpy()

    def gpu_best(views, occ_seen, known):
        return ctx.view_gain_headings(_t(views), _t(occ_seen), _t(known), dirs, 4).cpu().numpy()

    def gpu_step(occ_seen, known, pos):
        tk = _t(known)
        d2k = ctx.d2_known(ctx.edt(_t(occ_seen)), tk)
        g = ctx.cost_fields(d2k, _t(np.array([pos], np.int32)))["g"]
        goal = ctx.fleet_explore(d2k, tk, g, Cmax=256)["goal"]
        ctx.synchronize()
        return int(goal.cpu().numpy()[0])

    got = st.explore_loop_sectors(occ, start, gpu_step, dirs, 4, sense=gpu_sense, best=gpu_best)
    want = st.explore_loop_sectors(occ, start, ft.twin_step(oracle, fields), dirs, 4)
    assert got["goals"] == want["goals"] and got["headings"] == want["headings"] and got["fallbacks"] == want["fallbacks"]
    assert np.array_equal(got["known"], want["known"]) and (len(want["goals"]), want["fallbacks"]) == LOOP_COUNTS[name]
    assert (got["known"][ft.true_component(occ, start)] != 0).all()
