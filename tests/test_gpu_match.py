"""sc_scan_match_batch on the GPU: best and the volume bit-equal to the NumPy twin (tests/match_twin.py) at the smallest shapes
where the kernels can go wrong -- 64 x 64, 65 x 63 and 130 x 70; 1, 63, 64, 65 and 257 points (a wave takes 4 points a round, a
workgroup 16); 1, 3 and 4 rotations; 1, 2 and 5 scans with different centres; windows of 1, 3, 121, 67 x 5 (a row wider than a
wave), 5 x 67 and 129 x 129 candidates (one tile of 256 candidates, part of one, 66 of them); windows partly and wholly outside
the grid, a centre outside the grid; an ignored scan between two live ones; absent points, all of them and at points 0, 63 and
64; both builds of the score kernel on either side of the threshold between them; known NULL and given, unk 0 and = d2_cap, cap 1 and 32767, the empty grid, the int32 bound; score NULL and given; a reused
best; grids of changing size; the host form; every argument error; the binding's size checks; the chain on one stream; the
corrected walk; one larger case against the C statement."""
import numpy as np
import pytest

import frontier_twin as ft
import match_twin as mt
import scan_twin as st
import views_twin as vt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mt.Ref(tmp_path_factory.mktemp("match_ref"))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _eq(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{name}: {len(bad)} differ, first at {bad[0].tolist()}: gpu {got[tuple(bad[0])]} twin {want[tuple(bad[0])]}")


def _check(ctx, d2, known, pts, centre, wx, wy, cap, unk, want=None):
    """best and score of the GPU == the twin's, with the volume and without it; returns the twin's (best, score)."""
    pts = np.ascontiguousarray(pts, dtype=np.int32)
    centre = np.ascontiguousarray(centre, dtype=np.int32).reshape(-1, 2)
    td2, tk, tp, tc = _t(d2), None if known is None else _t(known), _t(pts), _t(centre)
    best, score = ctx.scan_match(tp, tc, td2, known=tk, wx=wx, wy=wy, d2_cap=cap, unk=unk, score=True)
    alone = ctx.scan_match(tp, tc, td2, known=tk, wx=wx, wy=wy, d2_cap=cap, unk=unk)
    ctx.synchronize()
    want = want or mt.match(d2, known, pts, centre, wx, wy, cap, unk)
    _eq("score", score.cpu().numpy(), want[1])
    _eq("best", best.cpu().numpy(), want[0])
    _eq("best without the volume", alone.cpu().numpy(), want[0])
    return want


def _map(kind, W, H):
    from sea_current_amd import synth
    return synth.block_grid(W, H, 0.3, seed=10, smin=3, smax=24) if kind == "blocks" else synth.salt_grid(W, H, 0.05, seed=3)


def _free_near(occ, x, y):
    H, W = occ.shape
    free = np.flatnonzero(occ.ravel() == 0)
    c = int(free[np.argmin((free % W - x) ** 2 + (free // W - y) ** 2)])
    return c % W, c // W


def _points(occ, x, y, n, seed=0):
    """n points of a scan from (x, y): the hits of a fan of half-side 20 (no-return beams stay absent), repeated or cut to n,
    every one moved by up to a cell so that no pose scores 0 and the sums are not trivial."""
    rays = st.square_fan(x, y, 20)
    p = mt.points_from_hits(rays, st.cast(occ, rays), occ.shape[1])
    p = p[np.arange(n) % len(p)].astype(np.int64)
    jitter = np.random.default_rng(seed).integers(-1, 2, p.shape)
    return np.where(mt.present(p)[:, None], p + jitter, mt.ABSENT).astype(np.int32)


def _scans(occ, S, R, N):
    """pts [S,R,N,2] and centre [S,2]: scans from different free cells, rotation r a turn by r quarter turns."""
    H, W = occ.shape
    at = [(W // 2, H // 2), (3, 2), (W - 2, H - 3), (W // 4, H - 1), (W - 1, 0)]
    pts, centre = [], []
    for s in range(S):
        x, y = _free_near(occ, *at[s])
        p = _points(occ, x, y, N, seed=s)
        pts.append(np.stack([mt.quarter_turns(p, r) for r in range(R)]))
        centre.append((x + s - 1, y + 1 - s))
    return np.stack(pts), np.array(centre, np.int32)


WINDOWS = [(0, 0), (1, 0), (0, 1), (5, 5), (33, 2), (2, 33)]


@pytest.mark.parametrize("kind", ["blocks", "salt"])
@pytest.mark.parametrize("W,H", [(64, 64), (65, 63), (130, 70)])
def test_maps_equal_the_twin(ctx, oracle, W, H, kind):
    occ = _map(kind, W, H)
    d2 = oracle.edt(occ)
    known = (np.random.default_rng(5).random((H, W)) < 0.8).astype(np.uint8)
    for i, (wx, wy) in enumerate(WINDOWS):
        S, R, N = [(1, 1, 1), (2, 3, 63), (5, 4, 64), (1, 3, 65), (2, 1, 257), (5, 4, 257)][i]
        pts, centre = _scans(occ, S, R, N)
        want = _check(ctx, d2, known if i % 2 else None, pts, centre, wx, wy, 64, 1)
        assert want[1].any()


def test_every_point_count_and_rotation_count(ctx, oracle):
    occ = _map("blocks", 65, 63)
    d2 = oracle.edt(occ)
    for N in (1, 63, 64, 65, 257):
        for R in (1, 3, 4):
            pts, centre = _scans(occ, 2, R, N)
            _check(ctx, d2, None, pts, centre, 5, 5, 64, 1)


def test_both_builds_of_the_score_kernel(ctx, oracle):
    """A launch of fewer than 512 workgroups shares a tile's points among 16 wavefronts, a larger one among 4: 256, 511, 512
    and 1320 workgroups (S R tiles of 256 candidates), with points inside the grid over the whole window and points near
    its edge in one scan, so that both ways to index a cell run in both."""
    occ = _map("salt", 65, 63)
    d2 = oracle.edt(occ)
    rng = np.random.default_rng(12)
    for S, R, wx, wy in ((1, 256, 1, 1), (7, 73, 2, 0), (2, 256, 1, 1), (5, 4, 64, 64)):
        N = 8 if wx == 64 else 37
        pts = rng.integers(-30, 31, (S, R, N, 2)).astype(np.int32)
        pts[:, :, ::5] //= 4                                            # every fifth point stays near the sensor
        pts[:, R // 2, 3] = mt.ABSENT
        centre = np.stack([rng.integers(25, 40, S), rng.integers(25, 38, S)], 1).astype(np.int32)
        tiles = -(-(2 * wx + 1) * (2 * wy + 1) // 256)
        assert S * R * tiles in (256, 511, 512, 1320)
        _check(ctx, d2, None, pts, centre, wx, wy, 64, 1)


def test_the_largest_window(ctx, oracle):
    occ = _map("salt", 130, 70)
    d2 = oracle.edt(occ)
    pts, centre = _scans(occ, 1, 1, 8)
    best, score = _check(ctx, d2, None, pts, centre, 64, 64, 64, 1)    # 129 x 129 candidates: most of the window is off the grid
    assert score.shape == (1, 1, 129, 129)


def test_windows_and_centres_outside_the_grid(ctx, oracle):
    occ = _map("blocks", 65, 63)
    H, W = occ.shape
    d2 = oracle.edt(occ)
    pts, _ = _scans(occ, 5, 3, 65)
    # partly outside on two sides; wholly outside (the points too: unk each); a centre outside, its window reaching in; the
    # far corner; the ends of the centre's range
    centre = [(2, 1), (-40, -40), (-3, H + 2), (W + 4, H - 1), (-mt.MAX_REACH, mt.MAX_DIM + mt.MAX_REACH)]
    best, score = _check(ctx, d2, None, pts, centre, 5, 5, 64, 3)
    n1 = int(mt.present(pts[1, 0]).sum())
    assert best[1].tolist() == [0, 0, 0, 3 * n1, n1, 3 * 121] and (best[:, 0] >= 0).all()


def test_an_ignored_scan_between_two_live_ones(ctx, oracle):
    occ = _map("salt", 64, 64)
    d2 = oracle.edt(occ)
    pts, centre = _scans(occ, 3, 3, 64)
    for bad in ((-mt.MAX_REACH - 1, 5), (5, mt.MAX_DIM + mt.MAX_REACH + 1), (2**31 - 1, -2**31)):
        centre[1] = bad
        best, score = _check(ctx, d2, None, pts, centre, 5, 5, 64, 1)
        assert best[1].tolist() == [mt.IGNORED, 0, 0, 0, 0, 0] and not score[1].any() and score[0].any() and score[2].any()


def test_absent_points(ctx, oracle):
    occ = _map("blocks", 130, 70)
    d2 = oracle.edt(occ)
    pts, centre = _scans(occ, 2, 3, 257)
    none = np.full_like(pts, mt.ABSENT)
    best, score = _check(ctx, d2, None, none, centre, 5, 5, 64, 1)
    assert best.tolist() == [[0, 0, 0, 0, 0, 3 * 121]] * 2 and not score.any()
    # points 0, 63 and 64 absent, each kind; then only those present
    full = np.stack([np.stack([np.where(mt.present(p)[:, None], p, (1, 2)) for p in s]) for s in pts]).astype(np.int32)
    some = full.copy()
    some[:, :, 0], some[:, :, 63], some[:, :, 64] = (mt.ABSENT, 0), (mt.MAX_REACH + 1, 0), (0, -mt.MAX_REACH - 1)
    best = _check(ctx, d2, None, some, centre, 5, 5, 64, 1)[0]
    assert (best[:, 4] == 254).all()
    few = none.copy()
    few[:, :, [0, 63, 64]] = full[:, :, [0, 63, 64]]
    assert (_check(ctx, d2, None, few, centre, 5, 5, 64, 1)[0][:, 4] == 3).all()
    # rotations with different numbers of points are compared as they are: the one that lost its points wins with 0
    mixed = full.copy()
    mixed[:, 2] = mt.ABSENT
    assert (_check(ctx, d2, None, mixed, centre, 5, 5, 64, 1)[0][:, [0, 3, 4]] == [2, 0, 0]).all()


def test_known_unk_and_cap(ctx, oracle):
    occ = _map("salt", 65, 63)
    H, W = occ.shape
    d2 = oracle.edt(occ)
    known = (np.random.default_rng(6).random((H, W)) < 0.5).astype(np.uint8)
    pts, centre = _scans(occ, 2, 3, 65)
    a = _check(ctx, d2, None, pts, centre, 5, 5, 64, 1)
    b = _check(ctx, d2, np.ones((H, W), np.uint8), pts, centre, 5, 5, 64, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))            # known NULL == all ones
    for cap, unk in ((64, 0), (64, 64), (1, 0), (1, 1), (32767, 0), (32767, 32767), (32767, 9)):
        _check(ctx, d2, known, pts, centre, 5, 5, cap, unk)
    # a grid without obstacles: every known cell costs the cap
    empty = np.full((H, W), mt.EDT_INF, np.int32)
    best, score = _check(ctx, empty, known, pts, centre, 5, 5, 32767, 2)
    assert score.max() > 32767
    _check(ctx, empty, None, pts, centre, 5, 5, 64, 1)


def test_int32_bound(ctx):
    N = mt.MAX_POINTS
    k = np.arange(N)
    pts = np.stack([k % 8 - 3, (k // 8) % 8 - 3], 1).astype(np.int32)[None, None]
    d2 = np.full((8, 8), mt.EDT_INF, np.int32)
    best, score = _check(ctx, d2, None, pts, [(3, 3)], 0, 0, 32767, 0)
    assert best[0].tolist() == [0, 0, 0, 2147418112, N, 1] and score.ravel().tolist() == [2147418112]


@pytest.mark.parametrize("shape", [(1, 200), (200, 1)])
def test_lines(ctx, oracle, shape):
    occ = np.zeros(shape, np.uint8)
    occ.ravel()[[80, 150]] = 1
    d2 = oracle.edt(occ)
    along = np.array([(-20, 0), (50, 0), (3, 0)], np.int32)            # the two obstacles seen from cell 100, and a stray point
    pts = (along if shape[0] == 1 else along[:, ::-1])[None, None]
    c = (103, 0) if shape[0] == 1 else (0, 103)
    best = _check(ctx, d2, None, pts, [c], 5, 5, 64, 64)[0]          # unk = cap: leaving the line is no way to score less
    assert best[0, 1:3].tolist() == ([-3, 0] if shape[0] == 1 else [0, -3])


def test_a_reused_best_and_grids_of_changing_size(ctx, oracle):
    import torch
    out = torch.full((2, 6), 77, dtype=torch.int32, device="cuda")
    vol = torch.full((2, 3, 11, 11), 77, dtype=torch.int32, device="cuda")
    for W, H in ((130, 70), (64, 64), (65, 63), (130, 70), (8, 8)):    # the cost map's scratch is larger than the later grids need
        occ = _map("salt", W, H)
        d2 = oracle.edt(occ)
        pts, centre = _scans(occ, 2, 3, 65)
        b, s = ctx.scan_match(_t(pts), _t(centre), _t(d2), wx=5, wy=5, out=out, score=vol)
        assert b is out and s is vol
        ctx.synchronize()
        want = mt.match(d2, None, pts, centre, 5, 5, 64, 1)
        _eq("best", out.cpu().numpy(), want[0])
        _eq("score", vol.cpu().numpy(), want[1])


def test_host_form(ctx, oracle):
    import sea_current_amd as sc
    occ = _map("blocks", 65, 63)
    H, W = occ.shape
    d2 = oracle.edt(occ)
    known = (np.random.default_rng(7).random((H, W)) < 0.8).astype(np.uint8)
    pts, centre = _scans(occ, 2, 3, 65)
    want = mt.match(d2, known, pts, centre, 4, 6, 50, 2)
    _eq("best", ctx.scan_match_host(pts, centre, d2, known, wx=4, wy=6, d2_cap=50, unk=2), want[0])
    best, score = ctx.scan_match_host(pts.tolist(), centre.tolist(), d2.tolist(), known.tolist(), wx=4, wy=6, d2_cap=50, unk=2, score=True)
    _eq("best", best, want[0])
    _eq("score", score, want[1])
    _eq("defaults", ctx.scan_match_host(pts, centre, d2), mt.match(d2, None, pts, centre, 8, 8, 64, 1)[0])
    assert ctx.scan_match_host(np.zeros((0, 1, 1, 2), np.int32), np.zeros((0, 2), np.int32), d2).shape == (0, 6)
    with pytest.raises(sc.SeaCurrentError):                            # the host form refuses an ignored centre
        ctx.scan_match_host(pts, [(0, 0), (-mt.MAX_REACH - 1, 0)], d2)


def test_argument_errors(ctx):
    import sea_current_amd as sc
    l, h, p = ctx._l, ctx._h, sc._ptr
    INV = 1
    d2, known = _t(np.ones((8, 8), np.int32)), _t(np.ones((8, 8), np.uint8))
    pts, centre = _t(np.zeros((1, 1, 1, 2), np.int32)), _t(np.array([[4, 4]], np.int32))
    best, score = _t(np.zeros((1, 6), np.int32)), _t(np.zeros(9, np.int32))
    f = lambda name="sc_scan_match_batch", d=d2, k=known, q=pts, c=centre, S=1, R=1, N=1, W=8, H=8, wx=1, wy=1, cap=64, unk=1, b=best, v=score: getattr(
        l, name)(h, p(d), p(k), p(q), p(c), S, R, N, W, H, wx, wy, cap, unk, p(b), p(v))
    assert f() == 0 and f(k=None) == 0 and f(v=None) == 0 and f(S=0) == 0
    assert f(wx=0, wy=0) == 0 and f(cap=1, unk=0) == 0 and f(cap=32767, unk=32767) == 0
    bad = [f(d=None), f(q=None), f(c=None), f(b=None), f(S=-1), f(R=0), f(R=257), f(N=0), f(N=65537), f(W=0), f(H=0), f(W=8193), f(H=8193),
           f(wx=-1), f(wy=-1), f(wx=65), f(wy=65), f(cap=0), f(cap=32768), f(unk=-1), f(unk=65), f(v=best)]
    assert bad == [INV] * len(bad)
    ctx.synchronize()
    hd, hk = np.ones((8, 8), np.int32), np.ones((8, 8), np.uint8)
    hq, hc, hb, hv = np.zeros((1, 1, 1, 2), np.int32), np.array([[4, 4]], np.int32), np.zeros((1, 6), np.int32), np.zeros(9, np.int32)
    g = lambda **kw: f(**dict(dict(name="sc_scan_match_batch_host", d=hd, k=hk, q=hq, c=hc, b=hb, v=hv), **kw))
    assert g() == 0 and hb[0].tolist() == [0, 0, 0, 1, 1, 9] and hv.tolist() == [1] * 9
    assert g(k=None, v=None) == 0 and g(S=0) == 0
    bad = [g(d=None), g(q=None), g(c=None), g(b=None), g(S=-1), g(R=0), g(N=0), g(W=8193), g(wx=65), g(cap=0), g(unk=65), g(v=hb),
           g(c=np.array([[-16385, 0]], np.int32)), g(c=np.array([[0, 8192 + 16385]], np.int32))]
    assert bad == [INV] * len(bad)


def test_binding_checks_sizes(ctx):
    import sea_current_amd as sc
    d2 = _t(np.ones((4, 8), np.int32))
    pts, centre = _t(np.zeros((2, 3, 5, 2), np.int32)), _t(np.array([[4, 2], [1, 1]], np.int32))
    ok = lambda **kw: ctx.scan_match(**dict(dict(pts=pts, centre=centre, d2=d2, wx=1, wy=2), **kw))
    b, s = ok(score=True)
    assert b.shape == (2, 6) and s.shape == (2, 3, 5, 3)
    i32 = lambda *shape: _t(np.zeros(shape, np.int32))
    for kw in (dict(known=_t(np.ones((4, 7), np.uint8))), dict(out=i32(1, 6)), dict(score=i32(2, 3, 5, 2)), dict(centre=i32(3, 2)),
               dict(pts=i32(2, 3, 5)), dict(pts=i32(2, 3, 5, 3)), dict(d2=i32(32))):
        with pytest.raises(sc.SeaCurrentError):
            ok(**kw)
    with pytest.raises(sc.SeaCurrentError):
        ctx.scan_match_host(np.zeros((1, 1, 1, 2), np.int32), [(1, 1), (2, 2)], np.ones((4, 8), np.int32))
    ctx.synchronize()


def test_the_chain_on_one_stream(ctx, oracle):
    """scan_cast -> logodds_update(occ_est, known) -> edt(occ_est) -> scan_match, one synchronise at the end.  The points are
    made on the host (points_from_hits takes the hits there), so they come from the twin's cast and are uploaded before the
    chain starts; that the GPU's cast gave the same hits is checked after the synchronise."""
    import sea_current_amd as sc
    W, H = 130, 70
    occ = _map("salt", W, H)
    ax, ay = _free_near(occ, 60, 35)
    first, second = st.square_fan(ax, ay, 20), st.square_fan(ax + 2, ay - 1, 20)
    occ[ay - 1, ax + 2] = 0
    pts = sc.points_from_hits(second, st.cast(occ, second), W)[None, None]
    tp, tc = _t(pts), _t(np.array([[ax + 4, ay + 1]], np.int32))       # the second pose, believed two cells off each way
    tfirst, tsecond, tocc = _t(first), _t(second), _t(occ)
    hit1 = ctx.scan_cast(tfirst, tocc)
    L, occ_est, known = ctx.logodds_update(tfirst, hit1, W, H, occ_est=True, known=True, **st.LOOP_PARAMS)
    hit2 = ctx.scan_cast(tsecond, tocc)
    best, score = ctx.scan_match(tp, tc, ctx.edt(occ_est), known=known, wx=3, wy=3, d2_cap=16, unk=1, score=True)
    ctx.synchronize()
    _eq("hit", hit2.cpu().numpy(), st.cast(occ, second))
    wl, we, wk = st.update(None, first, st.cast(occ, first), W, H, **st.LOOP_PARAMS)
    _eq("occ_est", occ_est.cpu().numpy(), we)
    _eq("known", known.cpu().numpy(), wk)
    want = mt.match(oracle.edt(we), wk, pts, [(ax + 4, ay + 1)], 3, 3, 16, 1)
    _eq("best", best.cpu().numpy(), want[0])
    _eq("score", score.cpu().numpy(), want[1])
    assert want[0][0].tolist()[:3] == [0, -2, -2] and want[0][0, 5] == 1          # and the pose is found


def test_the_corrected_walk_takes_the_twins_poses(ctx, oracle):
    occ = vt.salt(mt.WALK["W"], mt.WALK["H"], mt.WALK["p"], mt.WALK["seed"])
    start = ft.loop_start(occ)
    steps = []

    def matcher(d2, known, pts, centre, wx, wy, cap, unk):
        pts, centre = np.ascontiguousarray(pts, dtype=np.int32), np.array(centre, np.int32)
        best = ctx.scan_match(_t(pts), _t(centre), _t(d2), known=_t(known), wx=wx, wy=wy, d2_cap=cap, unk=unk).cpu().numpy()
        _eq("best at step %d" % len(steps), best, mt.match(d2, known, pts, centre, wx, wy, cap, unk)[0])
        steps.append(best)
        return best

    got = mt.walk(occ, start, oracle.edt, corrected=True, unk=1, matcher=matcher)
    assert got == dict(exact=33, unique=32, steps=33, sound=True) and len(steps) == 32


def test_a_larger_case_equals_the_c_statement(ctx, ref):
    """1000 x 700 blocks, one fan of half-side 300 from the middle, 16 rotations, window +-16: 17 424 candidates of up to
    2 400 points each."""
    import sea_current_amd as sc
    from sea_current_amd import synth
    occ = synth.block_grid(1000, 700, 0.2, seed=3, smin=4, smax=40)
    H, W = occ.shape
    x, y = _free_near(occ, 500, 350)
    rays = st.square_fan(x, y, 300)
    tocc = _t(occ)
    hit = ctx.scan_cast(_t(rays), tocc)
    d2 = ctx.edt(tocc)
    ctx.synchronize()
    p = sc.points_from_hits(rays, hit.cpu().numpy(), W)
    assert 1000 < int(mt.present(p).sum()) < len(p)
    pts = sc.rotate_points(p, np.arange(16) * (2 * np.pi / 16))[None]
    pts = np.ascontiguousarray(np.roll(pts, 3, axis=1))                # the unturned scan is rotation 3
    centre = np.array([[x + 9, y - 13]], np.int32)
    known = (np.random.default_rng(9).random((H, W)) < 0.97).astype(np.uint8)
    best, score = ctx.scan_match(_t(pts), _t(centre), d2, known=_t(known), wx=16, wy=16, d2_cap=64, unk=1, score=True)
    ctx.synchronize()
    want = ref.match(d2.cpu().numpy(), known, pts, centre, 16, 16, 64, 1)
    _eq("best", best.cpu().numpy(), want[0])
    _eq("score", score.cpu().numpy(), want[1])
    assert want[0][0, :3].tolist() == [3, -9, 13]
