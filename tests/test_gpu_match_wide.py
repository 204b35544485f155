"""sc_scan_match_wide_batch on the GPU: best and stats bit-equal to the NumPy twin (tests/match_wide_twin.py), and best equal
to Context.scan_match where the dense call can run (windows up to +-64), at the smallest shapes where the kernels can go
wrong -- grids 64 x 64, 65 x 63, 130 x 70 and 256 x 192; 1, 15, 16, 17, 63, 64, 65 and 257 points (a dive splits the points
into 16 slices, the bound kernel takes 4 a round); 1, 3 and 4 rotations; 1, 2 and 5 scans with different centres; absent
points at 0, 15 and 16; windows from a single candidate to +-100 x +-70 with top 0 .. 3, +-2048 x 0 with top 5; a parent list
that the bound kernel's grid strides over more than once, and one that is one short of a wave's four parents; the overflow
pair; ignored scans, all points absent, windows partly and wholly outside the grid, known NULL and given; stats NULL and
given; a reused best; grids of changing size; the host form; every argument error; the binding's size checks; the chain on
one stream; the kidnapped robot; one larger case against the C statement."""
import numpy as np
import pytest

import match_twin as mt
import match_wide_cases as mc
import match_wide_twin as mw
import scan_twin as st

pytestmark = pytest.mark.gpu

NODES = 1 << 17


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mw.Ref(tmp_path_factory.mktemp("match_wide_ref"))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _eq(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{name}: {len(bad)} differ, first at {bad[0].tolist()}: gpu {got[tuple(bad[0])]} twin {want[tuple(bad[0])]}\n"
                             f"gpu {got.tolist()}\ntwin {want.tolist()}")


def _check(ctx, d2, known, pts, centre, wx, wy, cap, unk, top, max_nodes=NODES):
    """best and stats of the GPU == the twin's, with stats and without; best == the dense call's where it can run.  Returns
    the twin's (best, stats)."""
    pts = np.ascontiguousarray(pts, dtype=np.int32)
    centre = np.ascontiguousarray(centre, dtype=np.int32).reshape(-1, 2)
    td2, tk, tp, tc = _t(d2), None if known is None else _t(known), _t(pts), _t(centre)
    kw = dict(known=tk, wx=wx, wy=wy, d2_cap=cap, unk=unk)
    best, stats = ctx.scan_match_wide(tp, tc, td2, top=top, max_nodes=max_nodes, stats=True, **kw)
    alone = ctx.scan_match_wide(tp, tc, td2, top=top, max_nodes=max_nodes, **kw)
    dense = ctx.scan_match(tp, tc, td2, **kw) if wx <= mt.MAX_HALF and wy <= mt.MAX_HALF else None
    ctx.synchronize()
    want = mw.match_wide(d2, known, pts, centre, wx, wy, cap, unk, top, max_nodes)
    what = f" (window {wx} x {wy}, top {top}, pts {pts.shape})"
    _eq("stats" + what, stats.cpu().numpy(), want[1])
    _eq("best" + what, best.cpu().numpy(), want[0])
    _eq("best without stats" + what, alone.cpu().numpy(), want[0])
    if dense is not None and not (want[0][:, 0] == mw.OVERFLOW).any():
        _eq("best of the dense call" + what, dense.cpu().numpy(), want[0])
    return want


def _map(kind, W, H):
    from sea_current_amd import synth
    return synth.block_grid(W, H, 0.3, seed=10, smin=3, smax=24) if kind == "blocks" else synth.salt_grid(W, H, 0.05, seed=3)


def _points(occ, x, y, n, seed=0):
    """n points of a scan from (x, y): the hits of a fan of half-side 20 (no-return beams stay absent), repeated or cut to n,
    every one moved by up to a cell so that no pose scores 0 and the sums are not trivial."""
    p = mc.scan_points(occ, x, y, 20)
    p = p[np.arange(n) % len(p)].astype(np.int64)
    jitter = np.random.default_rng(seed).integers(-1, 2, p.shape)
    return np.where(mt.present(p)[:, None], p + jitter, mt.ABSENT).astype(np.int32)


def _scans(occ, S, R, N):
    """pts [S,R,N,2] and centre [S,2]: scans from different free cells, rotation r a turn by r quarter turns, priors off."""
    H, W = occ.shape
    at = [(W // 2, H // 2), (3, 2), (W - 2, H - 3), (W // 4, H - 1), (W - 1, 0)]
    pts, centre = [], []
    for s in range(S):
        x, y = mc.free_near(occ, *at[s])
        p = _points(occ, x, y, N, seed=s)
        pts.append(np.stack([mt.quarter_turns(p, r) for r in range(R)]))
        centre.append((x + 3 * s - 2, y + 2 - s))
    return np.stack(pts), np.array(centre, np.int32)


WINDOWS = [(0, 0), (1, 0), (3, 3), (4, 4), (5, 2), (33, 2), (64, 64), (100, 70)]
SHAPES = [(1, 1, 1), (2, 3, 15), (5, 4, 16), (1, 3, 17), (2, 1, 63), (5, 4, 64), (1, 1, 65), (2, 3, 257)]   # S, R, N


@pytest.mark.parametrize("kind", ["blocks", "salt"])
@pytest.mark.parametrize("W,H", [(64, 64), (65, 63), (130, 70), (256, 192)])
def test_maps_equal_the_twin(ctx, oracle, W, H, kind):
    occ = _map(kind, W, H)
    d2 = oracle.edt(occ)
    known = (np.random.default_rng(5).random((H, W)) < 0.8).astype(np.uint8)
    g = [64, 65, 130, 256].index(W) + 4 * (kind == "salt")
    for i, (wx, wy) in enumerate(WINDOWS):
        S, R, N = SHAPES[(i + g) % 8]
        if (wx, wy) == (64, 64):
            S = min(S, 2)                                              # the twin bounds every candidate at top 0
        pts, centre = _scans(occ, S, R, N)
        _check(ctx, d2, known if (i + g) % 2 else None, pts, centre, wx, wy, 64, 1, (i + g) % 4)


def test_every_window_with_every_top(ctx, oracle):
    occ = _map("blocks", 130, 70)
    d2 = oracle.edt(occ)
    pts, centre = _scans(occ, 2, 3, 65)
    for wx, wy in WINDOWS:
        for top in range(4):
            _check(ctx, d2, None, pts[:, :1 + 2 * (wx < 64)], centre, wx, wy, 64, 1, top)


def test_every_point_count_and_rotation_count(ctx, oracle):
    occ = _map("salt", 65, 63)
    d2 = oracle.edt(occ)
    for N in (1, 15, 16, 17, 63, 64, 65, 257):
        for R in (1, 3, 4):
            pts, centre = _scans(occ, 2, R, N)
            _check(ctx, d2, None, pts, centre, 9, 6, 64, 1, 2)


def test_top_5_on_a_line(ctx, oracle):
    occ = mc.line()
    d2 = oracle.edt(occ)
    pts = np.full((1, 1, 8, 2), mt.ABSENT, np.int32)
    pts[0, 0, :5] = [(-20, 0), (50, 0), (3, 0), (-21, 0), (52, 0)]
    best = _check(ctx, d2, None, pts, [(100 - 1700, 0)], 2048, 0, 64, 64, 5, max_nodes=4096)[0]
    assert best[0, :3].tolist() == [0, 1700, 0] and best[0, 5] == 1
    _check(ctx, np.ascontiguousarray(d2.T), None, pts[..., ::-1], [(0, 100 + 900)], 0, 2048, 64, 64, 5, max_nodes=4096)


def test_list_lengths(ctx, oracle):
    """top 0 over +-100 x +-70 and 4 rotations: 7 344 parents, more than the 4 096 a sweep of the bound kernel's grid takes
    for one scan; 3 rotations of a window smaller than a node: 3 parents, one short of a wave's four."""
    occ = _map("salt", 256, 192)
    d2 = oracle.edt(occ)
    pts, centre = _scans(occ, 1, 4, 17)
    stats = _check(ctx, d2, None, pts, centre, 100, 70, 64, 1, 0)[1]
    assert stats[0, 0] == 4 * 201 * 141 and -(-201 // 4) * -(-141 // 4) * 4 == 7344
    stats = _check(ctx, d2, None, pts[:, :3], centre, 3, 3, 64, 1, 1)[1]
    assert stats[0, 1] == 3 * 4
    _check(ctx, d2, None, pts[:, :3], centre, 3, 3, 64, 1, 3)


def test_overflow_pair(ctx):
    d2, known, pts, centre, n = mc.overflow_case()
    best, stats = _check(ctx, d2, known, pts, centre, 20, 20, 64, 1, 2, max_nodes=1024)
    assert best[0].tolist() == [mw.OVERFLOW, 0, 0, 0, 0, 0] and stats[0, :3].tolist() == [0, 121, 9]
    best, stats = _check(ctx, d2, known, pts, centre, 20, 20, 64, 1, 2, max_nodes=2048)
    assert best[0].tolist() == [0, 0, 0, 8, 8, n] and stats[0, 0] == n
    # an overflowing scan between two that do not: a known grid of many costs, the middle scan's points far outside it
    three = np.concatenate([pts, pts + 1000, pts])
    varied = np.random.default_rng(2).integers(1, 60, d2.shape).astype(np.int32)
    varied[centre[0, 1] + pts[0, 0, :, 1], centre[0, 0] + pts[0, 0, :, 0]] = 0   # the prior of the live scans scores 0
    best = _check(ctx, varied, None, three, np.repeat(centre, 3, 0), 20, 20, 64, 1, 2, max_nodes=1024)[0]
    assert best[:, 0].tolist() == [0, mw.OVERFLOW, 0]


def test_ignored_absent_and_outside(ctx, oracle):
    occ = _map("blocks", 65, 63)
    H, W = occ.shape
    d2 = oracle.edt(occ)
    known = (np.random.default_rng(6).random((H, W)) < 0.5).astype(np.uint8)
    pts, centre = _scans(occ, 5, 3, 65)
    for bad in ((-mt.MAX_REACH - 1, 5), (5, mt.MAX_DIM + mt.MAX_REACH + 1), (2**31 - 1, -2**31)):
        c = centre[:3].copy()
        c[1] = bad
        best, stats = _check(ctx, d2, None, pts[:3], c, 20, 9, 64, 1, 2)
        assert best[1].tolist() == [mt.IGNORED, 0, 0, 0, 0, 0] and not stats[1].any() and stats[0].any() and stats[2].any()
    none = np.full_like(pts[:2], mt.ABSENT)
    best, stats = _check(ctx, d2, None, none, centre[:2], 100, 70, 64, 1, 3)
    assert best.tolist() == [[0, 0, 0, 0, 0, 3 * 201 * 141]] * 2 and not stats.any()
    some = pts.copy()
    some[:, :, 0], some[:, :, 15], some[:, :, 16] = (mt.ABSENT, 0), (mt.MAX_REACH + 1, 0), (0, -mt.MAX_REACH - 1)
    _check(ctx, d2, known, some, centre, 20, 9, 64, 1, 2)
    mixed = pts.copy()
    mixed[:, 2] = mt.ABSENT                                            # the rotation that lost its points wins with 0
    best = _check(ctx, d2, None, mixed, centre, 20, 9, 64, 1, 2)[0]
    assert (best[:, 3] == 0).all() and best[0, [0, 4]].tolist() == [2, 0]
    # windows partly outside on two sides, wholly outside, a centre outside with its window reaching in, the ends of the range
    out = [(2, 1), (-140, -140), (-30, H + 20), (W + 4, H - 1), (-mt.MAX_REACH, mt.MAX_DIM + mt.MAX_REACH)]
    for kn, cap, unk in ((None, 64, 3), (known, 64, 0), (known, 1, 1), (None, 32767, 32767)):
        _check(ctx, d2, kn, pts, out, 40, 30, cap, unk, 2)
    a = _check(ctx, d2, None, pts, centre, 20, 9, 64, 1, 2)
    b = _check(ctx, d2, np.ones((H, W), np.uint8), pts, centre, 20, 9, 64, 1, 2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))            # known NULL == all ones
    _check(ctx, np.full((H, W), mt.EDT_INF, np.int32), known, pts, centre, 20, 9, 32767, 2, 2)   # a grid without obstacles


def test_a_reused_best_and_grids_of_changing_size(ctx, oracle):
    import torch
    out = torch.full((2, 6), 77, dtype=torch.int32, device="cuda")
    stats = torch.full((2, 8), 77, dtype=torch.int32, device="cuda")
    for W, H, top in ((130, 70, 2), (64, 64, 3), (256, 192, 3), (65, 63, 1), (130, 70, 3), (8, 8, 2)):   # the scratch is larger than later calls need
        occ = _map("salt", W, H)
        d2 = oracle.edt(occ)
        pts, centre = _scans(occ, 2, 3, 65)
        b, s = ctx.scan_match_wide(_t(pts), _t(centre), _t(d2), wx=40, wy=30, top=top, max_nodes=1 << 15, out=out, stats=stats)
        assert b is out and s is stats
        ctx.synchronize()
        want = mw.match_wide(d2, None, pts, centre, 40, 30, 64, 1, top, 1 << 15)
        _eq("best", out.cpu().numpy(), want[0])
        _eq("stats", stats.cpu().numpy(), want[1])


def test_host_form(ctx, oracle):
    import sea_current_amd as sc
    occ = _map("blocks", 65, 63)
    H, W = occ.shape
    d2 = oracle.edt(occ)
    known = (np.random.default_rng(7).random((H, W)) < 0.8).astype(np.uint8)
    pts, centre = _scans(occ, 2, 3, 65)
    want = mw.match_wide(d2, known, pts, centre, 30, 40, 50, 2, 2, 4096)
    _eq("best", ctx.scan_match_wide_host(pts, centre, d2, known, wx=30, wy=40, d2_cap=50, unk=2, top=2, max_nodes=4096), want[0])
    best, stats = ctx.scan_match_wide_host(pts.tolist(), centre.tolist(), d2.tolist(), known.tolist(), wx=30, wy=40, d2_cap=50, unk=2, top=2,
                                           max_nodes=4096, stats=True)
    _eq("best", best, want[0])
    _eq("stats", stats, want[1])
    _eq("defaults", ctx.scan_match_wide_host(pts, centre, d2), mw.match_wide(d2, None, pts, centre, 256, 256, 64, 1, 3, 1 << 16)[0])
    assert ctx.scan_match_wide_host(np.zeros((0, 1, 1, 2), np.int32), np.zeros((0, 2), np.int32), d2).shape == (0, 6)
    with pytest.raises(sc.SeaCurrentError):                            # the host form refuses an ignored centre
        ctx.scan_match_wide_host(pts, [(0, 0), (-mt.MAX_REACH - 1, 0)], d2)


def test_argument_errors(ctx):
    import sea_current_amd as sc
    l, h, p = ctx._l, ctx._h, sc._ptr
    INV = 1
    d2, known = _t(np.ones((8, 8), np.int32)), _t(np.ones((8, 8), np.uint8))
    pts, centre = _t(np.zeros((1, 1, 1, 2), np.int32)), _t(np.array([[4, 4]], np.int32))
    best, stats = _t(np.zeros((1, 6), np.int32)), _t(np.zeros((1, 8), np.int32))
    f = lambda name="sc_scan_match_wide_batch", d=d2, k=known, q=pts, c=centre, S=1, R=1, N=1, W=8, H=8, wx=1, wy=1, cap=64, unk=1, top=1, mn=64, b=best, v=stats: getattr(
        l, name)(h, p(d), p(k), p(q), p(c), S, R, N, W, H, wx, wy, cap, unk, top, mn, p(b), p(v))
    assert f() == 0 and f(k=None) == 0 and f(v=None) == 0 and f(S=0) == 0
    assert f(wx=0, wy=0, top=0) == 0 and f(cap=1, unk=0) == 0 and f(cap=32767, unk=32767) == 0 and f(wx=2048, wy=0, top=5) == 0
    assert f(mn=1 << 22) == 0 and f(wx=3, wy=3, top=0, mn=64) == 0
    bad = [f(d=None), f(q=None), f(c=None), f(b=None), f(S=-1), f(R=0), f(R=257), f(N=0), f(N=65537), f(W=0), f(H=0), f(W=8193), f(H=8193),
           f(wx=-1), f(wy=-1), f(wx=2049), f(wy=2049), f(cap=0), f(cap=32768), f(unk=-1), f(unk=65), f(top=-1), f(top=6), f(mn=63),
           f(mn=(1 << 22) + 1), f(S=17, mn=1 << 22), f(wx=4, wy=4, top=0, mn=64), f(wx=100, wy=100, top=1, R=2, mn=4096),
           f(wx=2048, wy=2048, top=5, R=256, mn=1 << 16), f(v=best)]
    assert bad == [INV] * len(bad)
    ctx.synchronize()
    hd, hk = np.ones((8, 8), np.int32), np.ones((8, 8), np.uint8)
    hq, hc, hb, hv = np.zeros((1, 1, 1, 2), np.int32), np.array([[4, 4]], np.int32), np.zeros((1, 6), np.int32), np.zeros((1, 8), np.int32)
    g = lambda **kw: f(**dict(dict(name="sc_scan_match_wide_batch_host", d=hd, k=hk, q=hq, c=hc, b=hb, v=hv), **kw))
    assert g() == 0 and hb[0].tolist() == [0, 0, 0, 1, 1, 9] and hv[0].tolist() == [9, 1, 0, 0, 0, 0, 9, 1]
    assert g(k=None, v=None) == 0 and g(S=0) == 0
    bad = [g(d=None), g(q=None), g(c=None), g(b=None), g(S=-1), g(R=0), g(N=0), g(W=8193), g(wx=2049), g(cap=0), g(unk=65), g(top=6), g(mn=63),
           g(v=hb), g(c=np.array([[-16385, 0]], np.int32)), g(c=np.array([[0, 8192 + 16385]], np.int32))]
    assert bad == [INV] * len(bad)


def test_binding_checks_sizes(ctx):
    import sea_current_amd as sc
    d2 = _t(np.ones((4, 8), np.int32))
    pts, centre = _t(np.zeros((2, 3, 5, 2), np.int32)), _t(np.array([[4, 2], [1, 1]], np.int32))
    ok = lambda **kw: ctx.scan_match_wide(**dict(dict(pts=pts, centre=centre, d2=d2, wx=9, wy=2, top=1, max_nodes=64), **kw))
    b, s = ok(stats=True)
    assert b.shape == (2, 6) and s.shape == (2, 8)
    i32 = lambda *shape: _t(np.zeros(shape, np.int32))
    for kw in (dict(known=_t(np.ones((4, 7), np.uint8))), dict(out=i32(1, 6)), dict(stats=i32(2, 7)), dict(centre=i32(3, 2)),
               dict(pts=i32(2, 3, 5)), dict(pts=i32(2, 3, 5, 3)), dict(d2=i32(32)), dict(max_nodes=63), dict(top=6)):
        with pytest.raises(sc.SeaCurrentError):
            ok(**kw)
    with pytest.raises(sc.SeaCurrentError):
        ctx.scan_match_wide_host(np.zeros((1, 1, 1, 2), np.int32), [(1, 1), (2, 2)], np.ones((4, 8), np.int32))
    ctx.synchronize()


def test_the_chain_on_one_stream(ctx, oracle):
    """scan_cast -> logodds_update(occ_est, known) -> edt(occ_est) -> scan_match_wide, one synchronise at the end.  The points
    are made on the host, so they come from the twin's cast and are uploaded before the chain starts."""
    import sea_current_amd as sc
    W, H = 130, 70
    occ = _map("salt", W, H)
    ax, ay = mc.free_near(occ, 60, 35)
    first, second = st.square_fan(ax, ay, 20), st.square_fan(ax + 2, ay - 1, 20)
    occ[ay - 1, ax + 2] = 0
    pts = sc.points_from_hits(second, st.cast(occ, second), W)[None, None]
    prior = (ax + 2 + 31, ay - 1 - 17)                                 # the second pose, believed far off
    tp, tc = _t(pts), _t(np.array([prior], np.int32))
    tfirst, tsecond, tocc = _t(first), _t(second), _t(occ)
    hit1 = ctx.scan_cast(tfirst, tocc)
    L, occ_est, known = ctx.logodds_update(tfirst, hit1, W, H, occ_est=True, known=True, **st.LOOP_PARAMS)
    hit2 = ctx.scan_cast(tsecond, tocc)
    best, stats = ctx.scan_match_wide(tp, tc, ctx.edt(occ_est), known=known, wx=40, wy=30, d2_cap=16, unk=1, top=2, max_nodes=1 << 14, stats=True)
    ctx.synchronize()
    _eq("hit", hit2.cpu().numpy(), st.cast(occ, second))
    wl, we, wk = st.update(None, first, st.cast(occ, first), W, H, **st.LOOP_PARAMS)
    want = mw.match_wide(oracle.edt(we), wk, pts, [prior], 40, 30, 16, 1, 2, 1 << 14)
    _eq("best", best.cpu().numpy(), want[0])
    _eq("stats", stats.cpu().numpy(), want[1])
    assert want[0][0].tolist()[:3] == [0, -31, 17] and want[0][0, 5] == 1          # and the pose is found


def test_the_kidnapped_robot(ctx, oracle):
    k = mc.kidnapped(oracle.edt)
    cap = mt.WALK["d2_cap"]
    best, stats = ctx.scan_match_wide(_t(k["pts"]), _t(k["centre"]), _t(k["d2"]), known=_t(k["known"]), wx=24, wy=24, d2_cap=cap, unk=1, top=2,
                                      max_nodes=1 << 14, stats=True)
    near = ctx.scan_match(_t(k["pts"]), _t(k["centre"]), _t(k["d2"]), known=_t(k["known"]), wx=3, wy=3, d2_cap=cap, unk=1)
    ctx.synchronize()
    want = mw.match_wide(k["d2"], k["known"], k["pts"], k["centre"], 24, 24, cap, 1, 2, 1 << 14)
    _eq("best", best.cpu().numpy(), want[0])
    _eq("stats", stats.cpu().numpy(), want[1])
    b, n = best.cpu().numpy()[0], near.cpu().numpy()[0]
    assert b[5] == 1 and (b[1], b[2]) == (-mc.KIDNAP[0], -mc.KIDNAP[1])
    assert (k["centre"][0, 0] + n[1], k["centre"][0, 1] + n[2]) != k["true"]


def test_a_larger_case_equals_the_c_statement(ctx, ref):
    """1000 x 700 blocks, one fan of half-side 300 from the middle, 16 rotations.  The dense C search needs about 2 400 lookups
    per candidate and rotation: +-80 (25 921 candidates) is the largest window at which it finishes in a few seconds, so best
    is compared there; at +-256 with top 3 the GPU must find the same pose from the same prior, which the C statement's
    best implies as long as its score is 0 and the wider window holds no second pose at 0 (n_ties = 1)."""
    import sea_current_amd as sc
    from sea_current_amd import synth
    occ = synth.block_grid(1000, 700, 0.2, seed=3, smin=4, smax=40)
    H, W = occ.shape
    x, y = mc.free_near(occ, 500, 350)
    rays = st.square_fan(x, y, 300)
    tocc = _t(occ)
    hit = ctx.scan_cast(_t(rays), tocc)
    d2 = ctx.edt(tocc)
    ctx.synchronize()
    p = sc.points_from_hits(rays, hit.cpu().numpy(), W)
    assert 1000 < int(mt.present(p).sum()) < len(p)
    pts = sc.rotate_points(p, np.arange(16) * (2 * np.pi / 16))[None]
    pts = np.ascontiguousarray(np.roll(pts, 3, axis=1))                # the unturned scan is rotation 3
    centre = np.array([[x + 59, y - 73]], np.int32)
    known = (np.random.default_rng(9).random((H, W)) < 0.97).astype(np.uint8)
    tp, tc, tk = _t(pts), _t(centre), _t(known)
    best = ctx.scan_match_wide(tp, tc, d2, known=tk, wx=80, wy=80, d2_cap=64, unk=1, top=3, max_nodes=1 << 16)
    wide, stats = ctx.scan_match_wide(tp, tc, d2, known=tk, wx=256, wy=256, d2_cap=64, unk=1, top=3, max_nodes=1 << 18, stats=True)
    ctx.synchronize()
    want = ref.match(d2.cpu().numpy(), known, pts, centre, 80, 80, 64, 1, 3, 1 << 16, want_stats=False)[0]
    _eq("best", best.cpu().numpy(), want)
    assert want[0, :3].tolist() == [3, -59, 73]
    wide, stats = wide.cpu().numpy(), stats.cpu().numpy()
    assert wide[0, 0] >= 0 and wide[0, 3] <= want[0, 3] and mw.work(stats)[0] * 4 <= 16 * 513 * 513
    if wide[0, 5] == 1 and want[0, 3] == wide[0, 3]:
        assert wide[0, :5].tolist() == want[0, :5].tolist()
