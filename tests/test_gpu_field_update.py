"""sc_cost_field_update_batch / sc_cost_field_weighted_update_batch (Context.cost_fields_update): every case of the CPU
reference test on the device, bit-equal to the C statement (tests/cpp/field_update_ref.c) and to cost_fields of the new
map run on the device, in g, status and both stats; every `rounds`; the _host forms; many fields over several grids of
which one changes; the chain edt -> cost_fields_update -> field_paths -> path_waypoints with one synchronise; 20 chained
frames of the dynamic-obstacle stream; one 1024 x 700 frame."""
import numpy as np
import pytest

from sea_current_amd import synth
from field_twin import INF, Q_BAD_ENDPOINT, Q_OK, Twin, d2_of
from field_w_twin import TwinW
from field_update_twin import TwinU, cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(g, ref, what):
    if not np.array_equal(g, ref):
        bad = np.argwhere(g != ref)
        raise AssertionError(f"{what}: {len(bad)} cells differ, first {tuple(bad[0])} gpu {g[tuple(bad[0])]} ref {ref[tuple(bad[0])]}")


@pytest.fixture(scope="module")
def prepared(oracle, tmp_path_factory):
    """Every case with the old field and what the C statement makes of it: computed once, left unchanged."""
    t0, tw = Twin(tmp_path_factory.mktemp("fu_gpu_t0")), TwinW(tmp_path_factory.mktemp("fu_gpu_tw"))
    tu = TwinU(tmp_path_factory.mktemp("fu_gpu_tu"))
    out = {}
    for name, d0, d1, p0, p1, cap, r2, root in cases(oracle):
        H, W = d0.shape
        if not 0 <= root < W * H:
            g0 = np.full((H, W), INF, np.int32)
        else:
            g0 = (t0.field(d0, root, r2) if p0 is None else tw.field(d0, p0, root, r2, cap))[0]
        want, st, stats = tu.update(d0, d1, g0, root, r2, p0, p1, cap)
        for a in (g0, want):
            a.setflags(write=False)
        out[name] = dict(d0=d0, d1=d1, p0=p0, p1=p1, cap=cap, r2=r2, root=root, g0=g0, want=want, st=st, stats=stats)
    return out


def _run(ctx, c, rounds=-1, host=False):
    """The repair of one case on the device (or through the _host form): (g, status, stats) as numpy."""
    roots = np.array([c["root"]], np.int32)
    kw = dict(r2=c["r2"], rounds=rounds, pen_cap=c["cap"])
    if host:
        o = ctx.cost_fields_update_host(c["d0"], c["d1"], c["g0"][None], roots, pen_old=c["p0"], pen_new=c["p1"], **kw)
        return o["g"][0], int(o["status"][0]), [int(v) for v in o["stats"][0]]
    g = _t(c["g0"][None].copy())
    o = ctx.cost_fields_update(_t(c["d0"]), _t(c["d1"]), g, _t(roots), pen_old=_t(c["p0"]), pen_new=_t(c["p1"]), **kw)
    ctx.synchronize()
    assert o["g"] is g                                          # the caller's tensor, updated in place
    return g.cpu().numpy()[0], int(o["status"].cpu()[0]), [int(v) for v in o["stats"].cpu()[0]]


def _fresh(ctx, c):
    o = ctx.cost_fields(_t(c["d1"]), _t(np.array([c["root"]], np.int32)), r2=c["r2"], pen=_t(c["p1"]), pen_cap=c["cap"])
    ctx.synchronize()
    return o["g"].cpu().numpy()[0], int(o["status"].cpu()[0])


def _check(ctx, name, c, rounds=-1, host=False, fresh=True):
    g, st, stats = _run(ctx, c, rounds, host)
    what = f"{name} rounds {rounds}{' host' if host else ''}"
    _same(g, c["want"], what + " vs the C statement")
    assert st == c["st"] and stats == c["stats"], (what, st, c["st"], stats, c["stats"])
    if fresh:
        fg, fst = _fresh(ctx, c)
        _same(g, fg, what + " vs cost_fields on the device")
        assert st == fst, what


def test_every_reference_case(ctx, prepared):
    assert len(prepared) >= 50
    for name, c in prepared.items():
        _check(ctx, name, c)


ROUNDS_CASES = ["serpentine/closed", "serpentine/reopened", "serpentine/wall_opened", "rect_across_corner", "rect_across_corner/far_root",
                "weighted/both", "weighted/map_too", "root_freed", "root_blocked", "no_change", "salt130x70/x64", "r2_4", "200x1/block"]


@pytest.mark.parametrize("rounds", [0, 1, 2, 1000])
def test_every_rounds(ctx, prepared, rounds):
    for name in ROUNDS_CASES:
        _check(ctx, name, prepared[name], rounds=rounds, fresh=False)


def test_host_forms(ctx, prepared):
    for name in ("serpentine/closed", "weighted/both", "root_blocked", "root_freed", "blocks130x70/y63", "no_change"):
        _check(ctx, name, prepared[name], host=True, fresh=False)
    c = prepared["no_change"]
    neg = c["g0"][None].copy()
    neg[0, 3, 3] = -1
    import sea_current_amd as sc
    with pytest.raises(sc.SeaCurrentError, match="invalid"):
        ctx.cost_fields_update_host(c["d0"], c["d1"], neg, np.array([c["root"]], np.int32))


def test_stats_none_and_same_pointer(ctx, prepared):
    c = prepared["blocks130x70/x63"]
    g = _t(c["g0"][None].copy())
    o = ctx.cost_fields_update(_t(c["d0"]), _t(c["d1"]), g, _t(np.array([c["root"]], np.int32)), stats=False)
    ctx.synchronize()
    assert o["stats"] is None
    _same(g.cpu().numpy()[0], c["want"], "stats None")
    d = _t(c["d1"])                                               # d2_old == d2_new: nothing changes
    before = g.clone()
    o = ctx.cost_fields_update(d, d, g, _t(np.array([c["root"]], np.int32)))
    ctx.synchronize()
    assert o["stats"].cpu().tolist() == [[0, 0]] and bool((g == before).all())


def test_twelve_fields_three_grids_one_changes(ctx):
    """Fields on the grids that do not change come back bit for bit with stats 0 0; a blocked root, an out-of-range fgrid and
    an out-of-range root come back as the fresh call leaves them."""
    W, H = 130, 70
    occ = np.stack([synth.block_grid(W, H, 0.2, seed=s, smin=3, smax=12) for s in (31, 32, 33)])
    occ1 = occ.copy()
    occ1[1, 20:26, 60:68] ^= 1
    occ1[1, 63:66, 100:104] ^= 1
    d0, d1 = np.stack([d2_of(o) for o in occ]), np.stack([d2_of(o) for o in occ1])
    rng = np.random.default_rng(3)
    fgrid = np.array([0, 1, 2, 1, 0, 1, 2, 1, 3, 1, 1, -1], np.int32)
    roots = np.zeros(12, np.int32)
    for f in range(12):
        gi = fgrid[f] if 0 <= fgrid[f] < 3 else 0
        free = np.flatnonzero((d0[gi].ravel() >= 1) & (d1[gi].ravel() >= 1))
        roots[f] = free[rng.integers(0, free.size)]
    roots[3] = int(np.flatnonzero(d1[1].ravel() < 1)[0])                 # blocked in both maps
    closed = np.flatnonzero((d0[1].ravel() >= 1) & (d1[1].ravel() < 1))
    assert closed.size > 0
    roots[5] = closed[0]                                                 # free in the old map, blocked in the new one
    roots[9] = W * H                                                     # out of range
    old = ctx.cost_fields(_t(d0), _t(roots), fgrid=_t(fgrid))
    new = ctx.cost_fields(_t(d1), _t(roots), fgrid=_t(fgrid))
    ctx.synchronize()
    g_old = old["g"].cpu().numpy()
    g = old["g"].clone()
    o = ctx.cost_fields_update(_t(d0), _t(d1), g, _t(roots), fgrid=_t(fgrid))
    ctx.synchronize()
    got, stats = g.cpu().numpy(), o["stats"].cpu().numpy()
    np.testing.assert_array_equal(o["status"].cpu().numpy(), new["status"].cpu().numpy())
    assert o["status"].cpu().tolist() == [0, 0, 0, 2, 0, 2, 0, 0, 2, 2, 0, 2]
    want = new["g"].cpu().numpy()
    changed = int((d0[1] != d1[1]).sum())
    for f in range(12):
        _same(got[f], want[f], f"field {f}")
        on1 = fgrid[f] == 1
        assert stats[f, 0] == (changed if on1 else 0), f
        if not on1:
            assert stats[f, 1] == 0
            _same(got[f], g_old[f], f"field {f} on an unchanged grid")
    assert stats[5, 1] == int((g_old[5] < INF).sum()) > 0 and stats[3, 1] == 0 and stats[9, 1] == 0
    assert stats[[1, 7, 10], 1].min() >= 0 and stats[[1, 7, 10], 1].max() > 0


def test_chain_with_one_synchronise(ctx, oracle):
    """edt -> cost_fields_update -> field_paths -> path_waypoints, one synchronise: the read-outs equal astar_batch's on the
    new map."""
    import torch
    W, H = 200, 136
    rects = synth.block_rects(W, H, 0.15, seed=41, smin=3, smax=14)
    occ0 = synth.raster_rects(rects, W, H)
    occ1 = synth.raster_rects(synth.move_rects(rects, 0, W, H, K=8, step=2, seed=41), W, H)
    free = (occ0 == 0) & (occ1 == 0)
    s, tg = synth.queries(free, 200, seed=5)
    root = _t(s[:1].copy())
    d2_old = ctx.edt(_t(occ0))
    fl = ctx.cost_fields(d2_old, root, r2=1)
    ctx.synchronize()
    g = fl["g"]
    d2_new = ctx.edt(_t(occ1))
    o = ctx.cost_fields_update(d2_old, d2_new, g, root, r2=1)
    res = ctx.field_paths(d2_new, g, root, torch.zeros(200, dtype=torch.int32, device="cuda"), _t(tg), r2=1, Lmax=1024)
    wr = ctx.path_waypoints(d2_new, res, r2=1, Wmax=64)
    ref = ctx.astar_batch(d2_new, root.expand(200).contiguous(), _t(tg), r2=1, Lmax=1024)
    wref = ctx.path_waypoints(d2_new, ref, r2=1, Wmax=64)
    ctx.synchronize()
    assert o["stats"].cpu()[0, 0] > 0
    res, ref = {k: v.cpu().numpy() for k, v in res.items()}, {k: v.cpu().numpy() for k, v in ref.items()}
    for k in ("status", "len", "cost"):
        np.testing.assert_array_equal(res[k], ref[k], err_msg=k)
    ok = np.flatnonzero(ref["status"] == Q_OK)
    assert ok.size > 150
    for q in ok:
        np.testing.assert_array_equal(res["path"][q, :ref["len"][q]], ref["path"][q, :ref["len"][q]], err_msg=str(q))
    wr, wref = {k: v.cpu().numpy() for k, v in wr.items()}, {k: v.cpu().numpy() for k, v in wref.items()}
    for k in ("status", "n"):
        np.testing.assert_array_equal(wr[k], wref[k], err_msg=k)
    for q in ok:                                                 # past n the rows are not written
        np.testing.assert_array_equal(wr["wp"][q, :wref["n"][q]], wref["wp"][q, :wref["n"][q]], err_msg=str(q))


def test_twenty_chained_frames(ctx):
    """256 x 192, 8 of the rectangles move per frame; every frame is fed the previous repair, two roots."""
    W, H, K = 256, 192, 8
    rects = synth.block_rects(W, H, 0.15, seed=51, smin=4, smax=24)
    occ = synth.raster_rects(rects, W, H)
    keep = [5 * W + 5, (H - 6) * W + W - 6]
    occ.ravel()[keep] = 0
    roots = _t(np.array(keep, np.int32))
    d_prev = _t(d2_of(occ))
    g = ctx.cost_fields(d_prev, roots)["g"]
    raised = changed = 0
    for frame in range(20):
        rects = synth.move_rects(rects, frame, W, H, K=K, step=2, seed=51)
        occ = synth.raster_rects(rects, W, H)
        occ.ravel()[keep] = 0
        d_new = _t(d2_of(occ))
        o = ctx.cost_fields_update(d_prev, d_new, g, roots)
        want = ctx.cost_fields(d_new, roots)
        ctx.synchronize()
        assert bool((g == want["g"]).all()), f"frame {frame}: {int((g != want['g']).sum())} cells differ"
        assert o["status"].cpu().tolist() == [0, 0]
        st = o["stats"].cpu().numpy()
        assert st[0, 0] == st[1, 0] == int((d_prev != d_new).sum())
        changed += int(st[0, 0])
        raised += int(st[:, 1].sum())
        d_prev = d_new
    assert changed > 0 and raised > 0


@pytest.mark.parametrize("shape", [(8192, 72), (72, 8192)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_dimension_limit(ctx, shape):
    """W or H = SC_MAX_DIM = 8192 (128 tiles in a line): cells change next to the root, across 4095 | 4096 and at the far
    corner, one root at each end; against the device's fresh field."""
    W, H = shape
    occ0 = synth.salt_grid(W, H, 0.1, seed=81)
    occ0.ravel()[[0, W * H - 1]] = 0
    occ1 = occ0.copy()
    rng = np.random.default_rng(82)
    long_x = W > H
    for centre in (40, 4096, 8192 - 40):
        for _ in range(12):
            l, s = int(centre + rng.integers(-30, 30)), int(rng.integers(0, 72))
            x, y = (l, s) if long_x else (s, l)
            occ1[y, x] ^= 1
    wall = slice(8100, 8102)                                    # a wall near the far end with one gap, closed in the new map
    if long_x:
        occ0[:, wall] = 1; occ0[30:34, wall] = 0; occ1[:, wall] = 1
    else:
        occ0[wall, :] = 1; occ0[wall, 30:34] = 0; occ1[wall, :] = 1
    occ1.ravel()[[0, W * H - 1]] = 0
    d0, d1 = _t(d2_of(occ0)), _t(d2_of(occ1))
    roots = _t(np.array([0, W * H - 1], np.int32))
    g = ctx.cost_fields(d0, roots)["g"]
    o = ctx.cost_fields_update(d0, d1, g, roots)
    want = ctx.cost_fields(d1, roots)
    ctx.synchronize()
    assert bool((g == want["g"]).all()), f"{int((g != want['g']).sum())} cells differ"
    st = o["stats"].cpu().numpy()
    assert st[0, 0] == int((d0 != d1).sum()) > 0 and st[:, 1].min() > 50


def test_one_large_frame(ctx):
    """1024 x 700 (a partial last tile row), blocks with clearance, 32 rectangles moved: against the device's fresh field."""
    W, H = 1024, 700
    rects = synth.block_rects(W, H, 0.2, seed=61)
    occ0 = synth.raster_rects(rects, W, H)
    occ1 = synth.raster_rects(synth.move_rects(rects, 0, W, H, K=32, step=2, seed=61), W, H)
    d0, d1 = ctx.edt(_t(occ0)), ctx.edt(_t(occ1))
    ctx.synchronize()
    both = np.flatnonzero((d0.cpu().numpy().ravel() >= 4) & (d1.cpu().numpy().ravel() >= 4))
    roots = _t(both[[100, both.size // 2]].astype(np.int32))
    g = ctx.cost_fields(d0, roots, r2=4)["g"]
    o = ctx.cost_fields_update(d0, d1, g, roots, r2=4)
    want = ctx.cost_fields(d1, roots, r2=4)
    ctx.synchronize()
    assert bool((g == want["g"]).all()), f"{int((g != want['g']).sum())} cells differ"
    st = o["stats"].cpu().numpy()
    assert st[0, 0] == int(((d0 >= 4) != (d1 >= 4)).sum()) > 0 and st[:, 1].min() > 0
