"""sc_occ_from_polygons on the GPU: byte for byte the numpy twin of the rule (tests/occ_twin.py, itself checked against the
header's host rasteriser in test_polygons_host.py), on the special worlds, 300 seeded random worlds, every base mode, G
grids in one call, and invalid arguments; then the chain occ -> EDT (twice on one context) -> A* against the oracle."""
import numpy as np
import pytest
import torch

import sea_current_amd as sc
import occ_twin as tw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = sc.Context(0)
    yield c
    c.close()


def _dev(w, explicit_box=True, closed_arg=True):
    L, off, cl, bx = tw.flatten(w["obstacles"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(lines=t(L), obs_off=t(off), closed=t(cl) if closed_arg else None, box=t(bx) if explicit_box else None)


def _run(ctx, w, base=None, out=None, **kw):
    W, H, x0, y0, rx, ry = w["frame"]
    return ctx.occ_from_polygons(W=W, H=H, x_min=float(x0), y_min=float(y0), res_x=float(rx), res_y=float(ry), base=base, out=out,
                                 **_dev(w, **kw))


def _polygon_ctor_only(w):
    return all(ob["edges"] is None for ob in w["obstacles"])


@pytest.mark.parametrize("name", sorted(tw.special_worlds()))
def test_special_worlds(ctx, name):
    w = tw.special_worlds()[name]
    want = tw.rasterize_world(w)
    got = _run(ctx, w).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    if _polygon_ctor_only(w) and all(ob["closed"] for ob in w["obstacles"]):
        # box = NULL (each obstacle's own lines) and closed = NULL (all closed) give the same grid
        got = _run(ctx, w, explicit_box=False, closed_arg=False).cpu().numpy()
        assert np.array_equal(got, want)
    if name == "comb200":
        W, H, x0, y0, rx, ry = w["frame"]
        assert want[H // 2].sum() > 100 and want[H // 2].sum() < W - 100


def test_polygon_world_4096(ctx):
    w = tw.polygon_world(4096)
    got = _run(ctx, w).cpu().numpy()
    assert np.array_equal(got, tw.rasterize_world(w))


def test_random_worlds(ctx):
    bad = []
    for seed in range(300):
        w = tw.random_world(seed)
        want = tw.rasterize_world(w)
        got = _run(ctx, w, explicit_box=not _polygon_ctor_only(w) or seed % 2 == 0, closed_arg=True).cpu().numpy()
        if not np.array_equal(got, want):
            bad.append((seed, w["frame"][:2], int((got != want).sum())))
    assert not bad, bad[:10]


def test_base_modes(ctx):
    w = tw.polygon_world(300, H=257)
    W, H = w["frame"][:2]
    base = (np.random.default_rng(3).random((H, W)) < 0.05).astype(np.uint8)
    want = tw.rasterize_world(w, base=base)
    assert not np.array_equal(want, tw.rasterize_world(w))
    bd = torch.from_numpy(base).cuda()
    got = _run(ctx, w, base=bd).cpu().numpy()                       # separate base
    assert np.array_equal(got, want)
    assert np.array_equal(bd.cpu().numpy(), base)                   # base untouched
    got = _run(ctx, w, base=bd, out=bd).cpu().numpy()               # in place
    assert np.array_equal(got, want)
    out = torch.full((H, W), 7, dtype=torch.uint8, device="cuda")  # base NULL: all free first
    assert np.array_equal(_run(ctx, w, out=out).cpu().numpy(), tw.rasterize_world(w))


def test_host_form(ctx):
    w = tw.special_worlds()["nondyadic_300"]
    W, H, x0, y0, rx, ry = w["frame"]
    L, off, cl, bx = tw.flatten(w["obstacles"])
    base = (np.arange(W * H).reshape(H, W) % 97 == 0).astype(np.uint8)
    got = ctx.occ_from_polygons_host(L, off, W, H, float(x0), float(y0), float(rx), float(ry), closed=cl, box=bx, base=base)
    assert np.array_equal(got, tw.rasterize_world(w, base=base))


def test_many_grids_one_call(ctx):
    """G = 5, two of them empty: one call equals five single calls, and the twin."""
    fr = tw.frame_wh((5, -5, 5, -5), 640, 480)
    parts = [tw.polygon_world(640, H=480, n_poly=6)["obstacles"], [], tw.ngon_world(300)["obstacles"], [],
             tw.examples_obstacles(4.0) + tw.comb_world(20)["obstacles"]]
    L, off, cl, bx = tw.flatten([ob for p in parts for ob in p])
    grid_off = np.cumsum([0] + [len(p) for p in parts]).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    W, H, x0, y0, rx, ry = fr
    args = dict(W=W, H=H, x_min=float(x0), y_min=float(y0), res_x=float(rx), res_y=float(ry))
    many = ctx.occ_from_polygons(t(L), t(off), closed=t(cl), box=t(bx), grid_off=t(grid_off), **args).cpu().numpy()
    assert many.shape == (5, H, W)
    for g, p in enumerate(parts):
        Lg, offg, clg, bxg = tw.flatten(p)
        one = ctx.occ_from_polygons(t(Lg), t(offg), closed=t(clg), box=t(bxg), **args).cpu().numpy()
        assert np.array_equal(many[g], one), g
        assert np.array_equal(one, tw.rasterize(fr, Lg, offg, clg, bxg)), g
    assert many[1].sum() == 0 and many[3].sum() == 0 and many[0].sum() > 0


def test_invalid_arguments(ctx):
    w = tw.examples_world()
    W, H, x0, y0, rx, ry = (float(v) for v in w["frame"])
    W, H = int(W), int(H)
    L, off, cl, bx = tw.flatten(w["obstacles"])
    d = _dev(w)
    occ = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    f = ctx._l.sc_occ_from_polygons
    p = sc._ptr
    good = [ctx._h, None, 1, W, H, x0, y0, rx, ry, p(d["lines"]), L.shape[0], p(d["obs_off"]), len(off) - 1, None, None, None, p(occ)]
    assert f(*good) == 0
    for i, v in ((2, 0), (2, 65536), (3, 0), (3, 8193), (4, -1), (7, 0.0), (8, -1.0), (5, float("nan")), (10, -1), (12, -1),
                 (16, None), (2, 2)):
        a = list(good)
        a[i] = v
        assert f(*a) == 1, (i, v)
    # the host form checks the data before anything is launched
    h = ctx._l.sc_occ_from_polygons_host
    out = np.zeros((H, W), np.uint8)
    hp = lambda a: a.ctypes.data
    assert h(ctx._h, None, 1, W, H, x0, y0, rx, ry, hp(L), L.shape[0], hp(off), len(off) - 1, None, None, None, hp(out)) == 0
    Ln = L.copy()
    Ln[1, 2] = np.nan
    assert h(ctx._h, None, 1, W, H, x0, y0, rx, ry, hp(Ln), L.shape[0], hp(off), len(off) - 1, None, None, None, hp(out)) == 1
    Lb = np.array([[0, 0, 9.0e6, 0]], np.float32)                 # n = 1.8e7 > 2^24 at unit cells
    o1 = np.array([0, 1], np.int32)
    assert h(ctx._h, None, 1, 64, 64, 0.0, 0.0, 1.0, 1.0, hp(Lb), 1, hp(o1), 1, None, None, None, hp(out)) == 1
    Lf = np.array([[0, 0, 8.0e6, 0]], np.float32)                 # n = 1.6e7 <= 2^24: inside the contract
    assert h(ctx._h, None, 1, 64, 64, 0.0, 0.0, 1.0, 1.0, hp(Lf), 1, hp(o1), 1, None, None, None, hp(out)) == 0
    bad_off = np.array([0, 5], np.int32)                           # past n_lines
    assert h(ctx._h, None, 1, 64, 64, 0.0, 0.0, 1.0, 1.0, hp(Lf), 1, hp(bad_off), 1, None, None, None, hp(out)) == 1
    ctx.synchronize()


# ---- the chain: polygons -> EDT (twice, one context) -> A* --------------------------------------------------------------
@pytest.mark.parametrize("W", [1024, 700, 1000])
def test_chain_edt_twice_and_astar(oracle, W):
    from sea_current_amd import synth
    c = sc.Context(0)
    try:
        worlds = [tw.left60_world(W), tw.polygon_world(W)]
        assert worlds[0]["frame"] == worlds[1]["frame"]
        W_, H, x0, y0, rx, ry = worlds[0]["frame"]
        want = [tw.rasterize_world(w) for w in worlds]
        want_d2 = [oracle.edt(o) for o in want]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        # one grid at a time, each twice on the same context (the second EDT of a map runs the open-space build)
        for k, w in enumerate(worlds):
            for run in range(2):
                occ = _run(c, w)
                d2 = c.edt(occ)
                c.synchronize()
                assert np.array_equal(occ.cpu().numpy(), want[k]), (k, run)
                assert np.array_equal(d2.cpu().numpy(), want_d2[k]), (k, run)
        # both grids from one call (grid_off), one batched EDT, one multi-grid A*, twice
        L, off, cl, bx = tw.flatten(worlds[0]["obstacles"] + worlds[1]["obstacles"])
        grid_off = np.array([0, len(worlds[0]["obstacles"]), len(worlds[0]["obstacles"]) + len(worlds[1]["obstacles"])], np.int32)
        Q = 16
        qgrid, s, g = [], [], []
        for k in range(2):
            ss, gg = synth.queries(want_d2[k] >= 1, Q, seed=W + k)
            qgrid += [k] * Q
            s.append(ss)
            g.append(gg)
        s, g = np.concatenate(s).astype(np.int32), np.concatenate(g).astype(np.int32)
        Lmax = 4 * (W_ + H)
        for run in range(2):
            occ = c.occ_from_polygons(t(L), t(off), W_, H, float(x0), float(y0), float(rx), float(ry), closed=t(cl), box=t(bx),
                                      grid_off=t(grid_off))
            d2 = c.edt(occ)
            res = c.astar_batch_multi(d2, t(np.array(qgrid, np.int32)), t(s), t(g), Lmax=Lmax)
            c.synchronize()
            for k in range(2):
                assert np.array_equal(occ[k].cpu().numpy(), want[k]), (run, k)
                assert np.array_equal(d2[k].cpu().numpy(), want_d2[k]), (run, k)
                ref = oracle.astar_batch(want_d2[k], s[k * Q:(k + 1) * Q], g[k * Q:(k + 1) * Q], Lmax=Lmax)
                for key in ("status", "cost", "len"):
                    assert np.array_equal(res[key][k * Q:(k + 1) * Q].cpu().numpy(), ref[key]), (run, k, key)
                assert (ref["status"] == sc.Q_OK).sum() >= Q // 2
    finally:
        c.close()
