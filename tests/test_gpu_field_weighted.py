"""sc_clearance_penalty_u8, sc_cost_field_weighted_batch, sc_field_paths_weighted_batch (Context.clearance_penalty and the
pen / pen_cap keywords of cost_fields, field_paths): the penalty bit-equal to its integer formula, g bit-exact against
the CPU twin (tests/cpp/field_w_ref.c) under random full-range costmaps at sizes around the 64 x 64 tile and for every
`rounds`, the anchor pen_cap = 0 equal to the unweighted entries, read-outs equal to the twin's, the wall map on which
the weighted path keeps its distance, argument errors, and the device chain without a host hop."""
import numpy as np
import pytest

from field_twin import INF, Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED, d2_of, serpentine
from field_w_twin import TwinW, path_weighted_cost, penalty_numpy, wall_map

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return TwinW(tmp_path_factory.mktemp("field_w_ref_gpu"))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pen(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _roots(d2, r2, k, seed):
    rng = np.random.default_rng(seed)
    T = np.flatnonzero(d2.ravel() >= max(r2, 1))
    return np.array(rng.choice(T, size=min(k, T.size), replace=False), np.int32)


def _same(g, ref, what):
    if not np.array_equal(g, ref):
        bad = np.argwhere(g != ref)
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} cells differ, first ({x},{y}) gpu {g[y, x]} ref {ref[y, x]}")


def _check_fields(ctx, twin, d2, pen, roots, r2, cap, rounds_list=(-1,)):
    refs = [twin.field(d2, pen, int(r), r2, cap) for r in roots]
    d2t, pt, rt = _t(d2), _t(pen), _t(roots)
    for rounds in rounds_list:
        o = ctx.cost_fields(d2t, rt, r2=r2, rounds=rounds, pen=pt, pen_cap=cap)
        ctx.synchronize()
        g = o["g"].cpu().numpy()
        assert (o["status"].cpu().numpy() == Q_OK).all()
        for f, r in enumerate(roots):
            assert refs[f][1] == Q_OK
            _same(g[f], refs[f][0], f"r2 {r2} cap {cap} rounds {rounds} field {f} root {r}")


# ---- penalty helper ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pen_maps(oracle):
    from sea_current_amd import synth
    return {"salt": np.stack([oracle.edt(synth.salt_grid(200, 136, 0.05, seed=s)) for s in (1, 2)]),
            "blocks": np.stack([oracle.edt(synth.block_grid(130, 70, 0.2, seed=s, smin=3, smax=12)) for s in (3, 4)])}


@pytest.mark.parametrize("name", ["salt", "blocks"])
def test_penalty_equals_formula(ctx, pen_maps, name):
    d2 = pen_maps[name]
    d2t = _t(d2)
    for r2_soft in (2, 36, 50):
        for pen_max in (0, 40, 255):
            for r2 in (0, 4):
                ref = penalty_numpy(d2, r2, r2_soft, pen_max)
                got = ctx.clearance_penalty(d2t, r2=r2, r2_soft=r2_soft, pen_max=pen_max)
                ctx.synchronize()
                assert got.dtype.itemsize == 1 and tuple(got.shape) == d2.shape
                assert np.array_equal(got.cpu().numpy(), ref), (r2_soft, pen_max, r2)
    assert np.array_equal(ctx.clearance_penalty_host(d2, r2=4, r2_soft=50, pen_max=255), penalty_numpy(d2, 4, 50, 255))
    assert np.array_equal(ctx.clearance_penalty_host(d2[0], r2=0, r2_soft=36, pen_max=40), penalty_numpy(d2[0], 0, 36, 40))
    assert penalty_numpy(d2, 0, 36, 40).max() > 20      # the maps do exercise the formula


# ---- fields -----------------------------------------------------------------------------------------------------------
def _map(oracle, name):
    from sea_current_amd import synth
    if name == "serpentine128":
        return d2_of(serpentine(128))
    W, H = (int(v) for v in name.split("x"))
    if min(W, H) == 1:                          # a corridor cut in three
        occ = np.zeros((H, W), np.uint8)
        occ.ravel()[[40, 100]] = 1
        return oracle.edt(occ)
    return oracle.edt(synth.salt_grid(W, H, 0.15, seed=W + 3 * H))


@pytest.mark.parametrize("name", ["130x70", "65x63", "64x64", "200x136", "129x1", "1x129", "serpentine128"])
def test_field_bit_exact_random_costmap(ctx, twin, oracle, name):
    d2 = _map(oracle, name)
    pen = _pen(d2.shape, 7)
    for r2 in ((0,) if name == "serpentine128" else (0, 4)):
        roots = _roots(d2, r2, 2, 5)
        for cap in (255, 7, 0):
            _check_fields(ctx, twin, d2, pen, roots, r2, cap, rounds_list=(-1, 0, 1, 3))


def test_field_uniform_costmaps(ctx, twin, oracle):
    d2 = _map(oracle, "130x70")
    roots = _roots(d2, 0, 2, 5)
    for v in (0, 255):
        _check_fields(ctx, twin, d2, np.full(d2.shape, v, np.uint8), roots, 0, 255, rounds_list=(-1, 0))


def test_fields_over_two_grids(ctx, twin, oracle):
    from sea_current_amd import synth
    G, F, W, H = 2, 5, 130, 70
    d2 = np.stack([oracle.edt(synth.salt_grid(W, H, 0.1 + 0.05 * k, seed=10 + k)) for k in range(G)])
    pen = _pen(d2.shape, 9)
    rng = np.random.default_rng(3)
    fgrid = (np.arange(F) % G).astype(np.int32)
    roots = np.array([rng.choice(np.flatnonzero(d2[fgrid[f]].ravel() >= 1)) for f in range(F)], np.int32)
    roots[1] = np.flatnonzero(d2[fgrid[1]].ravel() < 1)[0]      # a blocked root
    fgrid_bad = fgrid.copy()
    fgrid_bad[3] = G                                             # a grid out of range
    o = ctx.cost_fields(_t(d2), _t(roots), fgrid=_t(fgrid_bad), pen=_t(pen), pen_cap=200)
    ctx.synchronize()
    g, st = o["g"].cpu().numpy(), o["status"].cpu().numpy()
    for f in range(F):
        if f in (1, 3):
            assert st[f] == Q_BAD_ENDPOINT and (g[f] == INF).all(), f
            continue
        ref, rs = twin.field(d2[fgrid[f]], pen[fgrid[f]], int(roots[f]), 0, 200)
        assert st[f] == rs == Q_OK
        _same(g[f], ref, f"field {f}")


def test_field_1024_with_the_helper_penalty(ctx, twin, oracle):
    from sea_current_amd import synth
    d2 = oracle.edt(synth.salt_grid(1024, 1024, 0.20))
    d2t = _t(d2)
    pt = ctx.clearance_penalty(d2t, r2=0, r2_soft=25, pen_max=60)
    root = _roots(d2, 0, 1, 1)
    o = ctx.cost_fields(d2t, _t(root), pen=pt)
    ctx.synchronize()
    pen = pt.cpu().numpy()
    assert np.array_equal(pen, penalty_numpy(d2, 0, 25, 60))
    ref, st = twin.field(d2, pen, int(root[0]))
    assert st == Q_OK
    _same(o["g"].cpu().numpy()[0], ref, "1024^2 salt20")


# ---- anchor -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["salt", "blocks_r2"])
def test_anchor_cap_zero_equals_unweighted(ctx, oracle, kind):
    import torch
    from sea_current_amd import synth
    if kind == "salt":
        d2, r2 = oracle.edt(synth.salt_grid(300, 200, 0.15, seed=6)), 0
    else:
        d2, r2 = oracle.edt(synth.block_grid(300, 200, 0.2, seed=7, smin=3, smax=16)), 4
    roots = _roots(d2, r2, 2, 2)
    d2t, rt, pt = _t(d2), _t(roots), _t(_pen(d2.shape, 8))
    a = ctx.cost_fields(d2t, rt, r2=r2, pen=pt, pen_cap=0)
    b = ctx.cost_fields(d2t, rt, r2=r2)
    assert torch.equal(a["g"], b["g"]) and torch.equal(a["status"], b["status"])
    tg = np.random.default_rng(4).integers(0, d2.size, size=256).astype(np.int32)
    tg[:2] = [roots[0], -1]
    qf = (np.arange(256) % 2).astype(np.int32)
    zeros = lambda Lmax: dict(path=torch.zeros((256, Lmax), dtype=torch.int32, device="cuda"),
                              **{k: torch.zeros(256, dtype=torch.int32, device="cuda") for k in ("len", "cost", "status")})
    for Lmax, to_root in ((4096, False), (4096, True), (8, False)):
        # zeroed outputs: the cells neither kernel writes compare equal, every cell either writes is compared
        pa = ctx.field_paths(d2t, a["g"], rt, _t(qf), _t(tg), r2=r2, Lmax=Lmax, to_root=to_root, pen=pt, pen_cap=0, out=zeros(Lmax))
        pb = ctx.field_paths(d2t, b["g"], rt, _t(qf), _t(tg), r2=r2, Lmax=Lmax, to_root=to_root, out=zeros(Lmax))
        ctx.synchronize()
        for k in ("status", "len", "cost", "path"):
            assert torch.equal(pa[k], pb[k]), (k, Lmax, to_root)
        assert int((pb["status"] == Q_OK).sum()) > (100 if Lmax > 8 else 0)


# ---- read-outs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["130x70", "200x136", "serpentine128"])
def test_readouts_equal_twin(ctx, twin, oracle, name):
    d2 = _map(oracle, name)
    H, W = d2.shape
    pen = _pen(d2.shape, 12)
    cap = 99
    if name == "130x70":                        # an enclosed pocket
        d2 = d2.copy()
        d2[20:31, 20] = d2[20:31, 30] = 0
        d2[20, 20:31] = d2[30, 20:31] = 0
        d2[21:30, 21:30] = 1
    root = _roots(d2, 0, 1, 3)
    if name == "130x70":
        assert not (20 <= root[0] // W <= 30 and 20 <= root[0] % W <= 30)
    rng = np.random.default_rng(6)
    tg = rng.integers(0, W * H, size=256).astype(np.int32)
    tg[:5] = [root[0], -1, W * H, int(np.flatnonzero(d2.ravel() < 1)[0]), 25 * W + 25 if name == "130x70" else root[0]]
    qf = np.zeros(256, np.int32)
    qf[5], qf[6] = 1, -1                        # bad field indices
    d2t, pt, rt = _t(d2), _t(pen), _t(root)
    fl = ctx.cost_fields(d2t, rt, pen=pt, pen_cap=cap)
    ctx.synchronize()
    g = fl["g"].cpu().numpy()
    ref_g, _ = twin.field(d2, pen, int(root[0]), 0, cap)
    _same(g[0], ref_g, name)
    for Lmax, to_root in ((4096, False), (4096, True), (8, False)):
        o = ctx.field_paths(d2t, fl["g"], rt, _t(qf), _t(tg), Lmax=Lmax, to_root=to_root, pen=pt, pen_cap=cap)
        ctx.synchronize()
        o = {k: v.cpu().numpy() for k, v in o.items()}
        ref = twin.paths(d2, pen, ref_g, int(root[0]), tg, cap=cap, Lmax=Lmax, to_root=to_root)
        ref["status"][5:7] = Q_BAD_ENDPOINT
        ref["len"][5:7] = 0
        ref["cost"][5:7] = -1
        for k in ("status", "len", "cost"):
            np.testing.assert_array_equal(o[k], ref[k], err_msg=f"{k} Lmax {Lmax} to_root {to_root}")
        for q in np.flatnonzero(ref["status"] == Q_OK):
            np.testing.assert_array_equal(o["path"][q, :ref["len"][q]], ref["path"][q, :ref["len"][q]], err_msg=str(q))
        assert (ref["status"][1:4] == Q_BAD_ENDPOINT).all() and ref["len"][0] == 1 and ref["cost"][0] == 0
        if name == "130x70":
            assert ref["status"][4] == Q_NO_PATH
        if Lmax == 8:
            assert (ref["status"] == Q_TRUNCATED).sum() > 50
        elif not to_root:
            for q in np.flatnonzero(ref["status"] == Q_OK)[:20]:
                assert path_weighted_cost(o["path"][q, :o["len"][q]], pen, cap) == o["cost"][q]
            # the host forms
            hf = ctx.cost_fields_host(d2, root, pen=pen, pen_cap=cap)
            assert np.array_equal(hf["g"], g)
            hp = ctx.field_paths_host(d2, hf["g"], root, qf, tg, Lmax=Lmax, pen=pen, pen_cap=cap)
            for k in ("status", "len", "cost"):
                np.testing.assert_array_equal(hp[k], o[k], err_msg=k)
            for q in np.flatnonzero(ref["status"] == Q_OK):
                np.testing.assert_array_equal(hp["path"][q, :o["len"][q]], o["path"][q, :o["len"][q]])


def test_wall_map_weighted_path_keeps_its_distance(ctx, oracle):
    occ, root, target = wall_map()
    d2 = oracle.edt(occ)
    d2t, rt, tt, qf = _t(d2), _t(np.array([root], np.int32)), _t(np.array([target], np.int32)), _t(np.zeros(1, np.int32))
    pt = ctx.clearance_penalty(d2t, r2=0, r2_soft=36, pen_max=40)
    fw = ctx.cost_fields(d2t, rt, pen=pt)
    f0 = ctx.cost_fields(d2t, rt)
    pw = ctx.field_paths(d2t, fw["g"], rt, qf, tt, pen=pt)
    p0 = ctx.field_paths(d2t, f0["g"], rt, qf, tt)
    ctx.synchronize()
    pen = pt.cpu().numpy()
    gw, g0 = fw["g"].cpu().numpy()[0], f0["g"].cpu().numpy()[0]
    assert pw["status"].item() == Q_OK and p0["status"].item() == Q_OK
    path_w = pw["path"].cpu().numpy()[0, :pw["len"].item()]
    path_0 = p0["path"].cpu().numpy()[0, :p0["len"].item()]
    print("wall map: weighted cost", gw.flat[target], "unweighted", g0.flat[target], "unweighted path weighted",
          path_weighted_cost(path_0, pen), "min d2", d2.ravel()[path_w].min(), d2.ravel()[path_0].min())
    assert path_weighted_cost(path_w, pen) == gw.flat[target] == pw["cost"].item()
    assert d2.ravel()[path_w].min() > d2.ravel()[path_0].min()
    assert gw.flat[target] < path_weighted_cost(path_0, pen)
    assert gw.flat[target] > g0.flat[target]


# ---- argument errors --------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import torch
    l, h = ctx._l, ctx._h
    i32 = lambda *s: torch.ones(s, dtype=torch.int32, device="cuda")
    d2, pen, root, g, st = i32(8, 8), torch.zeros((8, 8), dtype=torch.uint8, device="cuda"), i32(1) * 0, i32(1, 8, 8), i32(1)
    p = lambda t: t.data_ptr()
    field = lambda pn, cap, W, H: l.sc_cost_field_weighted_batch(h, p(d2), pn, cap, 1, None, W, H, 0, p(root), 1, -1, p(g), p(st))
    q, path = i32(1) * 0, i32(1, 4)
    paths = lambda pn, cap, W, H: l.sc_field_paths_weighted_batch(h, p(d2), pn, cap, 1, None, W, H, 0, p(g), p(root), 1, p(q), p(q), 1, 4,
                                                                  0, p(path), p(q), p(q), p(q))
    for fn in (field, paths):
        assert fn(p(pen), -1, 8, 8) == 1
        assert fn(p(pen), 256, 8, 8) == 1
        assert fn(p(pen), 255, 8192, 8192) == 1       # (14 + 255) * (8192^2 - 1) > INT32_MAX - 1: refused before anything is touched
        assert fn(p(pen), 115, 4096, 4096) == 1
        assert fn(None, 255, 8, 8) == 1
    assert field(p(pen), 255, 8, 8) == 0
    ctx.synchronize()
    assert paths(p(pen), 255, 8, 8) == 0
    ctx.synchronize()
    out = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    helper = lambda r2_soft, pen_max, W: l.sc_clearance_penalty_u8(h, p(d2), W, 8, 1, 0, r2_soft, pen_max, p(out))
    assert helper(36, -1, 8) == 1 and helper(36, 256, 8) == 1 and helper(0, 40, 8) == 1 and helper(36, 40, 0) == 1
    assert l.sc_clearance_penalty_u8(h, p(d2), 8, 8, 1, 0, 36, 40, None) == 1
    assert helper(36, 40, 8) == 0
    ctx.synchronize()


# ---- chain ------------------------------------------------------------------------------------------------------------
def test_device_chain_one_synchronise(ctx):
    """edt -> penalty -> weighted field -> weighted read-out -> waypoints -> cells_to_points -> smooth_paths with one
    synchronise at the end gives what the same steps give with a synchronise after each."""
    import torch
    from sea_current_amd import synth
    W, Q = 256, 64
    occ_np = synth.salt_grid(W, W, 0.05, seed=3)
    occ = torch.from_numpy(occ_np).cuda()
    s, tg = synth.queries(occ_np == 0, Q, seed=5)
    root = torch.from_numpy(s[:1].copy()).cuda()
    tg = torch.from_numpy(tg).cuda()
    lim = torch.tensor([[-1.0, 1.0, -0.5, 0.5]], dtype=torch.float64).cuda().expand(Q, 4).contiguous()

    def chain(stepwise):
        sync = ctx.synchronize if stepwise else (lambda: None)
        d2 = ctx.edt(occ); sync()
        pen = ctx.clearance_penalty(d2, r2=1, r2_soft=25, pen_max=60); sync()
        fl = ctx.cost_fields(d2, root, r2=1, pen=pen); sync()
        res = ctx.field_paths(d2, fl["g"], root, torch.zeros_like(tg), tg, r2=1, Lmax=1024, pen=pen); sync()
        wr = ctx.path_waypoints(d2, res, r2=1, Wmax=128); sync()
        path, npts = ctx.cells_to_points(wr, W, 0.0, 0.0, 0.05, 0.05); sync()
        o = ctx.smooth_paths(path, npts, lim, capacity=Q * 3000)
        ctx.synchronize()
        return ({k: v.cpu().numpy() for k, v in o.items()}, {k: v.cpu().numpy() for k, v in wr.items()},
                {k: v.cpu().numpy() for k, v in res.items()})

    (a, wa, ra), (b, wb, rb) = chain(False), chain(True)
    for k in ("status", "len", "cost"):
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    for k in ("status", "n"):
        np.testing.assert_array_equal(wa[k], wb[k], err_msg=k)
    for q in range(Q):
        np.testing.assert_array_equal(wa["wp"][q, :wa["n"][q]], wb["wp"][q, :wb["n"][q]])
    M, S = int(b["needed"][0]), int(b["seg_off"][-1])
    assert (rb["status"] == Q_OK).sum() >= Q // 2 and (b["status"] == 0).sum() > 0
    for k in b:
        n = S if k == "ctrl" else M if k in ("time", "pos", "vel", "acc", "pts", "curvature", "ang_vel", "tpar", "seg") else None
        assert np.array_equal(a[k][:n], b[k][:n], equal_nan=True), k
