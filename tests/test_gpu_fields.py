"""sc_cost_field_batch / sc_field_paths_batch (Context.cost_fields, field_paths): g bit-exact against the CPU twin
(tests/cpp/field_ref.c) on random, block, open and maze maps, odd sizes, many fields over several grids and every
`rounds`; read-outs equal to sc_astar_batch query for query; the device chain into waypoints and smoothing without a
host hop."""
import numpy as np
import pytest

from field_twin import INF, Q_BAD_ENDPOINT, Q_OK, Q_TRUNCATED, Twin, d2_of, serpentine, spiral

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return Twin(tmp_path_factory.mktemp("field_ref_gpu"))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _roots(d2, r2, k, seed):
    rng = np.random.default_rng(seed)
    T = np.flatnonzero(d2.ravel() >= max(r2, 1))
    return np.array(rng.choice(T, size=k, replace=False), np.int32)


def _check_fields(ctx, twin, d2, roots, r2=0, rounds=-1):
    o = ctx.cost_fields(_t(d2), _t(roots), r2=r2, rounds=rounds)
    ctx.synchronize()
    g = o["g"].cpu().numpy()
    assert (o["status"].cpu().numpy() == Q_OK).all()
    for f, r in enumerate(roots):
        ref, st = twin.field(d2, int(r), r2)
        assert st == Q_OK
        if not np.array_equal(g[f], ref):
            bad = np.argwhere(g[f] != ref)
            y, x = bad[0]
            raise AssertionError(f"field {f} root {r}: {len(bad)} cells differ, first ({x},{y}) gpu {g[f][y, x]} ref {ref[y, x]}")
    return g


@pytest.fixture(scope="module")
def maps1024(oracle):
    from sea_current_amd import synth
    return {
        "salt20": (oracle.edt(synth.salt_grid(1024, 1024, 0.20)), 0),
        "salt05": (oracle.edt(synth.salt_grid(1024, 1024, 0.05, seed=2)), 0),
        "blocks20": (oracle.edt(synth.block_grid(1024, 1024, 0.20)), 4),
        "open": (oracle.edt(synth.salt_grid(1024, 1024, 2e-5, seed=3)), 0),
    }


@pytest.mark.parametrize("name", ["salt20", "salt05", "blocks20", "open"])
def test_field_1024_bit_exact(ctx, twin, maps1024, name):
    d2, r2 = maps1024[name]
    _check_fields(ctx, twin, d2, _roots(d2, r2, 3, 1), r2)


@pytest.mark.parametrize("maze", ["serpentine", "spiral"])
def test_field_mazes(ctx, twin, maze):
    occ = serpentine(256) if maze == "serpentine" else spiral(257)[:256, :256]
    d2 = d2_of(occ)
    H, W = d2.shape
    roots = np.array([np.flatnonzero(d2.ravel() >= 1)[0], (H // 2) * W + W // 2], np.int32)
    roots = roots[d2.ravel()[roots] >= 1]
    for rounds in (-1, 0):
        _check_fields(ctx, twin, d2, roots, rounds=rounds)


@pytest.mark.parametrize("W,H", [(1000, 1000), (700, 300), (65, 63), (1, 4096), (4096, 1)])
def test_field_odd_sizes(ctx, twin, oracle, W, H):
    from sea_current_amd import synth
    d2 = oracle.edt(synth.salt_grid(W, H, 0.15 if min(W, H) > 1 else 0.0, seed=W + H))
    _check_fields(ctx, twin, d2, _roots(d2, 0, 2, W), 0)


def test_field_4096(ctx, twin, oracle):
    from sea_current_amd import synth
    d2 = oracle.edt(synth.salt_grid(4096, 4096, 0.20, seed=4))
    _check_fields(ctx, twin, d2, _roots(d2, 0, 1, 4), 0)


def test_many_fields_over_grids(ctx, twin, oracle):
    from sea_current_amd import synth
    G, F, W = 4, 64, 256
    d2 = np.stack([oracle.edt(synth.salt_grid(W, W, 0.1 + 0.05 * k, seed=10 + k)) for k in range(G)])
    rng = np.random.default_rng(3)
    fgrid = (np.arange(F) % G).astype(np.int32)
    roots = np.array([rng.choice(np.flatnonzero(d2[fgrid[f]].ravel() >= 1)) for f in range(F)], np.int32)
    roots[5] = np.flatnonzero(d2[fgrid[5]].ravel() < 1)[0]      # a blocked root
    fgrid_bad = fgrid.copy()
    fgrid_bad[7] = G                                             # a grid out of range
    o = ctx.cost_fields(_t(d2), _t(roots), fgrid=_t(fgrid_bad))
    ctx.synchronize()
    g, st = o["g"].cpu().numpy(), o["status"].cpu().numpy()
    for f in range(F):
        if f in (5, 7):
            assert st[f] == Q_BAD_ENDPOINT and (g[f] == INF).all(), f
            continue
        ref, rs = twin.field(d2[fgrid[f]], int(roots[f]))
        assert st[f] == rs == Q_OK
        assert np.array_equal(g[f], ref), f


def test_rounds_do_not_change_g(ctx, oracle):
    from sea_current_amd import synth
    d2 = oracle.edt(synth.salt_grid(256, 256, 0.25, seed=8))
    roots = _roots(d2, 0, 4, 8)
    base = ctx.cost_fields(_t(d2), _t(roots))["g"].cpu().numpy()
    for rounds in (0, 1, 2, 7, 1000):
        g = ctx.cost_fields(_t(d2), _t(roots), rounds=rounds)["g"].cpu().numpy()
        assert np.array_equal(g, base), rounds
    host = ctx.cost_fields_host(d2, roots)
    assert np.array_equal(host["g"], base) and (host["status"] == Q_OK).all()


@pytest.mark.parametrize("name", ["salt20", "blocks20"])
def test_readout_equals_gpu_astar(ctx, maps1024, name):
    from sea_current_amd import synth
    d2, r2 = maps1024[name]
    s, tg = synth.queries(d2 >= max(r2, 1), 1024, seed=7)
    root = np.array([s[0]], np.int32)
    tg = tg.copy()
    tg[:4] = [root[0], -1, d2.size, int(np.flatnonzero(d2.ravel() < max(r2, 1))[0])]   # r == t and three bad targets
    d2t = _t(d2)
    fl = ctx.cost_fields(d2t, _t(root), r2=r2)
    qf = _t(np.zeros(tg.size, np.int32))
    ref = ctx.astar_batch(d2t, _t(np.full(tg.size, root[0], np.int32)), _t(tg), r2=r2, Lmax=4096)
    fwd = ctx.field_paths(d2t, fl["g"], _t(root), qf, _t(tg), r2=r2, Lmax=4096)
    bwd = ctx.field_paths(d2t, fl["g"], _t(root), qf, _t(tg), r2=r2, Lmax=4096, to_root=True)
    ctx.synchronize()
    ref = {k: v.cpu().numpy() for k, v in ref.items()}
    fwd = {k: v.cpu().numpy() for k, v in fwd.items()}
    bwd = {k: v.cpu().numpy() for k, v in bwd.items()}
    for k in ("status", "len", "cost"):
        np.testing.assert_array_equal(fwd[k], ref[k], err_msg=k)
        np.testing.assert_array_equal(bwd[k], ref[k], err_msg=k)
    assert (ref["status"][1:4] == Q_BAD_ENDPOINT).all() and ref["len"][0] == 1
    ok = np.flatnonzero(ref["status"] == Q_OK)
    assert ok.size > 900
    for q in ok:
        L = ref["len"][q]
        np.testing.assert_array_equal(fwd["path"][q, :L], ref["path"][q, :L], err_msg=str(q))
        np.testing.assert_array_equal(bwd["path"][q, :L], ref["path"][q, :L][::-1], err_msg=str(q))
    # truncation: A*'s needed count and cost
    Lsmall = int(np.median(ref["len"][ok]))
    a = ctx.astar_batch(d2t, _t(np.full(tg.size, root[0], np.int32)), _t(tg), r2=r2, Lmax=Lsmall)
    b = ctx.field_paths(d2t, fl["g"], _t(root), qf, _t(tg), r2=r2, Lmax=Lsmall)
    ctx.synchronize()
    for k in ("status", "len", "cost"):
        np.testing.assert_array_equal(b[k].cpu().numpy(), a[k].cpu().numpy(), err_msg=k)
    assert (b["status"].cpu().numpy() == Q_TRUNCATED).sum() > 100
    # host forms
    hf = ctx.cost_fields_host(d2, root, r2=r2)
    assert np.array_equal(hf["g"], fl["g"].cpu().numpy())
    hp = ctx.field_paths_host(d2, hf["g"], root, np.zeros(tg.size, np.int32), tg, r2=r2, Lmax=4096)
    for k in ("status", "len", "cost"):
        np.testing.assert_array_equal(hp[k], fwd[k], err_msg=k)
    for q in ok:
        np.testing.assert_array_equal(hp["path"][q, :fwd["len"][q]], fwd["path"][q, :fwd["len"][q]])


def test_readout_bad_field_index(ctx, oracle):
    from sea_current_amd import synth
    d2 = oracle.edt(synth.salt_grid(128, 128, 0.1, seed=9))
    roots = _roots(d2, 0, 2, 9)
    fl = ctx.cost_fields(_t(d2), _t(roots))
    tg = _roots(d2, 0, 4, 10)
    qf = np.array([0, 1, 2, -1], np.int32)
    o = ctx.field_paths(_t(d2), fl["g"], _t(roots), _t(qf), _t(tg))
    ctx.synchronize()
    st = o["status"].cpu().numpy()
    assert st[2] == Q_BAD_ENDPOINT and st[3] == Q_BAD_ENDPOINT and st[0] != Q_BAD_ENDPOINT and st[1] != Q_BAD_ENDPOINT


def test_argument_errors(ctx):
    import sea_current_amd as sc
    l, h = ctx._l, ctx._h
    d2 = np.ones((8, 8), np.int32)
    root = np.zeros(1, np.int32)
    g = np.zeros((1, 8, 8), np.int32)
    st = np.zeros(1, np.int32)
    p = sc._ptr
    assert l.sc_cost_field_batch_host(h, p(d2), 1, None, 8, 8, 0, p(root), 0, -1, p(g), p(st)) == 1
    assert l.sc_cost_field_batch_host(h, p(d2), 2, None, 8, 8, 0, p(root), 1, -1, p(g), p(st)) == 1
    assert l.sc_cost_field_batch_host(h, p(d2), 1, None, 8, 9000, 0, p(root), 1, -1, p(g), p(st)) == 1
    assert l.sc_cost_field_batch_host(h, p(d2), 1, None, 8, 8, 0, p(root), 1, -1, p(g), p(st)) == 0
    q = np.zeros(1, np.int32)
    path = np.zeros((1, 4), np.int32)
    assert l.sc_field_paths_batch_host(h, p(d2), 1, None, 8, 8, 0, p(g), p(root), 1, p(q), p(q), 1, 0, 0, p(path), p(q), p(q), p(q)) == 1
    assert l.sc_field_paths_batch_host(h, p(d2), 1, None, 8, 8, 0, p(g), p(root), 1, p(q), p(q), 0, 4, 0, p(path), p(q), p(q), p(q)) == 0
    assert l.sc_field_paths_batch_host(h, p(d2), 1, None, 8, 8, 0, p(g), p(root), 0, p(q), p(q), 1, 4, 0, p(path), p(q), p(q), p(q)) == 1


def test_device_chain_matches_astar_chain(ctx):
    """cost field -> field_paths -> path_waypoints -> cells_to_points -> smooth_paths with no host synchronisation gives
    what the same chain gives when fed by astar_batch."""
    import torch
    from sea_current_amd import synth
    W = 1024
    occ_np = synth.salt_grid(W, W, 0.05, seed=3)
    occ = torch.from_numpy(occ_np).cuda()
    s, tg = synth.queries(occ_np == 0, 256, seed=5)
    root = torch.from_numpy(s[:1].copy()).cuda()
    tg = torch.from_numpy(tg).cuda()
    lim = torch.tensor([[-1.0, 1.0, -0.5, 0.5]], dtype=torch.float64).cuda().expand(256, 4).contiguous()

    def chain(use_field):
        d2 = ctx.edt(occ)
        if use_field:
            fl = ctx.cost_fields(d2, root, r2=1)
            res = ctx.field_paths(d2, fl["g"], root, torch.zeros_like(tg), tg, r2=1, Lmax=4096)
        else:
            res = ctx.astar_batch(d2, root.expand(256).contiguous(), tg, r2=1, Lmax=4096)
        wr = ctx.path_waypoints(d2, res, r2=1, Wmax=128)
        path, npts = ctx.cells_to_points(wr, W, 0.0, 0.0, 0.05, 0.05)
        o = ctx.smooth_paths(path, npts, lim, capacity=256 * 3000)
        ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}, {k: v.cpu().numpy() for k, v in wr.items()}

    (a, wa), (b, wb) = chain(True), chain(False)
    for k in ("status", "n"):
        np.testing.assert_array_equal(wa[k], wb[k], err_msg=k)
    for q in range(256):
        np.testing.assert_array_equal(wa["wp"][q, :wa["n"][q]], wb["wp"][q, :wb["n"][q]])
    M = int(b["needed"][0])
    S = int(b["seg_off"][-1])
    assert (b["status"] == 0).sum() >= 150
    for k in b:
        n = S if k == "ctrl" else M if k in ("time", "pos", "vel", "acc", "pts", "curvature", "ang_vel", "tpar", "seg") else None
        assert np.array_equal(a[k][:n], b[k][:n], equal_nan=True), k
