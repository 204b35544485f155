"""sc_cost_field_multi_batch / sc_field_paths_multi_batch (Context.cost_fields_multi, field_paths_multi): g and owner
bit-exact against the CPU twin (tests/cpp/field_multi_ref.c) on maps that cross tile edges, long parent chains and one
1024^2 map; the anchors to the single-root entries; read-outs equal to sc_astar_batch from the owning seed; ties,
duplicates, ragged seed lists over several grids; argument errors; the device chain into waypoints and smoothing."""
import numpy as np
import pytest

from field_twin import INF, Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED, d2_of, serpentine, spiral
from field_multi_twin import SEED_COST_MAX, TwinM, mirror_map, plug_map

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return TwinM(tmp_path_factory.mktemp("field_multi_ref_gpu"))


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(o):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _seeds(d2, r2, k, seed, cmax=400):
    rng = np.random.default_rng(seed)
    T = np.flatnonzero(d2.ravel() >= max(r2, 1))
    s = np.array(rng.choice(T, size=min(k, T.size), replace=False), np.int32)
    return s, rng.integers(0, cmax, size=s.size).astype(np.int32)


def _off(*counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _check_field(ctx, twin, d2, seeds, cost, r2=0, rounds=-1, pen=None, cap=255):
    o = _np(ctx.cost_fields_multi(_t(d2), _t(seeds), _t(_off(len(seeds))), _t(cost), r2=r2, rounds=rounds, pen=_t(pen), pen_cap=cap))
    g, owner, st = twin.field(d2, seeds, cost, r2, pen=pen, cap=cap)
    assert o["status"][0] == st
    for k, ref in (("g", g), ("owner", owner)):
        if not np.array_equal(o[k][0], ref):
            bad = np.argwhere(o[k][0] != ref)
            y, x = bad[0]
            raise AssertionError(f"{k}: {len(bad)} cells differ, first ({x},{y}) gpu {o[k][0][y, x]} ref {ref[y, x]} (rounds {rounds})")
    return o


@pytest.fixture(scope="module")
def salt1024(ctx, twin, oracle):
    """The 1024^2 salt20 map with K = 64 seeds (with costs): the twin's field and the GPU's, computed once."""
    from sea_current_amd import synth
    d2 = oracle.edt(synth.salt_grid(1024, 1024, 0.20))
    seeds, cost = _seeds(d2, 0, 64, 21, cmax=3000)
    ref = twin.field(d2, seeds, cost)
    d2t, st, ct = _t(d2), _t(seeds), _t(cost)
    fl = ctx.cost_fields_multi(d2t, st, _t(_off(64)), ct)
    ctx.synchronize()
    return dict(d2=d2, seeds=seeds, cost=cost, ref=ref, d2t=d2t, st=st, fl=fl)


@pytest.mark.parametrize("W,H,p", [(130, 70, 0.20), (65, 63, 0.15), (1, 200, 0.1), (200, 1, 0.1)])
def test_g_and_owner_bit_exact_small(ctx, twin, oracle, W, H, p):
    from sea_current_amd import synth
    d2 = oracle.edt(synth.salt_grid(W, H, p, seed=W + H))
    seeds, cost = _seeds(d2, 0, 5, W)
    for rounds in (-1, 0, 1):
        for c in (None, cost):
            _check_field(ctx, twin, d2, seeds, c, rounds=rounds)


@pytest.mark.parametrize("maze", ["serpentine", "spiral"])
def test_g_and_owner_bit_exact_mazes(ctx, twin, maze):
    """One seed at the corridor's end gives parent chains of thousands of cells (serpentine: more than 11 700)."""
    occ = serpentine(256) if maze == "serpentine" else spiral(257)[:256, :256]
    d2 = d2_of(occ)
    T = np.flatnonzero(d2.ravel() >= 1)
    o = _check_field(ctx, twin, d2, T[:1].astype(np.int32), None)
    if maze == "serpentine":
        assert o["g"][0][o["g"][0] < INF].max() >= 10 * 11700
    seeds, cost = _seeds(d2, 0, 3, 5, cmax=20000)
    _check_field(ctx, twin, d2, seeds, None)
    _check_field(ctx, twin, d2, seeds, cost)


def test_g_and_owner_bit_exact_1024(salt1024):
    g, owner, st = salt1024["ref"]
    o = _np(salt1024["fl"])
    assert o["status"][0] == st == Q_OK
    assert np.array_equal(o["g"][0], g) and np.array_equal(o["owner"][0], owner)
    assert len(np.unique(owner[owner >= 0])) > 32


def test_plug_map_and_its_transpose(ctx, twin):
    """A seed whose only free neighbour lies in the next tile: through the new entry and through sc_cost_field_batch."""
    d2, seed = plug_map()
    for m, s in ((d2, seed), (np.ascontiguousarray(d2.T), 63 * 3 + 1)):
        seeds = np.array([s], np.int32)
        ref = twin.field(m, seeds)[0]
        assert (ref < INF).sum() == 199
        for rounds in (-1, 0):
            o = _check_field(ctx, twin, m, seeds, None, rounds=rounds)
            assert (o["g"][0] < INF).sum() == 199
            one = _np(ctx.cost_fields(_t(m), _t(seeds), rounds=rounds))
            assert np.array_equal(one["g"][0], ref) and one["status"][0] == Q_OK


def test_anchor_one_seed_of_cost_zero(ctx, oracle):
    """K = 1, cost 0: bit-identical to the single-root entries, unweighted and with a costmap."""
    from sea_current_amd import synth
    d2 = oracle.edt(synth.salt_grid(130, 70, 0.2, seed=200))
    d2t = _t(d2)
    roots, _ = _seeds(d2, 0, 3, 9)
    roots[2] = int(np.flatnonzero(d2.ravel() < 1)[0])                      # a blocked root: BAD_ENDPOINT either way
    tg = np.random.default_rng(3).integers(-2, d2.size + 2, size=256).astype(np.int32)
    qf = (np.arange(256) % 3).astype(np.int32)
    pen = ctx.clearance_penalty(d2t, r2_soft=25, pen_max=60)
    for kw in ({}, dict(pen=pen, pen_cap=60)):
        a = ctx.cost_fields(d2t, _t(roots), **kw)
        b = ctx.cost_fields_multi(d2t, _t(roots), _t(np.arange(4, dtype=np.int32)), **kw)
        ctx.synchronize()
        assert np.array_equal(a["g"].cpu().numpy(), b["g"].cpu().numpy())
        assert np.array_equal(a["status"].cpu().numpy(), b["status"].cpu().numpy())
        g, owner = b["g"].cpu().numpy(), b["owner"].cpu().numpy()
        for f in range(3):
            assert np.array_equal(owner[f], np.where(g[f] < INF, f, -1))
        for to in (False, True):
            pa = _np(ctx.field_paths(d2t, a["g"], _t(roots), _t(qf), _t(tg), Lmax=64, to_root=to, **kw))
            pb = _np(ctx.field_paths_multi(d2t, b, _t(roots), _t(qf), _t(tg), Lmax=64, to_seed=to, **kw))
            # a field without a valid seed has no path (NO_PATH) where the single-root entry reports its bad root
            live = qf != 2
            for k in ("status", "len", "cost"):
                np.testing.assert_array_equal(pa[k][live], pb[k][live], err_msg=k)
            for q in np.flatnonzero(live & (pa["status"] == Q_OK)):
                np.testing.assert_array_equal(pa["path"][q, :pa["len"][q]], pb["path"][q, :pa["len"][q]])
            has = np.isin(pb["status"], (Q_OK, Q_TRUNCATED))
            assert np.array_equal(pb["which"], np.where(has, qf, -1))
            inr = (tg >= 0) & (tg < d2.size)
            blocked = ~inr.copy()
            blocked[inr] = d2.ravel()[tg[inr]] < 1
            assert np.array_equal(pb["status"][~live], np.where(blocked[~live], Q_BAD_ENDPOINT, Q_NO_PATH))


def test_anchor_minimum_of_single_fields(ctx, oracle):
    """K = 5: g equals the minimum over five single fields plus costs (computed on the GPU), weighted too."""
    import torch
    from sea_current_amd import synth
    d2 = oracle.edt(synth.salt_grid(130, 70, 0.2, seed=200))
    d2t = _t(d2)
    seeds, cost = _seeds(d2, 0, 5, 4)
    pen = ctx.clearance_penalty(d2t, r2_soft=25, pen_max=60)
    for kw in ({}, dict(pen=pen, pen_cap=60)):
        single = ctx.cost_fields(d2t, _t(seeds), **kw)["g"].to(torch.int64)
        single = torch.where(single < INF, single + _t(cost).to(torch.int64)[:, None, None], single)
        multi = ctx.cost_fields_multi(d2t, _t(seeds), _t(_off(5)), _t(cost), **kw)
        assert torch.equal(single.min(dim=0).values, multi["g"][0].to(torch.int64))


def _check_readout(ctx, d2, d2t, seeds, cost, fl, tg, Lbig):
    st_, ct = _t(seeds), cost if cost is not None else np.zeros(seeds.size, np.int32)
    qf = _t(np.zeros(tg.size, np.int32))
    owner = fl["owner"].cpu().numpy()[0].ravel()
    for Lmax in (Lbig, 8):
        fwd = _np(ctx.field_paths_multi(d2t, fl, st_, qf, _t(tg), Lmax=Lmax))
        bwd = _np(ctx.field_paths_multi(d2t, fl, st_, qf, _t(tg), Lmax=Lmax, to_seed=True))
        has = np.isin(fwd["status"], (Q_OK, Q_TRUNCATED))
        inr = (tg >= 0) & (tg < d2.size)
        assert np.array_equal(fwd["which"][has], owner[tg[has]]) and (fwd["which"][~has] == -1).all()
        w = np.where(has, fwd["which"], 0)
        ref = _np(ctx.astar_batch(d2t, _t(seeds[w]), _t(tg), Lmax=Lmax))
        for k in ("status", "len", "which"):
            np.testing.assert_array_equal(bwd[k], fwd[k], err_msg=k)
        np.testing.assert_array_equal(fwd["status"][has], ref["status"][has])
        np.testing.assert_array_equal(fwd["len"][has], ref["len"][has])
        np.testing.assert_array_equal(fwd["cost"][has] - ct[w[has]], ref["cost"][has])
        np.testing.assert_array_equal(bwd["cost"], fwd["cost"])
        for q in np.flatnonzero(fwd["status"] == Q_OK):
            L = ref["len"][q]
            np.testing.assert_array_equal(fwd["path"][q, :L], ref["path"][q, :L], err_msg=str(q))
            np.testing.assert_array_equal(bwd["path"][q, :L], ref["path"][q, :L][::-1], err_msg=str(q))
        # no path: a bad target is BAD_ENDPOINT, an unreachable one NO_PATH
        blocked = ~inr.copy()
        blocked[inr] = d2.ravel()[tg[inr]] < 1
        assert np.array_equal(fwd["status"][~has], np.where(blocked[~has], Q_BAD_ENDPOINT, Q_NO_PATH))
        assert (fwd["len"][~has] == 0).all() and (fwd["cost"][~has] == -1).all()
        if Lmax == 8:
            assert (fwd["status"] == Q_TRUNCATED).sum() >= tg.size // 4
        else:
            full = fwd
    return full


def test_readout_small(ctx, oracle):
    from sea_current_amd import synth
    d2 = oracle.edt(synth.salt_grid(130, 70, 0.2, seed=200))
    d2t = _t(d2)
    seeds, cost = _seeds(d2, 0, 5, 4)
    tg = np.random.default_rng(8).integers(0, d2.size, size=256).astype(np.int32)
    tg[:4] = [seeds[1], -1, d2.size, int(np.flatnonzero(d2.ravel() < 1)[0])]
    for c in (None, cost):
        fl = ctx.cost_fields_multi(d2t, _t(seeds), _t(_off(5)), _t(c))
        fwd = _check_readout(ctx, d2, d2t, seeds, c, fl, tg, 512)
        if c is None:
            assert fwd["len"][0] == 1 and fwd["which"][0] == 1 and fwd["cost"][0] == 0
        # the _host forms
        hf = ctx.cost_fields_multi_host(d2, seeds, _off(5), c)
        flh = _np(fl)
        for k in ("g", "owner", "status"):
            assert np.array_equal(hf[k], flh[k]), k
        hp = ctx.field_paths_multi_host(d2, hf, seeds, np.zeros(tg.size, np.int32), tg, Lmax=512)
        for k in ("status", "len", "cost", "which"):
            np.testing.assert_array_equal(hp[k], fwd[k], err_msg=k)
        for q in np.flatnonzero(fwd["status"] == Q_OK):
            np.testing.assert_array_equal(hp["path"][q, :fwd["len"][q]], fwd["path"][q, :fwd["len"][q]])


def test_readout_1024(ctx, salt1024):
    from sea_current_amd import synth
    s = salt1024
    _, tg = synth.queries(s["d2"] >= 1, 1024, seed=7)
    _check_readout(ctx, s["d2"], s["d2t"], s["seeds"], s["cost"], s["fl"], tg.astype(np.int32), 4096)


def test_bad_qfield_and_field_without_a_valid_seed(ctx, twin):
    d2 = np.ones((70, 130), np.int32)
    d2[10, 10] = 0
    seeds = np.array([5 * 130 + 5, 10 * 130 + 10, -1, 70 * 130], np.int32)           # field 1: blocked, negative, past the end
    off = np.array([0, 1, 4, 4], np.int32)                                          # field 2: an empty list
    fl = ctx.cost_fields_multi(_t(d2), _t(seeds), _t(off))
    o = _np(fl)
    assert list(o["status"]) == [Q_OK, Q_BAD_ENDPOINT, Q_BAD_ENDPOINT]
    assert (o["g"][1:] == INF).all() and (o["owner"][1:] == -1).all() and (o["g"][0][d2 >= 1] < INF).all()
    qf = np.array([0, 1, 2, 3, -1, 1, 0], np.int32)
    tg = np.array([0, 0, 0, 0, 0, 10 * 130 + 10, 10 * 130 + 10], np.int32)
    p = _np(ctx.field_paths_multi(_t(d2), fl, _t(seeds), _t(qf), _t(tg), Lmax=64))
    assert list(p["status"]) == [Q_OK, Q_NO_PATH, Q_NO_PATH, Q_BAD_ENDPOINT, Q_BAD_ENDPOINT, Q_BAD_ENDPOINT, Q_BAD_ENDPOINT]
    assert list(p["which"]) == [0, -1, -1, -1, -1, -1, -1] and list(p["len"][1:]) == [0] * 6 and list(p["cost"][1:]) == [-1] * 6
    # n_seed == 0: every field BAD_ENDPOINT
    import torch
    e = _np(ctx.cost_fields_multi(_t(d2), torch.empty(0, dtype=torch.int32, device="cuda"), _t(np.zeros(3, np.int32))))
    assert list(e["status"]) == [Q_BAD_ENDPOINT] * 2 and (e["g"] == INF).all() and (e["owner"] == -1).all()


def test_ties_and_duplicates(ctx, twin):
    d2, seeds = mirror_map()
    o = _check_field(ctx, twin, d2, seeds, None)
    col = (np.arange(17) * 33 + 16).astype(np.int32)
    fl = ctx.cost_fields_multi(_t(d2), _t(seeds), _t(_off(2)))
    p = _np(ctx.field_paths_multi(_t(d2), fl, _t(seeds), _t(np.zeros(17, np.int32)), _t(col), Lmax=64))
    t = twin.paths(d2, o["g"][0], seeds, col, Lmax=64)
    for k in ("status", "len", "cost", "which"):
        np.testing.assert_array_equal(p[k], t[k], err_msg=k)
    np.testing.assert_array_equal(p["which"], o["owner"][0].ravel()[col])
    for q in range(17):
        np.testing.assert_array_equal(p["path"][q, :t["len"][q]], t["path"][q, :t["len"][q]])
    d2 = np.ones((9, 140), np.int32)
    a, b = 4 * 140 + 55, 4 * 140 + 75                       # 20 cells apart on one row, a tile edge between them
    for seeds, cost in (([a, b, a], [7, 0, 7]),            # duplicates: the smaller index owns
                        ([a, b], [0, 300]),                # b is dominated
                        ([a, b], [0, 200]),                # b's cost equals the cost from a: it stays terminal
                        ([a, b, b], [0, SEED_COST_MAX, SEED_COST_MAX + 1])):   # the largest cost, and one past it (skipped)
        o = _check_field(ctx, twin, d2, np.array(seeds, np.int32), np.array(cost, np.int32))
    assert o["g"][0].flat[b] == 200 and o["owner"][0].flat[b] == 0
    o = _check_field(ctx, twin, d2, np.array([a, b], np.int32), np.array([0, 200], np.int32))
    assert o["owner"][0].flat[b] == 1 and o["owner"][0].flat[b - 1] == 0


def test_fields_over_grids_with_ragged_seed_lists(ctx, twin, oracle):
    from sea_current_amd import synth
    G, F = 2, 8
    d2 = np.stack([oracle.edt(synth.salt_grid(130, 70, 0.1 + 0.1 * k, seed=30 + k)) for k in range(G)])
    counts = [3, 1, 0, 7, 2, 16, 1, 4]
    fgrid = (np.arange(F) % G).astype(np.int32)
    rng = np.random.default_rng(6)
    seeds = np.concatenate([rng.choice(np.flatnonzero(d2[fgrid[f]].ravel() >= 1), size=counts[f]) for f in range(F)]).astype(np.int32)
    cost = rng.integers(0, 500, size=seeds.size).astype(np.int32)
    off = _off(*counts)
    fgrid_bad = fgrid.copy()
    fgrid_bad[6] = G                                             # a grid out of range
    fl = ctx.cost_fields_multi(_t(d2), _t(seeds), _t(off), _t(cost), fgrid=_t(fgrid_bad))
    o = _np(fl)
    for f in range(F):
        if f in (2, 6):
            assert o["status"][f] == Q_BAD_ENDPOINT and (o["g"][f] == INF).all() and (o["owner"][f] == -1).all(), f
            continue
        g, owner, st = twin.field(d2[fgrid[f]], seeds[off[f]:off[f + 1]], cost[off[f]:off[f + 1]], s0=off[f])
        assert o["status"][f] == st == Q_OK
        assert np.array_equal(o["g"][f], g) and np.array_equal(o["owner"][f], owner), f
    tg = rng.integers(0, 130 * 70, size=64).astype(np.int32)
    qf = (np.arange(64) % F).astype(np.int32)
    p = _np(ctx.field_paths_multi(_t(d2), fl, _t(seeds), _t(qf), _t(tg), Lmax=256, fgrid=_t(fgrid_bad)))
    for f in range(F):
        q = np.flatnonzero(qf == f)
        if f == 6:
            assert (p["status"][q] == Q_BAD_ENDPOINT).all()
            continue
        t = twin.paths(d2[fgrid[f]], o["g"][f], seeds[off[f]:off[f + 1]], tg[q], cost[off[f]:off[f + 1]], s0=off[f], Lmax=256)
        for k in ("status", "len", "cost", "which"):
            np.testing.assert_array_equal(p[k][q], t[k], err_msg=f"{f} {k}")
        for i, qq in enumerate(q):
            np.testing.assert_array_equal(p["path"][qq, :t["len"][i]], t["path"][i, :t["len"][i]])


def test_argument_errors(ctx):
    import sea_current_amd as sc
    l, h = ctx._l, ctx._h
    p = sc._ptr
    d2 = np.ones((8, 8), np.int32)
    pen = np.zeros((8, 8), np.uint8)
    seed = np.zeros(2, np.int32)
    off = np.array([0, 2], np.int32)
    g = np.zeros((1, 8, 8), np.int32)
    st = np.zeros(1, np.int32)
    own = np.zeros((1, 8, 8), np.int32)
    cf, fp = l.sc_cost_field_multi_batch_host, l.sc_field_paths_multi_batch_host
    assert cf(h, p(d2), None, 0, 1, None, 8, 8, 0, p(seed), None, p(off), 2, 1, -1, p(g), p(own), p(st)) == 0
    assert (g == 10 * np.maximum(np.arange(8)[:, None], np.arange(8)[None]) + 4 * np.minimum(np.arange(8)[:, None], np.arange(8)[None])).all()
    assert (own == 0).all() and st[0] == Q_OK
    assert cf(h, p(d2), None, 0, 1, None, 8, 8, 0, p(seed), None, p(off), 2, 0, -1, p(g), None, p(st)) == 1           # F == 0
    assert cf(h, p(d2), None, 0, 1, None, 8, 8, 0, p(seed), None, p(off), -1, 1, -1, p(g), None, p(st)) == 1          # n_seed < 0
    assert cf(h, p(d2), None, 0, 1, None, 8, 8, 0, p(seed), None, None, 2, 1, -1, p(g), None, p(st)) == 1             # no seed_off
    assert cf(h, p(d2), None, 0, 2, None, 8, 8, 0, p(seed), None, p(off), 2, 1, -1, p(g), None, p(st)) == 1           # G > 1 without fgrid
    assert cf(h, p(d2), p(pen), 256, 1, None, 8, 8, 0, p(seed), None, p(off), 2, 1, -1, p(g), None, p(st)) == 1       # pen_cap
    # the data checks of the _host form: seed_off that decreases or leaves 0..n_seed, a seed cost outside the contract
    for bad in ([2, 1], [0, 3], [-1, 2]):
        b = np.array(bad, np.int32)
        assert cf(h, p(d2), None, 0, 1, None, 8, 8, 0, p(seed), None, p(b), 2, 1, -1, p(g), None, p(st)) == 1
    for bad in ([0, -1], [SEED_COST_MAX + 1, 0]):
        b = np.array(bad, np.int32)
        assert cf(h, p(d2), None, 0, 1, None, 8, 8, 0, p(seed), p(b), p(off), 2, 1, -1, p(g), None, p(st)) == 1
    # the overflow contract precedes any launch: pen_cap 255 at 4096^2, tiny dummy buffers (device form)
    import torch
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    d8 = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dp = d.data_ptr()
    assert l.sc_cost_field_multi_batch(h, dp, d8.data_ptr(), 255, 1, None, 4096, 4096, 0, dp, None, dp, 1, 1, -1, dp, None, None) == 1
    assert l.sc_field_paths_multi_batch(h, dp, d8.data_ptr(), 255, 1, None, 4096, 4096, 0, dp, dp, dp, 1, 1, dp, dp, 1, 4, 0, dp, dp, dp, dp,
                                        None) == 1
    q = np.zeros(1, np.int32)
    path = np.zeros((1, 4), np.int32)
    gneg, own9 = g - 1, own + 9
    assert fp(h, p(d2), None, 0, 1, None, 8, 8, 0, p(g), p(own), p(seed), 2, 1, p(q), p(q), 1, 4, 0, p(path), p(q), p(q), p(q), None) == 0
    assert fp(h, p(d2), None, 0, 1, None, 8, 8, 0, p(g), p(own), p(seed), 2, 1, p(q), p(q), 1, 0, 0, p(path), p(q), p(q), p(q), None) == 1
    assert fp(h, p(d2), None, 0, 1, None, 8, 8, 0, p(g), None, p(seed), 2, 1, p(q), p(q), 1, 4, 0, p(path), p(q), p(q), p(q), None) == 1
    assert fp(h, p(d2), None, 0, 1, None, 8, 8, 0, p(gneg), p(own), p(seed), 2, 1, p(q), p(q), 1, 4, 0, p(path), p(q), p(q), p(q), None) == 1
    # an owner outside 0..n_seed-1 is NO_PATH, not a read out of bounds
    w = np.zeros(1, np.int32)
    assert fp(h, p(d2), None, 0, 1, None, 8, 8, 0, p(g), p(own9), p(seed), 2, 1, p(q), p(q), 1, 4, 0, p(path), p(q), p(q), p(st), p(w)) == 0
    assert st[0] == Q_NO_PATH and w[0] == -1


def test_device_chain_matches_astar_chain(ctx):
    """multi field -> multi read-out -> path_waypoints -> cells_to_points -> smooth_paths on one stream without a host
    synchronisation gives what the same chain gives when fed by astar_batch(seed[which], target)."""
    import torch
    from sea_current_amd import synth
    W = 256
    occ_np = synth.salt_grid(W, W, 0.05, seed=3)
    occ = torch.from_numpy(occ_np).cuda()
    s, tg = synth.queries(occ_np == 0, 64, seed=5)
    seeds = torch.from_numpy(s[:4].copy()).cuda()
    off = _t(_off(4))
    tg = torch.from_numpy(tg).cuda()
    lim = torch.tensor([[-1.0, 1.0, -0.5, 0.5]], dtype=torch.float64).cuda().expand(64, 4).contiguous()

    def tail(d2, res):
        wr = ctx.path_waypoints(d2, res, r2=1, Wmax=64)
        path, npts = ctx.cells_to_points(wr, W, 0.0, 0.0, 0.05, 0.05)
        return wr, ctx.smooth_paths(path, npts, lim, capacity=64 * 3000)

    d2 = ctx.edt(occ)
    fl = ctx.cost_fields_multi(d2, seeds, off, r2=1)
    res = ctx.field_paths_multi(d2, fl, seeds, torch.zeros_like(tg), tg, r2=1, Lmax=1024)
    wa, a = tail(d2, res)
    ctx.synchronize()
    which = res["which"].clamp(min=0).long()
    assert (res["status"] == Q_OK).sum().item() >= 48
    ref = ctx.astar_batch(d2, seeds[which].contiguous(), tg, r2=1, Lmax=1024)
    wb, b = tail(d2, ref)
    ctx.synchronize()
    a, b, wa, wb = _np(a), _np(b), _np(wa), _np(wb)
    for k in ("status", "n"):
        np.testing.assert_array_equal(wa[k], wb[k], err_msg=k)
    for q in range(64):
        np.testing.assert_array_equal(wa["wp"][q, :wa["n"][q]], wb["wp"][q, :wb["n"][q]])
    M = int(b["needed"][0])
    S = int(b["seg_off"][-1])
    for k in b:
        n = S if k == "ctrl" else M if k in ("time", "pos", "vel", "acc", "pts", "curvature", "ang_vel", "tpar", "seg") else None
        assert np.array_equal(a[k][:n], b[k][:n], equal_nan=True), k
