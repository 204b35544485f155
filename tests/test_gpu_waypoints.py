"""GPU parity of sc_path_waypoints_batch (line-of-sight waypoints of A* paths) with its C twin, bit for bit, on the GPU's
own A* paths; and the join with the smoother: the waypoints of a batch go through bezier_from_path with finite control
points that match the CPU restatement."""
import numpy as np
import pytest

from waypoints_twin import Q_BAD_PATH, Q_NO_PATH, Q_OK, Q_TRUNCATED, Twin, check_output, edge_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return Twin(tmp_path_factory.mktemp("waypoints_ref"))


def _plan(ctx, occ, Q, r2, Lmax, seed=None):
    import torch
    from sea_current_amd import synth
    d2 = ctx.edt(torch.from_numpy(occ).cuda())
    d2h = d2.cpu().numpy()
    s, g = synth.queries(d2h >= max(r2, 1), Q) if seed is None else synth.queries(d2h >= max(r2, 1), Q, seed=seed)
    res = ctx.astar_batch(d2, torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda(), r2=r2, Lmax=Lmax)
    ctx.synchronize()
    return d2, d2h, res


def _parity(ctx, twin, d2, d2h, res, r2, min_ok):
    out = ctx.path_waypoints(d2, res, r2=r2)
    ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    path, ln, st = (res[k].cpu().numpy() for k in ("path", "len", "status"))
    ref = twin.waypoints(d2h, path, ln, st, r2=r2)
    assert np.array_equal(got["status"], ref["status"])
    assert np.array_equal(got["n"], ref["n"])
    ok = ref["status"] == Q_OK
    assert ok.sum() >= min_ok
    for q in np.flatnonzero(ok):
        assert np.array_equal(got["wp"][q, :ref["n"][q]], ref["wp"][q, :ref["n"][q]]), q
    W = d2h.shape[1]
    for q in np.flatnonzero(ok)[:32]:       # the guarantees, on a sample (the twin is checked on all of them on the CPU)
        check_output(lambda u, v: twin.visible(d2h, r2, u, v), W, path[q, :ln[q]], got["wp"][q, :got["n"][q]])
    return got, path, ln, ok


def test_headline_salt_1024(ctx, twin):
    """(a) 1024^2 salt 0.20, 1024 queries, r2 = 0, Lmax 4096."""
    from sea_current_amd import synth
    d2, d2h, res = _plan(ctx, synth.salt_grid(1024, 1024, 0.20), 1024, 0, 4096)
    got, _, ln, ok = _parity(ctx, twin, d2, d2h, res, 0, 900)
    assert got["n"][ok].mean() < 0.5 * ln[ok].mean()


def test_blocks_1024_r2_4(ctx, twin):
    """(b) 1024^2 blocks 0.20, r2 = 4."""
    from sea_current_amd import synth
    d2, d2h, res = _plan(ctx, synth.block_grid(1024, 1024, 0.20), 1024, 4, 4096)
    _parity(ctx, twin, d2, d2h, res, 4, 800)


def test_open_map_long_segments(ctx, twin):
    """(c) an almost empty map: long segments that span many 64-candidate chunks."""
    from sea_current_amd import synth
    d2, d2h, res = _plan(ctx, synth.salt_grid(1024, 1024, 2e-5), 256, 0, 4096)
    got, _, ln, ok = _parity(ctx, twin, d2, d2h, res, 0, 250)
    assert (ln[ok] > 200).sum() > 100 and got["n"][ok].max() <= 8


def test_non_square_and_host_form(ctx, twin):
    """(d) 700 x 300 and (e) the host-pointer entry point on the same input."""
    from sea_current_amd import synth
    d2, d2h, res = _plan(ctx, synth.block_grid(700, 300, 0.20), 512, 0, 2048)
    got, path, ln, ok = _parity(ctx, twin, d2, d2h, res, 0, 400)
    host = ctx.path_waypoints_host(d2h, path, ln, res["status"].cpu().numpy(), r2=0)
    for k in ("n", "status"):
        assert np.array_equal(host[k], got[k]), k
    for q in np.flatnonzero(ok):
        assert np.array_equal(host["wp"][q, :got["n"][q]], got["wp"][q, :got["n"][q]]), q


def test_edge_cases_on_device(ctx, twin):
    """(f) len 1 and 2, border runs, status passthrough, BAD_PATH, TRUNCATED with the needed count."""
    import torch
    d2h, path, ln, st, exp, around = edge_cases()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d2 = t(d2h)
    res = dict(path=t(path), len=t(ln), status=t(st))
    out = ctx.path_waypoints(d2, res)
    ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    ref = twin.waypoints(d2h, path, ln, st)
    for k in ("n", "status"):
        assert np.array_equal(got[k], ref[k]), k
    for q, e in enumerate(exp):
        assert got["status"][q] == e["status"] and got["n"][q] == e["n"], q
        if e["wp"] is not None:
            assert got["wp"][q, :e["n"]].tolist() == e["wp"], q
    assert {Q_NO_PATH, Q_BAD_PATH} <= set(got["status"].tolist())
    tr = ctx.path_waypoints(d2, dict(path=t(path[-1:]), len=t(ln[-1:]), status=None), Wmax=2)
    ctx.synchronize()
    assert int(tr["status"][0]) == Q_TRUNCATED and int(tr["n"][0]) == 3
    assert tr["wp"][0].cpu().tolist() == [around[0], around[2]]


def test_waypoints_feed_the_smoother(ctx, twin, oracle):
    """(b)'s waypoints in metres -> bezier_from_path with ragged npts: every control point finite, and ctrl equal to the
    CPU restatement to 1e-5 on 64 paths."""
    import torch
    from sea_current_amd import synth
    W = 1024
    d2, d2h, res = _plan(ctx, synth.block_grid(W, W, 0.20), 1024, 4, 4096)
    out = ctx.path_waypoints(d2, res, r2=4)
    ctx.synchronize()
    n = out["n"].cpu().numpy()
    keep = np.flatnonzero((out["status"].cpu().numpy() == Q_OK) & (n >= 2))
    assert keep.size >= 800
    wp = out["wp"].cpu().numpy()[keep]
    n = n[keep]
    n_max = int(n.max())
    cell_m = np.float32(0.05)
    pts = np.zeros((keep.size, n_max, 2), np.float32)
    for b in range(keep.size):
        c = wp[b, :n[b]]
        pts[b, :n[b], 0] = (c % W).astype(np.float32) * cell_m
        pts[b, :n[b], 1] = (c // W).astype(np.float32) * cell_m
    ctrl = ctx.bezier_from_path(torch.from_numpy(pts).cuda(), torch.from_numpy(n.astype(np.int32)).cuda())
    ctx.synchronize()
    ctrl = ctrl.cpu().numpy()
    for b in range(keep.size):
        assert np.isfinite(ctrl[b, :n[b] - 1]).all(), b
    for b in range(64):
        ref = oracle.bezier_from_path(pts[b, :n[b]])
        assert np.abs(ctrl[b, :n[b] - 1] - ref).max() < 1e-5, b
