"""sc_smooth_paths_batch (Context.smooth_paths): the post-planner sequence of examples/zmq_test.cpp:66-93 for a batch of
ragged paths in one device call.  Checked against the recorded run, bit for bit against pipeline.smooth_batch (the same
kernels glued by torch), path by path against the CPU sequence with per-path limits, its statuses and capacity rule, the
device chain EDT -> A* -> waypoints -> cells_to_points -> smooth_paths without a host hop, and sc_cells_to_points_batch
against occupancy_grid::centre_of restated in NumPy."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SAMPLE_KEYS = ("time", "pos", "vel", "acc", "pts", "curvature", "ang_vel", "tpar", "seg")


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bench_wp(ctx):
    """The bench's smoothing workload: A* paths of a 1024^2 salt20 map, 16 waypoints each (0.05 m cells)."""
    import torch
    from sea_current_amd import pipeline, synth
    occ = synth.salt_grid(1024, 1024, 0.20)
    d2 = ctx.edt(torch.from_numpy(occ).cuda())
    s, g = synth.queries(d2.cpu().numpy() >= 1, 1024)
    res = ctx.astar_batch(d2, torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda(), Lmax=4096)
    ctx.synchronize()
    ln, st = res["len"].cpu().numpy(), res["status"].cpu().numpy()
    ok = (st == 0) & (ln >= 64)
    assert ok.sum() >= 900
    return pipeline.waypoints_from_cells(res["path"].cpu().numpy()[ok], ln[ok], 1024, n_wp=16, cell_m=0.05)


def _np(o):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in o.items()}


def _smooth(ctx, wp, npts=None, limits=(-1.0, 1.0, -0.5, 0.5), **kw):
    import torch
    wp_d = torch.from_numpy(np.ascontiguousarray(wp, dtype=np.float32)).cuda()
    if npts is None:
        npts = np.full(wp.shape[0], wp.shape[1], np.int32)
    lim = torch.from_numpy(np.array(np.broadcast_to(np.asarray(limits, np.float64), (wp.shape[0], 4)))).cuda()
    out = ctx.smooth_paths(wp_d, torch.from_numpy(np.asarray(npts, np.int32)).cuda(), lim, **kw)
    ctx.synchronize()
    return _np(out)


def _path(o, p):
    """Per-path view of a result: the path's legs and samples."""
    a, b = int(o["seg_off"][p]), int(o["seg_off"][p + 1])
    s, L = int(o["offsets"][p]), int(o["length"][p])
    d = dict(ctrl=o["ctrl"][a:b], arclength=o["arclength"][p], length=L, status=o["status"][p])
    if o["status"][p] == 0:
        d.update({k: o[k][s:s + L] for k in SAMPLE_KEYS})
    return d


def _same_path(x, y):
    for k in x:
        assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), k


def test_recorded_run_as_one_call(ctx, golden_dir):
    fx = np.load(os.path.join(golden_dir, "toppra_1dof_output.npz"))
    lim = (float(fx["vel_lim"][0]), float(fx["vel_lim"][1]), float(fx["acc_lim"][0]), float(fx["acc_lim"][1]))
    o = _smooth(ctx, fx["waypoints"][None], limits=lim)
    assert int(o["status"][0]) == 0 and int(o["length"][0]) == 4328 == int(o["needed"][0])
    # time: the recording's arclength is the reference's; this one comes from the GL-32 tables on the GPU, a few units in
    # the last place apart, which moves T as much.  Bit-equal to the TOPP-RA + sampler entries on this arclength, and
    # within test_cpp_header's bar of the recording.
    import torch
    t = lambda v: torch.tensor([[v]], dtype=torch.float64).cuda()
    AL = float(o["arclength"][0])
    assert abs(AL - float(fx["arclength"])) <= 2e-6 * float(fx["arclength"])
    tp = ctx.toppra(t(0.0), t(AL), t(0.0), t(0.0), t(lim[0]), t(lim[1]), t(lim[2]), t(lim[3]), N=100)
    smp = ctx.toppra_sample(t(0.0), t(AL), t(0.0), t(0.0), tp["x"], tp["t"], float(np.float32(0.02)), 4400)
    ctx.synchronize()
    assert int(smp["length"][0]) == 4328
    assert np.array_equal(o["time"], smp["time"][0, :4328].cpu().numpy())
    assert np.array_equal(o["vel"], smp["vel"][0, 0, :4328].cpu().numpy())
    assert np.abs(o["time"] - fx["time"]).max() < 2e-5
    assert np.abs(o["pts"][:, 0] - fx["pos_x"]).max() < 5e-5 and np.abs(o["pts"][:, 1] - fx["pos_y"]).max() < 5e-5
    assert np.abs(o["ang_vel"] - fx["ang_vel"]).max() < 2e-6


def test_bench_batch_bit_equal_to_pipeline(ctx, bench_wp):
    import torch
    from sea_current_amd import pipeline
    o = _smooth(ctx, bench_wp)
    ref = _np(pipeline.smooth_batch(ctx, torch.from_numpy(bench_wp).cuda(), vmax=1.0, amax=0.5, dt=0.02, N=100))
    ctx.synchronize()
    P = bench_wp.shape[0]
    assert (o["status"] == 0).all() and (ref["toppra_status"] == 0).all() and (ref["resample_status"] == 0).all()
    assert np.array_equal(o["seg_off"], np.arange(P + 1, dtype=np.int32) * 15)
    for k in ("ctrl", "arclength", "length", "offsets", "pos", "vel", "pts", "curvature", "ang_vel"):
        assert np.array_equal(o[k], ref[k]), k
    assert int(o["needed"][0]) == int(ref["offsets"][-1])


def _ragged(ctx, W=1024, Q=256, seed=7):
    import torch
    from sea_current_amd import synth
    occ = synth.block_grid(W, W, 0.2, seed=seed)
    d2 = ctx.edt(torch.from_numpy(occ).cuda())
    s, g = synth.queries(d2.cpu().numpy() >= 4, Q)
    res = ctx.astar_batch(d2, torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda(), r2=4, Lmax=4096)
    wr = ctx.path_waypoints(d2, res, r2=4, Wmax=256)
    path, npts = ctx.cells_to_points(wr, W, 0.0, 0.0, 0.05, 0.05)
    ctx.synchronize()
    return path, npts


def test_ragged_waypoints_match_cpu_sequence(ctx, oracle):
    import torch
    path, npts = _ragged(ctx)
    P = path.shape[0]
    pairs = np.array([(1.0, 0.5), (0.6, 0.3), (1.5, 1.0), (0.4, 0.8)])
    pick = np.random.default_rng(11).integers(0, len(pairs), P)
    lim = np.stack([-pairs[pick, 0], pairs[pick, 0], -pairs[pick, 1], pairs[pick, 1]], axis=1)
    out = _np(ctx.smooth_paths(path, npts, torch.from_numpy(lim).cuda()))
    wp, n = path.cpu().numpy(), npts.cpu().numpy()
    assert (n >= 2).sum() >= 200
    assert len(np.unique(n[n >= 2])) > 3                     # ragged
    checked = same_len = 0
    for b in range(P):
        if n[b] < 2:
            assert out["status"][b] == 1 and out["length"][b] == 0
            continue
        if out["status"][b] != 0:
            assert out["status"][b] == 2 and not np.isfinite(oracle.bezier_from_path(wp[b, :n[b]])).all(), b
            continue
        ref = oracle.smooth_one(wp[b, :n[b]], vmax=pairs[pick[b], 0], amax=pairs[pick[b], 1], dt=0.02, N=100)
        v = _path(out, b)
        checked += 1
        assert ref["toppra_status"] == 0
        assert abs(float(v["arclength"]) - float(ref["arclength"])) <= 2e-6 * float(ref["arclength"]), b
        assert np.abs(v["ctrl"] - ref["ctrl"]).max() < 1e-5, b
        assert abs(v["length"] - ref["length"]) <= 1, b
        if v["length"] != ref["length"]:
            continue
        same_len += 1
        assert ref["status"] == 0
        assert np.abs(v["pos"] - ref["pos"]).max() < 2e-4, b
        assert np.abs(v["vel"] - ref["vel"]).max() < 2e-5, b
        assert np.abs(v["pts"] - ref["pts"]).max() < 2e-4, b
        k = np.abs(ref["curvature"]) < 1e2
        assert np.allclose(v["curvature"][k], ref["curvature"][k], rtol=2e-3, atol=2e-3), b
    assert checked >= 0.9 * (n >= 2).sum() and same_len >= 0.95 * checked


def _collinear_candidates(oracle):
    """Waypoint lists whose middle triple is collinear up to float32 rounding; the oracle's tangent rule gives NaN."""
    rng = np.random.default_rng(0)
    out = []
    while len(out) < 4:
        a = rng.integers(1, 50, 2).astype(np.float32) * np.float32(0.05)
        d = rng.integers(1, 20, 2)
        wp = np.array([[0, 0], a, a + d * np.float32(0.05), a + 2 * d * np.float32(0.05), [3, 0.1]], np.float32)
        if not np.isfinite(oracle.bezier_from_path(wp)).all():
            out.append(wp)
    return out


def test_statuses_leave_the_other_paths_alone(ctx, bench_wp, oracle):
    import torch
    good = bench_wp[:12, :5].copy()                           # 5-point paths
    bad_n = good[0].copy()
    col = _collinear_candidates(oracle)
    assert oracle.toppra([0.0], [3.0], [0.0], [0.0], [0.1], [1.0], [-0.5], [0.5])["status"] != 0   # vel_min > 0: infeasible
    nan_wp = good[1].copy()
    nan_wp[2, 1] = np.nan
    zero = np.repeat(good[3][:1], 5, axis=0)                  # two equal waypoints: a path of length 0
    # 0-3 good, 4 npts = 1, 5-8 good, 9-12 float-collinear, 13-16 good, 17 vel_min > 0, 18 a NaN waypoint,
    # 19 npts = n_max + 1, 20 zero length, 21 good
    wp = np.concatenate([good[:4], bad_n[None], good[4:8], np.stack(col), good[8:12], good[:1], nan_wp[None], good[2:3],
                         zero[None], good[2:3]])
    npts = np.full(wp.shape[0], 5, np.int32)
    npts[4] = 1
    npts[19] = 6
    npts[20] = 2
    lim = np.tile(np.array([-1.0, 1.0, -0.5, 0.5]), (wp.shape[0], 1))
    lim[17] = (0.1, 1.0, -0.5, 0.5)
    o = _smooth(ctx, wp, npts, lim)
    ref = _smooth(ctx, good)
    st = o["status"]
    assert st[4] == 1 and o["length"][4] == 0 and o["seg_off"][5] == o["seg_off"][4]
    ctrl_col = ctx.bezier_from_path(torch.from_numpy(np.stack(col)).cuda(), torch.full((4,), 5, dtype=torch.int32).cuda()).cpu().numpy()
    nan_rows = ~np.isfinite(ctrl_col.reshape(4, -1)).all(axis=1)
    assert nan_rows.any()
    assert np.array_equal(st[9:13] == 2, nan_rows) and (st[9:13][~nan_rows] == 0).all()
    assert (o["length"][9:13][nan_rows] == 0).all()
    assert st[17] == 3 and o["length"][17] == 0
    for b in (18, 19):                                        # BAD_INPUT: no legs, no samples
        assert st[b] == 1 and o["length"][b] == 0 and o["seg_off"][b + 1] == o["seg_off"][b], b
    # zero length: the library's own steps give finite control points (the end tangent is 0.5 * (0, 0)), arclength 0 and
    # a feasible TOPP-RA problem whose knots after the first are all dropped: no sample, so the resample finds a leg
    # without one (where the reference indexes out of range)
    t = lambda v: torch.tensor([[v]], dtype=torch.float64).cuda()
    cz = ctx.bezier_from_path(torch.from_numpy(zero[None, :2].copy()).cuda(), torch.tensor([2], dtype=torch.int32).cuda())
    tz = ctx.toppra(t(0.0), t(0.0), t(0.0), t(0.0), t(-1.0), t(1.0), t(-0.5), t(0.5), N=100)
    sz = ctx.toppra_sample(t(0.0), t(0.0), t(0.0), t(0.0), tz["x"], tz["t"], float(np.float32(0.02)), 8)
    ctx.synchronize()
    assert np.isfinite(cz.cpu().numpy()).all() and int(tz["status"][0]) == 0 and int(sz["length"][0]) == 0
    assert o["arclength"][20] == 0 and st[20] == 5 and o["length"][20] == 0
    goods = [0, 1, 2, 3, 5, 6, 7, 8, 13, 14, 15, 16, 21]
    for i, b in zip(list(range(12)) + [2], goods):
        assert st[b] == 0
        _same_path(_path(o, b), _path(ref, i))


def test_capacity_truncates_a_suffix_and_keeps_the_rest(ctx, bench_wp):
    import torch
    full = _smooth(ctx, bench_wp)
    need = int(full["needed"][0])
    cap = need // 2
    P = bench_wp.shape[0]
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")
    canary = dict(ctrl=f(P * 15, 4, 2), seg_off=torch.zeros(P + 1, dtype=torch.int32, device="cuda"), arclength=f(P),
                  length=torch.zeros(P, dtype=torch.int32, device="cuda"), offsets=torch.zeros(P + 1, dtype=torch.int32, device="cuda"),
                  status=torch.zeros(P, dtype=torch.int32, device="cuda"), needed=torch.zeros(1, dtype=torch.int64, device="cuda"),
                  time=torch.full((cap,), -7.0, dtype=torch.float64, device="cuda"), pos=f(cap), vel=f(cap), acc=f(cap), pts=f(cap, 2),
                  curvature=f(cap), ang_vel=f(cap), tpar=f(cap), seg=torch.full((cap,), -7, dtype=torch.int32, device="cuda"))
    o = _smooth(ctx, bench_wp, capacity=cap, out=canary)
    assert int(o["needed"][0]) == need
    assert np.array_equal(o["length"], full["length"]) and np.array_equal(o["offsets"], full["offsets"])
    fits = full["offsets"][1:] <= cap
    assert fits.any() and not fits.all()
    assert (o["status"][fits] == 0).all() and (o["status"][~fits] == 4).all()
    assert np.all(np.diff(fits.astype(int)) <= 0)             # a prefix fits
    written = int(full["offsets"][np.argmin(fits)])
    for k in SAMPLE_KEYS:
        assert np.array_equal(o[k][:written], full[k][:written]), k
        assert (o[k][written:] == -7).all(), k
    for b in np.flatnonzero(fits):
        _same_path(_path(o, b), _path(full, b))


def test_device_chain_without_host_hop(ctx):
    import torch
    from sea_current_amd import synth
    W = 1024
    occ = torch.from_numpy(synth.salt_grid(W, W, 0.05, seed=3)).cuda()
    lim = torch.tensor([[-1.0, 1.0, -0.5, 0.5]], dtype=torch.float64).cuda().expand(512, 4).contiguous()
    s, g = synth.queries(synth.salt_grid(W, W, 0.05, seed=3) == 0, 512, seed=5)
    s, g = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()

    def chain(hop):
        def h(x):
            if not hop:
                return x
            ctx.synchronize()
            return {k: v.cpu().cuda() for k, v in x.items()} if isinstance(x, dict) else x.cpu().cuda()
        d2 = h(ctx.edt(occ))
        res = h(ctx.astar_batch(d2, s, g, r2=1, Lmax=4096))
        wr = h(ctx.path_waypoints(d2, res, r2=1, Wmax=128))
        path, npts = ctx.cells_to_points(wr, W, 0.0, 0.0, 0.05, 0.05)
        path, npts = h(path), h(npts)
        o = ctx.smooth_paths(path, npts, lim, capacity=512 * 3000)
        ctx.synchronize()
        return _np(o)

    a, b = chain(False), chain(True)
    M = int(a["needed"][0])
    assert (a["status"] == 0).sum() >= 300 and M <= 512 * 3000 and (a["status"] != 4).all()
    S = int(a["seg_off"][-1])
    for k in a:                                               # what the call wrote (the buffers come from torch.empty)
        n = S if k == "ctrl" else M if k in SAMPLE_KEYS else None
        assert np.array_equal(a[k][:n], b[k][:n], equal_nan=True), k


def test_cells_to_points_is_centre_of(ctx):
    import torch
    W, Q, Wmax = 300, 64, 40
    x_min, y_min = np.float32(-3.3), np.float32(-3.3)
    res = np.float32(np.float32(7.7) / np.float32(300))
    rng = np.random.default_rng(2)
    wp = rng.integers(0, W * W, (Q, Wmax)).astype(np.int32)
    n = rng.integers(0, Wmax + 3, Q).astype(np.int32)
    st = np.where(rng.random(Q) < 0.15, 1, 0).astype(np.int32)
    t = lambda a: torch.from_numpy(a).cuda()
    wr = dict(wp=t(wp), n=t(n), status=t(st))
    starts = rng.random((Q, 2)).astype(np.float32)
    goals = rng.random((Q, 2)).astype(np.float32)
    for ends in (False, True):
        path, npts = ctx.cells_to_points(wr, W, float(x_min), float(y_min), float(res), float(res),
                                         t(starts) if ends else None, t(goals) if ends else None)
        path, npts = path.cpu().numpy(), npts.cpu().numpy()
        for q in range(Q):
            ok = st[q] == 0 and 1 <= n[q] <= Wmax
            exp_n = (max(n[q], 2) if ends else n[q]) if ok else 0
            assert npts[q] == exp_n, q
            c = wp[q, :exp_n]
            cx = x_min + ((c % W).astype(np.float32) + np.float32(0.5)) * res
            cy = y_min + ((c // W).astype(np.float32) + np.float32(0.5)) * res
            e = np.stack([cx, cy], axis=1).astype(np.float32)
            if ends and exp_n:
                e[0], e[exp_n - 1] = starts[q], goals[q]
            assert np.array_equal(path[q, :exp_n], e), q
            assert (path[q, exp_n:] == 0).all(), q


def test_host_form_equals_device_form(ctx, bench_wp):
    """sc_smooth_paths_batch_host against Context.smooth_paths on the same inputs, (a) with a capacity that truncates a path and
    (b) with the optional outputs null: the per-path outputs byte-equal, the samples byte-equal as far as they are written,
    and nothing copied back past them."""
    import sea_current_amd as sc
    wp = np.ascontiguousarray(bench_wp[:256], dtype=np.float32)
    P, n_max, _ = wp.shape
    npts = np.full(P, n_max, np.int32)
    lim = (-1.0, 1.0, -0.5, 0.5)
    full = _smooth(ctx, wp)
    need = int(full["needed"][0])
    cap = need // 2
    dev = _smooth(ctx, wp, capacity=cap)
    assert (dev["status"] == 4).any() and (dev["status"] == 0).any()
    host = ctx.smooth_paths_host(wp, npts, lim, cap)
    written = int(dev["offsets"][np.argmax(dev["status"] == 4)])

    def same(d, h, keys, n):
        for k in ("seg_off", "arclength", "length", "offsets", "status", "needed"):
            assert d[k].tobytes() == h[k].tobytes(), k
        L = int(h["seg_off"][P])
        assert d["ctrl"][:L].tobytes() == h["ctrl"][:L].tobytes() and not h["ctrl"][L:].any()
        for k in keys:
            assert d[k][:n].tobytes() == h[k][:n].tobytes(), k
            assert not h[k][n:].any(), k

    same(dev, host, SAMPLE_KEYS, written)
    # (b) time, vel, acc, curvature, ang_vel, tpar, seg null; room for every sample
    o = dict(ctrl=np.zeros((P * (n_max - 1), 4, 2), np.float32), seg_off=np.zeros(P + 1, np.int32), arclength=np.zeros(P, np.float32),
             length=np.zeros(P, np.int32), offsets=np.zeros(P + 1, np.int32), status=np.zeros(P, np.int32), needed=np.zeros(1, np.int64),
             pos=np.zeros(need + 5, np.float32), pts=np.zeros((need + 5, 2), np.float32))
    p = sc._ptr
    limits = np.ascontiguousarray(np.broadcast_to(np.array(lim), (P, 4)))
    assert sc.lib().sc_smooth_paths_batch_host(ctx._h, p(wp), p(npts), P, n_max, p(limits), float("nan"), None, 0, 0.02, 100, 100, need + 5,
                                               *[p(o.get(k)) for k in ("ctrl", "seg_off", "arclength", "length", "offsets", "status",
                                                                       "needed", "time", "pos", "vel", "acc", "pts", "curvature",
                                                                       "ang_vel", "tpar", "seg")]) == 0
    same(full, o, ("pos", "pts"), need)
