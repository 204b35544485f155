"""Per-stage speed limits from curvature and clearance (sc_speed_limits_batch, sc_smooth_paths_limited_batch): the kernel
against its NumPy twin on the GPU's own legs and tables, the limited call against the plain one with every term off, against
its pieces run by hand and against the CPU chain, the effect on a tight corner, statuses, argument errors, host forms and
the device chain without a host hop.  Small shapes: 1, 2 and 69 legs, an empty path, a path leaving the grid."""
import os

import numpy as np
import pytest

import speed_twin

pytestmark = pytest.mark.gpu

INF = float("inf")
SAMPLE_KEYS = ("time", "pos", "vel", "acc", "pts", "curvature", "ang_vel", "tpar", "seg")
RES = np.float32(np.float32(7.7) / np.float32(300))
X_MIN = np.float32(-3.3)
FRAME = (X_MIN, X_MIN, RES, RES)                                  # 64 x 48 cells: x in [-3.3, -1.657], y in [-3.3, -2.068]
DYN = (0.8, 0.3, 0.05, 1.0)


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(o):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in o.items()}


def _zigzag(n, seed):
    """n waypoints left to right through the grid, alternating about y = -2.7 by a seeded amplitude."""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(-3.2, -1.8, n))
    y = -2.7 + np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * rng.uniform(0.1, 0.4, n)
    return np.stack([x, y], axis=1).astype(np.float32)


def _paths():
    """wp [5, 70, 2], npts: 2, 3 and 70 waypoints (1, 2 and 69 legs), an empty path, and 3 waypoints that leave the grid."""
    wp = np.zeros((5, 70, 2), np.float32)
    npts = np.array([2, 3, 70, 0, 3], np.int32)
    for p, seed in ((0, 21), (1, 22), (2, 23)):
        wp[p, :npts[p]] = _zigzag(npts[p], seed)
    wp[4, :3] = np.array([[-3.0, -2.5], [-1.9, -2.9], [-1.0, -1.6]], np.float32)
    return wp, npts


LIMITS = np.array([[-1.0, 1.0, -0.5, 0.5], [-0.6, 0.6, -0.3, 0.3], [-1.0, 1.0, -0.5, 0.5], [-1.0, 1.0, -0.5, 0.5], [-0.6, 0.6, -0.5, 0.5]])


@pytest.fixture(scope="module")
def grids(ctx):
    """name -> (d2 on the GPU, d2 as NumPy, frame)."""
    occ = np.zeros((48, 64), np.uint8)
    occ[4:9, 6:12] = 1
    occ[30:40, 22:30] = 1
    occ[10:14, 50:64] = 1
    occ[44:48, 0:64:3] = 1
    col = np.zeros((40, 1), np.uint8)                             # 1 x 40 and 40 x 1 cells of 0.03 m under the paths
    col[[3, 17, 18]] = 1
    row = np.zeros((1, 40), np.uint8)
    row[0, [0, 25]] = 1
    out = {}
    for name, o, fr in (("main", occ, FRAME), ("column", col, (np.float32(-2.6), np.float32(-3.2), np.float32(0.03), np.float32(0.03))),
                        ("row", row, (np.float32(-3.2), np.float32(-2.7), np.float32(0.03), np.float32(0.03))),
                        ("empty", np.zeros((48, 64), np.uint8), FRAME)):
        d2 = ctx.edt(_t(o))
        out[name] = (d2, d2.cpu().numpy(), fr)
    assert (out["empty"][1] == 2**31 - 1).all()
    out["none"] = (None, None, None)
    return out


_legs_cache = {}


def _legs(ctx, nsub):
    """The GPU's own legs of _paths(): ctrl, seg_off and status from smooth_paths, tables from bezier_arclength at nsub, and the
    arclength as the float32 sum of the legs in leg order (what smooth_paths itself reports at its nsub)."""
    import torch
    if nsub not in _legs_cache:
        wp, npts = _paths()
        o = ctx.smooth_paths(_t(wp), _t(npts), _t(LIMITS), nsub=100, capacity=1 << 17)
        S = int(o["seg_off"][-1])
        ctrl = o["ctrl"][:S].contiguous()
        cum, seg_len = ctx.bezier_arclength(ctrl, nsub)
        ctx.synchronize()
        st, so, sl = o["status"].cpu().numpy(), o["seg_off"].cpu().numpy(), seg_len.cpu().numpy()
        assert list(st) == [0, 0, 0, 1, 0] and S == 1 + 2 + 69 + 0 + 2
        AL = np.zeros(5, np.float32)
        for p in range(5):
            for j in range(so[p], so[p + 1]):
                AL[p] = sl[j] if j == so[p] else np.float32(AL[p] + sl[j])
        if nsub == 100:
            assert AL.tobytes() == o["arclength"].cpu().numpy().tobytes()
        _legs_cache[nsub] = dict(ctrl=ctrl, cum=cum, seg_off=o["seg_off"].clone(), arclength=torch.from_numpy(AL).cuda(), status=o["status"].clone())
    return _legs_cache[nsub]


def _against_twin(ctx, grids, grid, N, J, nsub, dyn=DYN):
    L = _legs(ctx, nsub)
    d2, d2_h, fr = grids[grid]
    got = _np(ctx.speed_limits(L["ctrl"], L["cum"], L["seg_off"], L["arclength"], _t(LIMITS), dyn, N=N, J=J, status=L["status"], d2=d2, frame=fr))
    ctx.synchronize()
    ctrl, cum, so, AL = (L[k].cpu().numpy() for k in ("ctrl", "cum", "seg_off", "arclength"))
    assert list(got["status"]) == [0, 0, 0, 1, 0]
    assert (got["vhi"][3] == 1.0).all() and got["min_clear"][3] == 0.0       # the empty path: a harmless problem
    stages = flagged = 0
    for p in (0, 1, 2, 4):
        tw = speed_twin.speed_limits(ctrl[so[p]:so[p + 1]], cum[so[p]:so[p + 1]], AL[p], LIMITS[p], dyn, N=N, J=J, d2=d2_h, frame=fr)
        keep = ~tw["flagged"]
        stages += N + 1
        flagged += int(tw["flagged"].sum())
        err = np.abs(got["vhi"][p] - tw["vhi"])[keep] / np.abs(tw["vhi"][keep])
        print(f"grid {grid} N {N} J {J} nsub {nsub} path {p}: max rel err vhi {err.max():.3e}, min vhi {tw['vhi'].min():.6f}, "
              f"min_clear {got['min_clear'][p]!r} / {tw['min_clear']!r}")
        assert (err <= 1e-9).all(), (p, err.max())
        if np.isinf(tw["min_clear"]):
            assert np.isinf(got["min_clear"][p]) and got["min_clear"][p] > 0
        else:
            assert abs(float(got["min_clear"][p]) - float(np.float32(tw["min_clear"]))) <= 1e-9 * float(np.float32(tw["min_clear"])), p
    assert flagged <= 1e-3 * stages and flagged == 0
    return got


@pytest.mark.parametrize("N,J,nsub", [(100, 4, 100), (1, 1, 1), (7, 32, 10), (300, 4, 100), (100, 4, 512)],
                         ids=["workload", "smallest", "wide-window", "two-stage-chunks", "tables-past-lds"])
def test_standalone_against_twin_shapes(ctx, grids, N, J, nsub):
    """(300: more stages than one reduction pass holds; nsub 512: the 69 legs' tables, 141 KB, are read from global memory.)"""
    got = _against_twin(ctx, grids, "main", N, J, nsub)
    if N >= 100:
        assert (got["vhi"][[0, 1, 2, 4]].min(axis=1) < LIMITS[[0, 1, 2, 4], 1]).all()   # the terms bite on every path


@pytest.mark.parametrize("grid", ["column", "row", "empty", "none"])
def test_standalone_against_twin_grids(ctx, grids, grid):
    got = _against_twin(ctx, grids, grid, 100, 4, 100)
    if grid == "none":
        assert np.isinf(got["min_clear"][[0, 1, 2, 4]]).all()
    else:
        assert np.isfinite(got["min_clear"]).all()


def test_standalone_curvature_terms_alone(ctx, grids):
    """omega alone, a_lat alone, and the clearance switched off by an infinite floor although a grid is passed."""
    _against_twin(ctx, grids, "main", 100, 4, 100, dyn=(0.8, INF, INF, 0.0))
    got = _against_twin(ctx, grids, "main", 100, 4, 100, dyn=(INF, 0.3, INF, 2.0))
    assert np.isinf(got["min_clear"][[0, 1, 2, 4]]).all()


def _cut(o):
    """What a call wrote: legs up to seg_off[P], samples up to needed."""
    S, M = int(o["seg_off"][-1]), int(o["needed"][0])
    return {k: (v[:S] if k == "ctrl" else v[:M] if k in SAMPLE_KEYS else v) for k, v in o.items()}


def test_terms_off_is_the_plain_call_bit_for_bit(ctx, grids):
    wp, npts = _paths()
    d2, _, fr = grids["main"]
    a = _cut(_np(ctx.smooth_paths(_t(wp), _t(npts), _t(LIMITS), capacity=1 << 17)))
    b = _cut(_np(ctx.smooth_paths(_t(wp), _t(npts), _t(LIMITS), capacity=1 << 17, dyn=(INF, INF, INF, 0.0), J=4, d2=d2, frame=fr)))
    assert int(a["needed"][0]) > 1000 and list(a["status"]) == [0, 0, 0, 1, 0]
    assert set(b) - set(a) == {"vmax_stage", "min_clear"}
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for p in (0, 1, 2, 4):
        assert (b["vmax_stage"][p] == LIMITS[p, 1]).all() and b["min_clear"][p] == INF


@pytest.fixture(scope="module")
def limited(ctx, grids):
    """The limited call on the four usable paths (all OK), with everything a check needs."""
    wp, npts = _paths()
    keep = [0, 1, 2, 4]
    wp, npts, lim = wp[keep], npts[keep], LIMITS[keep]
    d2, d2_h, fr = grids["main"]
    o = ctx.smooth_paths(_t(wp), _t(npts), _t(lim), capacity=1 << 18, dyn=DYN, J=4, d2=d2, frame=fr)
    ctx.synchronize()
    assert (o["status"] == 0).all() and int(o["needed"][0]) <= 1 << 18
    return dict(o=o, lim=lim, d2=d2, d2_h=d2_h, fr=fr)


def test_composition_limits_are_the_standalone_call(ctx, limited):
    o = limited["o"]
    S = int(o["seg_off"][-1])
    ctrl = o["ctrl"][:S].contiguous()
    cum, _ = ctx.bezier_arclength(ctrl, 100)
    sl = ctx.speed_limits(ctrl, cum, o["seg_off"], o["arclength"], _t(limited["lim"]), DYN, N=100, J=4, status=o["status"], d2=limited["d2"],
                          frame=limited["fr"])
    ctx.synchronize()
    assert o["vmax_stage"].cpu().numpy().tobytes() == sl["vhi"].cpu().numpy().tobytes()
    assert o["min_clear"].cpu().numpy().tobytes() == sl["min_clear"].cpu().numpy().tobytes()
    assert (o["vmax_stage"].cpu().numpy().min(axis=1) < limited["lim"][:, 1]).all()


def test_composition_samples_are_the_pieces_by_hand(ctx, limited):
    """toppra_hermite with these limits per stage, the sampler, the resample: the bits of the one call."""
    import torch
    o, lim = limited["o"], limited["lim"]
    P = lim.shape[0]
    S, M = int(o["seg_off"][-1]), int(o["needed"][0])
    ctrl = o["ctrl"][:S].contiguous()
    cum, _ = ctx.bezier_arclength(ctrl, 100)
    z = torch.zeros((P, 1), dtype=torch.float64, device="cuda")
    p1 = o["arclength"].double().reshape(P, 1)
    vhi = o["vmax_stage"].reshape(P, 101, 1).contiguous()
    vlo = _t(lim[:, 0]).reshape(P, 1, 1).expand(P, 101, 1).contiguous()
    tp = ctx.toppra(z, p1, z, z, vlo, vhi, _t(lim[:, 2:3]), _t(lim[:, 3:4]), N=100)
    max_len = int(o["length"].max())
    smp = ctx.toppra_sample(z, p1, z, z, tp["x"], tp["t"], float(np.float32(0.02)), max_len=max_len)
    assert (tp["status"] == 0).all() and torch.equal(smp["length"], o["length"])
    keep = torch.arange(max_len, device="cuda")[None, :] < smp["length"][:, None]
    pos = smp["pos"][:, 0, :][keep].contiguous()
    rs = ctx.bezier_resample(ctrl, cum, o["arclength"], o["seg_off"], pos, o["offsets"], nudge=True)
    ctx.synchronize()
    eq = lambda a, b: a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert eq(o["pos"][:M], pos) and eq(o["vel"][:M], smp["vel"][:, 0, :][keep]) and eq(o["acc"][:M], smp["acc"][:, 0, :][keep])
    assert eq(o["time"][:M], smp["time"][keep])
    assert eq(o["pts"][:M], rs["pts"]) and eq(o["curvature"][:M], rs["curvature"]) and eq(o["tpar"][:M], rs["t"]) and eq(o["seg"][:M], rs["seg"])
    assert eq(o["ang_vel"][:M], smp["vel"][:, 0, :][keep] * rs["curvature"])


def test_composition_matches_the_cpu_chain(ctx, limited, oracle):
    """Twin limits -> oracle.toppra -> toppra_sample -> bezier_resample on the GPU's legs, with test_gpu_pipeline's bars."""
    o, lim = _np(limited["o"]), limited["lim"]
    S = int(o["seg_off"][-1])
    import torch
    cum = ctx.bezier_arclength(torch.from_numpy(o["ctrl"][:S]).cuda(), 100)[0].cpu().numpy()
    same_len = 0
    for p in range(lim.shape[0]):
        a, b = int(o["seg_off"][p]), int(o["seg_off"][p + 1])
        AL = o["arclength"][p]
        tw = speed_twin.speed_limits(o["ctrl"][a:b], cum[a:b], AL, lim[p], DYN, N=100, J=4, d2=limited["d2_h"], frame=limited["fr"])
        assert not tw["flagged"].any()
        r = oracle.toppra([0.0], [float(AL)], [0.0], [0.0], tw["vlo"][:, None], tw["vhi"][:, None], [lim[p, 2]], [lim[p, 3]], N=100)
        assert r["status"] == 0
        s = oracle.toppra_sample([0.0], [float(AL)], [0.0], [0.0], r["x"], r["t"], float(np.float32(0.02)))
        L = int(s["length"])
        assert abs(L - int(o["length"][p])) <= 1, p
        if L != int(o["length"][p]):
            continue
        same_len += 1
        rs = oracle.bezier_resample(o["ctrl"][a:b], cum[a:b], AL, s["pos"][0, :L].astype(np.float32).copy(), True)
        sl = slice(int(o["offsets"][p]), int(o["offsets"][p]) + L)
        assert rs["status"] == 0
        assert np.abs(o["pos"][sl] - rs["pos"]).max() < 2e-4, p
        assert np.abs(o["vel"][sl] - s["vel"][0, :L]).max() < 2e-5, p
        assert np.abs(o["pts"][sl] - rs["pts"]).max() < 2e-4, p
        k = np.abs(rs["curvature"]) < 1e2
        assert np.allclose(o["curvature"][sl][k], rs["curvature"][k], rtol=2e-3, atol=2e-3), p
    assert same_len >= 3


def test_effect_on_a_tight_corner(ctx, golden_dir):
    """The recorded example's corner, driven at up to 1 m/s: with omega_max the angular velocity peaks lower and the run
    takes longer.  The profile's spline overshoots between knots, so max |ang_vel| / omega_max is measured, not bounded."""
    fx = np.load(os.path.join(golden_dir, "toppra_1dof_output.npz"))
    wp, npts, lim = _t(fx["waypoints"][None]), _t(np.array([3], np.int32)), (-1.0, 1.0, -0.5, 0.5)
    omega = 0.25
    a = _np(ctx.smooth_paths(wp, npts, lim))
    b = _np(ctx.smooth_paths(wp, npts, lim, dyn=(omega, INF, INF, 0.0)))
    assert a["status"][0] == 0 and b["status"][0] == 0
    wa, wb = np.abs(a["ang_vel"]).max(), np.abs(b["ang_vel"]).max()
    print(f"max |ang_vel| unlimited {wa:.4f}, limited {wb:.4f}, omega_max {omega}, ratio {wb / omega:.4f}, "
          f"T {a['time'][-1]:.3f} -> {b['time'][-1]:.3f}")
    assert wb < wa and b["time"][-1] > a["time"][-1]
    assert b["vmax_stage"].min() < 1.0 and b["vmax_stage"].max() == 1.0


def _path(o, p):
    a, b = int(o["seg_off"][p]), int(o["seg_off"][p + 1])
    s, L = int(o["offsets"][p]), int(o["length"][p])
    d = dict(ctrl=o["ctrl"][a:b], arclength=o["arclength"][p], length=L, status=o["status"][p], vmax_stage=o["vmax_stage"][p],
             min_clear=o["min_clear"][p])
    d.update({k: o[k][s:s + L] for k in SAMPLE_KEYS})
    return d


def test_statuses_leave_the_other_paths_alone(ctx, grids):
    d2, d2_h, fr = grids["main"]
    good = _zigzag(3, 31)
    through = np.array([[-3.2, -2.3], [-2.5, -2.4], [-1.8, -2.35]], np.float32)   # crosses the block of rows 30..39, columns 22..29
    wp = np.stack([good, good, good, through, good, good, through])
    npts = np.full(7, 3, np.int32)
    dyn = np.tile(np.array(DYN), (7, 1))
    dyn[1, 0] = np.nan
    dyn[2, 1] = -0.3
    dyn[3, 2] = 0.0                                               # no crawl speed, through an occupied cell
    dyn[5, 3] = INF
    lim = (-1.0, 1.0, -0.5, 0.5)
    o = _np(ctx.smooth_paths(_t(wp), _t(npts), lim, dyn=_t(dyn), d2=d2, frame=fr))
    assert list(o["status"]) == [0, 1, 1, 3, 0, 1, 0], o["status"]
    assert o["min_clear"][3] == 0.0 and o["vmax_stage"][3].min() == 0.0 and (o["length"][[1, 2, 3, 5]] == 0).all()
    assert o["vmax_stage"][6].min() == DYN[2]                     # the same curve with a crawl speed gets through
    assert (o["vmax_stage"][[1, 2, 5]] == 1.0).all() and (o["min_clear"][[1, 2, 5]] == 0.0).all()
    ref = _np(ctx.smooth_paths(_t(wp[[0, 6]]), _t(npts[:2]), lim, dyn=DYN, d2=d2, frame=fr))
    for b, i in ((0, 0), (4, 0), (6, 1)):
        x, y = _path(o, b), _path(ref, i)
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), (b, k)
    # the capacity rule of the plain call: a suffix is truncated, lengths stay, what fits is written as before
    need = int(ref["needed"][0])
    cut = _np(ctx.smooth_paths(_t(wp[[0, 6]]), _t(npts[:2]), lim, dyn=DYN, d2=d2, frame=fr, capacity=need - 1))
    assert list(cut["status"]) == [0, 4] and np.array_equal(cut["length"], ref["length"]) and int(cut["needed"][0]) == need
    L0 = int(ref["length"][0])
    for k in SAMPLE_KEYS:
        assert np.array_equal(cut[k][:L0], ref[k][:L0]), k
    assert np.array_equal(cut["vmax_stage"], ref["vmax_stage"])


def test_argument_errors(ctx, grids):
    import sea_current_amd as sc
    L = _legs(ctx, 100)
    d2, _, fr = grids["main"]
    lim, dyn = _t(LIMITS), _t(np.tile(np.array(DYN), (5, 1)))
    for J in (0, 33):
        with pytest.raises(sc.SeaCurrentError):
            ctx.speed_limits(L["ctrl"], L["cum"], L["seg_off"], L["arclength"], lim, dyn, J=J)
        with pytest.raises(sc.SeaCurrentError):
            wp, npts = _paths()
            ctx.smooth_paths(_t(wp), _t(npts), lim, capacity=1024, dyn=dyn, J=J)
    p = sc._ptr
    vhi = _t(np.zeros((5, 101)))
    call = lambda dynp, d2p, W, H, rx=float(RES): sc.lib().sc_speed_limits_batch(
        ctx._h, p(L["ctrl"]), p(L["cum"]), p(L["seg_off"]), p(L["arclength"]), None, 5, 100, 100, 4, p(lim), dynp, d2p, W, H, float(X_MIN),
        float(X_MIN), rx, float(RES), p(vhi), None, None)
    assert call(p(dyn), p(d2), 64, 48) == 0
    assert call(None, None, 0, 0) == 1                            # NULL dyn
    assert call(p(dyn), None, 0, 0) == 0                          # no grid: the frame is ignored
    for W, H in ((0, 48), (64, 0), (8193, 48), (64, 8193)):
        assert call(p(dyn), p(d2), W, H) == 1, (W, H)
    assert call(p(dyn), p(d2), 64, 48, rx=0.0) == 1 and call(p(dyn), p(d2), 64, 48, rx=float("nan")) == 1
    ctx.synchronize()


def test_host_forms_equal_device_forms(ctx, grids):
    import sea_current_amd as sc
    L = _legs(ctx, 100)
    d2, d2_h, fr = grids["main"]
    dev = _np(ctx.speed_limits(L["ctrl"], L["cum"], L["seg_off"], L["arclength"], _t(LIMITS), DYN, status=L["status"], d2=d2, frame=fr))
    host = ctx.speed_limits_host(*(L[k].cpu().numpy() for k in ("ctrl", "cum", "seg_off", "arclength")), LIMITS, DYN,
                                 status=L["status"].cpu().numpy(), d2=d2_h, frame=fr)
    for k in ("vhi", "min_clear", "status"):
        assert dev[k].tobytes() == host[k].tobytes(), k
    wp, npts = _paths()
    full = _np(ctx.smooth_paths(_t(wp), _t(npts), _t(LIMITS), dyn=DYN, d2=d2, frame=fr))
    need = int(full["needed"][0])
    h = ctx.smooth_paths_host(wp, npts, LIMITS, need + 7, dyn=DYN, d2=d2_h, frame=fr)
    S = int(full["seg_off"][-1])
    for k in full:
        n = S if k == "ctrl" else need if k in SAMPLE_KEYS else None
        assert full[k][:n].tobytes() == h[k][:n].tobytes(), k
        if n is not None:
            assert not h[k][n:].any(), k
    bad = np.tile(np.array(DYN), (5, 1))
    bad[2, 0] = -1.0
    with pytest.raises(sc.SeaCurrentError):                       # the host forms refuse what the kernel marks BAD_INPUT
        ctx.smooth_paths_host(wp, npts, LIMITS, need, dyn=bad, d2=d2_h, frame=fr)
    with pytest.raises(sc.SeaCurrentError):
        ctx.speed_limits_host(*(L[k].cpu().numpy() for k in ("ctrl", "cum", "seg_off", "arclength")), LIMITS, bad)


def test_device_chain_without_host_hop(ctx):
    """astar_batch -> path_waypoints -> cells_to_points -> smooth_paths(dyn, d2) on one stream equals the same calls fed
    from host copies."""
    import torch
    from sea_current_amd import synth
    W, Q = 256, 64
    occ_h = synth.block_grid(W, W, 0.2, seed=7)
    d2 = ctx.edt(torch.from_numpy(occ_h).cuda())
    s, g = synth.queries(d2.cpu().numpy() >= 4, Q, seed=5)
    s, g = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    fr = (0.0, 0.0, 0.05, 0.05)

    def chain(hop):
        def h(x):
            if not hop:
                return x
            ctx.synchronize()
            return {k: v.cpu().cuda() for k, v in x.items()} if isinstance(x, dict) else x.cpu().cuda()
        res = h(ctx.astar_batch(d2, s, g, r2=4, Lmax=2048))
        wr = h(ctx.path_waypoints(d2, res, r2=4, Wmax=64))
        path, npts = ctx.cells_to_points(wr, W, 0.0, 0.0, 0.05, 0.05)
        path, npts = h(path), h(npts)
        o = ctx.smooth_paths(path, npts, (-1.0, 1.0, -0.5, 0.5), capacity=Q * 12000, dyn=(1.0, 0.5, 0.1, 1.0), d2=h(d2), frame=fr)
        ctx.synchronize()
        return _np(o)

    a, b = chain(False), chain(True)
    M, S = int(a["needed"][0]), int(a["seg_off"][-1])
    assert (a["status"] == 0).sum() >= Q // 2 and M <= Q * 12000 and (a["status"] != 4).all()
    ok = a["status"] == 0
    assert (a["vmax_stage"][ok].min(axis=1) < 1.0).any() and np.isfinite(a["min_clear"][ok]).all()
    for k in a:
        n = S if k == "ctrl" else M if k in SAMPLE_KEYS else None
        assert np.array_equal(a[k][:n], b[k][:n], equal_nan=True), k
