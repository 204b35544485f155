"""Space-time re-planning on the GPU (sc_traj_reserve_batch, sc_tplan_batch, sc_fleet_replan_batch) against the NumPy twin
exactly: status, arrive, len, the written part of path, the bit patterns of knots_out, res word for word and reach word for word
on the layers the definition specifies (t_start .. arrive, or .. L-1 without an arrival).  The step kernel works on tiles of 64
rows x 8 words (256 cells) behind a halo and advances SC_TPLAN_LAYERS layers per launch: the shapes sit on either side of a
word, of a tile and of a launch.  Then the entry points against each other, host forms, argument errors and the device chain
behind fleet_schedule."""
import os

import numpy as np
import pytest

import tplan_twin as tw
import traj_twin

pytestmark = pytest.mark.gpu

FRAME = (-3.3, 1.1, 0.1, 0.07)          # cells that are not square
OUT_INTS = ("status", "arrive", "len")


def _ctx(**env):
    import sea_current_amd as sc
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return sc.Context(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def ctx():
    c = _ctx()
    yield c
    c.close()


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(o):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in o.items()}


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pad_for(frame, r_new):
    rx, ry = np.float64(np.float32(frame[2])), np.float64(np.float32(frame[3]))
    return r_new + np.sqrt(rx * rx + ry * ry) / 2 * (1 + 2.0 ** -20)


def make_case(W, H, L, P=3, B=10, seed=0, salt=0.1, frame=FRAME, start=None, goal=None, t_max=4):
    """A seeded case: salt obstacles (the corners stay free), P random motions as knot rows (steps of up to two cells, some
    knots absent), B robots; the first four go from corner to corner, the others to a free cell within 8 columns and rows."""
    rng = np.random.default_rng(1000 * W + H + 7 * L + seed)
    free = rng.random((H, W)) >= salt
    corners = [0, W - 1, (H - 1) * W, H * W - 1]
    free.ravel()[corners] = True
    d2 = free.astype(np.int32)
    cells = np.nonzero(free.ravel())[0]
    cx, cy = tw.centres(W, H, frame)
    pos = np.stack([rng.uniform(cx[0], cx[-1] + 1e-9, P), rng.uniform(cy[0], cy[-1] + 1e-9, P)], axis=1)
    steps = rng.uniform(-2, 2, (P, L, 2)) * np.array([frame[2], frame[3]])
    steps[:, 0] = 0
    knots = pos[:, None, :] + np.cumsum(steps, axis=1)
    knots[rng.random((P, L)) < 0.08] = np.nan
    radius = rng.uniform(0.3, 0.8, P) * frame[2]
    if start is None:
        near = rng.choice(cells, max(B - 4, 0))
        gx = np.clip(near % W + rng.integers(-8, 9, len(near)), 0, W - 1)
        gy = np.clip(near // W + rng.integers(-8, 9, len(near)), 0, H - 1)
        to = np.where(free[gy, gx], gy * W + gx, near)
        start = np.concatenate([corners, near])[:B]
        goal = np.concatenate([corners[::-1], to])[:B]
    B = len(start)
    r_new = np.full(B, 0.3 * frame[2])
    return dict(W=W, H=H, L=L, frame=frame, d2=d2, knots=knots, radius=radius, start=np.asarray(start, np.int32), goal=np.asarray(goal, np.int32),
                t_start=rng.integers(0, min(t_max, L), B).astype(np.int32), r_new=r_new, pad=pad_for(frame, r_new[0]))


def twin(c, sequential=False, hold=1, select=None, tstatus=None):
    return tw.fleet_replan(c["knots"], tstatus, c["radius"], select, c["pad"], c["W"], c["H"], c["frame"], None, c["d2"], 0, c["start"], c["goal"],
                           c["t_start"], hold, r_new=c["r_new"], sequential=sequential, want_reach=True)


def gpu(ctx, c, sequential=False, hold=1, select=None, tstatus=None, want_reach=True):
    P = len(c["radius"])
    ts = _t(np.zeros(P, np.int32) if tstatus is None else np.asarray(tstatus, np.int32))
    o = ctx.fleet_replan(_t(c["knots"]), ts, _t(c["radius"]), _t(c["d2"]), _t(c["start"]), _t(c["goal"]), c["frame"], c["pad"], r_new=_t(c["r_new"]),
                         select=None if select is None else _t(np.asarray(select, np.int32)), t_start=_t(c["t_start"]), hold=hold,
                         sequential=sequential, want_reach=want_reach)
    ctx.synchronize()
    return _np(o)


def same_plan(got, ref, c, reach=True):
    W, L = c["W"], c["L"]
    for k in OUT_INTS:
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    for b in range(len(ref["status"])):
        n = ref["len"][b]
        assert np.array_equal(got["path"][b, :n], ref["path"][b, :n]), ("path", b)
    if "knots_out" in ref:
        assert np.array_equal(_bits(got["knots_out"]), _bits(ref["knots_out"])), "knots_out"
    if reach:
        t_start = c["t_start"] if c["t_start"] is not None else np.zeros(len(ref["status"]), np.int32)
        for b in range(len(ref["status"])):
            if ref["status"][b] in (tw.TP_OK, tw.TP_NO_PATH):
                t1 = ref["arrive"][b] if ref["status"][b] == tw.TP_OK else L - 1
                sl = slice(int(t_start[b]), int(t1) + 1)
                assert np.array_equal(_words(got["reach"][b, sl]), tw.pack(ref["reach"][b, sl])), ("reach", b)


def same(got, ref, c, reach=True):
    same_plan(got, ref, c, reach)
    assert np.array_equal(_words(got["res"]), tw.pack(ref["res"])), "res"
    if got.get("tstatus") is not None:
        assert np.array_equal(got["tstatus"], ref["tstatus"]), "tstatus"


@pytest.mark.parametrize("H", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("W", [1, 31, 32, 33, 64, 65, 70])
def test_word_and_tile_edges(ctx, W, H):
    c = make_case(W, H, 24)
    ref = twin(c)
    same(gpu(ctx, c), ref, c)
    if W * H > 64:
        assert ref["res"].any() and (ref["status"] == tw.TP_OK).any()


def test_across_tile_boundaries(ctx):
    """300 x 140 cells: two tiles across (the seam is at x = 256) and three down (y = 64, 128).  Starts and goals on either side of a
    word (x = 31 | 32), of the tile seams, and a diagonal through the tile corner (256, 64)."""
    W, H = 300, 140
    cell = lambda x, y: y * W + x
    start = [cell(31, 5), cell(32, 5), cell(255, 20), cell(256, 20), cell(100, 63), cell(100, 64), cell(250, 58), cell(262, 70), cell(10, 127),
             cell(299, 139)]
    goal = [cell(32, 5), cell(31, 5), cell(256, 20), cell(255, 20), cell(100, 64), cell(100, 63), cell(262, 70), cell(250, 58), cell(10, 128),
            cell(270, 120)]
    c = make_case(W, H, 40, P=4, salt=0.0, start=start, goal=goal, t_max=1)
    c["t_start"][:] = 0
    ref = twin(c)
    same(gpu(ctx, c), ref, c)
    free = tw.plan(c["d2"], 0, None, c["L"], c["start"], c["goal"], c["t_start"], 1)
    assert list(free["arrive"][:8]) == [1, 1, 1, 1, 1, 1, 12, 12] and (ref["status"] == tw.TP_OK).sum() >= 6


def _launch_case(h, L):
    """Goals at every distance 0 .. 2h+1 from the start along row 0 of an open grid: an arrival in every layer of the first two
    launches, the first and the last of each included, and (where the distance exceeds L-1) no path."""
    W, H = 70, 20
    n = 2 * h + 2
    start = [0] * n + [W * 12 + 69] * 2
    goal = list(range(n)) + [W * 12 + 60, W * 19]
    c = make_case(W, H, L, P=2, salt=0.0, start=start, goal=goal, t_max=1)
    c["knots"][..., 1] = np.maximum(c["knots"][..., 1], tw.centres(W, H, c["frame"])[1][10])   # the fleet stays clear of row 0 (NaN stays NaN)
    c["t_start"][-1] = min(1, L - 1)
    return c


@pytest.mark.parametrize("h", [1, 2, 3, 8, 16])
def test_layers_per_launch_change_nothing(h):
    cx = _ctx(SC_TPLAN_LAYERS=h)
    try:
        for L in (h, h + 1, 2 * h, 2 * h + 1):
            c = _launch_case(h, L)
            res = tw.reserve(c["knots"], None, c["radius"], None, c["pad"], c["W"], c["H"], c["frame"])[0] if L >= 2 else None
            ref = tw.plan(c["d2"], 0, res, L, c["start"], c["goal"], c["t_start"], 1, c["frame"], want_reach=True)
            o = cx.tplan(_t(c["d2"]), _t(c["start"]), _t(c["goal"]), res=None if res is None else _t(tw.pack(res).view(np.int32)), L=L,
                         t_start=_t(c["t_start"]), hold=True, frame=c["frame"], want_reach=True)
            cx.synchronize()
            same_plan(_np(o), ref, c)
            arr = ref["arrive"][:2 * h + 2]
            assert list(arr[:min(L, 2 * h + 2)]) == list(range(min(L, 2 * h + 2))) and (arr[L:] == -1).all()
    finally:
        cx.close()


@pytest.mark.parametrize("B", [1, 2, 65])
def test_batch_sizes(ctx, B):
    c = make_case(70, 45, 60, P=5, B=B, seed=B, t_max=20)
    same(gpu(ctx, c), twin(c), c)


def test_groups_within_a_small_budget():
    """70 x 45 x 60 layers are 32400 bytes a query: a budget of 100000 bytes serves 11 queries in groups of 3; caller-provided layers
    are not bounded by it; a budget below one query is an error that names the need."""
    import sea_current_amd as sc
    c = make_case(70, 45, 60, P=5, B=11, seed=3, t_max=20)
    ref = twin(c)
    cx = _ctx(SC_TPLAN_GB=100000 / 2 ** 30)
    try:
        same(gpu(cx, c, want_reach=False), ref, c, reach=False)
        same(gpu(cx, c, want_reach=True), ref, c)
    finally:
        cx.close()
    cx = _ctx(SC_TPLAN_GB=30000 / 2 ** 30)
    try:
        with pytest.raises(sc.SeaCurrentError, match="32400"):
            gpu(cx, c, want_reach=False)
        same(gpu(cx, c, want_reach=True), ref, c)
    finally:
        cx.close()


def test_scratch_layers_and_null_reservations(ctx):
    c = make_case(70, 45, 60, P=5, B=9, seed=4, t_max=20)
    ref = twin(c)
    same(gpu(ctx, c, want_reach=False), ref, c, reach=False)
    for hold in (0, 1):
        free = tw.plan(c["d2"], 0, None, c["L"], c["start"], c["goal"], c["t_start"], hold, c["frame"], want_reach=True)
        args = (_t(c["d2"]), _t(c["start"]), _t(c["goal"]))
        kw = dict(L=c["L"], t_start=_t(c["t_start"]), hold=hold, frame=c["frame"], want_reach=True)
        a = ctx.tplan(*args, res=None, **kw)
        z = ctx.tplan(*args, res=_t(np.zeros((c["L"], c["H"], 3), np.int32)), **kw)
        ctx.synchronize()
        same_plan(_np(a), free, c)
        same_plan(_np(z), free, c)
    same(gpu(ctx, c, hold=0), twin(c, hold=0), c)


def test_reserve_accumulates_selects_and_marks(ctx):
    c = make_case(70, 45, 60, P=6, seed=5)
    P = 6
    tail = (c["pad"], c["W"], c["H"], c["frame"])
    whole, _ = tw.reserve(c["knots"], None, c["radius"], None, *tail)
    first = np.array([1, 1, 1, 0, 0, 0], np.int32)
    part, _ = tw.reserve(c["knots"], None, c["radius"], first, *tail)
    assert whole.any() and part.any() and not np.array_equal(part, whole)
    kn, rad = _t(c["knots"]), _t(c["radius"])
    ts = _t(np.zeros(P, np.int32))
    r1 = ctx.traj_reserve(kn, ts, rad, c["W"], c["H"], c["frame"], c["pad"], select=_t(first))
    ctx.synchronize()
    assert np.array_equal(_words(r1.cpu().numpy()), tw.pack(part))
    r2 = ctx.traj_reserve(kn, ts, rad, c["W"], c["H"], c["frame"], c["pad"], select=_t(1 - first), res=r1)
    one = ctx.traj_reserve(kn, None, rad, c["W"], c["H"], c["frame"], c["pad"])
    ctx.synchronize()
    assert r2 is r1 and np.array_equal(_words(r2.cpu().numpy()), tw.pack(whole)) and np.array_equal(_words(one.cpu().numpy()), tw.pack(whole))
    bad = c["radius"].copy()
    bad[1], bad[4] = np.nan, -0.1
    tsb = np.array([0, 0, 0, 1, 0, 0], np.int32)
    ref, ref_ts = tw.reserve(c["knots"], tsb, bad, None, c["pad"], c["W"], c["H"], c["frame"])
    ts = _t(tsb)
    rb = ctx.traj_reserve(kn, ts, _t(bad), c["W"], c["H"], c["frame"], c["pad"])
    ctx.synchronize()
    assert list(ref_ts) == [0, 2, 0, 1, 2, 0] and np.array_equal(ts.cpu().numpy(), ref_ts)
    assert np.array_equal(_words(rb.cpu().numpy()), tw.pack(ref))
    # without a tstatus there is nothing to mark: the bad paths still reserve nothing
    rn = ctx.traj_reserve(kn, None, _t(bad), c["W"], c["H"], c["frame"], c["pad"])
    ctx.synchronize()
    assert np.array_equal(_words(rn.cpu().numpy()), tw.pack(tw.reserve(c["knots"], None, bad, None, c["pad"], c["W"], c["H"], c["frame"])[0]))


def test_sequential_equals_a_host_loop_of_single_calls(ctx):
    c = make_case(70, 45, 80, P=4, B=10, seed=6, t_max=10)
    c["goal"][5:] = c["goal"][:5]                      # contested goals: later robots meet parked earlier ones
    ref = twin(c, sequential=True)
    got = gpu(ctx, c, sequential=True)
    same(got, ref, c)
    assert not np.array_equal(ref["status"], twin(c)["status"]) or not np.array_equal(ref["arrive"], twin(c)["arrive"])
    res = ctx.traj_reserve(_t(c["knots"]), None, _t(c["radius"]), c["W"], c["H"], c["frame"], c["pad"])
    for i in range(10):
        o = ctx.tplan(_t(c["d2"]), _t(c["start"][i:i + 1]), _t(c["goal"][i:i + 1]), res=res, t_start=_t(c["t_start"][i:i + 1]), hold=True,
                      frame=c["frame"])
        ctx.traj_reserve(o["knots_out"], None, float(c["r_new"][i]), c["W"], c["H"], c["frame"], c["pad"], res=res)
        ctx.synchronize()
        o = _np(o)
        assert o["status"][0] == ref["status"][i] and o["arrive"][0] == ref["arrive"][i]
        assert np.array_equal(_bits(o["knots_out"][0]), _bits(ref["knots_out"][i]))
    assert np.array_equal(_words(res.cpu().numpy()), tw.pack(ref["res"]))
    P = 4
    rows = np.concatenate([c["knots"], got["knots_out"]])
    rep = traj_twin.conflicts(rows, np.zeros(P + 10, np.int32), 0.0, 0.1, np.concatenate([c["radius"], c["r_new"]]))
    assert (rep["n_conf"][P:] == 0).all()
    # a robot whose r_new is outside the contract is planned like the others and its row reserves nothing
    c["r_new"] = c["r_new"].copy()
    c["r_new"][0] = np.nan
    odd = twin(c, sequential=True)
    same(gpu(ctx, c, sequential=True), odd, c)
    assert odd["status"][5] == tw.TP_OK and ref["status"][5] == tw.TP_NO_PATH      # robot 5 shares robot 0's goal


def test_no_path_exactly_where_components_differ(ctx):
    rng = np.random.default_rng(12)
    occ = (rng.random((45, 70)) < 0.3).astype(np.uint8)
    d2 = ctx.edt(_t(occ))
    lab = ctx.components(d2)["label"]
    free = np.nonzero(occ.ravel() == 0)[0]
    start, goal = rng.choice(free, 64).astype(np.int32), rng.choice(free, 64).astype(np.int32)
    o = ctx.tplan(d2, _t(start), _t(goal), L=200, hold=True)
    ctx.synchronize()
    lab, o = lab.cpu().numpy().ravel(), _np(o)
    differ = lab[start] != lab[goal]
    assert np.array_equal(o["status"] == tw.TP_NO_PATH, differ) and np.array_equal(o["status"] == tw.TP_OK, ~differ)
    assert 4 <= differ.sum() <= 60
    ref = tw.plan(d2.cpu().numpy(), 0, None, 200, start, goal, None, 1)
    same_plan(o, ref, dict(W=70, L=200, t_start=None), reach=False)


def test_device_chain_without_host_hop(ctx):
    """astar_batch -> path_waypoints -> cells_to_points -> smooth_paths -> fleet_schedule -> fleet_replan -> traj_conflicts on one
    stream, on the 64 x 48 map of test_gpu_traj.py with two slots only, so that some of the dozen crossing paths stay unresolved.
    Every robot is offered to fleet_replan; t_start = -1 (a bad endpoint, NaN rows) keeps the scheduled ones out of it without the
    host looking at the slots.  The re-planned rows conflict with no scheduled path and with none of each other, and everything
    equals the twin."""
    import torch
    occ = np.zeros((48, 64), np.uint8)
    occ[4:9, 6:12] = 1
    occ[30:40, 22:30] = 1
    occ[10:14, 50:64] = 1
    occ[44:48, 0:64:3] = 1
    res = float(np.float32(np.float32(7.7) / np.float32(300)))
    x0 = float(np.float32(-3.3))
    frame = (x0, x0, res, res)
    d2 = ctx.edt(_t(occ))
    cell = lambda x, y: y * 64 + x
    ys = (16, 20, 24, 27, 18, 22)
    s = [cell(2, y) for y in ys] + [cell(60, y) for y in ys]
    g = [cell(60, y) for y in reversed(ys)] + [cell(2, y) for y in reversed(ys)]
    s, g = _t(np.array(s, np.int32)), _t(np.array(g, np.int32))
    Q, D, stride, K = 12, 2, 5, 160
    radius, t0, flags = 0.5 * res, np.linspace(0.0, 1.1, Q), np.zeros(Q, np.int32)
    pad = pad_for(frame, radius)
    r = ctx.astar_batch(d2, s, g, r2=1, Lmax=512)
    wr = ctx.path_waypoints(d2, r, r2=1, Wmax=64)
    path, npts = ctx.cells_to_points(wr, 64, x0, x0, res, res)
    sm = ctx.smooth_paths(path, npts, (-1.0, 1.0, -0.5, 0.5), capacity=Q * 2000)
    o = ctx.fleet_schedule(sm, radius, t0=_t(t0), flags=_t(flags), dt_c=0.1, K=K, D=D, stride=stride, want_knots=True)
    t_start = torch.where(o["slot"] == -1, torch.ceil(_t(t0) / 0.1).to(torch.int32), -1).to(torch.int32)
    p = ctx.fleet_replan(o["knots_out"], o["tstatus"], radius, d2, s, g, frame, pad, r_new=radius, select=(o["slot"] >= 0).to(torch.int32),
                         t_start=t_start, hold=True, r2=1, sequential=True, want_reach=True)
    rows = torch.cat([o["knots_out"], p["knots_out"]])
    left = ctx.traj_conflicts(rows, torch.zeros(2 * Q, dtype=torch.int32, device="cuda"), radius, dt_c=0.1, want_matrix=True)
    ctx.synchronize()
    o, p, left = _np(o), _np(p), _np(left)
    unresolved = o["slot"] == -1
    assert 1 <= unresolved.sum() <= Q - 1 and (o["slot"][~unresolved] >= 0).all()
    assert np.array_equal(p["status"] == tw.TP_BAD_ENDPOINT, ~unresolved) and (p["status"] == tw.TP_OK).sum() >= 1
    assert (left["n_conf"][Q:] == 0).all()
    t_start = t_start.cpu().numpy()
    c = dict(W=64, H=48, L=K + 1, t_start=t_start)
    ref = tw.fleet_replan(o["knots_out"], o["tstatus"], np.full(Q, radius), (o["slot"] >= 0).astype(np.int32), pad, 64, 48, frame, None,
                          d2.cpu().numpy(), 1, s.cpu().numpy(), g.cpu().numpy(), t_start, 1, r_new=np.full(Q, radius), sequential=True,
                          want_reach=True)
    same(p, ref, c)


def test_argument_errors(ctx):
    import sea_current_amd as sc
    import torch
    c = make_case(33, 9, 12)
    kn, rad, d2, s, g = _t(c["knots"]), _t(c["radius"]), _t(c["d2"]), _t(c["start"]), _t(c["goal"])
    ok = lambda **kw: ctx.fleet_replan(kn, None, rad, d2, s, g, **{"frame": c["frame"], "pad": c["pad"], **kw})
    ok()
    for kw in (dict(pad=-1.0), dict(pad=float("nan")), dict(pad=float("inf")), dict(frame=(0.0, 0.0, 0.0, 1.0)), dict(frame=(0.0, float("nan"), 1.0, 1.0)),
               dict(sequential=True)):                                   # sequential without r_new
        with pytest.raises(sc.SeaCurrentError):
            ok(**kw)
    st = torch.zeros(8, dtype=torch.int32, device="cuda")
    call = lambda **kw: ctx._l.sc_tplan_batch(ctx._h, kw.get("d2", d2.data_ptr()), kw.get("W", 33), kw.get("H", 9), 0, None, kw.get("L", 12),
                                              kw.get("start", s.data_ptr()), g.data_ptr(), None, kw.get("B", 8), 1, None, None, None,
                                              kw.get("status", st.data_ptr()), None, 0.0, 0.0, 1.0, 1.0, None)
    assert call() == 0
    res = torch.zeros((12, 9, 2), dtype=torch.int32, device="cuda")
    both = lambda K, L: ctx._l.sc_fleet_replan_batch(ctx._h, kn.data_ptr(), None, 3, K, rad.data_ptr(), None, c["pad"], 33, 9, 0.0, 0.0, 1.0, 1.0,
                                                     res.data_ptr(), d2.data_ptr(), 0, L, s.data_ptr(), g.data_ptr(), None, 8, 1, None, None, None,
                                                     st.data_ptr(), None, None, None, 0)
    assert both(11, 12) == 0 and both(11, 11) == 1 and both(10, 12) == 1                  # L != K + 1
    for kw in (dict(d2=None), dict(start=None), dict(status=None), dict(W=0), dict(H=8193), dict(L=0), dict(L=65537), dict(B=0), dict(B=65537)):
        assert call(**kw) == 1, kw
    rcall = lambda **kw: ctx._l.sc_traj_reserve_batch(ctx._h, kw.get("knots", kn.data_ptr()), None, kw.get("P", 3), kw.get("K", 11),
                                                      kw.get("radius", rad.data_ptr()), None, c["pad"], 33, kw.get("H", 9), 0.0, 0.0, 1.0, 1.0,
                                                      kw.get("res", res.data_ptr()))
    assert rcall() == 0
    for kw in (dict(knots=None), dict(radius=None), dict(res=None), dict(P=0), dict(P=16385), dict(K=0), dict(K=65536), dict(H=0)):
        assert rcall(**kw) == 1, kw
    ctx.synchronize()


def test_host_forms_equal_device_forms(ctx):
    import sea_current_amd as sc
    c = make_case(70, 45, 40, P=4, B=7, seed=8)
    ref = twin(c)
    for seq in (False, True):
        h = ctx.fleet_replan_host(c["knots"], np.zeros(4, np.int32), c["radius"], c["d2"], c["start"], c["goal"], c["frame"], c["pad"],
                                  r_new=c["r_new"], t_start=c["t_start"], sequential=seq, want_reach=True)
        same(h, twin(c, sequential=True) if seq else ref, c)
    res, ts = ctx.traj_reserve_host(c["knots"], np.zeros(4, np.int32), c["radius"], c["W"], c["H"], c["frame"], c["pad"])
    assert np.array_equal(res, tw.pack(ref["res"])) and (ts == 0).all()
    o = ctx.tplan_host(c["d2"], c["start"], c["goal"], res=res, t_start=c["t_start"], hold=True, frame=c["frame"], want_reach=True)
    same_plan(o, ref, c)
    bad = c["radius"].copy()
    bad[2] = -1.0
    with pytest.raises(sc.SeaCurrentError):
        ctx.traj_reserve_host(c["knots"], None, bad, c["W"], c["H"], c["frame"], c["pad"])
