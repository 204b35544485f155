"""Curves against the grid on the GPU (sc_curve_clearance_batch, sc_curve_clear_batch, sc_smooth_paths_clear_batch): the
check and the repair against their NumPy twin on the device's own legs, every integer equal and every float32 equal as bits;
the smoothing call against the limited call, against the repair run by hand and on a path that cannot be fixed; host forms
and argument errors.  Small shapes: 32 x 32 and 48 x 48 cells, paths of 1 to 5 legs, one of SC_CURVE_MAX_LEGS legs."""
import numpy as np
import pytest

import curve_twin as tw
from test_curve_twin import CASE_A, CASE_B, centres, wall_map

pytestmark = pytest.mark.gpu

FRAME1 = (0.0, 0.0, 1.0, 1.0)
FRAME_WIDE = (-48.0, -48.0, 1.0, 1.0)                             # 128 x 128 cells around the 32 x 32 maps: no curve leaves it
FRAME2 = (np.float32(-3.3), np.float32(1.7), np.float32(0.25), np.float32(0.2))   # res_x != res_y, 48 x 40 cells
LIMITS = (-1.0, 1.0, -0.5, 0.5)
THROUGH = [(4, 10), (20, 10), (26, 4)]                            # its first leg crosses the wall: shrinking cannot help
SAMPLE_KEYS = ("time", "pos", "vel", "acc", "pts", "curvature", "ang_vel", "tpar", "seg")


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


def _legs(ctx, wp, npts):
    """The device's own legs of the waypoints: ctrl [S,4,2], seg_off, status (torch) from smooth_paths.  Only what the legs
    themselves decide stays in the status (BAD_INPUT, NONFINITE): a path whose samples did not fit still has its legs."""
    import torch
    o = ctx.smooth_paths(_t(wp), _t(npts), LIMITS, N=20, nsub=20, capacity=1 << 16)
    ctx.synchronize()
    S = int(o["seg_off"][-1])
    st = o["status"]
    return o["ctrl"][:S].contiguous(), o["seg_off"], torch.where(st <= 2, st, torch.zeros_like(st))


def _pack(paths):
    n_max = max(len(p) for p in paths)
    wp = np.zeros((len(paths), n_max, 2), np.float32)
    for i, p in enumerate(paths):
        wp[i, :len(p)] = p
    return wp, np.array([len(p) for p in paths], np.int32)


@pytest.fixture(scope="module")
def worlds(ctx):
    """name -> dict(d2 on the GPU, d2n as NumPy, frame, ctrl, seg_off, status (torch) and their NumPy copies c, so, st)."""
    out = {}

    def add(name, occ, frame, wp, npts, skip=()):
        d2 = ctx.edt(_t(occ))
        ctrl, seg_off, status = _legs(ctx, wp, npts)
        for p in skip:                                            # a path that has legs but is not OK
            status[p] = 2
        ctx.synchronize()
        out[name] = dict(d2=d2, d2n=d2.cpu().numpy(), frame=frame, ctrl=ctrl, seg_off=seg_off, status=status, c=ctrl.cpu().numpy(),
                         so=seg_off.cpu().numpy(), st=status.cpu().numpy())

    for W, seed in ((32, 5), (48, 6)):
        occ, d2, wp, npts = tw.sweep_paths(W, W, seed, 100)
        add("sweep%d" % W, occ, FRAME1, wp, npts)
        assert np.array_equal(out["sweep%d" % W]["d2n"], d2)
    add("walls", wall_map(), FRAME1, *_pack([centres(CASE_A), centres(CASE_B), centres(THROUGH)]))
    # 48 x 40 cells of 0.25 x 0.2: a single short leg (fewer than 64 samples), long legs (more than 64), a path with legs
    # that is skipped in the middle, an empty path, a path that leaves the frame, and five legs round the blocks
    occ = np.zeros((40, 48), np.uint8)
    occ[10:16, 10:13] = 1
    occ[24:30, 20:34] = 1
    occ[5:8, 36:40] = 1
    xy = lambda cells: (np.array(cells, np.float32) * np.array([0.25, 0.2], np.float32) + np.array([-3.3, 1.7], np.float32)).astype(np.float32)
    paths = [xy([(3.5, 3.5), (5.2, 4.1)]), xy([(2.5, 30.5), (40.5, 35.5), (44.5, 3.5)]), xy([(4.5, 20.5), (15.5, 22.5), (16.5, 5.5)]),
             np.zeros((0, 2), np.float32), xy([(40.5, 20.5), (46.5, 22.5), (52.5, 20.5)]),
             xy([(6.5, 6.5), (8.5, 18.5), (15.5, 19.5), (18.5, 31.5), (36.5, 32.5), (37.5, 12.5)])]
    add("mixed", occ, FRAME2, *_pack(paths), skip=(2,))
    assert list(out["mixed"]["st"]) == [0, 0, 2, 1, 0, 0] and list(np.diff(out["mixed"]["so"])) == [1, 2, 2, 0, 2, 5]
    return out


CHECK_KEYS = ("leg_min", "path_min", "hit_legs", "hit_leg", "hit_t")
CLEAR_KEYS = ("ctrl", "level", "rounds", "leg_min", "status")


def _same(got, ref, keys, what):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        assert got[k].tobytes() == ref[k].tobytes(), (what, k, np.nonzero(got[k].reshape(-1) != ref[k].reshape(-1))[0][:8])


@pytest.mark.parametrize("name,r2", [("sweep32", 1), ("sweep48", 0), ("sweep48", 5), ("walls", 1), ("walls", 4), ("mixed", 1), ("mixed", 3)])
def test_check_against_twin(ctx, worlds, name, r2):
    w = worlds[name]
    got = _np(ctx.curve_clearance(w["ctrl"], w["seg_off"], w["d2"], w["frame"], r2, status=w["status"]))
    ref = tw.clearance(w["c"], w["so"], w["d2n"], w["frame"], r2, status=w["st"])
    _same(got, ref, CHECK_KEYS, name)
    if name == "mixed":
        n = [tw.leg_count(c, w["frame"])[0] for c in w["c"]]
        assert n[0] < 63 and max(n) > 200                         # a short wave and several strides with a tail
        assert got["hit_leg"][4] >= 0 and got["path_min"][4] == 0   # leaves the frame
        assert got["path_min"][3] == 0 and got["hit_leg"][2] == -1 and (got["leg_min"][3:5] == -1).all()   # skipped: untouched
    if name.startswith("sweep"):
        assert (got["hit_legs"] > 0).sum() > len(got["hit_legs"]) / 4
    # status None: every path is evaluated
    if name == "walls":
        none = _np(ctx.curve_clearance(w["ctrl"], w["seg_off"], w["d2"], w["frame"], r2))
        _same(none, ref, CHECK_KEYS, name)
        assert list(got["leg_min"][:6]) == [13, 0, 0, 1, 0, 1]


@pytest.mark.parametrize("name,r2,max_level", [("sweep32", 1, 6), ("sweep48", 1, 6), ("sweep48", 3, 1), ("walls", 1, 6), ("walls", 1, 1),
                                               ("walls", 4, 30), ("mixed", 1, 6), ("mixed", 2, 30)])
def test_repair_against_twin(ctx, worlds, name, r2, max_level):
    w = worlds[name]
    got = _np(ctx.curve_clear(w["ctrl"], w["seg_off"], w["d2"], w["frame"], r2, max_level, status=w["status"]))
    ref = tw.clear(w["c"], w["so"], w["d2n"], w["frame"], r2, max_level, status=w["st"])
    _same(got, ref, CLEAR_KEYS, name)
    assert w["ctrl"].cpu().numpy().tobytes() == w["c"].tobytes()  # out of place: the input is not written
    # in place equals out of place
    c2 = w["ctrl"].clone()
    inp = _np(ctx.curve_clear(c2, w["seg_off"], w["d2"], w["frame"], r2, max_level, status=w["status"], inplace=True))
    _same(inp, got, CLEAR_KEYS, name + " in place")
    if name == "walls" and (r2, max_level) == (1, 6):
        assert list(got["level"]) == [0, 1, 2, 2] + [0, 2, 2, 0] + [6, 6, 0] and list(got["rounds"][:2]) == [2, 2]
        assert list(got["leg_min"][:6]) == [9, 1, 1, 1, 1, 1] and list(got["status"]) == [0, 0, tw.COLLIDES]
    if name == "walls" and r2 == 4:
        assert list(got["status"]) == [tw.COLLIDES] * 3 and got["level"].max() == 30
    if name.startswith("sweep") and max_level == 6:
        hit0 = tw.clearance(w["c"], w["so"], w["d2n"], w["frame"], r2)["hit_legs"] > 0
        assert hit0.sum() > len(hit0) / 4 and (got["status"][hit0] == 0).sum() > hit0.sum() / 2


def test_repair_longest_path_beside_one_leg(ctx):
    """A path of SC_CURVE_MAX_LEGS legs (a serpentine of short legs over a 48 x 48 map with a few blocked cells) and a path of one
    leg in one batch."""
    import sea_current_amd as sc
    n = sc.CURVE_MAX_LEGS + 1
    i = np.arange(n)
    row, col = i // 40, i % 40
    col = np.where(row % 2 == 0, col, 39 - col)
    long = np.stack([col + 4.5, row * 1.5 + 3.5 + 0.3 * (i % 2)], axis=1).astype(np.float32)
    occ = np.zeros((48, 48), np.uint8)
    occ[[6, 12, 13, 20, 33], [10, 30, 31, 7, 22]] = 1
    occ[27, 14:18] = 1
    wp, npts = _pack([long, np.array([[2.5, 45.5], [9.5, 46.5]], np.float32)])
    ctrl, seg_off, status = _legs(ctx, wp, npts)
    so = seg_off.cpu().numpy()
    assert list(so) == [0, sc.CURVE_MAX_LEGS, sc.CURVE_MAX_LEGS + 1] and not status.cpu().numpy().any()
    d2 = ctx.edt(_t(occ))
    got = _np(ctx.curve_clear(ctrl, seg_off, d2, FRAME1, 1, 6))
    ref = tw.clear(ctrl.cpu().numpy(), so, d2.cpu().numpy(), FRAME1, 1, 6)
    _same(got, ref, CLEAR_KEYS, "longest")
    assert got["level"].any() and got["rounds"][0] >= 2 and got["rounds"][1] == 0
    chk = _np(ctx.curve_clearance(ctrl, seg_off, d2, FRAME1, 1))
    _same(chk, tw.clearance(ctrl.cpu().numpy(), so, d2.cpu().numpy(), FRAME1, 1), CHECK_KEYS, "longest")
    # one leg more is refused by the host form, and skipped with BAD_INPUT by the device form
    import torch
    c3 = torch.cat([ctrl, ctrl[-1:]])
    so3 = np.array([0, sc.CURVE_MAX_LEGS + 1, sc.CURVE_MAX_LEGS + 2], np.int32)
    with pytest.raises(sc.SeaCurrentError):
        ctx.curve_clear_host(c3.cpu().numpy(), so3, d2.cpu().numpy(), FRAME1, 1, 6)
    over = _np(ctx.curve_clear(c3, _t(so3), d2, FRAME1, 1, 6))
    assert list(over["status"]) == [1, 0] and over["ctrl"].tobytes() == c3.cpu().numpy().tobytes() and not over["level"].any()


def test_no_hit_returns_the_input_bits(ctx, worlds):
    import torch
    w = worlds["sweep32"]
    free = torch.full((128, 128), 2**31 - 1, dtype=torch.int32, device="cuda")
    got = _np(ctx.curve_clear(w["ctrl"], w["seg_off"], free, FRAME_WIDE, 7, 6))
    assert got["ctrl"].tobytes() == w["c"].tobytes() and not got["level"].any() and not got["rounds"].any() and not got["status"].any()
    assert (got["leg_min"] == 2**31 - 1).all()
    chk = _np(ctx.curve_clearance(w["ctrl"], w["seg_off"], free, FRAME_WIDE, 7))
    assert not chk["hit_legs"].any() and (chk["hit_leg"] == -1).all() and (chk["hit_t"] == -1.0).all()


DYN = (0.8, 0.3, float("inf"), 0.0)


def _smooth(ctx, wp, npts, d2, frame, **kw):
    o = ctx.smooth_paths(_t(wp), _t(npts), LIMITS, N=50, nsub=50, capacity=1 << 16, dyn=DYN, d2=d2, frame=frame, **kw)
    ctx.synchronize()
    return _np(o)


def test_smoothing_without_hits_equals_the_limited_call(ctx):
    import torch
    _, _, wp, npts = tw.sweep_paths(32, 32, 5, 24)
    npts[7] = 0                                                   # a BAD_INPUT path among them
    free = torch.full((128, 128), 2**31 - 1, dtype=torch.int32, device="cuda")
    a = _smooth(ctx, wp, npts, free, FRAME_WIDE)
    b = _smooth(ctx, wp, npts, free, FRAME_WIDE, r2_clear=3, max_level=6)
    M = int(a["needed"][0])
    assert M > 0 and int(b["needed"][0]) == M and a["status"][7] == 1
    for k in a:
        n = M if k in SAMPLE_KEYS else (int(a["seg_off"][-1]) if k == "ctrl" else len(a[k]))
        assert a[k][:n].tobytes() == b[k][:n].tobytes(), k
    assert not b["level"].any() and not b["rounds"].any()


def test_smoothing_repairs_and_reports(ctx, worlds):
    w = worlds["walls"]
    wp, npts = _pack([centres(CASE_A), centres(THROUGH), centres(CASE_B)])
    o = _smooth(ctx, wp, npts, w["d2"], FRAME1, r2_clear=1, max_level=6)
    assert list(o["status"]) == [0, tw.COLLIDES, 0] and list(o["rounds"]) == [2, 6, 2]
    assert o["length"][1] == 0 and o["offsets"][2] == o["offsets"][1] and list(o["seg_off"]) == [0, 3, 5, 8]
    # the repaired legs are call 2's, on from_path's legs
    by_hand = _np(ctx.curve_clear(w["ctrl"], w["seg_off"], w["d2"], FRAME1, 1, 6))
    order = [0, 1, 2, 6, 7, 3, 4, 5]                              # walls holds A, B, THROUGH
    assert o["ctrl"][:8].tobytes() == by_hand["ctrl"][order].tobytes()
    assert list(o["leg_min"][:8]) == list(by_hand["leg_min"][order])
    assert list(o["level"][:11]) == [0, 1, 2, 2] + [6, 6, 0] + [0, 2, 2, 0]
    # the returned points of the OK paths lie in traversable cells, by the twin's cell rule
    for p in (0, 2):
        a, n = o["offsets"][p], o["length"][p]
        assert n > 50
        v = tw.cell_values(o["pts"][a:a + n].astype(np.float64), w["d2n"], FRAME1)
        print("path", p, "samples", n, "min d2 under the returned points", v.min())
        assert (v >= 1).all()
    # the neighbours of the unresolved path are what they are without it
    alone = _smooth(ctx, *_pack([centres(CASE_A), centres(CASE_B)]), w["d2"], FRAME1, r2_clear=1, max_level=6)
    assert list(alone["status"]) == [0, 0]
    for p, q in ((0, 0), (2, 1)):
        for k in ("arclength", "length", "min_clear", "rounds"):
            assert o[k][p].tobytes() == alone[k][q].tobytes(), (k, p)
        assert o["vmax_stage"][p].tobytes() == alone["vmax_stage"][q].tobytes()
        a, b, n = o["offsets"][p], alone["offsets"][q], o["length"][p]
        for k in SAMPLE_KEYS:
            assert o[k][a:a + n].tobytes() == alone[k][b:b + n].tobytes(), (k, p)
    # the limited call on the same input leaves the curves through the wall, and says nothing
    lim = _smooth(ctx, wp, npts, w["d2"], FRAME1)
    assert list(lim["status"]) == [0, 0, 0]
    assert tw.cell_values(lim["pts"][:lim["length"][0]].astype(np.float64), w["d2n"], FRAME1).min() == 0


def test_host_forms_equal_device_forms(ctx, worlds):
    w = worlds["mixed"]
    dev = _np(ctx.curve_clearance(w["ctrl"], w["seg_off"], w["d2"], w["frame"], 1, status=w["status"]))
    _same(ctx.curve_clearance_host(w["c"], w["so"], w["d2n"], w["frame"], 1, status=w["st"]), dev, CHECK_KEYS, "check host")
    dev = _np(ctx.curve_clear(w["ctrl"], w["seg_off"], w["d2"], w["frame"], 1, 6, status=w["status"]))
    _same(ctx.curve_clear_host(w["c"], w["so"], w["d2n"], w["frame"], 1, 6, status=w["st"]), dev, CLEAR_KEYS, "clear host")
    ww = worlds["walls"]
    wp, npts = _pack([centres(CASE_A), centres(THROUGH), centres(CASE_B)])
    d = _smooth(ctx, wp, npts, ww["d2"], FRAME1, r2_clear=1, max_level=6)
    h = ctx.smooth_paths_host(wp, npts, LIMITS, 1 << 16, N=50, nsub=50, dyn=DYN, d2=ww["d2n"], frame=FRAME1, r2_clear=1, max_level=6)
    M, S = int(d["needed"][0]), int(d["seg_off"][-1])
    for k in d:
        n = M if k in SAMPLE_KEYS else (S if k in ("ctrl", "leg_min") else (S + 3 if k == "level" else len(d[k])))
        assert np.asarray(h[k])[:n].tobytes() == d[k][:n].tobytes(), k


def test_argument_errors(ctx, worlds):
    import sea_current_amd as sc
    w = worlds["walls"]
    bad = [dict(frame=(0.0, 0.0, 0.0, 1.0)), dict(frame=(float("nan"), 0.0, 1.0, 1.0)), dict(r2_clear=-1)]
    for kw in bad:
        a = dict(frame=FRAME1, r2_clear=1)
        a.update(kw)
        with pytest.raises(sc.SeaCurrentError):
            ctx.curve_clearance(w["ctrl"], w["seg_off"], w["d2"], a["frame"], a["r2_clear"])
        with pytest.raises(sc.SeaCurrentError):
            ctx.curve_clear(w["ctrl"], w["seg_off"], w["d2"], a["frame"], a["r2_clear"], 6)
    for ml in (0, 31):
        with pytest.raises(sc.SeaCurrentError):
            ctx.curve_clear(w["ctrl"], w["seg_off"], w["d2"], FRAME1, 1, ml)
    l = ctx._l
    z = [None] * 5
    from sea_current_amd import _ptr
    assert l.sc_curve_clearance_batch(ctx._h, _ptr(w["ctrl"]), _ptr(w["seg_off"]), None, 3, _ptr(w["d2"]), 32, 32, 0.0, 0.0, 1.0, 1.0, 1, *z) == 1
    assert l.sc_curve_clearance_batch(ctx._h, _ptr(w["ctrl"]), _ptr(w["seg_off"]), None, 3, None, 32, 32, 0.0, 0.0, 1.0, 1.0, 1,
                                      _ptr(w["ctrl"]), *z[:4]) == 1
    wp, npts = _pack([centres(CASE_A)])
    with pytest.raises(ValueError):
        ctx.smooth_paths(_t(wp), _t(npts), LIMITS, capacity=1 << 12, r2_clear=1)
    with pytest.raises(sc.SeaCurrentError):
        ctx.smooth_paths(_t(wp), _t(npts), LIMITS, capacity=1 << 12, d2=w["d2"], frame=FRAME1, r2_clear=1, max_level=0)
