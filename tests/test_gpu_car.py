"""Car-like pose planning on the GPU (Context.arc_mask, car_fields, car_paths): masks, gp, statuses and every read-out output
bit-equal to the C statement (tests/cpp/car_ref.c), which tests/test_car_ref.py holds equal to the NumPy twin
(tests/car_twin.py), and to the twin itself on the small maps.  Maps: 64 x 64, 65 x 63, 130 x 70 salt and blocks, 1 x 200,
200 x 1 and a 64 x 64 serpentine; roots within 2 arc_n cells of the borders of 32- and 64-cell tiles and in the corners; an arc
whose start, corner and end lie in three tiles, mirrored into every quadrant of the tile corner; every `rounds` and the _host
forms; 12 fields over 3 grids with every bad-root kind; hmask NULL and given; both `toward` values; rev_cost -1 / 0 / 7,
arc_cost 0 / 1 / 40, arc_n 1 / 2 / 4; anchors (b) and (c) on the device; 300 read-outs; a wrong arc mask; every argument error;
the one-stream chain from the EDT to waypoints; one 1024 x 700 field."""
import numpy as np
import pytest

import car_twin as ct
import pose_twin as pt
from field_twin import serpentine
from pose_twin import HX, HY, INF, Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED

pytestmark = pytest.mark.gpu

FOOT = (2, 1, 1, 0)           # the body of the hmask-given cases: asymmetric, so heading k and k + 4 differ
# (hmask given, toward, arc_n, arc_cost, rev_cost, rhead)
CONFIGS = [(False, False, 1, 0, -1, 0), (True, False, 2, 1, 0, 3), (True, True, 4, 40, 7, 6), (False, True, 1, 1, -1, -1),
           (True, False, 4, 0, 7, -1), (True, True, 2, 40, 0, 1), (False, False, 4, 1, 7, 2)]


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ct.Ref(tmp_path_factory.mktemp("car_ref_gpu"))


def _t(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _line(n):
    occ = np.zeros(n, np.uint8)
    occ[[3 * n // 4]] = 1
    return occ


@pytest.fixture(scope="module")
def maps():
    return {
        "sq64": pt.d2_of(pt.salt(64, 64, 0.05, 1)),
        "odd65x63": pt.d2_of(pt.salt(65, 63, 0.05, 2)),
        "salt130x70": pt.d2_of(pt.salt(130, 70, 0.05, 3)),
        "blocks130x70": pt.d2_of(pt.blocks()),
        "row1x200": pt.d2_of(_line(200)[None, :]),
        "col200x1": pt.d2_of(_line(200)[:, None]),
        "serpentine64": pt.d2_of(serpentine(64)),
    }


NAMES = ["sq64", "odd65x63", "salt130x70", "blocks130x70", "row1x200", "col200x1", "serpentine64"]


def _near_free(d2, x, y):
    """The free cell of row y nearest to column x (keeps y), as a cell index."""
    H, W = d2.shape
    free = np.flatnonzero(d2[y] >= 1)
    return int(y * W + free[np.argmin(np.abs(free - x))])


def _gpu_field(ctx, d2, am, roots, rhead, n, ac, rev, toward, hmask, rounds=-1, r2=0, fgrid=None):
    o = ctx.car_fields(_t(d2), _t(am), _t(np.asarray(roots, np.int32)), _t(np.asarray(rhead, np.int32)), n, ac, rev, toward, r2, _t(hmask),
                       _t(fgrid), rounds)
    ctx.synchronize()
    return o["gp"].cpu().numpy(), o["status"].cpu().numpy()


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} entries differ, first {tuple(bad[0])}: gpu {got[tuple(bad[0])]} ref {want[tuple(bad[0])]}")


# ---- the mask ----
@pytest.mark.parametrize("name", NAMES)
def test_mask_equals_statement(ctx, ref, maps, name):
    d2 = maps[name]
    hm = pt.footprint_mask(d2, *FOOT)
    for n in (1, 2, 4):
        for hmask in (None, hm):
            got = ctx.arc_mask(_t(d2), n, hmask=_t(hmask))
            ctx.synchronize()
            _same(_u16(got), ref.arc_mask(d2, n, 0, hmask), f"{name} n {n} mask {hmask is not None}")
    if name == "sq64":
        _same(_u16(ctx.arc_mask(_t(d2), 2, hmask=_t(hm))), ct.arc_mask(d2, 2, 0, hm), "twin")


def test_mask_batch_r2_and_host(ctx, ref, oracle):
    occs = [pt.salt(130, 70, 0.01, s) for s in (5, 6, 7)]
    d2 = np.stack([oracle.edt(o) for o in occs])
    hm = np.stack([pt.footprint_mask(d, 1, 1, 1, 1, r2=2) for d in d2])
    for n, r2, hmask in ((1, 0, None), (3, 2, hm), (4, 2, None)):
        got = ctx.arc_mask(_t(d2), n, r2=r2, hmask=_t(hmask))
        ctx.synchronize()
        got = _u16(got)
        for b in range(3):
            _same(got[b], ref.arc_mask(d2[b], n, r2, None if hmask is None else hmask[b]), f"batch {b} n {n} r2 {r2}")
        host = ctx.arc_mask_host(d2, n, r2=r2, hmask=hmask)
        assert host.dtype == np.uint16 and np.array_equal(host, got)


# ---- the field ----
@pytest.mark.parametrize("name", NAMES)
def test_field_equals_statement(ctx, ref, maps, name):
    d2 = maps[name]
    hm = pt.footprint_mask(d2, *FOOT)
    cand = pt.free_cells(d2, 64, 11)
    bits = (hm.ravel()[cand][:, None] >> np.arange(8)) & 1
    i = int(np.argmax(bits.sum(1)))
    root, fits = int(cand[i]), np.flatnonzero(bits[i])
    finite = 0
    for given, toward, n, ac, rev, rhead in CONFIGS:
        hmask = hm if given else None
        if given and rhead >= 0 and rhead not in fits:
            rhead = int(fits[rhead % len(fits)])
        am = ref.arc_mask(d2, n, 0, hmask)
        gp, st = _gpu_field(ctx, d2, am, [root], [rhead], n, ac, rev, toward, hmask)
        want, ws = ref.car_field(d2, root, rhead, n, ac, rev, toward, 0, hmask)
        assert st[0] == ws == Q_OK
        _same(gp[0], want, f"{name} {(given, toward, n, ac, rev, rhead)}")
        finite += int((want < INF).sum())
    assert finite > 100
    if name in ("sq64", "serpentine64"):                  # the twin itself
        am = ct.arc_mask(d2, 2, 0, hm)
        for toward in (False, True):
            gp, st = _gpu_field(ctx, d2, am, [root], [int(fits[0])], 2, 1, 7, toward, hm)
            _same(gp[0], ct.car_field(d2, root, int(fits[0]), 2, 1, 7, toward, 0, hm)[0], f"twin {name} toward {toward}")


@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("name", ["sq64", "odd65x63", "salt130x70"])
def test_roots_near_tile_borders(ctx, ref, maps, name, n):
    """Roots at x or y of 31 - 2n, 31, 32, 32 + 2n, 63, 64 and in the corners, every heading seeded, both directions: one call."""
    d2 = maps[name]
    H, W = d2.shape
    vals = [31 - 2 * n, 31, 32, 32 + 2 * n, 63, 64]
    pts = [(v, 20) for v in vals] + [(20, v) for v in vals] + [(v, v) for v in vals] + [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    roots = sorted({_near_free(d2, min(x, W - 1), min(y, H - 1)) for x, y in pts})
    am = ref.arc_mask(d2, n)
    for toward, rev in ((False, 3), (True, -1)):
        gp, st = _gpu_field(ctx, d2, am, roots, [-1] * len(roots), n, 2, rev, toward, None)
        for f, r in enumerate(roots):
            want, ws = ref.car_field(d2, r, -1, n, 2, rev, toward)
            assert st[f] == ws == Q_OK
            _same(gp[f], want, f"{name} n {n} root ({r % W}, {r // W}) toward {toward}")


@pytest.mark.parametrize("fx,fy", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_arc_through_three_tiles(ctx, ref, fx, fy):
    """arc_n 4, heading 0, sense +1 from (29, 29): the corner (33, 29) and the end (37, 33) lie in two other tiles; mirrored
    into the other quadrants of the tile corner (32, 32).  Only the arc's cells and the side cells of its diagonal steps are
    free, so the arc is the only way."""
    n, S = 4, 64
    sx, sy = (-1 if fx else 1), (-1 if fy else 1)
    x0, y0 = (34 if fx else 29), (34 if fy else 29)
    k = 4 if fx else 0
    kn = [i for i in range(8) if (HX[i], HY[i]) == (sx, sy)][0]
    s = 1 if (k + 1) & 7 == kn else -1
    assert (k + s) & 7 == kn
    occ = np.ones((S, S), np.uint8)
    cells, _ = ct.arc_cells(x0, y0, k, s, n)
    for (ax, ay), (bx, by) in zip(cells, cells[1:]):
        occ[ay, ax] = occ[by, bx] = occ[ay, bx] = occ[by, ax] = 0
    d2 = pt.d2_of(occ)
    ex, ey = cells[-1]
    assert (ex, ey) == (x0 + 8 * sx, y0 + 4 * sy) and {(x0 // 32, y0 // 32), (cells[n][0] // 32, cells[n][1] // 32), (ex // 32, ey // 32)}.__len__() == 3
    am = ref.arc_mask(d2, n)
    assert am[y0, x0] >> (2 * k + (s < 0)) & 1
    got_am = ctx.arc_mask(_t(d2), n)
    _same(_u16(got_am), am, "mask")
    for toward, root, rh in ((False, y0 * S + x0, k), (True, ey * S + ex, kn), (False, ey * S + ex, kn), (True, y0 * S + x0, k)):
        for rounds in (-1, 0):
            gp, st = _gpu_field(ctx, d2, am, [root], [rh], n, 5, 3, toward, None, rounds)
            want, ws = ref.car_field(d2, root, rh, n, 5, 3, toward)
            _same(gp[0], want, f"toward {toward} root {root} rounds {rounds}")
    gp, _ = _gpu_field(ctx, d2, am, [y0 * S + x0], [k], n, 5, -1, False, None)
    assert gp[0, kn, ey, ex] == 24 * n + 5
    gp, _ = _gpu_field(ctx, d2, am, [y0 * S + x0], [k], n, 5, 3, True, None)
    assert gp[0, kn, ey, ex] == 24 * n + 5 + 2 * n * 3              # back along the arc


def test_rounds_and_host_forms(ctx, ref, maps):
    d2 = maps["odd65x63"]
    H, W = d2.shape
    hm = pt.footprint_mask(d2, *FOOT)
    n, ac, rev = 2, 1, 7
    am = ref.arc_mask(d2, n, 0, hm)
    roots = pt.free_cells(d2, 3, 5)
    rhead = np.array([-1, -1, -1], np.int32)
    want = [ref.car_field(d2, int(r), -1, n, ac, rev, True, 0, hm)[0] for r in roots]
    for rounds in (0, 1, 2, -1, 1000):
        gp, st = _gpu_field(ctx, d2, am, roots, rhead, n, ac, rev, True, hm, rounds)
        for f in range(3):
            _same(gp[f], want[f], f"rounds {rounds} field {f}")
    host = ctx.car_fields_host(d2, am, roots, rhead, n, ac, rev, True, 0, hm)
    assert list(host["status"]) == [Q_OK] * 3
    for f in range(3):
        _same(host["gp"][f], want[f], f"host field {f}")
    targets = pt.free_cells(d2, 30, 6)
    thead = (np.arange(30) % 9 - 1).astype(np.int32)
    qf = (np.arange(30) % 3).astype(np.int32)
    a = ctx.car_paths_host(d2, am, host["gp"], roots, rhead, qf, targets, thead, n, ac, rev, True, 0, hm, 300, True)
    b = ctx.car_paths(_t(d2), _t(am), _t(host["gp"]), _t(roots), _t(rhead), _t(qf), _t(targets), _t(thead), n, ac, rev, True, 0, _t(hm), 300, True)
    ctx.synchronize()
    assert ct.same_readout(a, {k: v.cpu().numpy() for k, v in b.items()}) and (a["status"] == Q_OK).sum() >= 5


def test_12_fields_over_3_grids_with_bad_roots(ctx, ref):
    d2 = np.stack([pt.d2_of(pt.salt(130, 70, 0.05, s)) for s in (21, 22)] + [pt.d2_of(pt.blocks(130, 70, seed=23))])
    G, H, W = d2.shape
    hm = np.stack([pt.footprint_mask(d, *FOOT) for d in d2])
    n, ac, rev = 2, 3, 5
    am = ctx.arc_mask(_t(d2), n, hmask=_t(hm))
    ctx.synchronize()
    am = _u16(am)
    for g in range(G):
        _same(am[g], ref.arc_mask(d2[g], n, 0, hm[g]), f"mask of grid {g}")
    fgrid = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 3, -1, 0], np.int32)
    good = [int(np.flatnonzero(hm[g].ravel() == 0xFF)[k]) for k, g in ((50, 0), (60, 1), (70, 2), (900, 0), (800, 1), (700, 2))]
    blocked = int(np.flatnonzero(d2[0].ravel() < 1)[0])
    roots = np.array(good + [blocked, good[1], -1, good[0], good[0], W * H], np.int32)
    rhead = np.array([0, 3, -1, 5, -1, 7, 0, 8, 0, 0, 0, 0], np.int32)
    for toward in (False, True):
        gp, st = _gpu_field(ctx, d2, am, roots, rhead, n, ac, rev, toward, hm, fgrid=fgrid)
        assert list(st) == [Q_OK] * 6 + [Q_BAD_ENDPOINT] * 6
        assert (gp[6:] == INF).all()
        for f in range(6):
            want, ws = ref.car_field(d2[fgrid[f]], int(roots[f]), int(rhead[f]), n, ac, rev, toward, 0, hm[fgrid[f]])
            assert ws == Q_OK
            _same(gp[f], want, f"field {f} toward {toward}")


def test_anchors_on_the_device(ctx, maps):
    """(b) every car value >= the pose field's with turn_cost = arc_cost and the same rev_cost; (c) min_k gp >= the plain field."""
    d2 = maps["blocks130x70"]
    hm = pt.footprint_mask(d2, *FOOT)
    roots = pt.free_cells(d2, 3, 31)
    g = ctx.cost_fields(_t(d2), _t(roots))["g"]
    finite = 0
    for given, toward, n, ac, rev, rhead in CONFIGS:
        hmask = _t(hm if given else None)
        rh = _t(np.full(3, rhead, np.int32))
        am = ctx.arc_mask(_t(d2), n, hmask=hmask)
        gp = ctx.car_fields(_t(d2), am, _t(roots), rh, n, ac, rev, toward, hmask=hmask)["gp"]
        pose = ctx.pose_fields(_t(d2), _t(roots), rh, ac, rev, toward, hmask=hmask)["gp"]
        ctx.synchronize()
        assert bool((gp >= pose).all()) and bool((gp.min(dim=1).values >= g).all()), (given, toward, n, ac, rev, rhead)
        finite += int((gp < INF).sum())
    assert finite > 10000


# ---- the read-out ----
def _gpu_paths(ctx, d2, am, gp, roots, rhead, qfield, targets, thead, n, ac, rev, toward, hmask, Lmax, to_root, fgrid=None):
    o = ctx.car_paths(_t(d2), _t(am), _t(gp), _t(np.asarray(roots, np.int32)), _t(np.asarray(rhead, np.int32)), _t(np.asarray(qfield, np.int32)),
                      _t(np.asarray(targets, np.int32)), _t(np.asarray(thead, np.int32)), n, ac, rev, toward, 0, _t(hmask), Lmax, to_root,
                      _t(fgrid))
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("toward", [False, True])
def test_readouts_300_targets(ctx, ref, maps, toward):
    d2 = maps["salt130x70"]
    H, W = d2.shape
    hm = pt.footprint_mask(d2, *FOOT)
    roots, rhead = pt.free_cells(d2, 2, 41), np.array([1, -1], np.int32)
    rng = np.random.default_rng(42)
    targets = rng.integers(0, W * H, 300).astype(np.int32)        # blocked cells among them
    targets[:4] = [roots[0], roots[1], -1, W * H]
    thead = (rng.integers(0, 9, 300) - 1).astype(np.int32)
    thead[4:6] = [8, -2]
    qfield = (np.arange(300) % 2).astype(np.int32)
    qfield[6:8] = [2, -1]                                          # a bad qfield
    for n, ac, rev, hmask in ((1, 3, 7, hm), (4, 0, 2, None), (2, 40, -1, hm)):
        am = ref.arc_mask(d2, n, 0, hmask)
        gp, st = _gpu_field(ctx, d2, am, roots, rhead, n, ac, rev, toward, hmask)
        for to_root in (False, True):
            for Lmax in (512, 24):
                got = _gpu_paths(ctx, d2, am, gp, roots, rhead, qfield, targets, thead, n, ac, rev, toward, hmask, Lmax, to_root)
                seen = set()
                for f in (0, 1):
                    q = np.flatnonzero(qfield == f)
                    want = ref.car_paths(d2, am, gp[f], roots[f], rhead[f], targets[q], thead[q], n, ac, rev, toward, 0, hmask, Lmax, to_root)
                    assert ct.same_readout(want, {k: v[q] for k, v in got.items()}), (n, ac, rev, to_root, Lmax, f)
                    seen |= set(want["status"].tolist())
                assert list(got["status"][6:8]) == [Q_BAD_ENDPOINT] * 2 and list(got["len"][6:8]) == [0, 0] and list(got["cost"][6:8]) == [-1, -1]
                if rev >= 0:
                    assert seen >= ({Q_OK, Q_BAD_ENDPOINT, Q_TRUNCATED} if Lmax == 24 else {Q_OK, Q_BAD_ENDPOINT})
    # the twin itself on 40 of the last fields' queries
    q = np.flatnonzero(qfield[:80] == 0)
    got = _gpu_paths(ctx, d2, am, gp, roots, rhead, qfield, targets, thead, n, ac, rev, toward, hmask, 512, True)
    want = ct.car_paths(d2, am, gp[0], int(roots[0]), int(rhead[0]), targets[q], thead[q], n, ac, rev, toward, 0, hmask, 512, True)
    assert ct.same_readout(want, {k: v[q] for k, v in got.items()})


def test_a_wrong_arc_mask_only_has_to_return(ctx, maps):
    """amask all ones: the values are unspecified, every access stays in bounds by construction, the calls end."""
    d2 = maps["odd65x63"]
    H, W = d2.shape
    am = np.full((H, W), 0xFFFF, np.uint16)
    roots = pt.free_cells(d2, 2, 9)
    rhead = np.array([-1, 0], np.int32)
    targets = np.arange(0, W * H, 37, dtype=np.int32)
    for n in (1, 4):
        for toward in (False, True):
            gp, st = _gpu_field(ctx, d2, am, roots, rhead, n, 1, 3, toward, None)
            got = _gpu_paths(ctx, d2, am, gp, roots, rhead, np.arange(len(targets)) % 2, targets, np.full(len(targets), -1), n, 1, 3, toward, None,
                             64, False)
            assert got["status"].min() >= 0 and got["status"].max() <= 3


# ---- errors ----
def test_argument_errors(ctx, maps):
    import sea_current_amd as sc
    import torch
    d2 = maps["sq64"]
    root = np.array([int(pt.free_cells(d2, 1, 1)[0])], np.int32)
    rh = np.zeros(1, np.int32)
    am = np.zeros((64, 64), np.uint16)
    E = sc.SeaCurrentError
    # the library's own checks, under the ranges the binding refuses first
    l, h, p = ctx._l, ctx._h, sc._ptr
    td2, tam, troot, trh = _t(d2), _t(am), _t(root), _t(rh)
    gp = torch.empty((1, 8, 64, 64), dtype=torch.int32, device="cuda")
    st = torch.empty(1, dtype=torch.int32, device="cuda")
    for n in (0, 5):
        assert l.sc_arc_mask_u16(h, p(td2), None, 64, 64, 1, 0, n, p(tam)) == 1
        assert l.sc_arc_mask_u16_host(h, p(d2), None, 64, 64, 1, 0, n, p(am)) == 1
    assert l.sc_arc_mask_u16(h, None, None, 64, 64, 1, 0, 1, p(tam)) == 1 and l.sc_arc_mask_u16(h, p(td2), None, 64, 64, 1, 0, 1, None) == 1
    assert l.sc_arc_mask_u16(h, p(td2), None, 0, 64, 1, 0, 1, p(tam)) == 1 and l.sc_arc_mask_u16(h, p(td2), None, 64, 64, 0, 0, 1, p(tam)) == 1
    for n, ac, rev in ((0, 0, 0), (5, 0, 0), (1, -1, 0), (1, 256, 0), (1, 0, -2), (1, 0, 256)):
        assert l.sc_car_field_batch(h, p(td2), None, p(tam), 1, None, 64, 64, 0, n, ac, rev, 0, p(troot), p(trh), 1, -1, p(gp), p(st)) == 1
        assert l.sc_car_field_batch_host(h, p(d2), None, p(am), 1, None, 64, 64, 0, n, ac, rev, 0, p(root), p(rh), 1, -1, p(gp.cpu().numpy()),
                                         None) == 1
        with pytest.raises(E):
            ctx.car_fields(td2, tam, troot, trh, n, ac, rev)
        with pytest.raises(E):
            ctx.car_fields_host(d2, am, root, rh, n, ac, rev)
    assert l.sc_car_field_batch(h, p(td2), None, None, 1, None, 64, 64, 0, 1, 0, 0, 0, p(troot), p(trh), 1, -1, p(gp), p(st)) == 1     # amask is mandatory
    assert l.sc_car_field_batch(h, p(td2), None, p(tam), 2, None, 64, 64, 0, 1, 0, 0, 0, p(troot), p(trh), 1, -1, p(gp), p(st)) == 1    # two grids, no fgrid
    assert l.sc_car_field_batch(h, p(td2), None, p(tam), 1, None, 64, 64, 0, 1, 0, 0, 0, p(troot), p(trh), 0, -1, p(gp), p(st)) == 1    # F = 0
    # (96 + 100 + 8 * 255) * (8 * 400 * 300 - 1) <= INT32_MAX - 1 < (96 + 101 + 8 * 255) * ...
    big = np.ones((300, 400), np.int32)
    bam = ctx.arc_mask(_t(big), 4)
    with pytest.raises(E):
        ctx.car_fields(_t(big), bam, troot, trh, 4, 101, 255)
    with pytest.raises(E):
        ctx.car_fields_host(big, _u16(bam), root, rh, 4, 101, 255)
    o = ctx.car_fields(_t(big), bam, troot, trh, 4, 100, 255)
    ctx.synchronize()
    assert int(o["status"][0]) == Q_OK                        # the largest costs the rule lets through
    fld = ctx.car_fields(td2, ctx.arc_mask(td2, 1), troot, trh, 1)
    ctx.synchronize()
    q = np.zeros(1, np.int32)
    with pytest.raises(E):
        ctx.car_paths(td2, tam, fld["gp"], troot, trh, _t(q), troot, _t(q), 1, Lmax=0)
    with pytest.raises(E):
        ctx.car_paths_host(d2, am, fld["gp"].cpu().numpy(), root, rh, q, root, q, 1, rev_cost=-2)
    with pytest.raises(E):
        ctx.car_paths(td2, None, fld["gp"], troot, trh, _t(q), troot, _t(q), 1)
    bad = fld["gp"].cpu().numpy().copy()
    bad[0, 0, 0, 0] = -5
    with pytest.raises(E):                                                # the _host form checks the data
        ctx.car_paths_host(d2, am, bad, root, rh, q, root, q, 1)
    z = torch.zeros(0, dtype=torch.int32, device="cuda")
    assert ctx.car_paths(td2, tam, fld["gp"], troot, trh, z, z, z, 1)["len"].numel() == 0


# ---- the chain ----
def test_one_stream_chain_with_one_synchronise(ctx, ref, oracle, tmp_path):
    """edt -> footprint_mask -> arc_mask -> car_fields(toward) -> car_paths -> path_waypoints: no host hop in between."""
    pref = pt.Ref(tmp_path)
    occ = pt.blocks(130, 70, seed=4)
    r2, foot, n, ac, rev = 2, (2, 2, 1, 1), 1, 4, 6
    ref_d2 = oracle.edt(occ)
    free = pt.free_cells(ref_d2, 40, 3, r2)
    hm_ref = pref.footprint_mask(ref_d2, *foot, r2=r2)
    goal = int(next(c for c in free if hm_ref.ravel()[c] & 1))
    starts, sh = np.array([c for c in free if c != goal][:32], np.int32), (np.arange(32) % 9 - 1).astype(np.int32)
    one, zero = _t(np.array([goal], np.int32)), _t(np.zeros(1, np.int32))
    d2 = ctx.edt(_t(occ))
    hm = ctx.footprint_mask(d2, *foot, r2=r2)
    am = ctx.arc_mask(d2, n, r2=r2, hmask=hm)
    fld = ctx.car_fields(d2, am, one, zero, n, ac, rev, toward=True, r2=r2, hmask=hm)
    res = ctx.car_paths(d2, am, fld["gp"], one, zero, _t(np.zeros(32, np.int32)), _t(starts), _t(sh), n, ac, rev, toward=True, r2=r2, hmask=hm,
                        Lmax=512, to_root=True)
    wp = ctx.path_waypoints(d2, res, r2=r2)
    ctx.synchronize()
    assert np.array_equal(d2.cpu().numpy(), ref_d2) and np.array_equal(hm.cpu().numpy(), hm_ref)
    am_ref = ref.arc_mask(ref_d2, n, r2, hm_ref)
    _same(_u16(am), am_ref, "arc mask")
    gp, st = ref.car_field(ref_d2, goal, 0, n, ac, rev, True, r2, hm_ref)
    assert st == Q_OK and np.array_equal(fld["gp"].cpu().numpy()[0], gp)
    want = ref.car_paths(ref_d2, am_ref, gp, goal, 0, starts, sh, n, ac, rev, True, r2, hm_ref, 512, True)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert ct.same_readout(want, got) and (got["status"] == Q_OK).sum() >= 8
    wph = ctx.path_waypoints_host(ref_d2, got["path"], got["len"], got["status"], r2=r2)
    for k in ("n", "status"):
        assert np.array_equal(wp[k].cpu().numpy(), wph[k]), k
    ok = got["status"] == Q_OK
    nw = wp["n"].cpu().numpy()
    w = wp["wp"].cpu().numpy()
    assert all(np.array_equal(w[q, :nw[q]], wph["wp"][q, :nw[q]]) for q in np.flatnonzero(ok))      # past n the device form writes nothing
    assert (wp["status"].cpu().numpy()[ok] == 0).all()
    assert all(w[q, 0] == starts[q] and w[q, nw[q] - 1] == goal for q in np.flatnonzero(ok))     # the driving order: start .. goal


def test_field_1024x700_against_c(ctx, ref, oracle):
    from sea_current_amd import synth
    d2 = oracle.edt(synth.block_grid(1024, 700, 0.2, seed=3))
    r2, n = 4, 2
    root = int(pt.free_cells(d2, 1, 8, r2)[0])
    hm = ctx.footprint_mask(_t(d2), 3, 1, 1, 1, r2=r2)
    am = ctx.arc_mask(_t(d2), n, r2=r2, hmask=hm)
    o = ctx.car_fields(_t(d2), am, _t(np.array([root], np.int32)), _t(np.array([-1], np.int32)), n, 5, 9, True, r2=r2, hmask=hm)
    ctx.synchronize()
    hmc = hm.cpu().numpy()
    amc = ref.arc_mask(d2, n, r2, hmc)
    _same(_u16(am), amc, "mask")
    want, st = ref.car_field(d2, root, -1, n, 5, 9, True, r2, hmc)
    assert st == Q_OK and o["status"].cpu().numpy()[0] == Q_OK
    _same(o["gp"].cpu().numpy()[0], want, "1024 x 700")
