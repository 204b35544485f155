"""Planning in poses on the GPU (Context.footprint_mask, pose_fields, pose_paths): masks, gp, statuses and every read-out
output bit-equal to the NumPy twin (tests/pose_twin.py); where a test needs many fields or read-outs, to the C statement
(tests/cpp/pose_ref.c), which tests/test_pose_ref.py holds equal to the twin.  Maps: 64 x 64, 65 x 63, 130 x 70 salt and
blocks, 1 x 200, 200 x 1 and a 64 x 64 serpentine; roots on the borders of 32- and 64-cell tiles and in the corners; every
`rounds` and the _host form; 12 fields over 3 grids with every bad-root kind; hmask NULL and given; both `toward` values;
rev_cost -1 / 0 / 7 and turn_cost 0 / 1 / 40; anchors (b), (c), (d) on the device; 300 read-outs; every argument error; the
one-stream chain from the EDT to waypoints; one 1024 x 700 field."""
import numpy as np
import pytest

import pose_twin as pt
from field_twin import serpentine
from pose_twin import INF, Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED

pytestmark = pytest.mark.gpu

FOOT = (2, 1, 1, 0)           # the body of the hmask-given cases: asymmetric, so heading k and k + 4 differ
EXTENTS = [(0, 0, 0, 0), (3, 3, 1, 1), (5, 0, 2, 1)]
# (hmask given, toward, turn_cost, rev_cost, rhead)
CONFIGS = [(False, False, 5, -1, 0), (True, False, 1, 0, 3), (True, True, 40, 7, 6), (False, True, 1, -1, -1), (True, False, 0, 7, -1),
           (True, True, 5, 0, 1)]


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pt.Ref(tmp_path_factory.mktemp("pose_ref_gpu"))


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


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


def _gpu_field(ctx, d2, roots, rhead, turn, rev, toward, hmask, rounds=-1, r2=0):
    o = ctx.pose_fields(_t(d2), _t(np.asarray(roots, np.int32)), _t(np.asarray(rhead, np.int32)), turn, rev, toward, r2, _t(hmask),
                        rounds=rounds)
    ctx.synchronize()
    return o["gp"].cpu().numpy(), o["status"].cpu().numpy()


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} entries differ, first {tuple(bad[0])}: gpu {got[tuple(bad[0])]} ref {want[tuple(bad[0])]}")


# ---- the mask ----
@pytest.mark.parametrize("name", NAMES)
def test_mask_equals_twin(ctx, maps, name):
    d2 = maps[name]
    for ext in EXTENTS:
        got = ctx.footprint_mask(_t(d2), *ext)
        ctx.synchronize()
        _same(got.cpu().numpy(), pt.footprint_mask(d2, *ext), f"{name} {ext}")
    assert np.array_equal(ctx.footprint_mask(_t(d2), 0, 0, 0, 0).cpu().numpy(), np.where(d2 >= 1, 0xFF, 0).astype(np.uint8))   # anchor (a)


def test_mask_large_extents_batch_r2_and_host(ctx, ref, maps, oracle):
    occs = [pt.salt(130, 70, 0.01, s) for s in (5, 6, 7)]
    d2 = np.stack([oracle.edt(o) for o in occs])
    for ext, r2 in (((32, 2, 1, 1), 0), ((1, 32, 0, 3), 2), ((4, 4, 32, 32), 0)):
        got = ctx.footprint_mask(_t(d2), *ext, r2=r2)
        ctx.synchronize()
        got = got.cpu().numpy()
        for b in range(3):
            _same(got[b], ref.footprint_mask(d2[b], *ext, r2=r2), f"batch {b} {ext} r2 {r2}")
        assert np.array_equal(ctx.footprint_mask_host(d2, *ext, r2=r2), got)
    _same(got[0], pt.footprint_mask(d2[0], 4, 4, 32, 32), "twin, left = right = 32")
    # everything the body covers is blocked or off the grid
    small = pt.d2_of(np.pad(np.zeros((3, 3), np.uint8), 2, constant_values=1))
    got = ctx.footprint_mask(_t(small), 32, 32, 32, 32).cpu().numpy()
    assert np.array_equal(got, pt.footprint_mask(small, 32, 32, 32, 32)) and not got.any()
    free = np.ones((5, 9), np.int32)
    assert (ctx.footprint_mask(_t(free), 32, 32, 32, 32).cpu().numpy() == 0xFF).all()      # offsets outside the grid are free


# ---- the field ----
@pytest.mark.parametrize("name", NAMES)
def test_field_equals_twin(ctx, maps, name):
    d2 = maps[name]
    hm = pt.footprint_mask(d2, *FOOT)
    cand = pt.free_cells(d2, 64, 11)
    bits = (hm.ravel()[cand][:, None] >> np.arange(8)) & 1
    root = int(cand[np.argmax(bits.sum(1))])                     # where the body fits at the most headings
    fits = np.flatnonzero(bits[np.argmax(bits.sum(1))])
    assert len(fits)
    for given, toward, turn, rev, rhead in CONFIGS:
        hmask = hm if given else None
        if given and rhead >= 0 and rhead not in fits:
            rhead = int(fits[rhead % len(fits)])
        want, wst = pt.pose_field(d2, root, rhead, turn, rev, toward, 0, hmask)
        gp, st = _gpu_field(ctx, d2, [root], [rhead], turn, rev, toward, hmask)
        assert st[0] == wst == Q_OK, (name, given, toward, turn, rev, rhead)
        _same(gp[0], want, f"{name} hmask {given} toward {toward} turn {turn} rev {rev} rhead {rhead}")


def test_roots_on_tile_borders_and_corners(ctx, ref, maps):
    d2 = maps["salt130x70"]
    H, W = d2.shape
    hm = pt.footprint_mask(d2, *FOOT)
    spots = [(31, 31), (32, 32), (63, 31), (64, 40), (31, 63), (40, 64), (63, 63), (64, 64), (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    roots = np.array([_near_free(d2, x, y) for x, y in spots], np.int32)
    rhead = np.array([k % 9 - 1 for k in range(len(roots))], np.int32)
    for toward, rev in ((False, 7), (True, 0)):
        gp, st = _gpu_field(ctx, d2, roots, rhead, 3, rev, toward, hm)
        for f in range(len(roots)):
            want, wst = ref.pose_field(d2, roots[f], rhead[f], 3, rev, toward, 0, hm)
            assert st[f] == wst
            _same(gp[f], want, f"root {spots[f]} rhead {rhead[f]} toward {toward}")
    want, _ = pt.pose_field(d2, int(roots[3]), int(rhead[3]), 3, 0, True, 0, hm)
    _same(gp[3], want, "twin")


@pytest.mark.parametrize("name", ["odd65x63", "serpentine64", "salt130x70"])
def test_every_rounds_and_the_host_form(ctx, maps, name):
    d2 = maps[name]
    hm = pt.footprint_mask(d2, *FOOT)
    root = int(next(c for c in pt.free_cells(d2, 64, 5) if hm.ravel()[c]))
    rh = int(np.flatnonzero((hm.ravel()[root] >> np.arange(8)) & 1)[-1])          # a heading the body fits at
    want, wst = pt.pose_field(d2, root, rh, 4, 7, True, 0, hm)
    assert wst == Q_OK
    for rounds in (0, 1, 2, -1, 1000):
        gp, st = _gpu_field(ctx, d2, [root], [rh], 4, 7, True, hm, rounds=rounds)
        assert st[0] == Q_OK
        _same(gp[0], want, f"{name} rounds {rounds}")
    o = ctx.pose_fields_host(d2, [root], [rh], 4, 7, True, 0, hm)
    assert o["status"][0] == Q_OK
    _same(o["gp"][0], want, f"{name} host form")


def test_fields_over_grids_and_bad_roots(ctx, ref, maps):
    d2 = np.stack([maps["salt130x70"], maps["blocks130x70"], pt.d2_of(pt.salt(130, 70, 0.1, 9))])
    H, W = d2.shape[1:]
    hm = np.stack([pt.footprint_mask(g, *FOOT) for g in d2])
    blocked = int(np.flatnonzero(d2[1].ravel() < 1)[0])
    nohead = int(np.flatnonzero((d2[0].ravel() >= 1) & (hm[0].ravel() != 0xFF) & (hm[0].ravel() != 0))[0])   # some headings valid
    dead = np.flatnonzero((d2[2].ravel() >= 1) & (hm[2].ravel() == 0))
    free = [pt.free_cells(g, 4, 20 + i) for i, g in enumerate(d2)]
    #        grid, root, rhead
    rows = [(0, free[0][0], 0), (1, free[1][0], 5), (2, free[2][0], -1), (1, blocked, 2), (0, free[0][1], 8), (0, free[0][1], -2),
            (3, free[0][2], 1), (-1, free[0][2], 1), (2, W * H, 0), (2, -1, -1), (0, nohead, -1), (1, free[1][1], 7)]
    if len(dead):
        rows[11] = (2, int(dead[0]), -1)            # a traversable cell where no heading fits: rhead -1 has no seed
    fgrid, roots, rhead = (np.array(c, np.int32) for c in zip(*rows))
    assert len(rows) == 12
    for toward in (False, True):
        o = ctx.pose_fields(_t(d2), _t(roots), _t(rhead), 6, 2, toward, hmask=_t(hm), fgrid=_t(fgrid))
        ctx.synchronize()
        gp, st = o["gp"].cpu().numpy(), o["status"].cpu().numpy()
        for f, (g, r, rh) in enumerate(rows):
            if 0 <= g < 3:
                want, wst = ref.pose_field(d2[g], r, rh, 6, 2, toward, 0, hm[g])
            else:
                want, wst = np.full((8, H, W), INF, np.int32), Q_BAD_ENDPOINT
            assert st[f] == wst, (f, rows[f])
            _same(gp[f], want, f"field {f} {rows[f]}")
    assert list(st[[3, 4, 5, 6, 7, 8, 9]]) == [Q_BAD_ENDPOINT] * 7 and st[10] == Q_OK
    want, _ = pt.pose_field(d2[0], nohead, -1, 6, 2, True, 0, hm[0])                 # rhead -1 where only some headings are valid
    _same(gp[10], want, "twin, partly valid root")


def test_anchors_on_the_device(ctx, maps):
    """(b) hmask NULL, turn_cost 0, rhead -1: every layer is the plain field; (d) min_k gp >= g for any arguments; (c) the
    toward field is the renamed toward = 0 field."""
    d2 = maps["blocks130x70"]
    hm = pt.footprint_mask(d2, *FOOT)
    roots = pt.free_cells(d2, 3, 31)
    g = ctx.cost_fields(_t(d2), _t(roots))["g"]
    for rev in (-1, 0, 7):
        gp = ctx.pose_fields(_t(d2), _t(roots), _t(np.full(3, -1, np.int32)), 0, rev)["gp"]
        ctx.synchronize()
        assert bool((gp == g[:, None]).all()), rev
    for given, toward, turn, rev, rhead in CONFIGS:
        gp = ctx.pose_fields(_t(d2), _t(roots), _t(np.full(3, rhead, np.int32)), turn, rev, toward, hmask=_t(hm if given else None))["gp"]
        ctx.synchronize()
        assert bool((gp.min(dim=1).values >= g).all()), (given, toward, turn, rev, rhead)
    for rh in (2, -1):
        for hmask in (None, hm):
            a = ctx.pose_fields(_t(d2), _t(roots), _t(np.full(3, rh, np.int32)), 5, 3, True, hmask=_t(hmask))["gp"]
            b = ctx.pose_fields(_t(d2), _t(roots), _t(np.full(3, rh if rh < 0 else (rh + 4) & 7, np.int32)), 5, 3, False,
                                hmask=_t(pt.rot4(hmask)))["gp"]
            ctx.synchronize()
            assert bool((a == b.roll(4, dims=1)).all()), (rh, hmask is None)


# ---- the read-out ----
def _gpu_paths(ctx, d2, gp, roots, rhead, qfield, targets, thead, turn, rev, toward, hmask, Lmax, to_root, cells_only, fgrid=None):
    o = ctx.pose_paths(_t(d2), _t(gp), _t(np.asarray(roots, np.int32)), _t(np.asarray(rhead, np.int32)), _t(np.asarray(qfield, np.int32)),
                       _t(np.asarray(targets, np.int32)), _t(np.asarray(thead, np.int32)), turn, rev, toward, 0, _t(hmask), Lmax, to_root,
                       cells_only, _t(fgrid))
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("toward", [False, True])
def test_readouts_300_targets(ctx, ref, maps, toward):
    d2 = maps["salt130x70"]
    H, W = d2.shape
    hm = pt.footprint_mask(d2, *FOOT)
    roots, rhead = pt.free_cells(d2, 2, 41), np.array([1, -1], np.int32)
    turn, rev = 3, 7
    gp, st = _gpu_field(ctx, d2, roots, rhead, turn, rev, toward, hm)
    rng = np.random.default_rng(42)
    targets = rng.integers(0, W * H, 300).astype(np.int32)        # blocked cells among them
    targets[:4] = [roots[0], roots[1], -1, W * H]
    thead = (rng.integers(0, 9, 300) - 1).astype(np.int32)
    thead[4:6] = [8, -2]
    qfield = (np.arange(300) % 2).astype(np.int32)
    qfield[6:8] = [2, -1]                                          # a bad qfield
    for hmask in (hm, None):
        if hmask is None:
            gp, st = _gpu_field(ctx, d2, roots, rhead, turn, rev, toward, None)
        for to_root in (False, True):
            for cells_only in (False, True):
                for Lmax in (512, 24):
                    got = _gpu_paths(ctx, d2, gp, roots, rhead, qfield, targets, thead, turn, rev, toward, hmask, Lmax, to_root, cells_only)
                    seen = set()
                    for f in (0, 1):
                        q = np.flatnonzero(qfield == f)
                        want = ref.pose_paths(d2, gp[f], roots[f], rhead[f], targets[q], thead[q], turn, rev, toward, 0, hmask, Lmax, to_root,
                                              cells_only)
                        assert pt.same_readout(want, {k: v[q] for k, v in got.items()}), (hmask is None, to_root, cells_only, Lmax, f)
                        seen |= set(want["status"].tolist())
                    assert list(got["status"][6:8]) == [Q_BAD_ENDPOINT] * 2 and list(got["len"][6:8]) == [0, 0] and list(got["cost"][6:8]) == [-1, -1]
                    assert seen >= ({Q_OK, Q_BAD_ENDPOINT, Q_TRUNCATED} if Lmax == 24 else {Q_OK, Q_BAD_ENDPOINT})
    # the twin itself on the first 40, and the _host form on all
    q = np.flatnonzero(qfield[:80] == 0)
    got = _gpu_paths(ctx, d2, gp, roots, rhead, qfield, targets, thead, turn, rev, toward, None, 512, True, True)
    want = pt.pose_paths(d2, gp[0], int(roots[0]), int(rhead[0]), targets[q], thead[q], turn, rev, toward, 0, None, 512, True, True)
    assert pt.same_readout(want, {k: v[q] for k, v in got.items()})
    host = ctx.pose_paths_host(d2, gp, roots, rhead, qfield, targets, thead, turn, rev, toward, 0, None, 512, True, True)
    assert pt.same_readout(got, host)


def test_readout_no_path_and_unreachable(ctx, ref):
    d2 = pt.d2_of(pt.door_map())
    H, W = d2.shape
    hm = pt.footprint_mask(d2, 3, 3, 3, 3)             # too wide for the door
    root, target = 11 * W + 5, 11 * W + 34
    gp, st = _gpu_field(ctx, d2, [root], [0], 2, -1, False, hm)
    got = _gpu_paths(ctx, d2, gp, [root], [0], [0, 0], [target, target], [0, -1], 2, -1, False, hm, 256, False, False)
    assert st[0] == Q_OK and list(got["status"]) == [Q_NO_PATH] * 2 and list(got["len"]) == [0, 0] and list(got["cost"]) == [-1, -1]
    want = ref.pose_paths(d2, gp[0], root, 0, [target, target], [0, -1], 2, -1, False, 0, hm, 256, False, False)
    assert pt.same_readout(want, got)


# ---- errors ----
def test_argument_errors(ctx, maps):
    import sea_current_amd as sc
    d2 = maps["sq64"]
    root = np.array([int(pt.free_cells(d2, 1, 1)[0])], np.int32)
    rh = np.zeros(1, np.int32)
    E = sc.SeaCurrentError
    for ext in ((-1, 0, 0, 0), (0, 33, 0, 0), (0, 0, -1, 0), (0, 0, 0, 33)):
        with pytest.raises(E):
            ctx.footprint_mask(_t(d2), *ext)
        with pytest.raises(E):
            ctx.footprint_mask_host(d2, *ext)
    for turn, rev in ((-1, -1), (256, -1), (1, -2), (1, 256)):
        with pytest.raises(E):
            ctx.pose_fields(_t(d2), _t(root), _t(rh), turn, rev)
        with pytest.raises(E):
            ctx.pose_fields_host(d2, root, rh, turn, rev)
    big = np.ones((1024, 1024), np.int32)                     # (14 + 243) * (8 * 1024^2 - 1) > INT32_MAX - 1 >= (14 + 242) * ...
    with pytest.raises(E):
        ctx.pose_fields_host(big, root, rh, 1, 243)
    with pytest.raises(E):
        ctx.pose_fields(_t(big), _t(root), _t(rh), 1, 243)
    with pytest.raises(E):
        ctx.pose_fields(_t(big), _t(root), _t(rh), 255, 243)
    o = ctx.pose_fields(_t(big), _t(root), _t(rh), 255, 242)
    ctx.synchronize()
    assert int(o["status"][0]) == Q_OK                        # the largest costs the rule lets through
    with pytest.raises(E):
        ctx.pose_fields(_t(np.stack([d2, d2])), _t(root), _t(rh), 1)      # two grids, no fgrid
    gp = ctx.pose_fields(_t(d2), _t(root), _t(rh), 0)["gp"]               # the field call accepts turn_cost 0 ...
    ctx.synchronize()
    q = np.zeros(1, np.int32)
    with pytest.raises(E):                                                # ... the read-out does not
        ctx.pose_paths(_t(d2), gp, _t(root), _t(rh), _t(q), _t(root), _t(q), 0)
    with pytest.raises(E):
        ctx.pose_paths(_t(d2), gp, _t(root), _t(rh), _t(q), _t(root), _t(q), 1, Lmax=0)
    with pytest.raises(E):
        ctx.pose_paths_host(d2, gp.cpu().numpy(), root, rh, q, root, q, 1, rev_cost=-2)
    bad = gp.cpu().numpy().copy()
    bad[0, 0, 0, 0] = -5
    with pytest.raises(E):                                                # the _host form checks the data
        ctx.pose_paths_host(d2, bad, root, rh, q, root, q, 1)
    import torch
    assert ctx.pose_paths(_t(d2), gp, _t(root), _t(rh), torch.zeros(0, dtype=torch.int32, device="cuda"),
                          torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), 1)["len"].numel() == 0


# ---- the chain ----
def test_one_stream_chain_with_one_synchronise(ctx, ref, oracle):
    """edt -> footprint_mask -> pose_fields(toward) -> pose_paths(cells_only) -> path_waypoints: no host hop in between."""
    occ = pt.blocks(130, 70, seed=4)
    r2, foot, turn, rev = 2, (2, 2, 1, 1), 4, 6
    ref_d2 = oracle.edt(occ)
    free = pt.free_cells(ref_d2, 40, 3, r2)
    hm_ref = ref.footprint_mask(ref_d2, *foot, r2=r2)
    goal = int(next(c for c in free if hm_ref.ravel()[c] & 1))
    starts, sh = np.array([c for c in free if c != goal][:32], np.int32), (np.arange(32) % 9 - 1).astype(np.int32)
    d2 = ctx.edt(_t(occ))
    hm = ctx.footprint_mask(d2, *foot, r2=r2)
    fld = ctx.pose_fields(d2, _t(np.array([goal], np.int32)), _t(np.zeros(1, np.int32)), turn, rev, toward=True, r2=r2, hmask=hm)
    res = ctx.pose_paths(d2, fld["gp"], _t(np.array([goal], np.int32)), _t(np.zeros(1, np.int32)), _t(np.zeros(32, np.int32)), _t(starts),
                         _t(sh), turn, rev, toward=True, r2=r2, hmask=hm, Lmax=512, to_root=True, cells_only=True)
    wp = ctx.path_waypoints(d2, res, r2=r2)
    ctx.synchronize()
    assert np.array_equal(d2.cpu().numpy(), ref_d2) and np.array_equal(hm.cpu().numpy(), hm_ref)
    gp, st = ref.pose_field(ref_d2, goal, 0, turn, rev, True, r2, hm_ref)
    assert st == Q_OK and np.array_equal(fld["gp"].cpu().numpy()[0], gp)
    want = ref.pose_paths(ref_d2, gp, goal, 0, starts, sh, turn, rev, True, r2, hm_ref, 512, True, True)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert pt.same_readout(want, got) and (got["status"] == Q_OK).sum() >= 8
    wph = ctx.path_waypoints_host(ref_d2, got["path"], got["len"], got["status"], r2=r2)
    for k in ("n", "status"):
        assert np.array_equal(wp[k].cpu().numpy(), wph[k]), k
    ok = got["status"] == Q_OK
    n = wp["n"].cpu().numpy()
    w = wp["wp"].cpu().numpy()
    assert all(np.array_equal(w[q, :n[q]], wph["wp"][q, :n[q]]) for q in np.flatnonzero(ok))      # past n the device form writes nothing
    assert (wp["status"].cpu().numpy()[ok] == 0).all()
    assert all(w[q, 0] == starts[q] and w[q, n[q] - 1] == goal for q in np.flatnonzero(ok))     # the driving order: start .. goal


def test_field_1024x700_against_c(ctx, ref, oracle):
    from sea_current_amd import synth
    d2 = oracle.edt(synth.block_grid(1024, 700, 0.2, seed=3))
    r2 = 4
    root = int(pt.free_cells(d2, 1, 8, r2)[0])
    hm = ctx.footprint_mask(_t(d2), 3, 1, 1, 1, r2=r2)
    o = ctx.pose_fields(_t(d2), _t(np.array([root], np.int32)), _t(np.array([-1], np.int32)), 5, 9, True, r2=r2, hmask=hm)
    ctx.synchronize()
    hmc = ref.footprint_mask(d2, 3, 1, 1, 1, r2=r2)
    _same(hm.cpu().numpy(), hmc, "mask")
    want, st = ref.pose_field(d2, root, -1, 5, 9, True, r2, hmc)
    assert st == Q_OK and o["status"].cpu().numpy()[0] == Q_OK
    _same(o["gp"].cpu().numpy()[0], want, "1024 x 700")
