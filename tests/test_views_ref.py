"""The CPU statements of line-of-sight sensing against each other: the NumPy twin (tests/views_twin.py) == the C reference
(tests/cpp/views_ref.c) in known, occ_seen and gain; the column walk == the four-corner sign test over the bounding box; the
corner rule; the consequences the definition states; ignored views, R = 0, base in place, the largest r2, a surface cell
outside the disc; the door map's counts; the gain identity; the exploration loop on a block map and on rooms with doors; the C
reference under AddressSanitizer and UBSan as a program of its own.  No GPU.

The two salt maps of frontier_twin.loop_maps() are left out of the loop test: under the supercover rule salt at p >= 0.2 blocks
nearly every ray, the loop needs 601 and 1 163 iterations there, which is correct, and slow for a test."""
import os
import subprocess

import numpy as np
import pytest

import frontier_twin as ft
import views_twin as vt
from field_twin import Twin as FieldTwin

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = os.path.join(HERE, "cpp", "views_ref_check.c")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return vt.Ref(tmp_path_factory.mktemp("views_ref"))


@pytest.fixture(scope="module")
def fields(tmp_path_factory):
    return FieldTwin(tmp_path_factory.mktemp("field_ref"))


def _cases():
    """name -> (occ, views)"""
    salt05, salt2, blocks = vt.salt(130, 70, 0.05, 2), vt.salt(130, 70, 0.2, 2), vt.blocks()
    line = np.zeros((1, 200), np.uint8)
    line[0, [80, 150]] = 1
    return {
        "salt0.05": (salt05, vt.free_centres(salt05, ft.three_discs(130, 70))),
        "salt0.2": (salt2, ft.three_discs(130, 70)),                  # the middle centre stands on an obstacle
        "blocks": (blocks, vt.free_centres(blocks, ft.three_discs(128, 96))),
        "door": (vt.door_map(), np.array([vt.DOOR_VIEW], np.int32)),
        "row": (line, np.array([(50, 0, 10000), (120, 0, 25)], np.int32)),
        "column": (np.ascontiguousarray(line.T), np.array([(0, 50, 10000), (0, 120, 25)], np.int32)),
    }


NAMES = ["salt0.05", "salt0.2", "blocks", "door", "row", "column"]


@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_c_reference(ref, name):
    occ, views = _cases()[name]
    rng = np.random.default_rng(3)
    base = (rng.random(occ.shape) < 0.1).astype(np.uint8) * 7
    for b in (None, base):
        known, occ_seen = vt.known_from_views(b, occ, views)
        k2, s2 = ref.known_from_views(b, occ, views)
        assert known.dtype == k2.dtype == np.uint8 and np.array_equal(known, k2) and np.array_equal(occ_seen, s2)
        assert set(np.unique(known)) <= {0, 1} and known.any()
        before = np.zeros_like(occ) if b is None else b
        gain = vt.view_gain(occ, before, views)
        assert gain.dtype == np.int32 and np.array_equal(gain, ref.view_gain(occ, before, views)) and gain.sum() > 0
    if name == "salt0.2":
        assert occ[35, 65] != 0 and gain[1] == 0
        known, _ = vt.known_from_views(None, occ, views)
        assert int(vt.seen(occ, views).sum()) == 200 and int(known.sum()) == 266
        assert int(ft.known_from_discs(None, views, 130, 70).sum()) == 3647


def test_column_walk_equals_the_four_corner_test(ref):
    rng = np.random.default_rng(11)
    cases = _cases()
    names = [NAMES[k % len(NAMES)] for k in range(40)]
    for k, name in enumerate(names):
        occ, _ = cases[name]
        H, W = occ.shape
        free = np.flatnonzero(occ.ravel() == 0)
        c = int(free[rng.integers(len(free))])
        cx, cy, r = c % W, c // W, int(rng.integers(1, 9))
        ys, xs = np.mgrid[max(cy - r, 0):min(cy + r, H - 1) + 1, max(cx - r, 0):min(cx + r, W - 1) + 1]
        xs, ys = xs.ravel(), ys.ravel()
        walk = vt.clear_targets(occ, cx, cy, xs, ys)
        for x, y, w in zip(xs.tolist(), ys.tolist(), walk.tolist()):
            naive = vt.clear_bruteforce(occ, cx, cy, x, y)
            assert w == naive == vt.clear(occ, cx, cy, x, y) == ref.clear(occ, cx, cy, x, y), (name, cx, cy, x, y)
    # long rays too: from one corner of the door map to every cell of the far columns
    occ = vt.door_map()
    for x, y in [(95, 63), (95, 0), (60, 31), (49, 29), (49, 33), (70, 40)]:
        assert vt.clear(occ, 20, 31, x, y) == vt.clear_bruteforce(occ, 20, 31, x, y) == ref.clear(occ, 20, 31, x, y)


def test_corner_rule():
    view = [(4, 4, 8)]
    for block, seen in (([(5, 4)], False), ([(4, 5)], False), ([], True)):
        occ = vt.corner_map(block)
        assert vt.clear(occ, 4, 4, 5, 5) == seen == vt.clear_bruteforce(occ, 4, 4, 5, 5)
        assert bool(vt.seen(occ, view)[5, 5]) == seen


def test_consequences(ref):
    # (i) on a free map with all centres in the grid: the discs
    free = np.zeros((70, 130), np.uint8)
    views = np.array([(10, 10, 30), (64, 35, 0), (129, 69, 100), (0, 0, 400), (65, 35, 2000)], np.int32)
    for impl in (vt, ref):
        known, occ_seen = impl.known_from_views(None, free, views)
        assert np.array_equal(known, ft.known_from_discs(None, views, 130, 70)) and not occ_seen.any()
    # (ii) vis inside the discs, known \ base inside the discs dilated by one orthogonal step
    for name in ("salt0.05", "salt0.2", "blocks", "door"):
        occ, views = _cases()[name]
        H, W = occ.shape
        disc = ft.known_from_discs(None, views, W, H) != 0
        vis = vt.seen(occ, views)
        known, occ_seen = vt.known_from_views(None, occ, views)
        assert not (vis & ~disc).any() and not (vis & (occ != 0)).any()
        assert not ((known != 0) & ~(disc | vt.neighbours4(disc))).any()
        assert np.array_equal(occ_seen, np.where(known != 0, occ, 0))
    # (iii) from a frontier cell with r2 >= 1 a view reveals every unknown orthogonal neighbour
    occ, views = _cases()["blocks"]
    H, W = occ.shape
    known, occ_seen = vt.known_from_views(None, occ, views)
    d2k = np.where((known != 0) & (occ_seen == 0), 9, 0).astype(np.int32)
    fr = np.flatnonzero(ft.frontier_mask(d2k, known).ravel())
    assert len(fr) > 20
    for c in fr[:: max(len(fr) // 25, 1)].tolist():
        x, y = c % W, c // W
        more, _ = vt.known_from_views(known, occ, [(x, y, 1)])
        for xx, yy in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
            if 0 <= xx < W and 0 <= yy < H:
                assert more[yy, xx] == 1


def test_ignored_views(ref):
    occ, _ = _cases()["salt0.05"]
    occ = occ.copy()
    occ[20, 40] = 1
    base = np.zeros_like(occ)
    base[3, 3] = 5
    ignored = np.array([(30, 35, -1), (-1, 35, 400), (130, 35, 400), (30, -1, 400), (30, 70, 400), (40, 20, 400)], np.int32)
    for impl in (vt, ref):
        known, occ_seen = impl.known_from_views(base, occ, ignored)
        assert np.array_equal(known, (base != 0).astype(np.uint8)) and np.array_equal(occ_seen, np.where(base != 0, occ, 0))
        assert not impl.view_gain(occ, base, ignored).any()
        # among live views they change nothing
        live = vt.free_centres(occ, ft.three_discs(130, 70))
        mixed = np.concatenate([ignored[:3], live, ignored[3:]])
        assert np.array_equal(impl.known_from_views(base, occ, mixed)[0], impl.known_from_views(base, occ, live)[0])
        assert np.array_equal(impl.view_gain(occ, base, mixed)[3:6], impl.view_gain(occ, base, live))


def test_no_views_copies_base_and_base_may_be_known(ref):
    occ, views = _cases()["blocks"]
    rng = np.random.default_rng(5)
    base = (rng.random(occ.shape) < 0.2).astype(np.uint8) * 9
    none = np.zeros((0, 3), np.int32)
    for impl in (vt, ref):
        known, occ_seen = impl.known_from_views(base, occ, none)
        assert np.array_equal(known, (base != 0).astype(np.uint8)) and np.array_equal(occ_seen, np.where(base != 0, occ, 0))
        assert not impl.known_from_views(None, occ, none)[0].any()
    want, want_seen = vt.known_from_views(base, occ, views)
    got, got_seen = ref.known_from_views(base, occ, views, in_place=True)      # base is the array known is written to
    assert np.array_equal(got, want) and np.array_equal(got_seen, want_seen)
    # order of the views
    assert np.array_equal(vt.known_from_views(base, occ, views[::-1])[0], want)


def test_largest_r2_needs_64_bit_squares(ref):
    occ, _ = _cases()["salt0.05"]
    views = np.array([(30, 35, 2**31 - 1)], np.int32)
    views = vt.free_centres(occ, views)
    known, _ = vt.known_from_views(None, occ, views)
    assert np.array_equal(known, ref.known_from_views(None, occ, views)[0])
    # the disc covers the grid: vis is what is Clear from the centre, wherever it lies
    cx, cy = int(views[0, 0]), int(views[0, 1])
    ys, xs = np.mgrid[0:70, 0:130]
    assert np.array_equal(vt.seen(occ, views), vt.clear_targets(occ, cx, cy, xs.ravel(), ys.ravel()).reshape(70, 130))
    assert np.array_equal(vt.view_gain(occ, np.zeros_like(occ), views), ref.view_gain(occ, np.zeros_like(occ), views))
    assert 1000 < known.sum() < 130 * 70


def test_surface_cell_outside_the_disc_is_known(ref):
    occ = np.zeros((9, 9), np.uint8)
    occ[:, 7] = 1
    view = [(4, 4, 4)]                                                 # reaches x = 6; the wall at x = 7 lies outside
    for impl in (vt, ref):
        known, occ_seen = impl.known_from_views(None, occ, view)
        assert known[4, 6] == 1 and known[4, 7] == 1 and occ_seen[4, 7] == 1 and (4 - 7) ** 2 > 4
        assert known[:, 7].sum() == 1 and not known[:, 8].any()


def test_door_map_counts(ref):
    """The prototype's figures: 3 215 seen free cells, 3 276 known, the whole of column 48 (61 wall cells and the 3 of the
    door), 140 known cells beyond the wall where the disc marks 1 820."""
    occ = vt.door_map()
    vis = vt.seen(occ, [vt.DOOR_VIEW])
    known, _ = vt.known_from_views(None, occ, [vt.DOOR_VIEW])
    assert int(vis.sum()) == 3215 and int(known.sum()) == 3276
    assert known[:, 48].all() and int((occ[:, 48] != 0).sum()) == 61 and vis[30:33, 48].all()
    assert int(known[:, 49:].sum()) == 140
    assert int(ft.known_from_discs(None, [vt.DOOR_VIEW], 96, 64)[:, 49:].sum()) == 1820


@pytest.mark.parametrize("name", ["salt0.05", "blocks", "door"])
def test_gain_identity_with_the_true_map(ref, name):
    occ, views = _cases()[name]
    H, W = occ.shape
    rng = np.random.default_rng(9)
    free = np.flatnonzero(occ.ravel() == 0)
    cand = free[rng.choice(len(free), 12, replace=False)]
    views = np.concatenate([views, np.stack([cand % W, cand // W, rng.integers(0, 300, 12)], 1).astype(np.int32)])
    known, _ = vt.known_from_views(None, occ, views[:1])
    gain = vt.view_gain(occ, known, views)
    assert np.array_equal(gain, ref.view_gain(occ, known, views)) and gain[0] == 0 and gain.max() > 0
    for i, v in enumerate(views):
        more, _ = vt.known_from_views(known, occ, v[None])
        assert gain[i] == int(((more != 0) & (known == 0) & (occ == 0)).sum()), i


@pytest.mark.parametrize("name", ["salt0.05", "salt0.2", "blocks"])
def test_gain_on_the_observed_map_is_no_less(name):
    """Removing obstacles only clears rays: with occ_seen (unknown cells read 0) every pose sees at least what it sees on the
    true map."""
    occ, views = _cases()[name]
    H, W = occ.shape
    known, occ_seen = vt.known_from_views(None, occ, views[:1])
    free = np.flatnonzero((known != 0).ravel() & (occ.ravel() == 0))
    cand = free[np.random.default_rng(2).choice(len(free), 16, replace=False)]
    poses = np.stack([cand % W, cand // W, np.full(16, 144)], 1).astype(np.int32)
    predicted, true = vt.view_gain(occ_seen, known, poses), vt.view_gain(occ, known, poses)
    assert (predicted >= true).all() and (predicted > true).any()


@pytest.mark.parametrize("name,iterations", [("blocks96x80", 104), ("rooms96x80", None)])
def test_exploration_ends_with_the_component_known(oracle, fields, name, iterations):
    occ = vt.loop_maps()[name]
    start = ft.loop_start(occ)
    goals, known = vt.explore_loop_views(occ, start, ft.twin_step(oracle, fields))
    comp = ft.true_component(occ, start)
    assert len(goals) >= 10 and len(set(goals)) == len(goals)
    assert (known[comp] != 0).all()
    assert comp.ravel()[goals].all()
    if iterations is not None:
        assert len(goals) == iterations                                # the disc sensor takes 74
        assert len(ft.explore_loop(occ, start, ft.twin_step(oracle, fields))[0]) == 74
    else:
        assert comp.sum() == (occ == 0).sum()                          # the doors join all six rooms


def test_check_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "views_ref_check")
    subprocess.check_call(["cc", "-g", "-O1", "-std=c11", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           CHECK, vt.SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("views_ref OK") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
