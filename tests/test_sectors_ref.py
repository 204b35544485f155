"""The CPU statements of sensors with a field of view against each other: the NumPy twin (tests/sectors_twin.py) == the C
statement (tests/cpp/sectors_ref.c) in every output, on salt 130 x 70 at p = 0.05, blocks 128 x 96, the door map, 1 x 200 and
200 x 1; the predicate along a (in), along b (out) and opposite to a for tables of 3, 8 and 64 directions at a phase != 0, its
four cases and every ignored kind; the identities (a), (b), (c) for every heading and span in {1, B/2, B - 1, B}; the heading
table's rules; a view on an occupied cell, r2 = 0, a surface cell outside the sector; rows from goal cells; the binding's host
helpers; the exploration loop with a quarter-circle sensor on a block map and on rooms with doors; the C statement under
AddressSanitizer and UBSan as a program of its own.  No GPU.

The loop maps are views_twin.loop_maps(): the two salt maps of frontier_twin.loop_maps() stay out for section 23.5's reason
(601 and 1 163 iterations with the full circle already)."""
import os
import subprocess

import numpy as np
import pytest

import frontier_twin as ft
import sectors_twin as st
import views_twin as vt
from field_twin import Twin as FieldTwin

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = os.path.join(HERE, "cpp", "sectors_ref_check.c")
PHASES = (0.0, 0.5, 0.123)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return st.Ref(tmp_path_factory.mktemp("sectors_ref"))


@pytest.fixture(scope="module")
def fields(tmp_path_factory):
    return FieldTwin(tmp_path_factory.mktemp("field_ref"))


def _cases():
    """name -> (occ, views)"""
    salt05, blocks = vt.salt(130, 70, 0.05, 2), vt.blocks()
    line = np.zeros((1, 200), np.uint8)
    line[0, [80, 150]] = 1
    return {
        "salt0.05": (salt05, vt.free_centres(salt05, ft.three_discs(130, 70))),
        "blocks": (blocks, vt.free_centres(blocks, ft.three_discs(128, 96))),
        "door": (vt.door_map(), np.array([vt.DOOR_VIEW], np.int32)),
        "row": (line, np.array([(50, 0, 10000), (120, 0, 25)], np.int32)),
        "column": (np.ascontiguousarray(line.T), np.array([(0, 50, 10000), (0, 120, 25)], np.int32)),
    }


NAMES = ["salt0.05", "blocks", "door", "row", "column"]
IGNORED_PAIRS = [((1, 0), (2, 0)), ((3, 3), (3, 3)), ((1, 0), (0, 0)), ((0, 0), (0, 1)), ((32768, 0), (0, 1)), ((1, 0), (0, -32768))]


def _known(occ, views):
    """a partly known map: what the first view sees at half its radius, and a sprinkle"""
    near = np.array(views[:1], np.int32)
    near[0, 2] //= 4
    known, _ = vt.known_from_views(None, occ, near)
    rng = np.random.default_rng(3)
    return (known | (rng.random(occ.shape) < 0.05)).astype(np.uint8)


@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_c_statement(ref, name):
    occ, views = _cases()[name]
    known = _known(occ, views)
    dirs = st.heading_dirs(8, 0.123)
    rows = np.concatenate([st.sector_views(views, dirs, h, span) for h, span in ((0, 1), (1, 2), (3, 4), (6, 5), (2, 8), (5, 7))])
    ignored = np.array([(int(views[0, 0]), int(views[0, 1]), 400, *a, *b) for a, b in IGNORED_PAIRS], np.int64)
    ignored = np.clip(ignored, -2**31, 2**31 - 1).astype(np.int32)
    rows = np.concatenate([rows[:4], ignored, rows[4:]])
    for base in (None, known):
        k, s = st.known_from_sectors(base, occ, rows)
        k2, s2 = ref.known_from_sectors(base, occ, rows)
        assert k.dtype == k2.dtype == np.uint8 and np.array_equal(k, k2) and np.array_equal(s, s2) and k.any()
    assert np.array_equal(ref.known_from_sectors(known, occ, rows, in_place=True)[0], k)
    gain = st.sector_gain(occ, known, rows)
    assert gain.dtype == np.int32 and np.array_equal(gain, ref.sector_gain(occ, known, rows)) and gain.sum() > 0
    assert not gain[4:4 + len(ignored)].any()
    # ignored rows alone: base, and nothing else
    k, s = st.known_from_sectors(known, occ, ignored)
    assert np.array_equal(k, (known != 0).astype(np.uint8)) and np.array_equal(ref.known_from_sectors(known, occ, ignored)[0], k)
    for B, span in ((3, 1), (8, 3), (64, 16)):
        d = st.heading_dirs(B, 0.5)
        tw, rf = st.view_gain_headings(occ, known, views, d, span), ref.view_gain_headings(occ, known, views, d, span)
        for key in ("hist", "gainh", "best"):
            assert tw[key].dtype == np.int32 and np.array_equal(tw[key], rf[key]), (B, span, key)


@pytest.mark.parametrize("B", [3, 8, 64])
def test_predicate_on_the_edges(ref, B):
    """Exactly along a: in; exactly along b: out; opposite to a: in only for a reflex sector."""
    dirs = st.heading_dirs(B, 0.123).astype(np.int64)
    for h in range(B):
        for span in sorted({1, B // 2, B - 1}):
            a, b = dirs[h], dirs[(h + span) % B]
            s = st.cross(a[0], a[1], b[0], b[1])
            for k in (1, 3):
                for d, want in ((k * a, True), (k * b, False), (-k * a, s < 0)):
                    assert bool(st.in_sector(d[0], d[1], a, b)) == want == bool(ref.in_sector(d[0], d[1], a, b)), (h, span, k)


def test_predicate_cases_and_ignored_kinds(ref):
    E, N, Wd, S = (1, 0), (0, 1), (-1, 0), (0, -1)
    table = [
        (E, N, [((3, 0), 1), ((0, 3), 0), ((-3, 0), 0), ((2, 2), 1), ((2, -1), 0)]),                 # s > 0
        (N, E, [((0, 3), 1), ((3, 0), 0), ((0, -3), 1), ((2, 2), 0), ((-2, 2), 1), ((2, -2), 1)]),   # s < 0
        (E, Wd, [((3, 0), 1), ((-3, 0), 0), ((0, 3), 1), ((0, -3), 0), ((-5, 1), 1), ((5, -1), 0)]),  # half a turn
        ((0, 0), (0, 0), [((-5, -7), 1), ((0, 0), 1)]),                                             # the full circle
        ((32767, -32767), (-32767, 32767), [((1, 1), 1), ((-1, -1), 0), ((1, -1), 1), ((-1, 1), 0)]),
    ]
    for a, b, cases in table:
        assert not st.sector_ignored(a, b)
        for d, want in cases:
            assert int(st.in_sector(d[0], d[1], a, b)) == want == ref.in_sector(d[0], d[1], a, b), (a, b, d)
        assert st.in_sector(0, 0, a, b) and ref.in_sector(0, 0, a, b) == 1                           # the centre
    for a, b in IGNORED_PAIRS:
        assert st.sector_ignored(a, b)
        assert ref.in_sector(0, 0, a, b) == -1 and ref.in_sector(1, 1, a, b) == -1


@pytest.mark.parametrize("B", [3, 4, 5, 8, 12, 16, 32, 64])
def test_tables(ref, B):
    """The issue's tables are valid and their bins partition the offsets; unions of consecutive bins are sectors; the broken
    tables are refused by the twin, the C statement and the binding's helper agrees with the twin's table."""
    import sea_current_amd as sc
    ys, xs = np.mgrid[-45:46, -45:46].astype(np.int64)
    xs, ys = xs.ravel(), ys.ravel()
    for phase in PHASES:
        d = st.heading_dirs(B, phase)
        assert d.dtype == np.int32 and np.array_equal(d, sc.heading_dirs(B, phase))
        assert st.dirs_valid(d) and ref.dirs_valid(d)
        bins = st.bins_of(d, xs, ys)                                  # asserts the partition
        assert (bins[(xs != 0) | (ys != 0)] >= 0).all() and bins[(xs == 0) & (ys == 0)].tolist() == [-1]
        for h in range(0, B, max(B // 8, 1)):
            for span in range(1, B):
                union = (bins >= 0) & ((bins - h) % B < span)
                got = st.in_sector(xs, ys, d[h], d[(h + span) % B]) & (bins >= 0)
                assert np.array_equal(union, got), (phase, h, span)
        swapped, repeated, far = d.copy(), d.copy(), d.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        repeated[1] = repeated[0]
        far[0] = (32768, 0)
        bad = [d[::-1], swapped, repeated, far, d[:2]]
        if 2 * B <= 64:
            bad.append(np.concatenate([d, d]))                         # two turns
        if B % 2 and B >= 5:
            bad.append(d[(2 * np.arange(B)) % B])                      # two turns without a repeated entry
        for t in bad:
            assert not st.dirs_valid(t) and not ref.dirs_valid(np.ascontiguousarray(t))
    assert ref.bins_of(st.heading_dirs(B), 0, 0) == (0, -1)
    for k in (0, len(xs) // 3, len(xs) - 1):
        assert ref.bins_of(st.heading_dirs(B), xs[k], ys[k]) == (1, int(st.bins_of(st.heading_dirs(B), xs[k:k + 1], ys[k:k + 1])[0]))


@pytest.mark.parametrize("name,B", [("salt0.05", 8), ("blocks", 64), ("door", 3), ("row", 8), ("column", 16)])
def test_identities(ref, name, B):
    occ, views = _cases()[name]
    H, W = occ.shape
    known = _known(occ, views)
    if name in ("salt0.05", "blocks"):                                # smaller discs keep 64 x 4 sector calls quick
        views = views.copy()
        views[:, 2] = (144, 400, 49)
    views = np.concatenate([views, [(0, 0, -1)], [(W, 0, 9)]]).astype(np.int32)      # ignored candidates among them
    d = st.heading_dirs(B, 0.123)
    full = vt.view_gain(occ, known, views)
    # (c)
    zero = st.sector_views(views, d, 0, B)
    assert not zero[:, 3:].any()
    for impl in (st, ref):
        k, s = impl.known_from_sectors(known, occ, zero)
        kv, sv = vt.known_from_views(known, occ, views)
        assert np.array_equal(k, kv) and np.array_equal(s, sv)
        assert np.array_equal(impl.sector_gain(occ, known, zero), full)
    for span in sorted({1, B // 2, B - 1, B}):
        tw = st.view_gain_headings(occ, known, views, d, span)
        rf = ref.view_gain_headings(occ, known, views, d, span)
        for key in ("hist", "gainh", "best"):
            assert np.array_equal(tw[key], rf[key]), (span, key)
        assert np.array_equal(tw["hist"].sum(1) + tw["c0"], full)                             # (a)
        assert set(np.unique(tw["c0"])) <= {0, 1}
        assert not tw["hist"][-2:].any() and tw["best"][-2:].tolist() == [[0, 0], [0, 0]]     # the ignored candidates
        for h in range(B):                                                                    # (b)
            want = ref.sector_gain(occ, known, st.sector_views(views, d, h, span))
            assert np.array_equal(tw["gainh"][:, h], want), (span, h)
            if span == B:
                assert np.array_equal(want, full)
        first = np.array([int(np.flatnonzero(g == g.max())[0]) for g in tw["gainh"]])
        assert np.array_equal(tw["best"][:, 1], first) and np.array_equal(tw["best"][:, 0], tw["gainh"].max(1))
    assert full[:-2].sum() > 0
    assert ref.view_gain_headings(occ, known, views, d, 0) is None and ref.view_gain_headings(occ, known, views, d, B + 1) is None
    assert ref.view_gain_headings(occ, known, views, d[::-1], 1) is None


def test_single_views(ref):
    occ = np.zeros((9, 9), np.uint8)
    occ[:, 7] = 1
    occ[2, 2] = 1
    d = st.heading_dirs(8)                                            # bins of 45 degrees from the x axis
    for impl in (st, ref):
        # a view on an occupied cell sees nothing, in any sector
        k, s = impl.known_from_sectors(None, occ, [(2, 2, 16, 1, 0, 0, 1)])
        assert not k.any() and not s.any() and impl.sector_gain(occ, np.zeros_like(occ), [(2, 2, 16, 1, 0, 0, 1)]).tolist() == [0]
        # r2 = 0: the centre, which belongs to every sector
        k, _ = impl.known_from_sectors(None, occ, [(4, 4, 0, 0, -1, -1, 0)])
        assert int(k.sum()) == 1 and k[4, 4] == 1
        # east to north, r2 = 4 reaches x = 6: the wall cell (7, 4) lies outside the disc, (7, 3) besides below the sector
        k, s = impl.known_from_sectors(None, occ, [(4, 4, 4, 1, 0, 0, 1)])
        assert k[4, 6] == 1 and k[4, 7] == 1 and s[4, 7] == 1
        assert [(int(y), int(x)) for y, x in zip(*np.nonzero(k))] == [(4, 4), (4, 5), (4, 6), (4, 7), (5, 5)]   # x = 4, along b, is out
        # a surface cell outside the sector: 0 .. 45 degrees from (5, 4) sees (6, 4); the obstacle (6, 3) beside it lies below a
        occ2 = occ.copy()
        occ2[3, 6] = 1
        k, s = impl.known_from_sectors(None, occ2, [(5, 4, 9, *d[0], *d[1])])
        assert not st.in_sector(1, -1, d[0], d[1]) and k[3, 6] == 1 and s[3, 6] == 1
        assert [(int(y), int(x)) for y, x in zip(*np.nonzero(k))] == [(3, 6), (4, 5), (4, 6), (4, 7)]


def test_rows_from_goals(ref):
    W, H = 130, 70
    cell = np.array([0, 129, 130, W * H - 1, -1, W * H, -2**31, 2**31 - 1, 35 * W + 64], np.int32)
    want = np.array([(0, 0, 100), (129, 0, 100), (0, 1, 100), (129, 69, 100), (0, 0, -1), (0, 0, -1), (0, 0, -1), (0, 0, -1), (64, 35, 100)], np.int32)
    assert np.array_equal(st.views_from_cells(cell, W, H, 100), want) and np.array_equal(ref.views_from_cells(cell, W, H, 100), want)
    assert st.views_from_cells(np.zeros(0, np.int32), W, H, 100).shape == (0, 3)
    # an ignored row sees nothing
    occ = np.zeros((H, W), np.uint8)
    assert not vt.known_from_views(None, occ, want[4:5])[0].any()


def test_binding_helpers():
    import sea_current_amd as sc
    views = np.array([(3, 4, 100), (5, 6, 9)], np.int32)
    d = sc.heading_dirs(16, 0.5)
    for h, span in ((0, 4), (15, 4), (np.array([3, 14]), 15), (2, 16)):
        got = sc.sector_views(views, d, h, span)
        assert got.dtype == np.int32 and np.array_equal(got, st.sector_views(views, d, h, span))
    assert not sc.sector_views(views, d, 5, 16)[:, 3:].any()
    for bad in (2, 65):
        with pytest.raises(sc.SeaCurrentError):
            sc.heading_dirs(bad)
    for bad in (0, 17):
        with pytest.raises(sc.SeaCurrentError):
            sc.sector_views(views, d, 0, bad)
    assert sc.VIEW_MAX_BINS == st.MAX_BINS == 64


LOOP_COUNTS = {"blocks96x80": (189, 0), "rooms96x80": (229, 0)}     # (iterations, full-circle fallbacks); the full circle: 104 and 87


@pytest.mark.parametrize("name", ["blocks96x80", "rooms96x80"])
def test_exploration_ends_with_the_component_known(oracle, fields, name):
    occ = vt.loop_maps()[name]
    start = ft.loop_start(occ)
    dirs = st.heading_dirs(16)
    r = st.explore_loop_sectors(occ, start, ft.twin_step(oracle, fields), dirs, 4, sense_r2=100)
    comp = ft.true_component(occ, start)
    assert (r["known"][comp] != 0).all() and comp.ravel()[r["goals"]].all()
    assert len(r["headings"]) == len(r["goals"]) + 1 and all(0 <= h < 16 for h in r["headings"])
    assert (len(r["goals"]), r["fallbacks"]) == LOOP_COUNTS[name]
    # a quarter of the circle per look needs more looks than the full circle
    assert len(r["goals"]) > len(vt.explore_loop_views(occ, start, ft.twin_step(oracle, fields))[0])


def test_check_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sectors_ref_check")
    subprocess.check_call(["cc", "-g", "-O1", "-std=c11", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           CHECK, st.SRC, vt.SRC, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("sectors_ref OK") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
