"""Wide-window scan matching on the CPU: the NumPy twin (tests/match_wide_twin.py), the C statement
(tests/cpp/match_wide_ref.c: a plain dense search for best, the procedure for stats) and, for windows up to +-64, the dense
twin (match_twin.match) agree in best; twin and C statement agree in stats.  The contract cases; recovery of known poses
from priors anywhere in a wide window; the condition that pruning happens; the kidnapped robot; the C statement under
AddressSanitizer and UBSan as a program of its own.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import match_twin as mt
import match_wide_cases as mc
import match_wide_twin as mw

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = os.path.join(HERE, "cpp", "match_wide_ref_check.c")
NAMES = ["blocks", "salt0.05", "door", "rooms", "row", "column"]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mw.Ref(tmp_path_factory.mktemp("match_wide_ref"))


def _agree(ref, d2, known, pts, centre, wx, wy, cap, unk, top, max_nodes=1 << 14):
    """Twin == C statement in best and stats (and without stats in best); == the dense twin where it can run."""
    tb, ts = mw.match_wide(d2, known, pts, centre, wx, wy, cap, unk, top, max_nodes)
    cb, cs = ref.match(d2, known, pts, centre, wx, wy, cap, unk, top, max_nodes)
    what = (wx, wy, cap, unk, top)
    assert tb.dtype == cb.dtype == np.int32 and np.array_equal(tb, cb), (what, tb.tolist(), cb.tolist())
    assert np.array_equal(ts, cs), (what, ts.tolist(), cs.tolist())
    if not (tb[:, 0] == mw.OVERFLOW).any():
        assert np.array_equal(ref.match(d2, known, pts, centre, wx, wy, cap, unk, top, max_nodes, want_stats=False)[0], tb)
        if wx <= mt.MAX_HALF and wy <= mt.MAX_HALF:
            assert np.array_equal(mt.match(d2, known, pts, centre, wx, wy, cap, unk)[0], tb), what
    return tb, ts


@pytest.mark.parametrize("name", NAMES)
def test_twin_c_statement_and_dense_twin_agree(oracle, ref, name):
    occ = mc.maps()[name]
    H, W = occ.shape
    d2 = oracle.edt(occ)
    known = (np.random.default_rng(4).random((H, W)) < 0.7).astype(np.uint8)
    # three scans of two rotations: a fan from the middle with the prior off, one from a corner with a window that sticks out
    # of the grid, and one whose prior lies outside the grid
    x0, y0 = mc.free_near(occ, W // 2, H // 2)
    x1, y1 = mc.free_near(occ, 1, 0)
    p0, p1 = mc.scan_points(occ, x0, y0, 25), mc.scan_points(occ, x1, y1, 25)
    pts = np.stack([np.stack([p, mt.quarter_turns(p, 1)]) for p in (p0, p1, p0)])
    centre = [(x0 + 2, y0 - min(1, y0)), (x1 - 1, y1), (-3, H + 2)]
    for top in range(4):
        for kn, (wx, wy, cap, unk) in zip((None, known, None, known, known),
                                          ((9, 6, 64, 1), (3, 3, 1, 0), (33, 2, 32767, 32767), (2, 21, 9, 9), (0, 0, 64, 0))):
            best, stats = _agree(ref, d2, kn, pts, centre, wx, wy, cap, unk, top)
            n_top = 2 * (2 * wx // 4**top + 1) * (2 * wy // 4**top + 1)  # a scan without a present point (the door map's corner) has zero stats
            assert (stats[:, top + 1:6] == 0).all() and np.isin(stats[:, top], (0, n_top)).all() and stats[0, top] == n_top
    assert best[0, 4] > 0


def test_top_5_on_a_line(oracle, ref):
    occ = mc.line()
    d2 = oracle.edt(occ)
    pts = np.array([(-20, 0), (50, 0), (3, 0)], np.int32)[None, None]  # the two obstacles seen from cell 100, and a stray point
    for off in (1500, -1900, 0):
        best, stats = _agree(ref, d2, None, pts, [(100 + off, 0)], 2048, 0, 64, 64, 5, max_nodes=4096)
        assert best[0].tolist() == [0, -off, 0, 64, 3, 1] and stats[0, 5] == 5
    best, stats = _agree(ref, np.ascontiguousarray(d2.T), None, pts[..., ::-1], [(0, 100 + 700)], 0, 2048, 64, 64, 5, max_nodes=4096)
    assert best[0].tolist() == [0, 0, -700, 64, 3, 1]


def test_a_window_smaller_than_one_node(oracle, ref):
    occ = mc.maps()["blocks"]
    d2 = oracle.edt(occ)
    x, y = mc.free_near(occ, 60, 50)
    pts = mc.scan_points(occ, x, y, 20)[None, None]
    for top, n in ((1, [4]), (2, [4, 1]), (3, [4, 1, 1])):
        best, stats = _agree(ref, d2, None, pts, [(x + 2, y - 3)], 3, 3, 64, 1, top)
        assert stats[0, 1:top + 1].tolist() == n and best[0, :4].tolist() == [0, -2, 3, 0]


def test_all_points_absent_and_an_ignored_scan_between_live_ones(oracle, ref):
    occ = mc.maps()["salt0.05"]
    d2 = oracle.edt(occ)
    x, y = mc.free_near(occ, 60, 30)
    p = mc.scan_points(occ, x, y, 20)
    pts = np.stack([np.stack([p, mt.quarter_turns(p, 1), mt.quarter_turns(p, 2)])] * 3)
    none = np.full_like(pts, mt.ABSENT)
    best, stats = _agree(ref, d2, None, none, [(x, y)] * 3, 100, 70, 64, 1, 3)
    assert best.tolist() == [[0, 0, 0, 0, 0, 3 * 201 * 141]] * 3 and not stats.any()
    for bad in ((-mt.MAX_REACH - 1, 5), (5, mt.MAX_DIM + mt.MAX_REACH + 1), (2**31 - 1, -2**31)):
        best, stats = _agree(ref, d2, None, pts, [(x + 30, y - 20), bad, (x - 7, y + 9)], 40, 30, 64, 1, 2)
        assert best[1].tolist() == [mt.IGNORED, 0, 0, 0, 0, 0] and not stats[1].any()
        assert best[0, :4].tolist() == [0, -30, 20, 0] and best[2, :4].tolist() == [0, 7, -9, 0] and stats[0, 2] == stats[2, 2] == 3 * 6 * 4
    # a rotation that lost its points wins with 0, as in the dense matcher
    mixed = pts.copy()
    mixed[:, 2] = mt.ABSENT
    assert (_agree(ref, d2, None, mixed, [(x + 3, y)] * 3, 20, 20, 64, 1, 2)[0][:, [0, 3, 4]] == [2, 0, 0]).all()


def test_tie_order(oracle, ref):
    occ = np.zeros((9, 9), np.uint8)
    occ[4, 3] = occ[3, 4] = occ[4, 5] = occ[5, 4] = 1                 # a plus without its centre
    d2 = oracle.edt(occ)
    one = np.zeros((1, 1, 1, 2), np.int32)
    two = np.zeros((1, 3, 1, 2), np.int32)
    two[0, 0, 0], two[0, 1, 0], two[0, 2, 0] = (1, 1), (0, 1), (0, 1)
    for top in range(3):
        assert _agree(ref, d2, None, one, [(4, 4)], 1, 1, 64, 1, top)[0][0].tolist() == [0, 0, -1, 0, 1, 4]
        assert _agree(ref, d2, None, one, [(4, 4)], 1, 0, 64, 1, top)[0][0].tolist() == [0, -1, 0, 0, 1, 2]
        assert _agree(ref, d2, None, one, [(4, 3)], 1, 1, 64, 1, top)[0][0].tolist() == [0, 0, 0, 0, 1, 3]
        assert _agree(ref, d2, None, two, [(4, 4)], 1, 1, 64, 1, top)[0][0].tolist() == [1, 0, 0, 0, 1, 2 + 3 + 3]
        # far ties: the plus seen from 30 cells away in a window that holds all four
        assert _agree(ref, d2, None, one, [(34, 4)], 40, 9, 64, 1, top)[0][0].tolist() == [0, -29, 0, 0, 1, 4]


def test_overflow_and_too_many_top_nodes(ref):
    d2, known, pts, centre, n = mc.overflow_case()
    best, stats = _agree(ref, d2, known, pts, centre, 20, 20, 64, 1, 2, max_nodes=1024)
    assert best[0].tolist() == [mw.OVERFLOW, 0, 0, 0, 0, 0] and stats[0].tolist() == [0, 121, 9, 0, 0, 0, 2 * 16 + 16, 8]   # one dive of two rounds, one of one
    best, stats = _agree(ref, d2, known, pts, centre, 20, 20, 64, 1, 2, max_nodes=2048)
    assert best[0].tolist() == [0, 0, 0, 8, 8, n] and stats[0, 0] == n == 1681
    assert np.array_equal(best, mt.match(d2, known, pts, centre, 20, 20, 64, 1)[0])
    for kw in (dict(top=0, max_nodes=1024), dict(top=1, max_nodes=64), dict(top=6), dict(max_nodes=63), dict(max_nodes=(1 << 22) + 1),
               dict(wx=2049), dict(wy=-1)):
        a = dict(dict(wx=20, wy=20, top=2, max_nodes=1024), **kw)
        for f in (mw.match_wide, ref.match):
            with pytest.raises(mw.Invalid):
                f(d2, known, pts, centre, a["wx"], a["wy"], 64, 1, a["top"], a["max_nodes"])
    with pytest.raises(mw.Invalid):                                    # S max_nodes <= 2^26
        mw.match_wide(d2, known, np.repeat(pts, 17, 0), np.repeat(centre, 17, 0), 2, 2, 64, 1, 1, 1 << 22)


# ---- recovery, and the condition that pruning happens ----
@pytest.fixture(scope="module")
def recovered(oracle):
    out = {}
    for name, (occ, wx, wy, top) in mc.recovery_maps().items():
        pts, centre, want = mc.recovery_cases(occ, wx, wy)
        best, stats = mw.match_wide(oracle.edt(occ), None, pts, centre, wx, wy, 64, 1, top, 1 << 16)
        out[name] = (best, stats, want, 4 * (2 * wx + 1) * (2 * wy + 1))
    return out


@pytest.mark.parametrize("name", ["blocks", "salt0.03", "rooms"])
def test_recovery_where_unique(recovered, name):
    best, stats, want, _ = recovered[name]
    assert (best[:, 0] >= 0).all() and (best[:, 3] == 0).all()         # the true pose lies in the window and scores 0
    unique = best[:, 5] == 1
    assert np.array_equal(best[unique, :3], want[unique]) and unique.sum() >= 8
    assert (stats[:, 7] >= 0).all()


@pytest.mark.parametrize("name", ["blocks", "salt0.03", "rooms"])
def test_pruning_happens(recovered, name):
    """A condition, not a measurement: on every recovery case the twin bounds or scores at most a quarter of the candidates
    of the dense volume."""
    _, stats, _, dense = recovered[name]
    work = mw.work(stats)
    print(name, "work / dense: max %.4f, median %.4f" % (work.max() / dense, np.median(work) / dense))
    assert (4 * work <= dense).all(), (work / dense).tolist()


# ---- the kidnapped robot ----
def test_kidnapped_robot(oracle):
    k = mc.kidnapped(oracle.edt)
    cfg = mt.WALK
    wide = mw.match_wide(k["d2"], k["known"], k["pts"], k["centre"], 24, 24, cfg["d2_cap"], 1, 2, 1 << 14)[0][0]
    assert wide[5] == 1 and (wide[1], wide[2]) == (-mc.KIDNAP[0], -mc.KIDNAP[1])   # back where it is, and no other pose ties
    assert np.array_equal(wide, mt.match(k["d2"], k["known"], k["pts"], k["centre"], 24, 24, cfg["d2_cap"], 1)[0][0])
    near = mt.match(k["d2"], k["known"], k["pts"], k["centre"], cfg["window"], cfg["window"], cfg["d2_cap"], 1)[0][0]
    assert (k["centre"][0, 0] + near[1], k["centre"][0, 1] + near[2]) != k["true"] and near[3] > wide[3]


# ---- a program of its own under the sanitizers ----
SAN = ["-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_check_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "match_wide_ref_check")
    subprocess.check_call(["cc", "-std=c11"] + SAN + ["-o", exe, CHECK, mw.SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("match_wide_ref OK") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
