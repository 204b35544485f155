"""Scan matching on the CPU: the NumPy twin (tests/match_twin.py) against the C statement (tests/cpp/match_ref.c) in best and
the volume; every consequence the header states; the tie order; the int32 bound; ignored and absent kinds; recovery of known
poses where the answer is unique, and ties where it is not; the walk of DESIGN.md section 25 with and without the matcher's
correction; the host helpers; the C statement under AddressSanitizer and UBSan as a program of its own.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import frontier_twin as ft
import match_twin as mt
import scan_twin as st
import views_twin as vt

import sea_current_amd as sc

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = os.path.join(HERE, "cpp", "match_ref_check.c")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mt.Ref(tmp_path_factory.mktemp("match_ref"))


def _line():
    line = np.zeros((1, 200), np.uint8)
    line[0, [80, 150]] = 1
    return line


def _maps():
    return {"salt0.05": vt.salt(130, 70, 0.05, 3), "blocks": vt.blocks(), "door": vt.door_map(), "rooms": vt.rooms_map(), "row": _line(),
            "column": np.ascontiguousarray(_line().T)}


NAMES = ["salt0.05", "blocks", "door", "rooms", "row", "column"]


def _free_near(occ, x, y):
    H, W = occ.shape
    free = np.flatnonzero(occ.ravel() == 0)
    c = int(free[np.argmin((free % W - x) ** 2 + (free // W - y) ** 2)])
    return c % W, c // W


def scan_points(occ, x, y, r):
    """The hits of square_fan(r) from the free cell (x, y) as offsets: int32 [8 r, 2]."""
    rays = st.square_fan(x, y, r)
    return mt.points_from_hits(rays, st.cast(occ, rays), occ.shape[1])


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ---- twin == C statement ----
@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_c_statement(oracle, ref, name):
    occ = _maps()[name]
    H, W = occ.shape
    d2 = oracle.edt(occ)
    rng = np.random.default_rng(4)
    known = (rng.random((H, W)) < 0.7).astype(np.uint8)
    # three scans of two rotations: a fan from the middle with the prior a little off, one from a corner with a window that
    # sticks out of the grid, and one whose prior lies outside the grid
    x0, y0 = _free_near(occ, W // 2, H // 2)
    x1, y1 = _free_near(occ, 1, 0)
    p0, p1 = scan_points(occ, x0, y0, 25), scan_points(occ, x1, y1, 25)
    pts = np.stack([np.stack([p, mt.quarter_turns(p, 1)]) for p in (p0, p1, p0)])
    centre = [(x0 + 2, y0 - min(1, y0)), (x1 - 1, y1), (-3, H + 2)]
    for kn in (None, known):
        for wx, wy, cap, unk in ((4, 3, 64, 1), (0, 0, 1, 0), (7, 0, 32767, 32767), (1, 6, 9, 9)):
            got, want = ref.match(d2, kn, pts, centre, wx, wy, cap, unk), mt.match(d2, kn, pts, centre, wx, wy, cap, unk)
            assert _same(got, want), (name, wx, wy, cap, unk)
            assert np.array_equal(ref.match(d2, kn, pts, centre, wx, wy, cap, unk, want_score=False)[0], want[0])
    assert want[0][0, 4] > 0                                           # the fan from the middle meets obstacles on every map


# ---- consequences ----
def test_all_points_absent(ref):
    d2 = np.full((5, 7), 3, np.int32)
    pts = np.full((2, 3, 4, 2), mt.ABSENT, np.int32)
    pts[1, :, :, 0] = 0                                               # one coordinate absent is enough
    pts[1, 1, :, 1] = mt.MAX_REACH + 1
    pts[1, 2, :, 1] = 2**31 - 1
    for f in (mt.match, ref.match):
        best, score = f(d2, None, pts, [(3, 2), (0, 0)], 2, 1, 64, 1)
        assert best.tolist() == [[0, 0, 0, 0, 0, 3 * 5 * 3]] * 2 and not score.any()


@pytest.mark.parametrize("name", ["salt0.05", "blocks", "door", "rooms"])
def test_true_pose_scores_zero(oracle, name):
    occ = _maps()[name]
    H, W = occ.shape
    d2 = oracle.edt(occ)
    rng = np.random.default_rng(2)
    free = np.flatnonzero(occ.ravel() == 0)
    for c in free[rng.integers(0, len(free), 6)]:
        ax, ay = int(c % W), int(c // W)
        ex, ey = (int(v) for v in rng.integers(-3, 4, 2))
        pts = scan_points(occ, ax, ay, 18)[None, None]
        best, score = mt.match(d2, None, pts, [(ax + ex, ay + ey)], 3, 3, 64, 1)
        assert score[0, 0, 3 - ey, 3 - ex] == 0 and best[0, 3] == 0
        if best[0, 5] == 1:
            assert best[0, :3].tolist() == [0, -ex, -ey]


def test_rotations_are_compared_as_they_are(ref):
    """A rotation that has lost its points scores 0 and wins: the caller's business, as the header says."""
    occ = vt.door_map()
    d2 = np.minimum(np.arange(64 * 96, dtype=np.int32).reshape(64, 96), 50) + 1   # no cell costs 0
    p = scan_points(occ, 20, 31, 30)
    pts = np.stack([p, np.full_like(p, mt.ABSENT)])[None]
    for f in (mt.match, ref.match):
        best = f(d2, None, pts, [(20, 31)], 2, 2, 64, 1)[0]
        assert best[0].tolist() == [1, 0, 0, 0, 0, 25]


# ---- the tie order ----
def test_tie_order(oracle, ref):
    occ = np.zeros((9, 9), np.uint8)
    occ[4, 3] = occ[3, 4] = occ[4, 5] = occ[5, 4] = 1                 # a plus without its centre
    d2 = oracle.edt(occ)
    one = np.zeros((1, 1, 1, 2), np.int32)
    for f in (mt.match, ref.match):
        # four candidates at displacement 1 score 0: the smallest dy wins, then the smallest dx
        best, score = f(d2, None, one, [(4, 4)], 1, 1, 64, 1)
        assert best[0].tolist() == [0, 0, -1, 0, 1, 4]
        assert score[0, 0].tolist() == [[1, 0, 1], [0, 1, 0], [1, 0, 1]]
        # a row only: (dy, dx) = (0, -1) before (0, 1)
        assert f(d2, None, one, [(4, 4)], 1, 0, 64, 1)[0][0].tolist() == [0, -1, 0, 0, 1, 2]
        # the smaller displacement before the smaller score's position: (0, 0) scores 0 from (4, 3) ...
        assert f(d2, None, one, [(4, 3)], 1, 1, 64, 1)[0][0].tolist() == [0, 0, 0, 0, 1, 3]
        # two equal rotations: the earlier; a later rotation only wins with a smaller score or displacement
        two = np.zeros((1, 3, 1, 2), np.int32)
        two[0, 0, 0] = (1, 1)                                          # rotation 0 needs (-1, 0)-type moves: displacement 1
        two[0, 1, 0] = (0, 1)                                          # rotation 1 lands on (4, 5) from (4, 4): displacement 0
        two[0, 2, 0] = (0, 1)
        assert f(d2, None, two, [(4, 4)], 1, 1, 64, 1)[0][0].tolist() == [1, 0, 0, 0, 1, 2 + 3 + 3]


# ---- the int32 bound ----
def test_int32_bound(ref):
    N = mt.MAX_POINTS
    d2 = np.full((8, 8), mt.EDT_INF, np.int32)
    k = np.arange(N)
    pts = np.stack([k % 8 - 3, (k // 8) % 8 - 3], 1).astype(np.int32)[None, None]
    for f in (mt.match, ref.match):
        best, score = f(d2, None, pts, [(3, 3)], 0, 0, 32767, 0)
        assert best[0].tolist() == [0, 0, 0, 2147418112, N, 1] and score.ravel().tolist() == [2147418112]
    assert 32767 * 65536 == 2147418112 < 2**31


def test_empty_grid_known_and_unk(oracle, ref):
    occ = np.zeros((20, 30), np.uint8)
    d2 = oracle.edt(occ)
    assert (d2 == mt.EDT_INF).all()
    rng = np.random.default_rng(1)
    pts = rng.integers(-4, 5, (1, 2, 40, 2)).astype(np.int32)           # with the window they stay inside the grid
    ones = np.ones((20, 30), np.uint8)
    for f in (mt.match, ref.match):
        a = f(d2, None, pts, [(15, 10)], 5, 5, 64, 1)
        assert _same(a, f(d2, ones, pts, [(15, 10)], 5, 5, 64, 1))       # known NULL == all ones
        assert (a[1] == 40 * 64).all()                                 # every point inside: the cap each
        z = f(d2, 0 * ones, pts, [(15, 10)], 5, 5, 64, 0)              # nothing known, unk 0
        assert z[0][0].tolist() == [0, 0, 0, 0, 40, 2 * 121] and not z[1].any()
        c = f(d2, 0 * ones, pts, [(15, 10)], 5, 5, 64, 64)             # unk = d2_cap: unknown costs what open space does
        assert (c[1] == 40 * 64).all() and _same(c, f(d2, None, pts, [(15, 10)], 5, 5, 64, 64))


def test_ignored_and_absent_kinds(oracle, ref):
    occ = vt.blocks()
    H, W = occ.shape
    d2 = oracle.edt(occ)
    x, y = _free_near(occ, 40, 40)
    p = scan_points(occ, x, y, 20)
    n_hits = int(mt.present(p).sum())
    assert 0 < n_hits < len(p)                                         # no-return beams are in it
    lo, hi = -mt.MAX_REACH, mt.MAX_DIM + mt.MAX_REACH
    centres = [(x, y), (lo - 1, y), (x, hi + 1), (-2**31, 2**31 - 1), (lo, hi), (hi, lo), (x, y)]
    pts = np.repeat(p[None, None], len(centres), 0)
    odd = [(mt.MAX_REACH + 1, 0), (0, -mt.MAX_REACH - 1), (2**31 - 1, 0), (mt.ABSENT, mt.ABSENT), (mt.MAX_REACH, -mt.MAX_REACH)]
    pts[6, 0, :len(odd)] = odd                                         # four absent kinds and one point at the reach limit
    for f in (mt.match, ref.match):
        best, score = f(d2, None, pts, centres, 2, 2, 64, 3)
        assert best[1:4].tolist() == [[mt.IGNORED, 0, 0, 0, 0, 0]] * 3 and not score[1:4].any()
        assert best[0, 3] == 0 and best[0, 4] == n_hits
        assert best[4].tolist() == best[5].tolist() == [0, 0, 0, 3 * n_hits, n_hits, 25]      # far outside: unk a point
        assert best[6, 4] == n_hits - int(mt.present(p[:len(odd)]).sum()) + 1
    assert _same(mt.match(d2, None, pts, centres, 2, 2, 64, 3), ref.match(d2, None, pts, centres, 2, 2, 64, 3))


# ---- recovery ----
def recovery_cases(occ, seed, n=24, r=20, err=5):
    """n poses on free cells, each with a fan of half-side r seen by a sensor turned by q quarter turns, and a prior that is
    off by up to err cells per axis: [(pts [4,N,2], centre, (q, dx, dy) that recover the pose)].  Drawn on the CPU from the
    map alone."""
    H, W = occ.shape
    rng = np.random.default_rng(seed)
    free = np.flatnonzero(occ.ravel() == 0)
    out = []
    for c in free[rng.integers(0, len(free), n)]:
        ax, ay = int(c % W), int(c // W)
        q = int(rng.integers(0, 4))
        ex, ey = (int(v) for v in rng.integers(-err, err + 1, 2))
        seen = mt.quarter_turns(scan_points(occ, ax, ay, r), -q)       # candidate rotation q undoes the sensor's turn
        out.append((np.stack([mt.quarter_turns(seen, k) for k in range(4)]), (ax + ex, ay + ey), (q, -ex, -ey)))
    return out


@pytest.mark.parametrize("name,unique", [("salt0.05", 24), ("blocks", 15), ("rooms", 17)])
def test_recovery_where_unique(oracle, name, unique):
    occ = _maps()[name]
    d2 = oracle.edt(occ)
    cases = recovery_cases(occ, 0)
    best = mt.match(d2, None, np.stack([c[0] for c in cases]), [c[1] for c in cases], 5, 5, 64, 1)[0]
    assert (best[:, 3] == 0).all()                                     # the true pose lies in the window and scores 0
    for b, (_, _, want) in zip(best.tolist(), cases):
        if b[5] == 1:
            assert tuple(b[:3]) == want
    # the salt map pins every pose; walls and blocks leave ties, and they are reported
    assert int((best[:, 5] == 1).sum()) == unique
    assert (unique == 24) == (name == "salt0.05")


def test_a_scan_along_a_flat_wall_ties_along_it(oracle):
    occ = vt.door_map()
    d2 = oracle.edt(occ)
    pts = scan_points(occ, 40, 10, 8)[None, None]                      # the fan reaches the wall in column 48, far from the door
    best, score = mt.match(d2, None, pts, [(40, 10)], 2, 2, 64, 1)
    assert best[0].tolist()[:4] == [0, 0, 0, 0] and best[0, 5] == 5 and (score[0, 0, :, 2] == 0).all()


# ---- the walk ----
def test_walk_with_and_without_correction(oracle):
    occ = vt.salt(mt.WALK["W"], mt.WALK["H"], mt.WALK["p"], mt.WALK["seed"])
    start = ft.loop_start(occ)
    assert mt.walk(occ, start, oracle.edt, corrected=False) == dict(exact=2, unique=0, steps=33, sound=False)
    for unk in (1, 2):
        assert mt.walk(occ, start, oracle.edt, corrected=True, unk=unk) == dict(exact=33, unique=32, steps=33, sound=True)
    # the parameter matters
    assert mt.walk(occ, start, oracle.edt, corrected=True, unk=4)["exact"] == 31


# ---- the host helpers ----
def test_points_from_hits_and_rotate_points():
    occ = vt.blocks()
    W = occ.shape[1]
    rays = np.concatenate([st.square_fan(40, 40, 20), [[-1, 3, 5, 5]]]).astype(np.int32)
    rays[:, :2] = _free_near(occ, 40, 40)
    rays[-1, 0] = -1
    hit = st.cast(occ, rays)
    assert (hit >= 0).any() and (hit == st.NO_RETURN).any() and hit[-1] == st.IGNORED
    p = sc.points_from_hits(rays, hit, W)
    assert p.dtype == np.int32 and np.array_equal(p, mt.points_from_hits(rays, hit, W))
    ok = hit >= 0
    assert (p[~ok] == sc.SCAN_MATCH_ABSENT).all()
    assert np.array_equal((rays[ok, 1] + p[ok, 1]) * W + rays[ok, 0] + p[ok, 0], hit[ok])
    with pytest.raises(sc.SeaCurrentError):
        sc.points_from_hits(rays, hit[:-1], W)
    # quarter turns: the integer rotation (x, y) -> (-y, x), at the reach limit too
    rng = np.random.default_rng(0)
    big = rng.integers(-mt.MAX_REACH, mt.MAX_REACH + 1, (300, 2)).astype(np.int32)
    big[:4] = [(mt.MAX_REACH, -mt.MAX_REACH), (mt.ABSENT, mt.ABSENT), (0, 0), (1, mt.ABSENT)]
    turns = list(range(-8, 9))
    rot = sc.rotate_points(big, [k * np.pi / 2 for k in turns])
    assert rot.shape == (len(turns), 300, 2) and rot.dtype == np.int32
    for i, k in enumerate(turns):
        assert np.array_equal(rot[i], mt.quarter_turns(big, k)), k
    assert mt.quarter_turns([(3, 1)], 1).tolist() == [[-1, 3]]
    assert (rot[:, 1] == sc.SCAN_MATCH_ABSENT).all() and (rot[:, 3] == sc.SCAN_MATCH_ABSENT).all()
    # a batch of scans keeps its leading axes: [S, N, 2] -> [S, R, N, 2]
    assert sc.rotate_points(np.stack([p, p]), [0.0, 0.1, 0.2]).shape == (2, 3, len(p), 2)
    # any angle keeps a point's length to within the rounding of a cell
    a = sc.rotate_points(big[4:], [0.3])[0].astype(np.float64)
    assert np.abs(np.hypot(a[:, 0], a[:, 1]) - np.hypot(big[4:, 0], big[4:, 1])).max() <= np.sqrt(0.5) + 1e-9


# ---- a program of its own under the sanitizers ----
SAN = ["-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_check_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "match_ref_check")
    subprocess.check_call(["cc", "-std=c11"] + SAN + ["-o", exe, CHECK, mt.SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("match_ref OK") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
