"""The CPU statements of car-like pose planning against each other and against the definition: the NumPy twin
(tests/car_twin.py) == the C statement (tests/cpp/car_ref.c) in every output on salt 65 x 63 at p = 0.05, blocks 130 x 70,
1 x 200, 200 x 1, the two-room map with a door 3 cells wide and a dead-end corridor, for arc_n 1, 2 and 4; anchors (a) - (e) of
DESIGN.md section 32; every read-out a chain of legal edges that sums to its cost, 8-connected; truncation; every bad-root and
bad-target kind; the argument and overflow rules at their boundaries; the C statement under AddressSanitizer and UBSan as a
program of its own.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import car_twin as ct
import pose_twin as pt
from field_twin import Twin as FieldTwin
from pose_twin import HX, HY, INF, Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = os.path.join(HERE, "cpp", "car_ref_check.c")
FOOT = (2, 1, 1, 0)
# (hmask given, toward, arc_n, arc_cost, rev_cost, rhead)
CONFIGS = [(False, False, 1, 0, -1, 0), (True, True, 2, 40, 7, 3), (False, True, 4, 1, 0, -1), (True, False, 1, 1, 0, 5)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ct.Ref(tmp_path_factory.mktemp("car_ref"))


@pytest.fixture(scope="module")
def pose_ref(tmp_path_factory):
    return pt.Ref(tmp_path_factory.mktemp("pose_ref"))


@pytest.fixture(scope="module")
def fields(tmp_path_factory):
    return FieldTwin(tmp_path_factory.mktemp("field_ref"))


def _line(n):
    occ = np.zeros(n, np.uint8)
    occ[3 * n // 4] = 1
    return occ


def _maps():
    return {
        "salt65x63": pt.d2_of(pt.salt(65, 63, 0.05, 2)),
        "blocks130x70": pt.d2_of(pt.blocks()),
        "row1x200": pt.d2_of(_line(200)[None, :]),
        "col200x1": pt.d2_of(_line(200)[:, None]),
        "door": pt.d2_of(pt.door_map()),
        "dead_end": pt.d2_of(ct.dead_end()),
    }


NAMES = ["salt65x63", "blocks130x70", "row1x200", "col200x1", "door", "dead_end"]


def _fitting_root(d2, hm, seed):
    """A free cell where the body fits at the most headings, and those headings."""
    cand = pt.free_cells(d2, 64, seed)
    bits = (hm.ravel()[cand][:, None] >> np.arange(8)) & 1
    i = int(np.argmax(bits.sum(1)))
    return int(cand[i]), np.flatnonzero(bits[i])


@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_c_statement(ref, name):
    d2 = _maps()[name]
    H, W = d2.shape
    hm = pt.footprint_mask(d2, *FOOT)
    masks = {}
    for n in (1, 2, 4):
        for given in (False, True):
            masks[n, given] = ct.arc_mask(d2, n, 0, hm if given else None)
            assert np.array_equal(masks[n, given], ref.arc_mask(d2, n, 0, hm if given else None)), (n, given)
            assert not masks[n, given][d2 < 1].any()
    root, fits = _fitting_root(d2, hm, 11)
    rng = np.random.default_rng(7)
    targets = rng.integers(0, W * H, 24).astype(np.int32)
    thead = (rng.integers(0, 9, 24) - 1).astype(np.int32)
    statuses = set()
    for given, toward, n, ac, rev, rhead in CONFIGS:
        hmask = hm if given else None
        if given and rhead >= 0 and rhead not in fits:
            rhead = int(fits[rhead % len(fits)])
        a, sa = ct.car_field(d2, root, rhead, n, ac, rev, toward, 0, hmask)
        b, sb = ref.car_field(d2, root, rhead, n, ac, rev, toward, 0, hmask)
        assert sa == sb == Q_OK and np.array_equal(a, b), (given, toward, n, ac, rev, rhead)
        am = masks[n, given]
        for to_root, Lmax in ((False, 400), (True, 400), (False, 12), (True, 12)):
            pa = ct.car_paths(d2, am, a, root, rhead, targets, thead, n, ac, rev, toward, 0, hmask, Lmax, to_root)
            pb = ref.car_paths(d2, am, a, root, rhead, targets, thead, n, ac, rev, toward, 0, hmask, Lmax, to_root)
            assert ct.same_readout(pa, pb), (given, toward, n, ac, rev, rhead, to_root, Lmax)
            statuses |= set(pa["status"].tolist())
    assert Q_OK in statuses and Q_TRUNCATED in statuses


def test_anchor_a_straight_ahead_of_the_root(ref):
    d2 = np.ones((40, 40), np.int32)
    for field, ks in ((ct.car_field, (0, 3)), (ref.car_field, range(8))):
        for k in ks:
            for n, rev in ((1, -1), (2, 3), (4, 0)):
                gp, st = field(d2, 20 * 40 + 20, k, n, 5, rev)
                assert st == Q_OK
                for i in range(0, 19):
                    assert gp[k][20 + i * HY[k], 20 + i * HX[k]] == i * (14 if k & 1 else 10), (k, n, i)


@pytest.mark.parametrize("name", ["salt65x63", "door", "dead_end"])
def test_anchors_b_and_c_against_the_pose_and_the_plain_field(ref, pose_ref, fields, name):
    """(b) a car path is a pose path of equal cost (turn_cost = arc_cost, the same rev_cost); (c) and a cell path."""
    d2 = _maps()[name]
    hm = pt.footprint_mask(d2, *FOOT)
    root, fits = _fitting_root(d2, hm, 3)
    g, st = fields.field(d2, root)
    assert st == Q_OK
    finite = 0
    for given, toward, n, ac, rev, rhead in CONFIGS:
        rh = rhead if rhead < 0 or rhead in fits or not given else int(fits[0])
        hmask = hm if given else None
        gp, st = ref.car_field(d2, root, rh, n, ac, rev, toward, 0, hmask)
        pose, st2 = pose_ref.pose_field(d2, root, rh, ac, rev, toward, 0, hmask)
        assert st == st2 == Q_OK and (gp >= pose).all() and (gp.min(axis=0) >= g).all()
        finite += int((gp < INF).sum())
    assert finite > 1000


def _brute_arc(d2, hm, x, y, k, s, n):
    """A(c, k, s) by walking its 2n steps, written out without the twin."""
    H, W = d2.shape
    T = lambda a, b: 0 <= a < W and 0 <= b < H and d2[b, a] >= 1
    V = lambda a, b, h: T(a, b) and (hm is None or (hm[b, a] >> h) & 1)
    kn = (k + s) % 8
    if not V(x, y, k):
        return False
    for leg, h in ((0, k), (1, kn)):
        if leg == 1 and not V(x, y, kn):
            return False
        for _ in range(n):
            nx, ny = x + HX[h], y + HY[h]
            if not (T(x, y) and T(nx, ny) and (HX[h] == 0 or HY[h] == 0 or (T(nx, y) and T(x, ny))) and V(nx, ny, h)):
                return False
            x, y = nx, ny
    return True


@pytest.mark.parametrize("n", [1, 2, 4])
def test_anchor_d_mask_bits_by_brute_force(ref, n):
    d2 = pt.d2_of(pt.salt(33, 31, 0.08, 5))
    hm = pt.footprint_mask(d2, *FOOT)
    for hmask in (None, hm):
        am = ref.arc_mask(d2, n, 0, hmask)
        H, W = d2.shape
        for y in range(H):
            for x in range(W):
                for k in range(8):
                    assert bool(am[y, x] >> (2 * k) & 1) == _brute_arc(d2, hmask, x, y, k, 1, n), (x, y, k)
                    assert bool(am[y, x] >> (2 * k + 1) & 1) == _brute_arc(d2, hmask, x, y, k, -1, n), (x, y, k)


def test_anchor_e_open_grid_values(ref):
    d2 = np.ones((64, 64), np.int32)
    root = 32 * 64 + 32
    for field in (ct.car_field, ref.car_field):
        gp, st = field(d2, root, 0, 1, 0, -1)
        assert st == Q_OK and (gp[0][32, 37], gp[4][32, 32], gp[0][33, 32], int((gp == INF).sum())) == (50, 220, 202, 1340)
        gp, st = field(d2, root, 0, 2, 0, -1)
        assert (gp[4][32, 32], gp[0][33, 32], int((gp == INF).sum())) == (440, 394, 2800)
        gp, st = field(d2, root, 0, 1, 0, 10)
        assert (gp[4][32, 32], gp[0][32, 31], gp[0][33, 32]) == (156, 20, 102)
        gp, st = field(d2, root, 0, 2, 0, 10)
        assert (gp[4][32, 32], gp[0][33, 32]) == (312, 170)


@pytest.mark.parametrize("w,n,want0,want4", [(1, 1, INF, 560), (3, 1, 396, 512), (3, 2, INF, 560), (5, 2, 512, 560)])
def test_anchor_e_corridor_values(ref, w, n, want0, want4):
    """A corridor w cells wide, the car facing its closed end: backing out, and a three-point turn where it fits."""
    d2 = pt.d2_of(ct.corridor(w))
    H, W = d2.shape
    y = 1 + w // 2
    root = y * W + 2
    for field in (ct.car_field, ref.car_field):
        gp, st = field(d2, root, 4, n, 0, 10)
        assert st == Q_OK and (gp[0][y, 30], gp[4][y, 30]) == (want0, want4)
        # without reversing the car only rolls on into the end of the corridor: the root and the one cell ahead of it
        gp, st = field(d2, root, 4, n, 0, -1)
        assert st == Q_OK and gp[4][y, 2] == 0 and gp[4][y, 1] == 10 and int((gp < INF).sum()) == 2


def _parse_totals(gr, drive, i, memo):
    """The totals of every way to read drive[i:] as a chain of legal edges of the definition."""
    if i == len(drive) - 1:
        return {0}
    if i in memo:
        return memo[i]
    (x, y), k = drive[i]
    n = gr.n
    totals = set()
    for kind, fx, fy, fk, c in gr.out_edges(x, y, k):
        if kind <= 2:
            want = [((fx, fy), fk)]
        elif kind <= 4:          # driven forwards: the corner is reached by the first leg
            cells, kn = ct.arc_cells(x, y, k, 1 if kind == 3 else -1, n)
            want = list(zip(cells[1:], [k] * n + [kn] * n))
        else:                    # driven backwards from the arc's end: the corner is reached by the second leg
            cells, kn = ct.arc_cells(fx, fy, fk, 1 if kind == 5 else -1, n)
            assert kn == k and cells[-1] == (x, y)
            want = list(zip(cells[-2::-1], [k] * n + [fk] * n))
        if drive[i + 1:i + 1 + len(want)] == want:
            totals |= {c + t for t in _parse_totals(gr, drive, i + len(want), memo)}
    memo[i] = totals
    return totals


@pytest.mark.parametrize("toward", [False, True])
@pytest.mark.parametrize("n,ac,rev", [(1, 0, 6), (2, 3, 0), (4, 40, 2), (1, 1, -1)])
def test_readouts_are_chains_of_legal_edges(ref, toward, n, ac, rev):
    d2 = _maps()["blocks130x70"]
    H, W = d2.shape
    hm = pt.footprint_mask(d2, *FOOT)
    root, fits = _fitting_root(d2, hm, 21)
    rh = int(fits[0])
    gr = ct.Graph(d2, 0, hm, n, ac, rev)
    am = ref.arc_mask(d2, n, 0, hm)
    gp, st = ref.car_field(d2, root, rh, n, ac, rev, toward, 0, hm)
    reach = np.flatnonzero((gp < INF).any(axis=0).ravel())
    targets = reach[np.random.default_rng(22).permutation(len(reach))[:40]].astype(np.int32)
    # a heading the field reaches at every target; every ninth: the cheapest, and one the field may not reach
    thead = np.array([-1 if q % 9 == 0 else q % 8 if q % 9 == 1 else int(np.flatnonzero(gp[:, t // W, t % W] < INF)[q % 3 % (gp[:, t // W, t % W] < INF).sum()])
                      for q, t in enumerate(targets)], np.int32)
    seen_ok = arcs = 0
    for to_root in (False, True):
        full = ref.car_paths(d2, am, gp, root, rh, targets, thead, n, ac, rev, toward, 0, hm, 900, to_root)
        short = ref.car_paths(d2, am, gp, root, rh, targets, thead, n, ac, rev, toward, 0, hm, 16, to_root)
        for q in range(len(targets)):
            if full["status"][q] != Q_OK:
                fits_there = gr.valid(int(targets[q]) % W, int(targets[q]) // W, int(thead[q]))
                assert thead[q] >= 0 and gp[thead[q]].ravel()[targets[q]] == INF
                assert full["status"][q] == (Q_NO_PATH if fits_there else Q_BAD_ENDPOINT)
                continue
            seen_ok += 1
            L = full["len"][q]
            entries = [((int(c) % W, int(c) // W), int(h)) for c, h in zip(full["path"][q, :L], full["head"][q, :L])]
            first, last = (entries[0], entries[-1]) if not to_root else (entries[-1], entries[0])
            assert first == ((root % W, root // W), rh) and last[0] == (targets[q] % W, targets[q] // W)
            if thead[q] >= 0:
                assert last[1] == thead[q]
            else:                                         # the cheapest heading, the smallest on a tie
                col = gp[:, targets[q] // W, targets[q] % W]
                assert last[1] == int(np.argmin(col)) and col[last[1]] == full["cost"][q]
            drive = entries if (toward == to_root) else entries[::-1]         # the order the edges point in
            assert full["cost"][q] in _parse_totals(gr, drive, 0, {}), q
            arcs += any(a[1] != b[1] for a, b in zip(entries, entries[1:]))
            cells = np.array([c for c, _ in entries])
            assert L == 1 or (np.abs(np.diff(cells, axis=0)).max() == 1 and (np.abs(np.diff(cells, axis=0)).sum(axis=1) > 0).all())   # 8-connected, no cell twice in a row
            want = Q_OK if L <= 16 else Q_TRUNCATED
            assert (short["status"][q], short["len"][q], short["cost"][q]) == (want, L, full["cost"][q])
    # where nothing reverses, few poses reach this root at all
    assert (seen_ok >= 30 and arcs >= 10) if len(reach) >= 40 else seen_ok >= 2


def test_dead_end_needs_reversing(ref):
    """Into a corridor as wide as the body there is no turning round: the way out is backwards, or there is none."""
    d2 = pt.d2_of(ct.dead_end(width=1))
    H, W = d2.shape
    y = H // 2
    inside, outside = y * W + 25, y * W + 3
    for n in (1, 2):
        am = ref.arc_mask(d2, n)
        gp, st = ref.car_field(d2, outside, 0, n, 0, -1, True)             # toward the pose in the room, facing the corridor
        assert st == Q_OK and (gp[[0, 1, 2, 3, 5, 6, 7], y, 25] == INF).all()      # heading 4 faces the way out
        gp, st = ref.car_field(d2, outside, 0, n, 0, 4, True)
        assert gp[0, y, 25] == 22 * (10 + 4) and (gp[[1, 2, 3, 5, 6, 7], y, 25] == INF).all()
        out = ref.car_paths(d2, am, gp, outside, 0, [inside], [0], n, 0, 4, True, 0, None, 64, True)
        assert out["status"][0] == Q_OK and out["len"][0] == 23 and (out["head"][0, :23] == 0).all()
        assert list(out["path"][0, :23]) == [y * W + x for x in range(25, 2, -1)]


def test_every_bad_root_and_target_kind(ref):
    d2 = _maps()["salt65x63"]
    H, W = d2.shape
    hm = pt.footprint_mask(d2, 3, 3, 3, 3)
    am = ref.arc_mask(d2, 1, 0, hm)
    blocked = int(np.flatnonzero(d2.ravel() < 1)[0])
    dead = int(np.flatnonzero((d2.ravel() >= 1) & (hm.ravel() == 0))[0])       # traversable, no heading fits
    free = int(np.flatnonzero(hm.ravel() == 0xFF)[0])
    for root, rhead, hmask in ((-1, 0, None), (W * H, 0, None), (blocked, 0, None), (blocked, -1, None), (dead, 3, hm), (dead, -1, hm),
                               (free, 8, hm), (free, -2, hm)):
        a = am if hmask is not None else ref.arc_mask(d2, 1)
        for toward in (False, True):
            for field in (ct.car_field, ref.car_field):
                gp, st = field(d2, root, rhead, 1, 2, 0, toward, 0, hmask)
                assert st == Q_BAD_ENDPOINT and (gp == INF).all(), (root, rhead)
        gp = np.full((8, H, W), INF, np.int32)
        assert ct.car_path(d2, a, gp, root, rhead, free, 0, 1, 2, 0, False, 0, hmask)[2:] == (0, -1, Q_BAD_ENDPOINT)
        out = ref.car_paths(d2, a, gp, root, rhead, [free], [0], 1, 2, 0, False, 0, hmask)
        assert (out["len"][0], out["cost"][0], out["status"][0]) == (0, -1, Q_BAD_ENDPOINT)
    gp, st = ct.car_field(d2, free, 0, 1, 2, 0, False, 0, hm)
    for target, th in ((-1, 0), (W * H, 0), (blocked, 0), (blocked, -1), (dead, 2), (free, 8), (free, -2)):
        assert ct.car_path(d2, am, gp, free, 0, target, th, 1, 2, 0, False, 0, hm)[2:] == (0, -1, Q_BAD_ENDPOINT), (target, th)
    assert ct.car_path(d2, am, gp, free, 0, dead, -1, 1, 2, 0, False, 0, hm)[2:] == (0, -1, Q_NO_PATH)     # traversable, nothing fits
    out = ref.car_paths(d2, am, gp, free, 0, [-1, W * H, blocked, blocked, dead, free, free, dead], [0, 0, 0, -1, 2, 8, -2, -1], 1, 2, 0, False, 0, hm)
    assert list(out["status"]) == [Q_BAD_ENDPOINT] * 7 + [Q_NO_PATH]


def test_argument_and_overflow_rules(ref):
    for W, H, n, ac, rev, want in ((9, 9, 1, 0, -1, True), (9, 9, 4, 255, 255, True), (9, 9, 0, 0, 0, False), (9, 9, 5, 0, 0, False),
                                   (9, 9, 1, -1, 0, False), (9, 9, 1, 256, 0, False), (9, 9, 1, 0, -2, False), (9, 9, 1, 0, 256, False),
                                   (1024, 1024, 1, 232, 0, True), (1024, 1024, 1, 233, 0, False), (1024, 1024, 1, 232, -1, True),
                                   (1024, 1024, 1, 30, 101, True), (1024, 1024, 1, 31, 101, False), (1024, 1024, 4, 0, 20, True),
                                   (1024, 1024, 4, 1, 20, False), (3344, 3344, 1, 0, -1, True), (3345, 3345, 1, 0, -1, False),
                                   (8192, 8192, 1, 0, -1, False)):
        assert ct.args_ok(W, H, n, ac, rev) == ref.args_ok(W, H, n, ac, rev) == want, (W, H, n, ac, rev)
    d2 = np.ones((9, 9), np.int32)
    gp = np.zeros((8, 9, 9), np.int32)
    assert ref.lib.cx_car_field(d2.ctypes.data, None, 9, 9, 0, 5, 0, 0, 0, 0, 0, gp.ctypes.data) == -1
    assert ref.lib.cx_arc_mask(d2.ctypes.data, None, 9, 9, 0, 0, gp.ctypes.data) == 1


def test_check_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "car_ref_check")
    subprocess.check_call(["cc", "-g", "-O1", "-std=c11", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           CHECK, ct.SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("car_ref OK") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
