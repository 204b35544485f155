"""The CPU statements of planning in poses against each other and against the definition: the NumPy twin (tests/pose_twin.py)
== the C statement (tests/cpp/pose_ref.c) in every output on salt 65 x 63 at p = 0.05, blocks 130 x 70, 1 x 200, 200 x 1 and
the two-room map with a door 3 cells wide; anchors (a) - (e) of include/sea_current_hip.h; the masks of four bodies against a
single-obstacle reading of the definition; the door that a long body passes lengthwise only; a turn price that buys a longer
route; rev_cost -1 / 0 / 7; a root where only some headings fit; every bad-root kind; every read-out a chain of legal edges
that sums to its cost; cells_only 8-connected; truncation; the thead = -1 tie; the argument and overflow rules; the C
statement under AddressSanitizer and UBSan as a program of its own.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import pose_twin as pt
from field_twin import Twin as FieldTwin
from pose_twin import HX, HY, INF, Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = os.path.join(HERE, "cpp", "pose_ref_check.c")
FOOT = (2, 1, 1, 0)
EXTENTS = [(0, 0, 0, 0), (3, 3, 1, 1), (5, 0, 2, 1)]
# (hmask given, toward, turn_cost, rev_cost, rhead)
CONFIGS = [(False, False, 5, -1, 0), (True, False, 1, 0, 3), (True, True, 40, 7, 6), (False, True, 1, -1, -1), (True, True, 5, 0, -1)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
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
    }


NAMES = ["salt65x63", "blocks130x70", "row1x200", "col200x1", "door"]


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
    for ext in EXTENTS:
        assert np.array_equal(pt.footprint_mask(d2, *ext), ref.footprint_mask(d2, *ext)), ext
    hm = pt.footprint_mask(d2, *FOOT)
    root, fits = _fitting_root(d2, hm, 11)
    rng = np.random.default_rng(7)
    targets = rng.integers(0, W * H, 24).astype(np.int32)
    thead = (rng.integers(0, 9, 24) - 1).astype(np.int32)
    statuses = set()
    for given, toward, turn, rev, rhead in CONFIGS:
        hmask = hm if given else None
        if given and rhead >= 0 and rhead not in fits:
            rhead = int(fits[rhead % len(fits)])
        a, sa = pt.pose_field(d2, root, rhead, turn, rev, toward, 0, hmask)
        b, sb = ref.pose_field(d2, root, rhead, turn, rev, toward, 0, hmask)
        assert sa == sb == Q_OK and np.array_equal(a, b), (given, toward, turn, rev, rhead)
        for to_root, cells_only, Lmax in ((False, False, 400), (True, True, 400), (False, True, 12), (True, False, 12)):
            pa = pt.pose_paths(d2, a, root, rhead, targets, thead, turn, rev, toward, 0, hmask, Lmax, to_root, cells_only)
            pb = ref.pose_paths(d2, a, root, rhead, targets, thead, turn, rev, toward, 0, hmask, Lmax, to_root, cells_only)
            assert pt.same_readout(pa, pb), (given, toward, turn, rev, rhead, to_root, cells_only, Lmax)
            statuses |= set(pa["status"].tolist())
    assert Q_OK in statuses and Q_TRUNCATED in statuses


def test_anchor_a_zero_extents(ref):
    for d2 in _maps().values():
        want = np.where(d2 >= 1, 0xFF, 0).astype(np.uint8)
        assert np.array_equal(pt.footprint_mask(d2, 0, 0, 0, 0), want) and np.array_equal(ref.footprint_mask(d2, 0, 0, 0, 0), want)


@pytest.mark.parametrize("name", ["salt65x63", "door"])
def test_anchors_b_and_d_against_the_plain_field(ref, fields, name):
    d2 = _maps()[name]
    hm = pt.footprint_mask(d2, *FOOT)
    root, fits = _fitting_root(d2, hm, 3)
    g, st = fields.field(d2, root)
    assert st == Q_OK
    for rev in (-1, 0, 7):                                   # (b): turning is free, every heading seeded: eight copies of g
        gp, st = pt.pose_field(d2, root, -1, 0, rev)
        assert st == Q_OK and all(np.array_equal(gp[k], g) for k in range(8)), rev
        assert np.array_equal(ref.pose_field(d2, root, -1, 0, rev)[0], gp)
    for given, toward, turn, rev, rhead in CONFIGS:          # (d): a pose path is a cell path
        rh = rhead if rhead < 0 or rhead in fits or not given else int(fits[0])
        gp, st = ref.pose_field(d2, root, rh, turn, rev, toward, 0, hm if given else None)
        assert st == Q_OK and (gp.min(axis=0) >= g).all()


@pytest.mark.parametrize("name", NAMES)
def test_anchor_c_toward_is_the_renamed_field(ref, name):
    """Dijkstra on the transposed graph == the toward = 0 field of rhead + 4 with layers (and mask bits) renamed k -> k + 4."""
    d2 = _maps()[name]
    hm = pt.footprint_mask(d2, *FOOT)
    root, fits = _fitting_root(d2, hm, 5)
    for hmask in (None, hm):
        for rev in (-1, 0, 7):
            for rh in (-1, int(fits[0])):
                a, sa = pt.pose_field(d2, root, rh, 3, rev, True, 0, hmask)
                b, sb = pt.pose_field_by_identity(d2, root, rh, 3, rev, 0, hmask)
                assert sa == sb == Q_OK and np.array_equal(a, b), (hmask is None, rev, rh)
                assert np.array_equal(ref.pose_field(d2, root, rh, 3, rev, True, 0, hmask)[0], a)


def test_anchor_e_hand_values(ref):
    d2 = np.ones((9, 9), np.int32)
    root = 4 * 9 + 4
    for field in (pt.pose_field, ref.pose_field):
        gp, st = field(d2, root, 0, 5, -1)
        assert st == Q_OK
        assert gp[0][4, 6] == 20 and gp[2][6, 4] == 30 and gp[4][4, 4] == 20 and gp[1][6, 6] == 33 and gp[0][6, 6] == 38 and gp[0][4, 2] == 60
        assert field(d2, root, 0, 5, 3)[0][0][4, 2] == 26
        # rev_cost -1 / 0 / 7: two cells behind the root costs a half turn and back, two reverse moves, two dearer ones
        assert [int(field(d2, root, 0, 5, rev)[0][0][4, 2]) for rev in (-1, 0, 7)] == [60, 20, 34]


@pytest.mark.parametrize("ext", EXTENTS + [(32, 32, 32, 32), (0, 32, 0, 0), (1, 2, 3, 4)])
def test_mask_of_one_obstacle_is_the_covered_set(ref, ext):
    """On an otherwise free grid, bit k of cell c is clear exactly where the obstacle's offset from c is covered at heading k."""
    n = 2 * max(ext) * 2 + 3 if max(ext) <= 5 else 41
    d2 = np.ones((n, n), np.int32)
    o = n // 2
    d2[o, o] = 0
    want = np.zeros((n, n), np.uint8)
    for y in range(n):
        for x in range(n):
            for k in range(8):
                if not pt.covered(k, o - x, o - y, *ext):
                    want[y, x] |= 1 << k
    assert np.array_equal(pt.footprint_mask(d2, *ext), want) and np.array_equal(ref.footprint_mask(d2, *ext), want)
    if ext == (5, 0, 2, 1):        # the asymmetric body at heading 0: 5 ahead (+x), none behind, 2 to the left (+y), 1 to the right
        clear0 = {(x - o, y - o) for y in range(n) for x in range(n) if not want[y, x] & 1}
        assert clear0 == {(-dx, -dy) for dx in range(0, 6) for dy in range(-1, 3)}


def test_mask_all_blocked_or_off_grid(ref):
    small = pt.d2_of(np.pad(np.zeros((3, 3), np.uint8), 2, constant_values=1))
    for f in (pt.footprint_mask, ref.footprint_mask):
        assert not f(small, 32, 32, 32, 32).any()
        assert (f(np.ones((5, 9), np.int32), 32, 32, 32, 32) == 0xFF).all()        # offsets outside the grid are free


def test_door_is_passed_lengthwise_only(ref):
    d2 = pt.d2_of(pt.door_map())
    H, W = d2.shape
    start, goal = 3 * W + 5, 20 * W + 34                    # one in each room, away from the door's row
    hm = pt.footprint_mask(d2, 3, 3, 1, 1)                  # 7 long, 3 wide: fits the 3-cell door lengthwise
    assert np.array_equal(hm, ref.footprint_mask(d2, 3, 3, 1, 1))
    costs = []
    for rev in (-1, 4):
        gp, st = pt.pose_field(d2, goal, 2, 3, rev, True, 0, hm)
        assert st == Q_OK and np.array_equal(gp, ref.pose_field(d2, goal, 2, 3, rev, True, 0, hm)[0])
        cells, heads, n, cost, status = pt.pose_path(d2, gp, goal, 2, start, 6, 3, rev, True, 0, hm, 512, True)
        assert status == Q_OK and cells[0] == start and heads[0] == 6 and cells[-1] == goal and heads[-1] == 2
        in_door = [h for c, h in zip(cells, heads) if 19 <= c % W <= 21]
        assert in_door and all(h in (0, 4) for h in in_door)              # along the door's axis
        assert not any(hm[11, x] & 0b11101110 for x in (19, 20, 21))      # no other heading fits there
        costs.append(cost)
    assert costs == [376, 376]                              # twin == C; pinned
    wide = pt.footprint_mask(d2, 3, 3, 3, 3)                # 7 x 7: no heading fits the door
    gp, st = pt.pose_field(d2, goal, 2, 3, -1, True, 0, wide)
    assert st == Q_OK and np.array_equal(gp, ref.pose_field(d2, goal, 2, 3, -1, True, 0, wide)[0])
    for th in (6, -1):
        assert pt.pose_path(d2, gp, goal, 2, start, th, 3, -1, True, 0, wide, 512, True)[2:] == (0, -1, Q_NO_PATH)
    out = ref.pose_paths(d2, gp, goal, 2, [start, start], [6, -1], 3, -1, True, 0, wide, 512, True)
    assert list(out["status"]) == [Q_NO_PATH] * 2 and list(out["len"]) == [0, 0] and list(out["cost"]) == [-1, -1]


def _turns_and_moves(cells, heads):
    turns = sum(1 for i in range(1, len(cells)) if cells[i] == cells[i - 1])
    moves = sum((14 if heads[i] & 1 else 10) for i in range(1, len(cells)) if cells[i] != cells[i - 1])
    return turns, moves


def test_turn_cost_buys_a_longer_route(ref):
    d2 = pt.d2_of(pt.turn_map())
    H, W = d2.shape
    root, target = 1 * W + 1, 9 * W + 9
    got = {}
    for turn in (1, 40):
        gp, st = pt.pose_field(d2, root, 0, turn)
        assert st == Q_OK and np.array_equal(gp, ref.pose_field(d2, root, 0, turn)[0])
        cells, heads, n, cost, status = pt.pose_path(d2, gp, root, 0, target, -1, turn)
        assert status == Q_OK
        turns, moves = _turns_and_moves(cells, heads)
        assert cost == moves + turn * turns
        got[turn] = (turns, moves, cost)
    assert got[40][0] < got[1][0] and got[40][1] > got[1][1]      # fewer turns, a longer way
    assert got == {1: (26, 154, 180), 40: (4, 200, 360)}         # row 1, then down the staircase; the corridor round it


def test_rhead_minus_one_seeds_the_headings_that_fit(ref):
    d2 = _maps()["blocks130x70"]
    hm = pt.footprint_mask(d2, 4, 4, 1, 1)
    part = np.flatnonzero((d2.ravel() >= 1) & (hm.ravel() != 0) & (hm.ravel() != 0xFF))
    root = int(part[len(part) // 2])
    H, W = d2.shape
    fits = [k for k in range(8) if hm.ravel()[root] >> k & 1]
    assert 0 < len(fits) < 8
    for toward in (False, True):
        gp, st = pt.pose_field(d2, root, -1, 2, 5, toward, 0, hm)
        assert st == Q_OK and np.array_equal(gp, ref.pose_field(d2, root, -1, 2, 5, toward, 0, hm)[0])
        at_root = gp[:, root // W, root % W]
        assert all(at_root[k] == 0 for k in fits) and all(at_root[k] == INF for k in range(8) if k not in fits)
        k_bad = next(k for k in range(8) if k not in fits)
        assert pt.pose_field(d2, root, k_bad, 2, 5, toward, 0, hm)[1] == Q_BAD_ENDPOINT


def test_every_bad_root_kind(ref):
    d2 = _maps()["salt65x63"]
    H, W = d2.shape
    hm = pt.footprint_mask(d2, 3, 3, 3, 3)
    blocked = int(np.flatnonzero(d2.ravel() < 1)[0])
    dead = int(np.flatnonzero((d2.ravel() >= 1) & (hm.ravel() == 0))[0])       # traversable, no heading fits
    free = int(np.flatnonzero(hm.ravel() == 0xFF)[0])
    for root, rhead, hmask in ((-1, 0, None), (W * H, 0, None), (blocked, 0, None), (blocked, -1, None), (dead, 3, hm), (dead, -1, hm),
                               (free, 8, hm), (free, -2, hm)):
        for toward in (False, True):
            for field in (pt.pose_field, ref.pose_field):
                gp, st = field(d2, root, rhead, 2, 0, toward, 0, hmask)
                assert st == Q_BAD_ENDPOINT and (gp == INF).all(), (root, rhead)
        gp = np.full((8, H, W), INF, np.int32)
        assert pt.pose_path(d2, gp, root, rhead, free, 0, 2, 0, False, 0, hmask)[2:] == (0, -1, Q_BAD_ENDPOINT)
        out = ref.pose_paths(d2, gp, root, rhead, [free], [0], 2, 0, False, 0, hmask)
        assert (out["len"][0], out["cost"][0], out["status"][0]) == (0, -1, Q_BAD_ENDPOINT)
    gp, st = pt.pose_field(d2, free, 0, 2, 0, False, 0, hm)
    for target, th in ((-1, 0), (W * H, 0), (blocked, 0), (blocked, -1), (dead, 2), (free, 8), (free, -2)):
        assert pt.pose_path(d2, gp, free, 0, target, th, 2, 0, False, 0, hm)[2:] == (0, -1, Q_BAD_ENDPOINT), (target, th)
    assert pt.pose_path(d2, gp, free, 0, dead, -1, 2, 0, False, 0, hm)[2:] == (0, -1, Q_NO_PATH)     # traversable, nothing fits
    out = ref.pose_paths(d2, gp, free, 0, [-1, W * H, blocked, blocked, dead, free, free, dead], [0, 0, 0, -1, 2, 8, -2, -1], 2, 0, False, 0, hm)
    assert list(out["status"]) == [Q_BAD_ENDPOINT] * 7 + [Q_NO_PATH]


@pytest.mark.parametrize("toward", [False, True])
def test_readouts_are_chains_of_legal_edges(ref, toward):
    d2 = _maps()["blocks130x70"]
    H, W = d2.shape
    hm = pt.footprint_mask(d2, *FOOT)
    root, fits = _fitting_root(d2, hm, 21)
    turn, rev = 3, 6
    gr = pt.Graph(d2, 0, hm, turn, rev)
    gp, st = ref.pose_field(d2, root, int(fits[0]), turn, rev, toward, 0, hm)
    targets = pt.free_cells(d2, 40, 22)
    thead = (np.arange(40) % 9 - 1).astype(np.int32)
    seen_ok = 0
    for to_root in (False, True):
        full = ref.pose_paths(d2, gp, root, int(fits[0]), targets, thead, turn, rev, toward, 0, hm, 600, to_root, False)
        only = ref.pose_paths(d2, gp, root, int(fits[0]), targets, thead, turn, rev, toward, 0, hm, 600, to_root, True)
        short = ref.pose_paths(d2, gp, root, int(fits[0]), targets, thead, turn, rev, toward, 0, hm, 16, to_root, False)
        for q in range(40):
            if full["status"][q] != Q_OK:
                continue
            seen_ok += 1
            L = full["len"][q]
            states = [(int(c) % W, int(c) // W, int(h)) for c, h in zip(full["path"][q, :L], full["head"][q, :L])]
            # root .. target unless to_root; the edges of a toward field run target -> root
            first, last = (states[0], states[-1]) if not to_root else (states[-1], states[0])
            assert first[:2] == (root % W, root // W) and first[2] == fits[0] and last[:2] == (targets[q] % W, targets[q] // W)
            if thead[q] >= 0:
                assert last[2] == thead[q]
            else:                                         # the cheapest heading, the smallest on a tie
                col = gp[:, targets[q] // W, targets[q] % W]
                assert last[2] == int(np.argmin(col)) and col[last[2]] == full["cost"][q]
            drive = states if (toward == to_root) else states[::-1]         # the order the edges point in
            total = 0
            for a, b in zip(drive, drive[1:]):
                c = gr.legal_edge(a, b)
                assert c is not None, (q, a, b)
                total += c
            assert total == full["cost"][q] and len(set(states)) == L
            # cells_only: the same cells with repeats dropped, 8-connected, heads of the first state of each cell
            cells = [c for i, c in enumerate(full["path"][q, :L]) if i == 0 or c != full["path"][q, i - 1]]
            heads = [h for i, h in enumerate(full["head"][q, :L]) if i == 0 or full["path"][q, i] != full["path"][q, i - 1]]
            n = only["len"][q]
            assert only["status"][q] == Q_OK and list(only["path"][q, :n]) == cells and list(only["head"][q, :n]) == heads
            steps = np.abs(np.diff(np.array(cells) % W)).max(initial=0), np.abs(np.diff(np.array(cells) // W)).max(initial=0)
            assert max(steps) <= 1 and only["cost"][q] == full["cost"][q]
            # truncation: the needed count and the cost
            want = Q_OK if L <= 16 else Q_TRUNCATED
            assert (short["status"][q], short["len"][q], short["cost"][q]) == (want, L, full["cost"][q])
    assert seen_ok >= 40


def test_thead_minus_one_takes_the_smallest_heading_on_a_tie(ref):
    d2 = np.ones((9, 9), np.int32)
    root = 4 * 9 + 4
    gp, _ = pt.pose_field(d2, root, -1, 5, -1)              # every heading seeded: an eight-way tie at the root
    assert pt.pose_path(d2, gp, root, -1, root, -1, 5) == ([root], [0], 1, 0, Q_OK)
    out = ref.pose_paths(d2, gp, root, -1, [root, root + 2], [-1, -1], 5)
    assert out["head"][0, 0] == 0 and out["len"][0] == 1
    # two cells to the right of the root: heading 0 (20), then 1 and 7 tie at 25: -1 takes 0; among 1 and 7 alone the rule is smallest k
    assert out["cost"][1] == 20 and out["head"][1, out["len"][1] - 1] == 0
    # a tie that is not at heading 0: the body fits (6, 4) at headings 1 and 7 only, and by symmetry they cost the same
    hm = np.full((9, 9), 0xFF, np.uint8)
    hm[4, 6] = 0x82
    for toward in (False, True):
        gp, _ = pt.pose_field(d2, root, -1, 5, -1, toward, 0, hm)
        best = int(gp[:, 4, 6].min())
        assert gp[0, 4, 6] == INF and gp[1, 4, 6] == gp[7, 4, 6] == best and (best == 38 or toward)
        a = pt.pose_path(d2, gp, root, -1, root + 2, -1, 5, -1, toward, 0, hm)
        b = ref.pose_paths(d2, gp, root, -1, [root + 2], [-1], 5, -1, toward, 0, hm)
        assert a[3] == b["cost"][0] == best and a[4] == b["status"][0] == Q_OK
        assert a[1][-1] == b["head"][0, b["len"][0] - 1] == 1          # the smallest k of the caller's numbering, toward or not


def test_argument_and_overflow_rules(ref):
    for W, H, turn, rev, want in ((9, 9, 0, -1, True), (9, 9, 255, 255, True), (9, 9, 256, 0, False), (9, 9, -1, 0, False), (9, 9, 1, -2, False),
                                  (9, 9, 1, 256, False), (1024, 1024, 1, 242, True), (1024, 1024, 1, 243, False), (1024, 1024, 255, 0, True),
                                  (4096, 4096, 1, 2, True), (4096, 4096, 1, 3, False), (4096, 4096, 16, -1, True), (4096, 4096, 17, -1, False), (8192, 8192, 1, -1, False),
                                  (8192, 2340, 1, -1, True)):
        assert pt.args_ok(W, H, turn, rev) == ref.args_ok(W, H, turn, rev) == want, (W, H, turn, rev)
    assert pt.args_ok(9, 9, 0, -1, readout=True) is False and ref.args_ok(9, 9, 0, -1, readout=True) is False
    assert pt.args_ok(9, 9, 1, -1, readout=True) and ref.args_ok(9, 9, 1, -1, readout=True)
    d2 = np.ones((9, 9), np.int32)
    gp = np.zeros((8, 9, 9), np.int32)
    assert ref.lib.px_pose_field(d2.ctypes.data, None, 9, 9, 0, 256, 0, 0, 0, 0, gp.ctypes.data) == -1
    assert ref.lib.px_footprint_mask(d2.ctypes.data, 9, 9, 0, 33, 0, 0, 0, gp.ctypes.data) == 1
    assert ref.lib.px_footprint_mask(d2.ctypes.data, 9, 9, 0, 0, 0, 0, -1, gp.ctypes.data) == 1


def test_check_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pose_ref_check")
    subprocess.check_call(["cc", "-g", "-O1", "-std=c11", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           CHECK, pt.SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("pose_ref OK") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
