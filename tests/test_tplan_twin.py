"""The NumPy statement of the space-time re-planning (tests/tplan_twin.py) on hand cases with exact answers, and the safety
property it exists for on a seeded random fleet: a robot planned around reservations padded by r_new + hyp / 2 conflicts with no
fleet path in the sense of the path conflicts (tests/traj_twin.py).  No GPU."""
from collections import deque

import numpy as np
import pytest

import tplan_twin as tw
import traj_twin

FRAME = (0.0, 0.0, 1.0, 1.0)
HYP = np.sqrt(2.0)
PAD = 0.3 + HYP / 2 * (1 + 2.0 ** -20)     # r_new = 0.3 on a unit grid: R = 0.3 + PAD = 1.307.., the cell itself and its 4 neighbours


def corridor(W=11, pocket_x=None):
    """d2 of a corridor one cell wide along row 2 of a 4-row grid, with a pocket two cells deep above column pocket_x."""
    free = np.zeros((4, W), bool)
    free[2, :] = True
    if pocket_x is not None:
        free[0:2, pocket_x] = True
    return free.astype(np.int32)


def row_knots(cells, W, L, hold_from=None):
    """A knot row that is at the centre of cells[k] at tick k (None = absent) and, past the list, at its last cell."""
    kn = np.full((L, 2), np.nan)
    cx, cy = tw.centres(W, 4, FRAME)
    for k in range(L):
        c = cells[k] if k < len(cells) else cells[-1]
        if c is not None:
            kn[k] = cx[c % W], cy[c // W]
    return kn


def head_on(W, L):
    """The other robot: along the corridor from x = W-1 to x = 0, one cell a tick, then parked there."""
    return row_knots([2 * W + (W - 1 - k) for k in range(W)], W, L)[None]


def test_head_on_in_a_corridor_has_no_path():
    W, L = 11, 24
    res, _ = tw.reserve(head_on(W, L), None, [0.3], None, PAD, W, 4, FRAME)
    for hold in (1, 0):
        out = tw.plan(corridor(W), 0, res, L, [2 * W], [2 * W + W - 1], None, hold, FRAME)
        assert out["status"][0] == tw.TP_NO_PATH and out["arrive"][0] == -1 and out["len"][0] == 0
        assert np.isnan(out["knots_out"]).all()


def test_pocket_step_in_wait_and_arrive():
    """The reservation at layer t is x in 8-t .. 12-t of the corridor, and the pocket's upper cell (3, 1) at layers 6 .. 8.  The
    robot is at (3, 2) at layer 3, (3, 1) at 4, (3, 0) at 5, waits there through 8, is back at (3, 1) at 9 and (3, 2) at 10 (free
    from layer 10), and needs 7 more moves: 17.  In free space it needs 10."""
    W, L = 11, 24
    d2 = corridor(W, pocket_x=3)
    res, _ = tw.reserve(head_on(W, L), None, [0.3], None, PAD, W, 4, FRAME)
    assert list(np.nonzero(res[3, 2])[0]) == [5, 6, 7, 8, 9]
    assert list(np.nonzero(res[:, 1, 3])[0]) == [6, 7, 8] and not res[:, 0, 3].any()
    out = tw.plan(d2, 0, res, L, [2 * W], [2 * W + W - 1], None, 1, FRAME)
    assert out["status"][0] == tw.TP_OK and out["arrive"][0] == 17 and out["len"][0] == 18
    p = list(out["path"][0, :18])
    assert p[:6] == [2 * W, 2 * W + 1, 2 * W + 2, 2 * W + 3, W + 3, 3]
    assert p[5:9] == [3, 3, 3, 3] and p[9:11] == [W + 3, 2 * W + 3] and p[17] == 2 * W + 10
    free = tw.plan(d2, 0, None, L, [2 * W], [2 * W + W - 1], None, 1)
    assert free["arrive"][0] == 10
    # the knots: the centres along the path, then parked at the goal
    kn = out["knots_out"][0]
    assert np.array_equal(kn[4], [3.5, 1.5]) and np.array_equal(kn[17], [10.5, 2.5]) and np.array_equal(kn[23], [10.5, 2.5])


def test_waiting_k_ticks_is_the_optimum():
    """A robot stands at x = 5 for ticks 0 .. 6 and is gone afterwards: cells 4 .. 6 are reserved at layers 0 .. 6.  The new robot
    reaches x = 3 at layer 3, waits 3 ticks, enters x = 4 at layer 7: 13 = 10 + 3."""
    W, L = 11, 20
    other = row_knots([2 * W + 5] * 7 + [None] * 13, W, L)[None]
    res, _ = tw.reserve(other, None, [0.3], None, PAD, W, 4, FRAME)
    assert [list(np.nonzero(res[t, 2])[0]) for t in (0, 6, 7)] == [[4, 5, 6], [4, 5, 6], []]
    out = tw.plan(corridor(W), 0, res, L, [2 * W], [2 * W + 10], None, 0, FRAME)
    assert out["arrive"][0] == 13
    assert list(out["path"][0, :14] - 2 * W) == [0, 1, 2, 3, 3, 3, 3, 4, 5, 6, 7, 8, 9, 10]
    assert np.isnan(out["knots_out"][0, 14:]).all()          # no hold: absent after the arrival


def test_goal_reserved_until_layer_m():
    """Only the goal cell (R = 0.4 < 1) is reserved, at layers 5 .. 8: without hold the robot is there at layer 3; with hold it
    may only stay once the goal is never reserved again, and arrives at 9 = m + 1 from the cell beside it."""
    W, L = 11, 16
    other = row_knots([None] * 5 + [2 * W + 10] * 4 + [None] * 7, W, L)[None]
    res, _ = tw.reserve(other, None, [0.2], None, 0.2, W, 4, FRAME)
    assert list(np.nonzero(res[:, 2, 10])[0]) == [5, 6, 7, 8] and res.sum() == 4
    a = tw.plan(corridor(W), 0, res, L, [2 * W + 7], [2 * W + 10], None, 0)
    b = tw.plan(corridor(W), 0, res, L, [2 * W + 7], [2 * W + 10], None, 1)
    assert a["arrive"][0] == 3 and b["arrive"][0] == 9
    assert list(b["path"][0, :10] - 2 * W) == [7, 8, 9, 9, 9, 9, 9, 9, 9, 10]


def test_start_blocked_and_bad_endpoints():
    W, L = 11, 12
    other = row_knots([2 * W + 5] * L, W, L)[None]
    res, _ = tw.reserve(other, None, [0.3], None, PAD, W, 4, FRAME)
    start = np.array([2 * W + 4, 2 * W + 4, 2 * W, 0, 2 * W, -1, 2 * W], np.int32)
    goal = np.array([2 * W, 2 * W, 2 * W + 1, 2 * W, 4 * W, 2 * W, 2 * W + 1], np.int32)
    t_start = np.array([0, 3, 0, 0, 0, 0, L], np.int32)
    out = tw.plan(corridor(W), 0, res, L, start, goal, t_start, 1, FRAME)
    assert list(out["status"]) == [tw.TP_START_BLOCKED, tw.TP_START_BLOCKED, tw.TP_OK, tw.TP_BAD_ENDPOINT, tw.TP_BAD_ENDPOINT,
                                   tw.TP_BAD_ENDPOINT, tw.TP_BAD_ENDPOINT]
    assert list(out["arrive"]) == [-1, -1, 1, -1, -1, -1, -1]


def test_t_start_later_than_zero():
    W, L = 11, 20
    out = tw.plan(corridor(W), 0, None, L, [2 * W + 1, 2 * W + 4], [2 * W + 6, 2 * W + 4], np.array([4, 7]), 1, FRAME)
    assert list(out["arrive"]) == [9, 7] and list(out["len"]) == [6, 1]
    assert np.isnan(out["knots_out"][0, :4]).all() and np.array_equal(out["knots_out"][0, 4], [1.5, 2.5])
    assert np.array_equal(out["knots_out"][0, 9:], np.broadcast_to([6.5, 2.5], (11, 2)))
    assert np.isnan(out["knots_out"][1, :7]).all() and np.array_equal(out["knots_out"][1, 7:], np.broadcast_to([4.5, 2.5], (13, 2)))


def test_diagonal_forbidden_by_the_corner_rule():
    open4 = np.ones((2, 2), np.int32)
    assert tw.plan(open4, 0, None, 4, [0], [3], None, 0)["arrive"][0] == 1
    cut = open4.copy()
    cut[0, 1] = 0
    out = tw.plan(cut, 0, None, 4, [0], [3], None, 0)
    assert out["arrive"][0] == 2 and list(out["path"][0, :3]) == [0, 2, 3]


def bfs_depth(mv, start):
    H, W = mv.shape
    depth = np.full(H * W, -1)
    depth[start] = 0
    dq = deque([start])
    while dq:
        c = dq.popleft()
        y, x = divmod(c, W)
        for d in range(8):
            if mv[y, x] >> d & 1:
                n = (y + tw.DY[d]) * W + x + tw.DX[d]
                if depth[n] < 0:
                    depth[n] = depth[c] + 1
                    dq.append(n)
    return depth


def salt(W, H, frac, seed):
    rng = np.random.default_rng(seed)
    return rng, (rng.random((H, W)) >= frac).astype(np.int32)


def test_without_reservations_arrival_is_bfs_depth():
    rng, d2 = salt(37, 29, 0.3, 5)
    free = np.nonzero(d2.ravel())[0]
    start = rng.choice(free, 24).astype(np.int32)
    goal = rng.choice(free, 24).astype(np.int32)
    mv = tw.moves(d2, 0)
    L = 80
    out = tw.plan(d2, 0, None, L, start, goal, None, 1)
    n_unreach = 0
    for b in range(24):
        d = bfs_depth(mv, int(start[b]))[goal[b]]
        if d < 0:
            n_unreach += 1
            assert out["status"][b] == tw.TP_NO_PATH
        else:
            assert d < L and out["status"][b] == tw.TP_OK and out["arrive"][b] == d and out["len"][b] == d + 1
    assert 0 < n_unreach < 24
    # all-zero reservations are no reservations
    z = tw.plan(d2, 0, np.zeros((L, 29, 37), bool), L, start, goal, None, 1)
    assert all(np.array_equal(z[k], out[k]) for k in ("status", "arrive", "len", "path"))


def test_pack_and_unpack():
    rng = np.random.default_rng(0)
    for W in (1, 31, 32, 33, 70):
        b = rng.random((3, 4, W)) < 0.5
        w = tw.pack(b)
        assert w.shape == (3, 4, (W + 31) // 32) and w.dtype == np.uint32
        assert np.array_equal(tw.unpack(w, W), b)
        assert w[0, 0, 0] & 1 == b[0, 0, 0] and (int(w[..., -1].max()) >> ((W - 1) % 32 + 1)) == 0


def random_fleet(seed=1, W=70, H=45, P=24, K=160, B=40):
    """A seeded fleet on 12 % salt: P grid motions between random free cells (planned in free space, parked at their goals), B
    robots with random ends and start layers.  Frame: 5 cm cells; every radius 2 cm."""
    rng, d2 = salt(W, H, 0.12, seed)
    frame = (-1.0, 2.0, 0.05, 0.05)
    free = np.nonzero(d2.ravel())[0]
    L = K + 1
    fleet = tw.plan(d2, 0, None, L, rng.choice(free, P).astype(np.int32), rng.choice(free, P).astype(np.int32),
                    rng.integers(0, 30, P).astype(np.int32), 1, frame)
    start = rng.choice(free, B).astype(np.int32)
    goal = rng.choice(free, B).astype(np.int32)
    t_start = rng.integers(0, 40, B).astype(np.int32)
    return dict(d2=d2, frame=frame, W=W, H=H, L=L, K=K, knots=fleet["knots_out"], radius=np.full(P, 0.02), start=start, goal=goal,
                t_start=t_start, r_new=np.full(B, 0.02))


@pytest.fixture(scope="module")
def fleet_case():
    f = random_fleet()
    hyp = np.sqrt(np.float64(np.float32(0.05)) ** 2 * 2)
    f["pad"] = 0.02 + hyp / 2 * (1 + 2.0 ** -20)
    f["out"] = tw.fleet_replan(f["knots"], None, f["radius"], None, f["pad"], f["W"], f["H"], f["frame"], None, f["d2"], 0, f["start"],
                               f["goal"], f["t_start"], 1)
    f["free"] = tw.plan(f["d2"], 0, None, f["L"], f["start"], f["goal"], f["t_start"], 1)
    return f


def test_planned_robots_conflict_with_no_fleet_path(fleet_case):
    f, out = fleet_case, fleet_case["out"]
    P, B = len(f["radius"]), len(f["start"])
    rows = np.concatenate([f["knots"], out["knots_out"]])
    group = np.concatenate([np.full(P, -1), np.zeros(B)]).astype(np.int32)          # the new rows are not compared with each other
    rep = traj_twin.conflicts(rows, np.zeros(P + B, np.int32), 0.0, 0.1, np.concatenate([f["radius"], f["r_new"]]), group)
    assert (rep["n_conf"][P:] == 0).all()
    ok = out["status"] == tw.TP_OK
    assert (rep["min_sep"][P:][ok] >= 0.04).all()
    print("minimum separation of a planned robot", rep["min_sep"][P:][ok].min(), "against", 0.04)


def test_the_random_fleet_is_not_vacuous(fleet_case):
    f, out, free = fleet_case, fleet_case["out"], fleet_case["free"]
    st = out["status"]
    ok = st == tw.TP_OK
    later = ok & (out["arrive"] > free["arrive"])
    waits = [b for b in np.nonzero(ok)[0] if (np.diff(out["path"][b, :out["len"][b]]) == 0).any()]
    counts = (int(ok.sum()), int(later.sum()), int((st == tw.TP_NO_PATH).sum()), int((st == tw.TP_START_BLOCKED).sum()), len(waits))
    print("ok, later than free, no path, start blocked, paths that wait:", counts)
    assert (free["status"] == tw.TP_OK)[ok].all() and (out["arrive"] >= free["arrive"])[ok].all()
    assert 3 * counts[1] >= counts[0] and counts[2] >= 1 and counts[3] >= 1 and counts[4] >= 1
    assert counts == PINNED_COUNTS


PINNED_COUNTS = (36, 23, 3, 1, 10)   # (ok, later than free, no path, start blocked, paths that wait) of random_fleet()


def test_sequential_robots_also_avoid_each_other(fleet_case):
    f = fleet_case
    n = 12
    out = tw.fleet_replan(f["knots"], None, f["radius"], None, f["pad"], f["W"], f["H"], f["frame"], None, f["d2"], 0, f["start"][:n],
                          f["goal"][:n], f["t_start"][:n], 1, r_new=f["r_new"][:n], sequential=True)
    P = len(f["radius"])
    rows = np.concatenate([f["knots"], out["knots_out"]])
    rep = traj_twin.conflicts(rows, np.zeros(P + n, np.int32), 0.0, 0.1, np.concatenate([f["radius"], f["r_new"][:n]]))
    assert (rep["n_conf"][P:] == 0).all()
    assert (out["status"] == tw.TP_OK).sum() >= 6
