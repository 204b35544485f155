"""Inputs the CPU and the GPU tests of wide-window scan matching share: the maps, fans as points, recovery cases with priors
anywhere in a wide window, the overflow pair, and the kidnapped robot at the end of the walk of DESIGN.md section 25.
Checker only."""
import numpy as np

import frontier_twin as ft
import match_twin as mt
import scan_twin as st
import views_twin as vt


def line():
    occ = np.zeros((1, 200), np.uint8)
    occ[0, [80, 150]] = 1
    return occ


def maps():
    return {"blocks": vt.blocks(), "salt0.05": vt.salt(130, 70, 0.05, 3), "door": vt.door_map(), "rooms": vt.rooms_map(), "row": line(),
            "column": np.ascontiguousarray(line().T)}


def free_near(occ, x, y):
    H, W = occ.shape
    free = np.flatnonzero(occ.ravel() == 0)
    c = int(free[np.argmin((free % W - x) ** 2 + (free // W - y) ** 2)])
    return c % W, c // W


def scan_points(occ, x, y, r):
    """The hits of square_fan(r) from the free cell (x, y) as offsets: int32 [8 r, 2]."""
    rays = st.square_fan(x, y, r)
    return mt.points_from_hits(rays, st.cast(occ, rays), occ.shape[1])


# name -> (map, wx, wy, top): the maps of the recovery cases
def recovery_maps():
    return {"blocks": (vt.blocks(256, 192, 10), 100, 70, 3), "salt0.03": (vt.salt(256, 192, 0.03, 3), 100, 70, 3),
            "rooms": (vt.rooms_map(), 40, 30, 2)}


def recovery_cases(occ, wx, wy, seed=0, n=24, r=30):
    """n poses on free cells, each with a fan of half-side r seen by a sensor turned by q quarter turns and a prior that is
    off by anything inside the window: (pts [n,4,N,2], centre [n,2], want [n,3] = the (q, dx, dy) that recover the pose)."""
    H, W = occ.shape
    rng = np.random.default_rng(seed)
    free = np.flatnonzero(occ.ravel() == 0)
    pts, centre, want = [], [], []
    for c in free[rng.integers(0, len(free), n)]:
        ax, ay = int(c % W), int(c // W)
        q = int(rng.integers(0, 4))
        ex, ey = int(rng.integers(-wx, wx + 1)), int(rng.integers(-wy, wy + 1))
        seen = mt.quarter_turns(scan_points(occ, ax, ay, r), -q)       # candidate rotation q undoes the sensor's turn
        pts.append(np.stack([mt.quarter_turns(seen, k) for k in range(4)]))
        centre.append((ax + ex, ay + ey))
        want.append((q, -ex, -ey))
    return np.stack(pts), np.array(centre, np.int32), np.array(want, np.int32)


def overflow_case():
    """A grid nobody knows: every candidate of the +-20 window ties.  (d2, known, pts [1,1,8,2], centre, 1681)."""
    d2 = np.full((50, 60), 7, np.int32)
    known = np.zeros((50, 60), np.uint8)
    pts = np.array([(k - 4, 2 * k - 7) for k in range(8)], np.int32)[None, None]
    return d2, known, pts, np.array([[30, 25]], np.int32), 41 * 41


KIDNAP = (17, -11)


def kidnapped(edt, matcher=None):
    """The walk of DESIGN.md section 25 run to its end with the +-3 matcher; at its last pose the believed cell is then
    displaced by KIDNAP from the true one.  dict(d2, known: the robot's own map before that scan is put in, pts [1,1,N,2]:
    the scan, true: the cell it was taken from, centre: the displaced prior)."""
    occ = vt.salt(mt.WALK["W"], mt.WALK["H"], mt.WALK["p"], mt.WALK["seed"])
    W = occ.shape[1]
    start = ft.loop_start(occ)
    last = {}

    def record(d2, known, pts, centre, wx, wy, cap, unk):
        best = (matcher or (lambda *a: mt.match(*a)[0]))(d2, known, pts, centre, wx, wy, cap, unk)
        last.update(d2=np.array(d2), known=np.array(known), pts=np.array(pts, np.int32))
        return best

    got = mt.walk(occ, start, edt, corrected=True, unk=1, matcher=record)
    assert got["exact"] == got["steps"]                                # the robot knew where it was until now
    true = mt.bfs_path(occ, start)[::mt.WALK["every"]][-1]
    tx, ty = true % W, true // W
    return dict(last, true=(tx, ty), centre=np.array([[tx + KIDNAP[0], ty + KIDNAP[1]]], np.int32))
