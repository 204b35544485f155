"""NumPy twin of line-of-sight sensing (sc_known_from_views, sc_view_gain_batch) straight from the definition in
include/sea_current_hip.h: Clear(a, b) as the column walk of DESIGN.md section 9 with the cell test occ == 0 (scalar, and
vectorised over the targets of one view), a second, deliberately naive Clear by the four-corner sign test over every cell of
the bounding box, the builder of the C reference (tests/cpp/views_ref.c), the maps both are run on and the exploration loop
with the sensing line replaced.  Checker only: the library never imports it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import frontier_twin as ft

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "views_ref.c")


# ---- Clear(a, b) ----
def clear(occ, ax, ay, bx, by):
    """Every cell whose closed unit square meets the closed segment between the centres of a and b has occ == 0.  Column i
    (0 .. D) of the major axis, doubled coordinates relative to a: the segment spans t in [max(2i-1, 0), min(2i+1, 2D)] and
    rises t * m / (2D) on the minor axis; it meets rows ceil((tlo m - D) / 2D) .. floor((thi m + D) / 2D).  Python integers."""
    dx, dy = int(bx) - int(ax), int(by) - int(ay)
    if dx == 0 and dy == 0:
        return occ[ay, ax] == 0
    xmajor = abs(dx) >= abs(dy)
    D, m = (abs(dx), abs(dy)) if xmajor else (abs(dy), abs(dx))
    smaj = -1 if (dx if xmajor else dy) < 0 else 1
    smin = -1 if (dy if xmajor else dx) < 0 else 1
    for i in range(D + 1):
        tlo, thi = max(2 * i - 1, 0), min(2 * i + 1, 2 * D)
        nlo, nhi = tlo * m - D, thi * m + D
        rlo = 0 if nlo <= 0 else -((-nlo) // (2 * D))
        rhi = nhi // (2 * D)
        for r in range(rlo, rhi + 1):
            x, y = (ax + smaj * i, ay + smin * r) if xmajor else (ax + smin * r, ay + smaj * i)
            if occ[y, x] != 0:
                return False
    return True


def clear_bruteforce(occ, ax, ay, bx, by):
    """The naive statement: for every cell of the bounding box of a and b, does its closed unit square meet the closed
    segment?  Doubled coordinates: centres at (2x, 2y), squares [2x-1, 2x+1] x [2y-1, 2y+1].  The segment is the part of its
    line inside the box R spanned by the two centres, so the square is clipped to R and the clipped rectangle meets the line
    iff its four corners are not all strictly on one side (the sign of the cross product)."""
    ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
    ux, uy = 2 * (bx - ax), 2 * (by - ay)
    X0, X1, Y0, Y1 = 2 * min(ax, bx), 2 * max(ax, bx), 2 * min(ay, by), 2 * max(ay, by)
    for y in range(min(ay, by), max(ay, by) + 1):
        for x in range(min(ax, bx), max(ax, bx) + 1):
            x0, x1, y0, y1 = max(2 * x - 1, X0), min(2 * x + 1, X1), max(2 * y - 1, Y0), min(2 * y + 1, Y1)
            s = [ux * (py - 2 * ay) - uy * (px - 2 * ax) for px in (x0, x1) for py in (y0, y1)]
            if min(s) <= 0 <= max(s) and occ[y, x] != 0:
                return False
    return True


def clear_targets(occ, cx, cy, xs, ys):
    """Clear((cx, cy), (xs[k], ys[k])) for arrays of targets inside the grid: the column walk with every target advancing one
    column per round, int64 throughout."""
    occ = np.asarray(occ)
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    dx, dy = xs - cx, ys - cy
    xmajor = np.abs(dx) >= np.abs(dy)
    D = np.where(xmajor, np.abs(dx), np.abs(dy))
    m = np.where(xmajor, np.abs(dy), np.abs(dx))
    smaj = np.where(np.where(xmajor, dx, dy) < 0, -1, 1)
    smin = np.where(np.where(xmajor, dy, dx) < 0, -1, 1)
    twoD = np.maximum(2 * D, 1)                                        # D == 0: one column, row 0
    ok = np.ones(xs.shape, bool)
    for i in range(int(D.max()) + 1 if D.size else 0):
        live = ok & (i <= D)
        if not live.any():
            break
        tlo, thi = max(2 * i - 1, 0), np.minimum(2 * i + 1, 2 * D)
        nlo, nhi = tlo * m - D, thi * m + D
        rlo = np.where(nlo <= 0, 0, -((-nlo) // twoD))
        rhi = np.where(D == 0, 0, nhi // twoD)
        for k in range(3):                                             # at most three cells per column
            r = rlo + k
            use = live & (r <= rhi)
            x = np.where(xmajor, cx + smaj * i, cx + smin * r)
            y = np.where(xmajor, cy + smin * r, cy + smaj * i)
            blocked = np.zeros(xs.shape, bool)
            blocked[use] = occ[y[use], x[use]] != 0
            ok &= ~blocked
        assert not (live & (rhi - rlo > 2)).any()
    return ok


# ---- the definitions ----
def live_views(views, W, H):
    """The views that are not ignored: r2 >= 0 and the centre inside the grid."""
    v = np.asarray(views, dtype=np.int64).reshape(-1, 3)
    return [(int(cx), int(cy), int(r2)) for cx, cy, r2 in v.tolist() if r2 >= 0 and 0 <= cx < W and 0 <= cy < H]


def seen_by(occ, cx, cy, r2):
    """vis of one view that is not ignored: bool [H,W]."""
    occ = np.asarray(occ)
    H, W = occ.shape
    vis = np.zeros((H, W), bool)
    if occ[cy, cx] != 0:
        return vis                                                     # a view standing on an occupied cell sees nothing
    r = math.isqrt(r2)
    x0, x1, y0, y1 = max(cx - r, 0), min(cx + r, W - 1), max(cy - r, 0), min(cy + r, H - 1)
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    inside = (xs - cx) ** 2 + (ys - cy) ** 2 <= r2
    xs, ys = xs[inside], ys[inside]
    ok = clear_targets(occ, cx, cy, xs, ys)
    vis[ys[ok], xs[ok]] = True
    return vis


def seen(occ, views):
    occ = np.asarray(occ)
    H, W = occ.shape
    vis = np.zeros((H, W), bool)
    for cx, cy, r2 in live_views(views, W, H):
        vis |= seen_by(occ, cx, cy, r2)
    return vis


def neighbours4(m):
    """True where one of the four orthogonal neighbours inside the grid is set."""
    out = np.zeros_like(m)
    out[1:, :] |= m[:-1, :]
    out[:-1, :] |= m[1:, :]
    out[:, 1:] |= m[:, :-1]
    out[:, :-1] |= m[:, 1:]
    return out


def surface(occ, vis):
    """An occupied cell with a seen free orthogonal neighbour inside the grid."""
    return (np.asarray(occ) != 0) & neighbours4(vis)


def known_from_views(base, occ, views):
    """(known, occ_seen) uint8 [H,W]: known = base != 0 | vis | surf, occ_seen = occ where known, 0 elsewhere."""
    occ = np.ascontiguousarray(occ, dtype=np.uint8)
    vis = seen(occ, views)
    known = vis | surface(occ, vis)
    if base is not None:
        known = known | (np.asarray(base) != 0)
    return known.astype(np.uint8), np.where(known, occ, 0).astype(np.uint8)


def view_gain(occ, known, views):
    """gain int32 [N]: the cells with known == 0 that view i alone sees; 0 for an ignored view."""
    occ, known = np.asarray(occ), np.asarray(known)
    H, W = occ.shape
    v = np.asarray(views, dtype=np.int64).reshape(-1, 3)
    gain = np.zeros(len(v), np.int32)
    for i, (cx, cy, r2) in enumerate(v.tolist()):
        if r2 >= 0 and 0 <= cx < W and 0 <= cy < H:
            gain[i] = int((seen_by(occ, cx, cy, r2) & (known == 0)).sum())
    return gain


# ---- the C reference ----
class Ref:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libviews_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        self.lib.vx_clear.restype = i
        self.lib.vx_clear.argtypes = [vp, i, i, i, i, i, i]
        self.lib.vx_known_from_views.restype = i
        self.lib.vx_known_from_views.argtypes = [vp, vp, vp, i, i, i, vp, vp]
        self.lib.vx_view_gain.restype = None
        self.lib.vx_view_gain.argtypes = [vp, vp, vp, i, i, i, vp]

    def clear(self, occ, ax, ay, bx, by):
        occ = np.ascontiguousarray(occ, dtype=np.uint8)
        return bool(self.lib.vx_clear(occ.ctypes.data, occ.shape[1], occ.shape[0], ax, ay, bx, by))

    def known_from_views(self, base, occ, views, in_place=False):
        occ = np.ascontiguousarray(occ, dtype=np.uint8)
        H, W = occ.shape
        views = np.ascontiguousarray(views, dtype=np.int32).reshape(-1, 3)
        base = None if base is None else np.array(base, dtype=np.uint8)
        known = base if in_place else np.empty((H, W), np.uint8)
        occ_seen = np.empty((H, W), np.uint8)
        st = self.lib.vx_known_from_views(None if base is None else base.ctypes.data, occ.ctypes.data, views.ctypes.data, len(views), W, H,
                                          known.ctypes.data, occ_seen.ctypes.data)
        assert st == 0
        return known, occ_seen

    def view_gain(self, occ, known, views):
        occ, known = np.ascontiguousarray(occ, dtype=np.uint8), np.ascontiguousarray(known, dtype=np.uint8)
        H, W = occ.shape
        views = np.ascontiguousarray(views, dtype=np.int32).reshape(-1, 3)
        gain = np.full(len(views), -7, np.int32)
        self.lib.vx_view_gain(occ.ctypes.data, known.ctypes.data, views.ctypes.data, len(views), W, H, gain.ctypes.data)
        return gain


# ---- maps ----
def door_map(W=96, H=64, wall=48, door=(30, 32)):
    """A wall in column `wall` with a door in rows door[0] .. door[1]."""
    occ = np.zeros((H, W), np.uint8)
    occ[:, wall] = 1
    occ[door[0]:door[1] + 1, wall] = 0
    return occ


DOOR_VIEW = (20, 31, 3600)


def rooms_map(W=96, H=80):
    """Six rooms of 32 x 40 behind one-cell walls (columns 32 and 64, row 40), each wall stretch with a door of three cells;
    every room is reachable from every other."""
    occ = np.zeros((H, W), np.uint8)
    occ[:, 32] = occ[:, 64] = 1
    occ[40, :] = 1
    for x, y in ((32, 18), (64, 22), (32, 60), (64, 56)):             # doors in the vertical walls
        occ[y:y + 3, x] = 0
    for x in (10, 46, 80):                                             # doors in the horizontal wall
        occ[40, x:x + 3] = 0
    return occ


def corner_map(block):
    """9 x 9, free but for the cells listed."""
    occ = np.zeros((9, 9), np.uint8)
    for x, y in block:
        occ[y, x] = 1
    return occ


def salt(W, H, p, seed):
    from sea_current_amd import synth
    return synth.salt_grid(W, H, p, seed=seed)


def blocks(W=128, H=96, seed=10):
    from sea_current_amd import synth
    return synth.block_grid(W, H, 0.3, seed=seed, smin=3, smax=24)


def free_centres(occ, views):
    """The views with every in-grid centre moved onto a free cell of its row where there is one (so that they see something)."""
    occ = np.asarray(occ)
    H, W = occ.shape
    out = np.array(views, np.int32).reshape(-1, 3).copy()
    for v in out:
        if 0 <= v[0] < W and 0 <= v[1] < H and occ[v[1], v[0]] != 0:
            free = np.flatnonzero(occ[v[1]] == 0)
            if len(free):
                v[0] = free[np.argmin(np.abs(free - v[0]))]
    return out


def loop_maps():
    return {"blocks96x80": ft.loop_maps()["blocks96x80"], "rooms96x80": rooms_map()}


# ---- the exploration loop ----
def explore_loop_views(occ, start, step, sense_r2=100, sense=None):
    """frontier_twin.explore_loop with the sensing line replaced: the robot sees what known_from_views of the true map gives
    from where it stands, and occ_seen comes from that call.  `sense(base, occ, views)` -> (known, occ_seen) defaults to the
    twin's.  Every iteration reveals at least one cell (consequence (iii)), so W * H bounds the loop: a guard, not a tolerance."""
    sense = sense or known_from_views
    occ = np.asarray(occ)
    H, W = occ.shape
    pos = int(start)
    known, occ_seen = sense(None, occ, [(pos % W, pos // W, sense_r2)])
    goals = []
    for _ in range(W * H):
        goal = int(step(occ_seen, known, pos))
        if goal < 0:
            return goals, known
        goals.append(goal)
        pos = goal
        known, occ_seen = sense(known, occ, [(pos % W, pos // W, sense_r2)])
    raise AssertionError("exploration did not end within W * H iterations")
