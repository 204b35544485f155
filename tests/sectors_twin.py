"""NumPy twin of sensors with a field of view (sc_known_from_sectors, sc_sector_gain_batch, sc_view_gain_headings_batch,
sc_views_from_cells) straight from the definitions in include/sea_current_hip.h: the half-open sector In(d; a, b) in int64, the
heading table's rules, the bin of an offset by trying every bin, sector views on views_twin's Clear, the gain of every heading
from the histogram of bins, the builder of the C statement (tests/cpp/sectors_ref.c) and the exploration loop with sector
sensing.  Checker only: the library never imports it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import views_twin as vt

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "sectors_ref.c")
MAX_BINS = 64
LIM = 32767


def cross(px, py, qx, qy):
    return px * qy - py * qx


def dot(px, py, qx, qy):
    return px * qx + py * qy


# ---- In(d; a, b) ----
def sector_ignored(a, b):
    """True for the pairs (a, b) that make an ignored view."""
    ax, ay, bx, by = (int(v) for v in (*a, *b))
    if ax == ay == bx == by == 0:
        return False
    if max(abs(ax), abs(ay), abs(bx), abs(by)) > LIM:
        return True
    if (ax == 0 and ay == 0) != (bx == 0 and by == 0):
        return True
    return cross(ax, ay, bx, by) == 0 and dot(ax, ay, bx, by) > 0


def in_sector(dx, dy, a, b):
    """In(d; a, b) for arrays of offsets (int64) and one pair that is not ignored: bool array."""
    dx, dy = np.asarray(dx, np.int64), np.asarray(dy, np.int64)
    ax, ay, bx, by = (int(v) for v in (*a, *b))
    assert not sector_ignored(a, b)
    centre = (dx == 0) & (dy == 0)
    if ax == ay == bx == by == 0:
        return np.ones(dx.shape, bool)
    s = cross(ax, ay, bx, by)
    if s > 0:
        r = (cross(ax, ay, dx, dy) >= 0) & (cross(dx, dy, bx, by) > 0)
    elif s < 0:
        r = ~((cross(bx, by, dx, dy) >= 0) & (cross(dx, dy, ax, ay) > 0))
    else:
        r = (cross(ax, ay, dx, dy) > 0) | ((cross(ax, ay, dx, dy) == 0) & (dot(ax, ay, dx, dy) > 0))
    return r | centre


# ---- the heading table ----
def dirs_valid(dirs):
    d = np.asarray(dirs)
    if d.ndim != 2 or d.shape[1] != 2 or not 3 <= len(d) <= MAX_BINS:
        return False
    d = d.astype(np.int64)
    if (np.abs(d) > LIM).any():
        return False
    n = np.roll(d, -1, axis=0)
    if (cross(d[:, 0], d[:, 1], n[:, 0], n[:, 1]) <= 0).any():
        return False
    up = (d[:, 1] > 0) | ((d[:, 1] == 0) & (d[:, 0] > 0))
    return int((up & ~np.roll(up, -1)).sum()) == 1


def heading_dirs(B, phase=0.0):
    """round(32767 (cos, sin)(2 pi (b + phase) / B)), the issue's tables."""
    return np.array([[round(LIM * math.cos(2 * math.pi * (b + phase) / B)), round(LIM * math.sin(2 * math.pi * (b + phase) / B))]
                     for b in range(B)], np.int32)


def bin_counts(dirs, dx, dy):
    """[B, n] bool: offset k lies in bin b.  Every bin is tried; a valid table puts an offset d != 0 in exactly one."""
    dirs = np.asarray(dirs, np.int64)
    B = len(dirs)
    return np.stack([in_sector(dx, dy, dirs[b], dirs[(b + 1) % B]) & ~((np.asarray(dx) == 0) & (np.asarray(dy) == 0)) for b in range(B)])


def bins_of(dirs, dx, dy):
    """The bin of every offset, -1 for the centre."""
    m = bin_counts(dirs, dx, dy)
    centre = (np.asarray(dx) == 0) & (np.asarray(dy) == 0)
    assert (m.sum(0)[~centre] == 1).all() and not m[:, centre].any()
    return np.where(centre, -1, m.argmax(0))


def sector_views(views, dirs, h, span):
    views = np.asarray(views, np.int32).reshape(-1, 3)
    dirs = np.asarray(dirs, np.int32)
    B = len(dirs)
    h = np.broadcast_to(np.asarray(h, np.int64), (len(views),)) % B
    out = np.zeros((len(views), 7), np.int32)
    out[:, :3] = views
    if span < B:
        out[:, 3:5], out[:, 5:7] = dirs[h], dirs[(h + span) % B]
    return out


# ---- sector views ----
def seen_by_sector(occ, row):
    """(vis bool [H,W], xs, ys of the seen cells) of one sector row; nothing for an ignored one."""
    occ = np.asarray(occ)
    H, W = occ.shape
    cx, cy, r2 = (int(v) for v in row[:3])
    a, b = row[3:5], row[5:7]
    vis = np.zeros((H, W), bool)
    if sector_ignored(a, b) or r2 < 0 or not (0 <= cx < W and 0 <= cy < H) or occ[cy, cx] != 0:
        return vis
    r = math.isqrt(r2)
    x0, x1, y0, y1 = max(cx - r, 0), min(cx + r, W - 1), max(cy - r, 0), min(cy + r, H - 1)
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    inside = ((xs - cx) ** 2 + (ys - cy) ** 2 <= r2) & in_sector(xs - cx, ys - cy, a, b)
    xs, ys = xs[inside], ys[inside]
    ok = vt.clear_targets(occ, cx, cy, xs, ys)
    vis[ys[ok], xs[ok]] = True
    return vis


def seen(occ, sviews):
    occ = np.asarray(occ)
    vis = np.zeros(occ.shape, bool)
    for row in np.asarray(sviews, np.int64).reshape(-1, 7):
        vis |= seen_by_sector(occ, row)
    return vis


def known_from_sectors(base, occ, sviews):
    """(known, occ_seen) uint8 [H,W]: views_twin.known_from_views with sector rows."""
    occ = np.ascontiguousarray(occ, dtype=np.uint8)
    vis = seen(occ, sviews)
    known = vis | vt.surface(occ, vis)
    if base is not None:
        known = known | (np.asarray(base) != 0)
    return known.astype(np.uint8), np.where(known, occ, 0).astype(np.uint8)


def sector_gain(occ, known, sviews):
    occ, known = np.asarray(occ), np.asarray(known)
    rows = np.asarray(sviews, np.int64).reshape(-1, 7)
    return np.array([int((seen_by_sector(occ, row) & (known == 0)).sum()) for row in rows], np.int32).reshape(len(rows))


def view_gain_headings(occ, known, views, dirs, span):
    """dict(hist int32 [N,B], c0 int32 [N], gainh int32 [N,B], best int32 [N,2]); the table and span must be valid."""
    occ, known = np.asarray(occ), np.asarray(known)
    assert dirs_valid(dirs) and 1 <= span <= len(dirs)
    B = len(dirs)
    v = np.asarray(views, np.int64).reshape(-1, 3)
    hist, c0 = np.zeros((len(v), B), np.int32), np.zeros(len(v), np.int32)
    for i, (cx, cy, r2) in enumerate(v.tolist()):
        vis = seen_by_sector(occ, (cx, cy, r2, 0, 0, 0, 0)) & (known == 0)
        ys, xs = np.nonzero(vis)
        if len(xs):
            bins = bins_of(dirs, xs - cx, ys - cy)
            c0[i] = int((bins < 0).sum())
            hist[i] = np.bincount(bins[bins >= 0], minlength=B)
    return dict(hist=hist, c0=c0, **headings_from_hist(hist, c0, span))


def headings_from_hist(hist, c0, span):
    """dict(gainh, best): the circular window sums of `span` bins, their maximum and the smallest heading attaining it."""
    gainh = (c0[:, None] + sum(np.roll(hist, -j, axis=1) for j in range(span))).astype(np.int32)
    best = np.stack([gainh.max(1), gainh.argmax(1)], 1).astype(np.int32) if len(hist) else np.zeros((0, 2), np.int32)
    return dict(gainh=gainh, best=best)


def views_from_cells(cell, W, H, r2):
    c = np.asarray(cell, np.int64).reshape(-1)
    ok = (c >= 0) & (c < W * H)
    return np.stack([np.where(ok, c % W, 0), np.where(ok, c // W, 0), np.where(ok, r2, -1)], 1).astype(np.int32)


# ---- the C statement ----
class Ref:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libsectors_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC, vt.SRC])
        self.lib = C.CDLL(so)
        vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
        self.lib.sx_in.restype = i
        self.lib.sx_in.argtypes = [i64] * 6
        self.lib.sx_dirs_valid.restype = i
        self.lib.sx_dirs_valid.argtypes = [vp, i]
        self.lib.sx_bins_of.restype = i
        self.lib.sx_bins_of.argtypes = [vp, i, i64, i64, vp]
        self.lib.sx_known_from_sectors.restype = i
        self.lib.sx_known_from_sectors.argtypes = [vp, vp, vp, i, i, i, vp, vp]
        self.lib.sx_sector_gain.restype = None
        self.lib.sx_sector_gain.argtypes = [vp, vp, vp, i, i, i, vp]
        self.lib.sx_view_gain_headings.restype = i
        self.lib.sx_view_gain_headings.argtypes = [vp, vp, vp, i, i, i, vp, i, i, vp, vp, vp]
        self.lib.sx_views_from_cells.restype = None
        self.lib.sx_views_from_cells.argtypes = [vp, i, i, i, C.c_int32, vp]

    def in_sector(self, dx, dy, a, b):
        """1 / 0, -1 for an ignored pair"""
        return int(self.lib.sx_in(int(dx), int(dy), int(a[0]), int(a[1]), int(b[0]), int(b[1])))

    def dirs_valid(self, dirs):
        d = np.ascontiguousarray(dirs, dtype=np.int32)
        return bool(self.lib.sx_dirs_valid(d.ctypes.data, len(d)))

    def bins_of(self, dirs, dx, dy):
        """(how many bins hold d, the first of them)"""
        d = np.ascontiguousarray(dirs, dtype=np.int32)
        b = C.c_int(-9)
        n = self.lib.sx_bins_of(d.ctypes.data, len(d), int(dx), int(dy), C.byref(b))
        return int(n), b.value

    def known_from_sectors(self, base, occ, sviews, in_place=False):
        occ = np.ascontiguousarray(occ, dtype=np.uint8)
        H, W = occ.shape
        sviews = np.ascontiguousarray(sviews, dtype=np.int32).reshape(-1, 7)
        base = None if base is None else np.array(base, dtype=np.uint8)
        known = base if in_place else np.empty((H, W), np.uint8)
        occ_seen = np.empty((H, W), np.uint8)
        st = self.lib.sx_known_from_sectors(None if base is None else base.ctypes.data, occ.ctypes.data, sviews.ctypes.data, len(sviews), W, H,
                                            known.ctypes.data, occ_seen.ctypes.data)
        assert st == 0
        return known, occ_seen

    def sector_gain(self, occ, known, sviews):
        occ, known = np.ascontiguousarray(occ, dtype=np.uint8), np.ascontiguousarray(known, dtype=np.uint8)
        H, W = occ.shape
        sviews = np.ascontiguousarray(sviews, dtype=np.int32).reshape(-1, 7)
        gain = np.full(len(sviews), -7, np.int32)
        self.lib.sx_sector_gain(occ.ctypes.data, known.ctypes.data, sviews.ctypes.data, len(sviews), W, H, gain.ctypes.data)
        return gain

    def view_gain_headings(self, occ, known, views, dirs, span):
        """dict(hist, gainh, best), or None when the C statement refuses the table or the span"""
        occ, known = np.ascontiguousarray(occ, dtype=np.uint8), np.ascontiguousarray(known, dtype=np.uint8)
        H, W = occ.shape
        views = np.ascontiguousarray(views, dtype=np.int32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 2)
        N, B = len(views), len(dirs)
        hist, gainh, best = np.full((N, B), -7, np.int32), np.full((N, B), -7, np.int32), np.full((N, 2), -7, np.int32)
        st = self.lib.sx_view_gain_headings(occ.ctypes.data, known.ctypes.data, views.ctypes.data, N, W, H, dirs.ctypes.data, B, span,
                                            hist.ctypes.data, gainh.ctypes.data, best.ctypes.data)
        return None if st else dict(hist=hist, gainh=gainh, best=best)

    def views_from_cells(self, cell, W, H, r2):
        cell = np.ascontiguousarray(cell, dtype=np.int32).reshape(-1)
        views = np.full((len(cell), 3), -7, np.int32)
        self.lib.sx_views_from_cells(cell.ctypes.data, len(cell), W, H, r2, views.ctypes.data)
        return views


# ---- the exploration loop ----
def explore_loop_sectors(occ, start, step, dirs, span, sense_r2=100, sense=None, best=None):
    """views_twin.explore_loop_views with a sensor of `span` bins of the table `dirs`.  Wherever the robot stands (its start, then
    every goal) it senses with the heading of largest predicted gain on the observed map (best(views, occ_seen, known) -> int32
    [1,2]; ties go to the smallest heading); if that adds no known cell it senses the full circle once, a turn on the spot.
    At a goal, a frontier cell, the full circle reveals a cell (consequence (iii) of the full-circle sensor), so every
    iteration adds one and W * H bounds the loop: a guard, not a tolerance.  Returns dict(goals, headings (one more than goals:
    the start's comes first), fallbacks, known)."""
    sense = sense or known_from_sectors
    best = best or (lambda views, occ_seen, known: view_gain_headings(occ_seen, known, views, dirs, span)["best"])
    occ = np.asarray(occ)
    H, W = occ.shape
    B = len(dirs)
    state = dict(known=np.zeros((H, W), np.uint8), occ_seen=np.zeros((H, W), np.uint8), fallbacks=0, headings=[])

    def look(pos):
        view = np.array([(pos % W, pos // W, sense_r2)], np.int32)
        h = int(np.asarray(best(view, state["occ_seen"], state["known"]))[0, 1])
        known, occ_seen = sense(state["known"], occ, sector_views(view, dirs, h, span))
        if int((known != 0).sum()) == int((state["known"] != 0).sum()):
            known, occ_seen = sense(state["known"], occ, sector_views(view, dirs, 0, B))
            state["fallbacks"] += 1
        state["headings"].append(h)
        state["known"], state["occ_seen"] = known, occ_seen

    pos = int(start)
    look(pos)
    goals = []
    for _ in range(W * H):
        goal = int(step(state["occ_seen"], state["known"], pos))
        if goal < 0:
            return dict(goals=goals, headings=state["headings"], fallbacks=state["fallbacks"], known=state["known"])
        goals.append(goal)
        pos = goal
        look(pos)
    raise AssertionError("exploration did not end within W * H iterations")
