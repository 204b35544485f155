"""NumPy twin of the range-scan calls (sc_scan_cast_batch, sc_logodds_update) straight from the definition in
include/sea_current_hip.h: the ordered walk (Python integers, one division per column), cast, the miss / hit marks and the
update, square_fan ("a scan" without trigonometry), a deliberately naive membership test of the walk (the four-corner test of
views_twin.clear_bruteforce, reused by import), the builder of the C statement (tests/cpp/scan_ref.c) and the exploration loop
with a log-odds map in place of the mask.  Checker only: the library never imports it."""
import ctypes as C
import os
import subprocess

import numpy as np

import views_twin as vt

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "scan_ref.c")
NO_RETURN, IGNORED, MAX_REACH = -1, -2, 16384
LOOP_PARAMS = dict(l_hit=2, l_miss=1, l_clamp=8, t_occ=2, t_free=1)


# ---- the walk ----
def ray_ok(ray, W, H):
    ax, ay, bx, by = (int(v) for v in ray)
    return 0 <= ax < W and 0 <= ay < H and abs(bx - ax) <= MAX_REACH and abs(by - ay) <= MAX_REACH


def walk_unbounded(ax, ay, bx, by):
    """The cells (x, y) of the supercover of a -> b in sequence order, whatever grid there is: column i = 0 .. D of the major
    axis, inside a column rows rlo(i) .. rhi(i) away from a."""
    ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
    dx, dy = bx - ax, by - ay
    xmajor = abs(dx) >= abs(dy)
    D, m = (abs(dx), abs(dy)) if xmajor else (abs(dy), abs(dx))
    smaj = -1 if (dx if xmajor else dy) < 0 else 1
    smin = -1 if (dy if xmajor else dx) < 0 else 1
    for i in range(D + 1):
        if D == 0:
            rlo = rhi = 0
        else:
            tlo, thi = max(2 * i - 1, 0), min(2 * i + 1, 2 * D)
            nlo, nhi = tlo * m - D, thi * m + D
            rlo = 0 if nlo <= 0 else -((-nlo) // (2 * D))
            rhi = nhi // (2 * D)
        for r in range(rlo, rhi + 1):
            yield (ax + smaj * i, ay + smin * r) if xmajor else (ax + smin * r, ay + smaj * i)


def walk(ray, W, H):
    """Walk(a, b) as a list of cell indices: the sequence up to, not including, its first cell outside the grid.  The ray must
    not be ignored."""
    out = []
    for x, y in walk_unbounded(*ray):
        if not (0 <= x < W and 0 <= y < H):
            break
        out.append(y * W + x)
    return out


class _Probe:
    """An `occ` that is free everywhere and remembers which cells it was asked for."""

    def __init__(self):
        self.cells = set()

    def __getitem__(self, yx):
        self.cells.add((int(yx[1]), int(yx[0])))
        return 0


def supercover_bruteforce(ax, ay, bx, by):
    """The set of cells (x, y) whose closed unit square meets the closed segment a -> b, by views_twin.clear_bruteforce's
    four-corner test over every cell of the bounding box (it asks occ for exactly those cells)."""
    p = _Probe()
    assert vt.clear_bruteforce(p, ax, ay, bx, by)
    return p.cells


# ---- the definitions ----
def _rays(rays):
    return np.asarray(rays, dtype=np.int64).reshape(-1, 4)


def cast(occ, rays):
    """hit int32 [N]: IGNORED for an ignored ray or a sensor on an occupied cell, else the first occupied cell of the walk in
    sequence order, else NO_RETURN."""
    occ = np.asarray(occ)
    H, W = occ.shape
    flat = occ.ravel()
    rays = _rays(rays)
    hit = np.full(len(rays), IGNORED, np.int32)
    for k, ray in enumerate(rays.tolist()):
        if not ray_ok(ray, W, H) or flat[ray[1] * W + ray[0]] != 0:
            continue
        hit[k] = next((c for c in walk(ray, W, H) if flat[c] != 0), NO_RETURN)
    return hit


def marks(rays, hit, W, H):
    """(miss, hitmap) bool [H,W]: the cells missed and the cells hit by some beam.  A beam with hit below -1 or >= W * H is
    ignored, as the device form does."""
    rays, hit = _rays(rays), np.asarray(hit, dtype=np.int64).reshape(-1)
    miss, hitmap = np.zeros(W * H, bool), np.zeros(W * H, bool)
    for ray, h in zip(rays.tolist(), hit.tolist()):
        if not ray_ok(ray, W, H) or h < NO_RETURN or h >= W * H:
            continue
        if h >= 0:
            hitmap[h] = True
        cells = walk(ray, W, H)
        if h in cells:
            cells = cells[:cells.index(h)]
        miss[cells] = True
    return miss.reshape(H, W), hitmap.reshape(H, W)


def update(L, rays, hit, W, H, l_hit, l_miss, l_clamp, t_occ, t_free):
    """(Lout int32, occ_est uint8, known uint8) [H,W]; L None is a map of zeros."""
    miss, hitmap = marks(rays, hit, W, H) if len(_rays(rays)) else (np.zeros((H, W), bool), np.zeros((H, W), bool))
    l = np.zeros((H, W), np.int64) if L is None else np.asarray(L, dtype=np.int64).reshape(H, W)
    l = np.clip(l + np.where(hitmap, l_hit, np.where(miss, -l_miss, 0)), -l_clamp, l_clamp)
    return l.astype(np.int32), (l >= t_occ).astype(np.uint8), ((l >= t_occ) | (l <= -t_free)).astype(np.uint8)


def square_fan(cx, cy, r):
    """The 8 r rays from (cx, cy) to every cell on the perimeter of the square of half-side r around it, going round once:
    int32 [8 r, 4].  On a free grid they miss exactly the cells of the square, clipped to the grid."""
    assert r >= 1
    t = np.arange(-r, r)
    ex = np.concatenate([t, np.full(2 * r, r), -t, np.full(2 * r, -r)])
    ey = np.concatenate([np.full(2 * r, -r), t, np.full(2 * r, r), -t])
    out = np.empty((8 * r, 4), np.int32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = cx, cy, cx + ex, cy + ey
    return out


# ---- the C statement ----
class Ref:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libscan_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i, i32 = C.c_void_p, C.c_int, C.c_int32
        self.lib.sx_walk.restype = i
        self.lib.sx_walk.argtypes = [vp, i, i, vp, i]
        self.lib.sx_cast.restype = None
        self.lib.sx_cast.argtypes = [vp, vp, i, i, i, vp]
        self.lib.sx_miss_steps.restype = C.c_int64
        self.lib.sx_miss_steps.argtypes = [vp, vp, i, i, i]
        self.lib.sx_update.restype = i
        self.lib.sx_update.argtypes = [vp, vp, vp, i, i, i, i32, i32, i32, i32, i32, vp, vp, vp]

    def walk(self, ray, W, H):
        """The cells of the walk, or None for an ignored ray."""
        ray = np.ascontiguousarray(ray, dtype=np.int32)
        cells = np.empty(3 * (2 * MAX_REACH + 2), np.int32)
        n = self.lib.sx_walk(ray.ctypes.data, W, H, cells.ctypes.data, len(cells))
        assert n <= len(cells)
        return None if n < 0 else cells[:n].tolist()

    def cast(self, occ, rays):
        occ = np.ascontiguousarray(occ, dtype=np.uint8)
        rays = np.ascontiguousarray(rays, dtype=np.int32).reshape(-1, 4)
        hit = np.full(len(rays), -7, np.int32)
        self.lib.sx_cast(occ.ctypes.data, rays.ctypes.data, len(rays), occ.shape[1], occ.shape[0], hit.ctypes.data)
        return hit

    def miss_steps(self, rays, hit, W, H):
        """The cells the beams miss, counted beam by beam."""
        rays = np.ascontiguousarray(rays, dtype=np.int32).reshape(-1, 4)
        hit = np.ascontiguousarray(hit, dtype=np.int32)
        return int(self.lib.sx_miss_steps(rays.ctypes.data, hit.ctypes.data, len(rays), W, H))

    def update(self, L, rays, hit, W, H, l_hit, l_miss, l_clamp, t_occ, t_free, in_place=False):
        rays = np.ascontiguousarray(rays, dtype=np.int32).reshape(-1, 4)
        hit = np.ascontiguousarray(hit, dtype=np.int32)
        L = None if L is None else np.array(L, dtype=np.int32).reshape(H, W)
        Lout = L if in_place else np.full((H, W), -7, np.int32)
        occ_est, known = np.full((H, W), 7, np.uint8), np.full((H, W), 7, np.uint8)
        st = self.lib.sx_update(None if L is None else L.ctypes.data, rays.ctypes.data, hit.ctypes.data, len(rays), W, H, l_hit, l_miss,
                                l_clamp, t_occ, t_free, Lout.ctypes.data, occ_est.ctypes.data, known.ctypes.data)
        assert st == 0
        return Lout, occ_est, known


# ---- the exploration loop ----
def sound(occ, occ_est, known):
    """The estimate never contradicts the true map: an estimated obstacle is one, a cell known free is free."""
    occ = np.asarray(occ) != 0
    return bool((occ[np.asarray(occ_est) != 0]).all() and (~occ[(np.asarray(known) != 0) & (np.asarray(occ_est) == 0)]).all())


def sense_twin(L, occ, pos, r, params):
    H, W = occ.shape
    rays = square_fan(pos % W, pos // W, r)
    return update(L, rays, cast(occ, rays), W, H, **params)


def explore_loop_scan(occ, start, step, r=10, params=LOOP_PARAMS, sense=None):
    """views_twin.explore_loop_views with a range sensor and a log-odds map: where it stands the robot casts square_fan of
    half-side r on the true map and updates its map; it explores on (known, occ_est).  `sense(L, occ, pos, r, params)` ->
    (L, occ_est, known) defaults to the twin's.  Soundness is asserted at every step.  With l_hit >= t_occ and l_miss >= t_free
    one look settles a cell, soundness keeps it settled, and from a frontier cell the fan reaches the unknown orthogonal
    neighbour first (a miss if it is free, the hit if it is not): every iteration reveals at least one cell, so W * H bounds
    the loop -- a guard, not a tolerance.  Returns (goals, known, L)."""
    sense = sense or sense_twin
    occ = np.asarray(occ)
    H, W = occ.shape
    pos = int(start)
    L, occ_est, known = sense(None, occ, pos, r, params)
    assert sound(occ, occ_est, known)
    goals = []
    for _ in range(W * H):
        goal = int(step(occ_est, known, pos))
        if goal < 0:
            return goals, known, L
        goals.append(goal)
        pos = goal
        L, occ_est, known = sense(L, occ, pos, r, params)
        assert sound(occ, occ_est, known)
    raise AssertionError("exploration did not end within W * H iterations")
