"""NumPy twin of scan matching (sc_scan_match_batch) straight from the definition in include/sea_current_hip.h: the cost of a
cell, the score volume, the best pose and its ties; the two host helpers restated (points_from_hits, the integer quarter
turn); the loader of the C statement (tests/cpp/match_ref.c); and the walk of DESIGN.md section 25: a robot with noisy
odometry that builds a log-odds map, with and without the matcher's correction.  Checker only: the library never imports it."""
import ctypes as C
import os
import subprocess
from collections import deque

import numpy as np

import scan_twin as st

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "match_ref.c")
ABSENT, IGNORED, MAX_HALF, MAX_POINTS, MAX_ROT = -2**31, -1, 64, 65536, 256
MAX_REACH, MAX_DIM, EDT_INF = st.MAX_REACH, 8192, 2**31 - 1


# ---- the definition ----
def cost_map(d2, known, d2_cap, unk):
    """cost of every cell of the grid, int64 [H,W]."""
    c = np.minimum(np.asarray(d2, dtype=np.int64), d2_cap)
    return c if known is None else np.where(np.asarray(known) != 0, c, unk)


def present(pts):
    """bool [...]: the points of int [..., 2] that are there."""
    p = np.asarray(pts, dtype=np.int64)
    return (np.abs(p) <= MAX_REACH).all(-1)


def centre_ok(c):
    return all(-MAX_REACH <= int(v) <= MAX_DIM + MAX_REACH for v in c)


def match(d2, known, pts, centre, wx, wy, d2_cap, unk):
    """(best int32 [S,6], score int32 [S,R,2wy+1,2wx+1]) of pts int [S,R,N,2] and centre int [S,2]."""
    d2 = np.asarray(d2)
    H, W = d2.shape
    pts = np.asarray(pts, dtype=np.int64)
    S, R, N, _ = pts.shape
    centre = np.asarray(centre, dtype=np.int64).reshape(S, 2)
    assert 0 <= wx <= MAX_HALF and 0 <= wy <= MAX_HALF and 1 <= d2_cap <= 32767 and 0 <= unk <= d2_cap
    assert 1 <= N <= MAX_POINTS and 1 <= R <= MAX_ROT
    # the grid inside a border of unk: a coordinate clipped to the border reads what a cell outside the grid costs
    padded = np.full((H + 2, W + 2), unk, np.int64)
    padded[1:-1, 1:-1] = cost_map(d2, known, d2_cap, unk)
    dxs, dys = np.arange(-wx, wx + 1), np.arange(-wy, wy + 1)
    best = np.zeros((S, 6), np.int32)
    score = np.zeros((S, R, len(dys), len(dxs)), np.int64)
    disp = dys[:, None] ** 2 + dxs[None, :] ** 2
    for s in range(S):
        if not centre_ok(centre[s]):
            best[s, 0] = IGNORED
            continue
        npts = np.zeros(R, np.int64)
        for r in range(R):
            p = pts[s, r][present(pts[s, r])]
            npts[r] = len(p)
            if not len(p):
                continue
            x = np.clip(centre[s, 0] + dxs[:, None] + p[None, :, 0], -1, W) + 1          # [ndx, K]
            for i, dy in enumerate(dys):
                y = np.clip(centre[s, 1] + dy + p[:, 1], -1, H) + 1                      # [K]
                score[s, r, i] = padded[y[None, :], x].sum(1)
        v = score[s]
        smin = v.min()
        cand = [(int(disp[i, j]), int(r), int(i), int(j)) for r, i, j in zip(*np.nonzero(v == smin))]
        _, r, i, j = min(cand)
        best[s] = (r, dxs[j], dys[i], smin, npts[r], len(cand))
    assert score.max(initial=0) < 2**31
    return best, score.astype(np.int32)


# ---- the host helpers, restated ----
def points_from_hits(rays, hit, W):
    """int32 [N,2]: the hit cell of every beam as an offset from its origin; ABSENT for a beam without a hit."""
    rays, hit = np.asarray(rays, dtype=np.int64).reshape(-1, 4), np.asarray(hit, dtype=np.int64).reshape(-1)
    out = np.full((len(hit), 2), ABSENT, np.int64)
    ok = hit >= 0
    out[ok, 0], out[ok, 1] = hit[ok] % W - rays[ok, 0], hit[ok] // W - rays[ok, 1]
    return out.astype(np.int32)


def quarter_turns(pts, q):
    """The integer rotation (x, y) -> (-y, x) applied q times; absent points stay ABSENT."""
    p = np.asarray(pts, dtype=np.int64)
    ok = present(p)
    x, y = p[..., 0], p[..., 1]
    for _ in range(q % 4):
        x, y = -y, x
    return np.where(ok[..., None], np.stack([x, y], -1), ABSENT).astype(np.int32)


# ---- the C statement ----
class Ref:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libmatch_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i, i32 = C.c_void_p, C.c_int, C.c_int32
        self.lib.mx_match.restype = i
        self.lib.mx_match.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, i, i32, i32, vp, vp]

    def match(self, d2, known, pts, centre, wx, wy, d2_cap, unk, want_score=True):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        H, W = d2.shape
        known = None if known is None else np.ascontiguousarray(known, dtype=np.uint8)
        pts = np.ascontiguousarray(pts, dtype=np.int32)
        S, R, N, _ = pts.shape
        centre = np.ascontiguousarray(centre, dtype=np.int32).reshape(S, 2)
        best = np.full((S, 6), -7, np.int32)
        score = np.full((S, R, 2 * wy + 1, 2 * wx + 1), -7, np.int32) if want_score else None
        status = self.lib.mx_match(d2.ctypes.data, None if known is None else known.ctypes.data, pts.ctypes.data, centre.ctypes.data, S, R, N,
                                   W, H, wx, wy, d2_cap, unk, best.ctypes.data, None if score is None else score.ctypes.data)
        assert status == 0
        return best, score


# ---- the walk ----
WALK = dict(W=130, H=70, p=0.05, seed=3, r=12, every=3, noise_seed=7, noise=2, window=3, d2_cap=16)


def bfs_path(occ, start):
    """The 4-connected BFS path (cells) from start to the last cell (largest index) of its free component; neighbours are
    tried in the order left, right, up, down."""
    H, W = occ.shape
    free = np.asarray(occ).ravel() == 0
    prev = {start: -1}
    q = deque([start])
    while q:
        c = q.popleft()
        x, y = c % W, c // W
        for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
            n = ny * W + nx
            if 0 <= nx < W and 0 <= ny < H and free[n] and n not in prev:
                prev[n] = c
                q.append(n)
    c = max(prev)
    path = []
    while c >= 0:
        path.append(c)
        c = prev[c]
    return path[::-1]


def walk(occ, start, edt, corrected, unk=1, matcher=None, cfg=WALK):
    """A robot follows every cfg['every']-th cell of bfs_path.  At each pose it casts square_fan(r) on the true map from
    where it truly is.  Its odometry tells it where it is up to a fresh error of -noise .. noise cells per axis and step (at
    the first pose it knows).  Corrected: it matches the scan against its map so far (d2 = edt(occ_est), known) in a window
    around the odometry's cell and believes the best pose; uncorrected: it believes the odometry.  It then updates its
    log-odds map with the scan placed at the pose it believes.  `matcher(d2, known, pts, centre, wx, wy, d2_cap, unk)` ->
    best defaults to the twin's.  Returns dict(exact, unique, steps, sound): the steps at which the believed pose is the
    true one, those at which the matcher reported n_ties = 1 (corrected only), the number of poses, and whether the final
    estimate never contradicts the true map."""
    matcher = matcher or (lambda *a: match(*a)[0])
    H, W = occ.shape
    poses = bfs_path(occ, start)[::cfg["every"]]
    rng = np.random.RandomState(cfg["noise_seed"])
    L, occ_est, known = None, None, None
    exact = unique = 0
    for step, true in enumerate(poses):
        tx, ty = true % W, true // W
        rays = st.square_fan(tx, ty, cfg["r"])
        hit = st.cast(occ, rays)
        pts = points_from_hits(rays, hit, W)
        bx, by = tx, ty
        if step > 0:
            ex, ey = rng.randint(-cfg["noise"], cfg["noise"] + 1, 2)
            bx, by = tx + int(ex), ty + int(ey)
            if corrected:
                b = matcher(edt(occ_est), known, pts[None, None], [(bx, by)], cfg["window"], cfg["window"], cfg["d2_cap"], unk)[0]
                bx, by = bx + int(b[1]), by + int(b[2])
                unique += int(b[5] == 1)
        exact += int((bx, by) == (tx, ty))
        # the scan as the robot places it: the same beams from the believed cell; a believed cell outside the grid places nothing
        shift = np.array([bx - tx, by - ty, bx - tx, by - ty], np.int32)
        placed = rays + shift
        ok = hit >= 0
        hx, hy = hit % W + shift[0], hit // W + shift[1]
        inside = ok & (hx >= 0) & (hx < W) & (hy >= 0) & (hy < H)
        believed_hit = np.where(inside, hy * W + hx, np.where(ok, st.IGNORED, hit)).astype(np.int32)
        L, occ_est, known = st.update(L, placed, believed_hit, W, H, **st.LOOP_PARAMS)
    return dict(exact=exact, unique=unique, steps=len(poses), sound=st.sound(occ, occ_est, known))
