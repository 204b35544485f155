"""NumPy restatement of the curve check and repair (sc_curve_clearance_batch, sc_curve_clear_batch; the definition is in
include/sea_current_hip.h and DESIGN.md section 21).  Every product and sum is the fp64 one of the definition in its order,
so the integer outputs and the float32 bits are the kernel's."""
import math

import numpy as np

OK, COLLIDES = 0, 6
N_CLAMP = 1 << 20
INT_MAX = 2**31 - 1


def edt(occ):
    """Exact squared distance to the nearest occupied cell, int32 [H,W] (brute force, small maps)."""
    H, W = occ.shape
    ys, xs = np.nonzero(occ)
    if len(ys) == 0:
        return np.full((H, W), INT_MAX, np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(-1).astype(np.int32)


def block_map(W, H, seed, nblocks=7):
    """A seeded map of rectangular blocks with a free border."""
    rng = np.random.default_rng(seed)
    occ = np.zeros((H, W), np.uint8)
    for _ in range(nblocks):
        w, h = rng.integers(2, W // 4, 2)
        x, y = rng.integers(2, W - w - 2), rng.integers(2, H - h - 2)
        occ[y:y + h, x:x + w] = 1
    return occ


def leg_samples(c, n):
    """The n + 1 points of leg c float32 [4,2] at t_k = k / n, fp64 [n+1,2] (bez_eval, order 0)."""
    p = c.astype(np.float64)
    s = np.arange(n + 1, dtype=np.float64) / float(n)
    r = 1 - s
    out = np.empty((n + 1, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(2):
            p0, p1, p2, p3 = p[0, a], p[1, a], p[2, a], p[3, a]
            out[:, a] = r * r * r * p0 + 3 * r * r * s * p1 + 3 * r * s * s * p2 + s * s * s * p3
    return out


def leg_count(c, frame):
    """(n, forced): the sample count of a leg, and whether the count or the length alone make it hit."""
    p = c.astype(np.float64)
    Lp = None
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(3):
            dx, dy = p[j + 1, 0] - p[j, 0], p[j + 1, 1] - p[j, 1]
            l = np.sqrt(dx * dx + dy * dy)
            Lp = l if j == 0 else Lp + l
    if not np.isfinite(Lp):
        return 1, True
    h = np.float64(min(np.float32(frame[2]), np.float32(frame[3])))
    q = np.ceil(6.0 * Lp / h)
    if q > N_CLAMP:
        return N_CLAMP, True
    return (1 if q < 1.0 else int(q)), False


def cell_values(pts, d2, frame):
    """d2 of the cell of every point fp64 [n,2]; 0 where the point is not finite or outside the map."""
    H, W = d2.shape
    x_min, y_min, res_x, res_y = (np.float64(np.float32(v)) for v in frame)
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = (pts[:, 0] - x_min) / res_x, (pts[:, 1] - y_min) / res_y
        inside = (fx >= 0.0) & (fy >= 0.0) & (fx < W) & (fy < H)
    ix = np.where(inside, np.floor(np.where(inside, fx, 0.0)), 0).astype(np.int64)
    iy = np.where(inside, np.floor(np.where(inside, fy, 0.0)), 0).astype(np.int64)
    return np.where(inside, d2[iy, ix], 0).astype(np.int32)


def leg_eval(c, d2, frame, r2c, dense=1):
    """(leg_min, hit, hit_t float32, n) of one leg.  dense > 1 samples that many times as densely (cross-checks only)."""
    n, forced = leg_count(c, frame)
    v = cell_values(leg_samples(c, n * dense), d2, frame)
    mn = int(v.min())
    hit = forced or mn < r2c
    bad = np.nonzero(v < r2c)[0]
    t = np.float32(-1.0) if not hit else (np.float32(0.0) if len(bad) == 0 else np.float32(np.float64(bad[0]) / np.float64(n * dense)))
    return mn, hit, t, n


def clearance(ctrl, seg_off, d2, frame, r2_clear, status=None):
    """sc_curve_clearance_batch.  leg_min of skipped paths' legs is left at -1 here (the call does not touch them)."""
    P, S = len(seg_off) - 1, int(seg_off[-1])
    r2c = max(int(r2_clear), 1)
    o = dict(leg_min=np.full(S, -1, np.int32), path_min=np.zeros(P, np.int32), hit_legs=np.zeros(P, np.int32),
             hit_leg=np.full(P, -1, np.int32), hit_t=np.full(P, -1.0, np.float32))
    for p in range(P):
        if status is not None and status[p] != OK:
            continue
        pm = INT_MAX
        for i in range(seg_off[p], seg_off[p + 1]):
            mn, hit, t, _ = leg_eval(ctrl[i], d2, frame, r2c)
            o["leg_min"][i] = mn
            pm = min(pm, mn)
            if hit:
                o["hit_legs"][p] += 1
                if o["hit_leg"][p] < 0:
                    o["hit_leg"][p], o["hit_t"][p] = i - seg_off[p], t
        o["path_min"][p] = pm
    return o


def leg_ctrl(c0, la, lb):
    """Leg c0 float32 [4,2] (level 0) with its waypoints at levels la and lb."""
    c = c0.copy()
    d = c0.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if la > 0:
            c[1] = (d[0] + math.ldexp(1.0, -int(la)) * (d[1] - d[0])).astype(np.float32)
        if lb > 0:
            c[2] = (d[3] - math.ldexp(1.0, -int(lb)) * (d[3] - d[2])).astype(np.float32)
    return c


def repair_path(c0, d2, frame, r2c, max_level):
    """One path: c0 float32 [ns,4,2] -> (ctrl, level uint8 [ns+1], rounds, leg_min int32 [ns], resolved)."""
    ns = len(c0)
    lv = np.zeros(ns + 1, np.int64)
    dirty = np.ones(ns, bool)
    hit = np.zeros(ns, bool)
    mins = np.zeros(ns, np.int32)
    c = c0.copy()
    r = 0
    while True:
        for i in np.nonzero(dirty)[0]:
            c[i] = leg_ctrl(c0[i], lv[i], lv[i + 1])
            mins[i], hit[i], _, _ = leg_eval(c[i], d2, frame, r2c)
        if not hit.any():
            return c, lv.astype(np.uint8), r, mins, True
        bump = np.zeros(ns + 1, bool)
        bump[:-1] |= hit
        bump[1:] |= hit
        new = np.where(bump, np.minimum(lv + 1, max_level), lv)
        chg = new != lv
        if not chg.any():
            return c, lv.astype(np.uint8), r, mins, False
        lv = new
        dirty = chg[:-1] | chg[1:]
        r += 1


def clear(ctrl, seg_off, d2, frame, r2_clear, max_level, status=None):
    """sc_curve_clear_batch.  leg_min of skipped paths' legs is left at -1 here (the call does not touch them)."""
    P, S = len(seg_off) - 1, int(seg_off[-1])
    r2c = max(int(r2_clear), 1)
    o = dict(ctrl=ctrl[:S].copy(), level=np.zeros(S + P, np.uint8), rounds=np.zeros(P, np.int32), leg_min=np.full(S, -1, np.int32),
             status=np.zeros(P, np.int32))
    for p in range(P):
        if status is not None and status[p] != OK:
            o["status"][p] = status[p]
            continue
        a, b = int(seg_off[p]), int(seg_off[p + 1])
        c, lv, r, mins, ok = repair_path(ctrl[a:b], d2, frame, r2c, max_level)
        o["ctrl"][a:b], o["level"][a + p:b + p + 1], o["rounds"][p], o["leg_min"][a:b] = c, lv, r, mins
        o["status"][p] = OK if ok else COLLIDES
    return o


def sweep_paths(W, H, seed, count):
    """count paths of three to six waypoints at cell centres of free cells of a W x H map (res 1, origin 0) whose straight
    legs are clear, so that only the curves can hit: (occ, d2, wp float32 [count,6,2], npts int32 [count])."""
    rng = np.random.default_rng(seed)
    occ = block_map(W, H, seed)
    d2 = edt(occ)
    free = np.argwhere(d2 >= 2)

    def straight_clear(a, b):
        """the straight leg between two cell centres stays in cells with d2 >= 1 (sampled eight times per cell)"""
        m = 8 * int(np.abs(b - a).max()) + 1
        t = np.linspace(0.0, 1.0, m)[:, None]
        q = np.floor(a + 0.5 + t * (b - a)).astype(int)
        return bool((d2[q[:, 0], q[:, 1]] >= 1).all())

    wp = np.zeros((count, 6, 2), np.float32)
    npts = rng.integers(3, 7, count).astype(np.int32)
    for p in range(count):
        # consecutive waypoints at least four cells apart
        pts = [free[rng.integers(len(free))]]
        while len(pts) < npts[p]:
            q = free[rng.integers(len(free))]
            if np.abs(q - pts[-1]).max() >= 4 and straight_clear(pts[-1], q):
                pts.append(q)
        a = np.array(pts)
        wp[p, :npts[p], 0], wp[p, :npts[p], 1] = a[:, 1] + 0.5, a[:, 0] + 0.5
    return occ, d2, wp, npts
