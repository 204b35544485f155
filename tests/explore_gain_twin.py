"""NumPy twin of coordinated exploration goals by gain (sc_explore_gain_batch, sc_frontier_centres,
sc_fleet_explore_gain_batch) straight from the definitions in include/sea_current_hip.h.  This is the naive form: every round
calls views_twin.view_gain / sectors_twin.view_gain_headings over all candidates and known_from_views / known_from_sectors for
the pick; the library's delta pass has to equal it.  Also the builder of the C statement (tests/cpp/explore_gain_ref.c) and the
behavioural fixture (a room with two doorways and a farther room).  Checker only: the library never imports it."""
import ctypes as C
import os
import subprocess

import numpy as np

import frontier_twin as ft
import sectors_twin as st
import views_twin as vt

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "explore_gain_ref.c")
INF = 2**31 - 1
MAX_DIM, MAX_R, MAX_N, MAX_W = 8192, 1024, 65536, 1 << 20
OUT_KEYS = ("goal", "gcost", "ggain", "head", "cand_of", "pick", "npick", "gain0", "gain_end", "known_out")


def args_ok(occ, known, g, cand, r2, dirs, span, wg, wc, min_gain, rounds):
    """The arguments the definition accepts (shapes apart)."""
    H, W = occ.shape
    R, N = g.shape[0], len(cand)
    if not (1 <= W <= MAX_DIM and 1 <= H <= MAX_DIM and 1 <= R <= MAX_R and 0 <= N <= MAX_N and R * N <= 1 << 26):
        return False
    if r2 < 0 or not 0 <= wg <= MAX_W or not 0 <= wc <= MAX_W or min_gain < 0 or not 0 <= rounds <= MAX_R:
        return False
    if dirs is not None and not (st.dirs_valid(dirs) and 1 <= span < len(dirs)):
        return False
    return not (np.asarray(g) < 0).any()


def alive(occ, cand):
    """A candidate is dead when its cell lies outside the grid or stands on occ != 0."""
    occ, c = np.asarray(occ), np.asarray(cand, np.int64).reshape(-1)
    inside = (c >= 0) & (c < occ.size)
    return inside & (occ.ravel()[np.where(inside, c, 0)] == 0)


def gains(occ, kw, views, dirs, span):
    """(gain int32 [N], heading int32 [N]) of every candidate against kw."""
    if dirs is None:
        return vt.view_gain(occ, kw, views), np.full(len(views), -1, np.int32)
    best = st.view_gain_headings(occ, kw, views, dirs, span)["best"]
    return best[:, 0].copy(), best[:, 1].copy()


def explore_gain(occ, known, g, cand, r2, dirs=None, span=0, wg=1, wc=1, min_gain=1, rounds=None):
    """dict(goal, gcost, ggain, head, cand_of, pick int32 [R], npick int32 [1], gain0, gain_end int32 [N], known_out uint8
    [H,W]), or None for arguments the definition refuses."""
    occ, known = np.ascontiguousarray(occ, dtype=np.uint8), np.ascontiguousarray(known, dtype=np.uint8)
    g, cand = np.asarray(g), np.asarray(cand, np.int64).reshape(-1)
    H, W = occ.shape
    R, N = g.shape[0], len(cand)
    rounds = min(R, N) if rounds is None else rounds
    if not args_ok(occ, known, g, cand, r2, dirs, span, wg, wc, min_gain, rounds):
        return None
    gf = g.reshape(R, H * W).astype(np.int64)
    out = {k: np.full(R, -1, np.int32) for k in ("goal", "gcost", "head", "cand_of", "pick")}
    out.update(ggain=np.zeros(R, np.int32), npick=np.zeros(1, np.int32))
    kw = known.copy()
    free, untaken, live = np.ones(R, bool), np.ones(N, bool), alive(occ, cand)
    views = st.views_from_cells(cand, W, H, r2)
    gain, heading = gains(occ, kw, views, dirs, span) if N else (np.zeros(0, np.int32), np.zeros(0, np.int32))
    out["gain0"] = gain.copy()
    for t in range(min(rounds, R, N)):
        best = None
        for r in range(R):
            for n in range(N):
                if not (free[r] and live[n] and untaken[n]) or gf[r, cand[n]] == INF or gain[n] < min_gain:
                    continue
                score = int(wg) * int(gain[n]) - int(wc) * int(gf[r, cand[n]])
                if best is None or score > best[0]:                    # ascending r, then n: the first of equals stays
                    best = (score, r, n)
        if best is None:
            break
        _, r, n = best
        out["goal"][r], out["cand_of"][r], out["gcost"][r] = cand[n], n, gf[r, cand[n]]
        out["ggain"][r], out["head"][r], out["pick"][r] = gain[n], heading[n], t
        free[r], untaken[n] = False, False
        out["npick"][0] = t + 1
        if dirs is None:
            kw = vt.known_from_views(kw, occ, views[n:n + 1])[0]
        else:
            kw = st.known_from_sectors(kw, occ, st.sector_views(views[n:n + 1], dirs, int(heading[n]), span))[0]
        gain, heading = gains(occ, kw, views, dirs, span)
    out.update(gain_end=gain.copy(), known_out=kw)
    return out


def frontier_centres(slot, csize, csum, Cmax):
    """centre int32 [G,Cmax] of slot [H,W] or [G,H,W], csize [G,Cmax] and csum [G,Cmax,2]: the cell of cluster k that minimises
    |csize x - sumx| + |csize y - sumy| in Python integers, the smallest cell among equals, -1 for a row without cells."""
    slot = np.asarray(slot)
    slot = slot[None] if slot.ndim == 2 else slot
    G, H, W = slot.shape
    csize, csum = np.asarray(csize).reshape(G, Cmax), np.asarray(csum).reshape(G, Cmax, 2)
    centre = np.full((G, Cmax), -1, np.int32)
    for gi in range(G):
        flat = slot[gi].ravel()
        for k in range(Cmax):
            cells = np.flatnonzero(flat == k)
            if len(cells):
                s, sx, sy = int(csize[gi, k]), int(csum[gi, k, 0]), int(csum[gi, k, 1])
                keys = [abs(s * int(c % W) - sx) + abs(s * int(c // W) - sy) for c in cells]
                centre[gi, k] = cells[int(np.argmin(keys))]           # argmin: the first, hence smallest, cell among equals
    return centre


def fleet_explore_gain(d2, known, occ, g, r2_sense, r2=0, min_size=1, Cmax=128, dirs=None, span=0, wg=1, wc=1, min_gain=1, rounds=None):
    """The chain of sc_fleet_explore_gain_batch on one grid: frontiers -> centres -> explore_gain with cand = centre."""
    fr = ft.frontiers(d2, known, r2, min_size, Cmax)
    out = {k: (v if k in ("label", "slot") else v[0]) for k, v in fr.items()}
    out["centre"] = frontier_centres(out["slot"], out["csize"], out["csum"], Cmax)[0]
    R = np.asarray(g).shape[0]
    rounds = min(R, Cmax, MAX_R) if rounds is None else rounds
    res = explore_gain(occ, known, g, out["centre"], r2_sense, dirs, span, wg, wc, min_gain, rounds)
    if res is None:
        return None
    out.update(res)
    return out


# ---- the C statement ----
class Ref:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libexplore_gain_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC, st.SRC, vt.SRC])
        self.lib = C.CDLL(so)
        vp, i, i32 = C.c_void_p, C.c_int, C.c_int32
        self.lib.ex_explore_gain.restype = i
        self.lib.ex_explore_gain.argtypes = [vp, vp, vp, i, vp, i, i, i, i32, vp, i, i, i32, i32, i32, i] + [vp] * 10
        self.lib.ex_frontier_centres.restype = None
        self.lib.ex_frontier_centres.argtypes = [vp, vp, vp, i, i, i, vp]

    def explore_gain(self, occ, known, g, cand, r2, dirs=None, span=0, wg=1, wc=1, min_gain=1, rounds=None):
        """explore_gain's dict, or None when the C statement refuses the arguments"""
        occ, known = np.ascontiguousarray(occ, dtype=np.uint8), np.ascontiguousarray(known, dtype=np.uint8)
        g, cand = np.ascontiguousarray(g, dtype=np.int32), np.ascontiguousarray(cand, dtype=np.int32).reshape(-1)
        dirs = None if dirs is None else np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 2)
        H, W = occ.shape
        R, N = g.shape[0], len(cand)
        rounds = min(R, N) if rounds is None else rounds
        out = {k: np.full(R, -7, np.int32) for k in ("goal", "gcost", "ggain", "head", "cand_of", "pick")}
        out.update(npick=np.full(1, -7, np.int32), gain0=np.full(N, -7, np.int32), gain_end=np.full(N, -7, np.int32),
                   known_out=np.full((H, W), 7, np.uint8))
        s = self.lib.ex_explore_gain(occ.ctypes.data, known.ctypes.data, g.ctypes.data, R, cand.ctypes.data, N, W, H, r2,
                                     None if dirs is None else dirs.ctypes.data, 0 if dirs is None else len(dirs), span, wg, wc, min_gain, rounds,
                                     *(out[k].ctypes.data for k in OUT_KEYS))
        assert s in (0, 1)
        return None if s else out

    def frontier_centres(self, slot, csize, csum, Cmax):
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        s3 = slot[None] if slot.ndim == 2 else slot
        G, H, W = s3.shape
        csize = np.ascontiguousarray(csize, dtype=np.int32).reshape(G, Cmax)
        csum = np.ascontiguousarray(csum, dtype=np.int64).reshape(G, Cmax, 2)
        centre = np.full((G, Cmax), -7, np.int32)
        for gi in range(G):
            self.lib.ex_frontier_centres(s3[gi].ctypes.data, csize[gi].ctypes.data, csum[gi].ctypes.data, W, H, Cmax, centre[gi].ctypes.data)
        return centre


# ---- fields without a planner: 4-connected breadth-first distances, 10 per step ----
def bfs_field(free, root):
    """int32 [H,W]: 10 * the 4-connected step count from cell `root` through the True cells of `free`, INF elsewhere."""
    free = np.asarray(free, bool)
    H, W = free.shape
    g = np.full(H * W, INF, np.int64)
    if 0 <= root < H * W and free.ravel()[root]:
        g[root] = 0
        todo = [root]
        while todo:
            nxt = []
            for c in todo:
                x, y = c % W, c // W
                for q, ok in ((c - 1, x > 0), (c + 1, x + 1 < W), (c - W, y > 0), (c + W, y + 1 < H)):
                    if ok and free.ravel()[q] and g[q] == INF:
                        g[q] = g[c] + 10
                        nxt.append(q)
            todo = nxt
    return g.reshape(H, W).astype(np.int32)


# ---- the behavioural fixture ----
SENSE_R2 = 18 * 18


def two_doorways():
    """96 x 80.  A corridor (rows 33 .. 46) runs across the map and is known, with its walls.  Room A lies above it
    (columns 8 .. 48, rows 4 .. 31) with two doorways into the corridor, at columns 24 .. 26 and 32 .. 34; room B lies below it
    at the far end (columns 60 .. 88, rows 48 .. 75) with one doorway at columns 72 .. 74.  Both rooms are unknown.  Two robots
    stand in the corridor under A's doorways, so each of A's two frontier clusters is nearer to both than B's one is.  Returns
    dict(occ, known, occ_seen, d2k-like free mask, robots, g): g are breadth-first fields through the known free cells."""
    W, H = 96, 80
    occ = np.zeros((H, W), np.uint8)
    occ[32, :] = occ[47, :] = 1                                        # the corridor's walls
    occ[3, 7:50] = 1                                                   # room A
    occ[3:33, 7] = occ[3:33, 49] = 1
    occ[47:77, 59] = occ[47:77, 89] = 1                                # room B
    occ[76, 59:90] = 1
    occ[32, 24:27] = occ[32, 32:35] = 0                                # A's doorways
    occ[47, 72:75] = 0                                                 # B's doorway
    known = np.zeros((H, W), np.uint8)
    known[32:48, :] = 1                                                # the corridor with both walls, doorway cells included
    occ_seen = np.where(known != 0, occ, 0).astype(np.uint8)
    robots = np.array([39 * W + 25, 39 * W + 33], np.int32)
    free = (known != 0) & (occ == 0)
    g = np.stack([bfs_field(free, int(r)) for r in robots])
    d2k = np.where(free, 100, 0).astype(np.int32)                      # a d2 that makes every known free cell traversable
    return dict(occ=occ, known=known, occ_seen=occ_seen, d2k=d2k, robots=robots, g=g, W=W, H=H)


def revealed(occ, known, goals, r2):
    """The free cells the full-circle views at `goals` (cells, -1 skipped) newly mark known."""
    H, W = np.asarray(occ).shape
    views = [(int(c) % W, int(c) // W, r2) for c in goals if c >= 0]
    after = vt.known_from_views(known, occ, views)[0]
    return int(((after != 0) & (np.asarray(known) == 0) & (np.asarray(occ) == 0)).sum())
