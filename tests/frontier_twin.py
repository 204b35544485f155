"""NumPy twin of the exploration frontiers (sc_known_from_discs, sc_d2_known_i32, sc_frontier_batch, sc_frontier_cost_matrix,
sc_fleet_explore_batch) straight from the definitions in include/sea_current_hip.h, the builder of the C reference
(tests/cpp/frontier_ref.c), scipy's labelling in the library's canonical form, the maps both are run on and the exploration
loop of the tests.  Checker only: the library never imports it."""
import ctypes as C
import os
import subprocess

import numpy as np

import assign_twin

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "frontier_ref.c")
INF = 2**31 - 1
KEYS = ("label", "slot", "ncl", "rep", "csize", "cbox", "csum")


# ---- the definitions ----
def known_from_discs(base, discs, W, H):
    """known uint8 [H,W]: base != 0, or inside a disc (cx, cy, r2) with r2 >= 0; exact integers."""
    known = np.zeros((H, W), bool) if base is None else np.asarray(base) != 0
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    for cx, cy, r2 in np.asarray(discs, dtype=np.int64).reshape(-1, 3).tolist():
        if r2 >= 0:
            known = known | ((xs - cx) ** 2 + (ys - cy) ** 2 <= r2)
    return known.astype(np.uint8)


def d2_known(d2, known):
    return np.where(np.asarray(known) != 0, np.asarray(d2), 0).astype(np.int32)


def frontier_mask(d2, known, r2=0):
    """Fr of one grid: known, d2 >= max(r2, 1), an orthogonal neighbour inside the grid unknown."""
    k = np.asarray(known) != 0
    u = ~k
    nb = np.zeros_like(k)
    nb[1:, :] |= u[:-1, :]
    nb[:-1, :] |= u[1:, :]
    nb[:, 1:] |= u[:, :-1]
    nb[:, :-1] |= u[:, 1:]
    return k & (np.asarray(d2) >= max(int(r2), 1)) & nb


def _clusters(fr):
    """label int32 [H,W] of a boolean mask, 8-connected, each cluster named by its smallest cell; the clusters as
    (representative, cells) in ascending order of representative.  One flood fill per cluster, started in index order."""
    H, W = fr.shape
    label = np.full(H * W, -1, np.int64)
    todo = set(np.flatnonzero(fr.ravel()).tolist())
    out = []
    for r in sorted(todo):
        if r not in todo:
            continue
        todo.discard(r)
        cells, stack = [], [r]
        while stack:
            c = stack.pop()
            cells.append(c)
            x, y = c % W, c // W
            for yy in (y - 1, y, y + 1):
                for xx in (x - 1, x, x + 1):
                    q = yy * W + xx
                    if 0 <= xx < W and 0 <= yy < H and q in todo:
                        todo.discard(q)
                        stack.append(q)
        label[cells] = r
        out.append((r, np.array(sorted(cells), np.int64)))
    return label.reshape(H, W).astype(np.int32), out


def frontiers_one(d2, known, r2=0, min_size=1, Cmax=128):
    d2 = np.asarray(d2)
    H, W = d2.shape
    label, clusters = _clusters(frontier_mask(d2, known, r2))
    out = dict(label=label, slot=np.full((H, W), -1, np.int32), ncl=np.zeros(2, np.int32), rep=np.full(Cmax, -1, np.int32),
               csize=np.zeros(Cmax, np.int32), cbox=np.zeros((Cmax, 4), np.int32), csum=np.zeros((Cmax, 2), np.int64))
    listed = [(r, cells) for r, cells in clusters if len(cells) >= min_size]
    out["ncl"][:] = (len(listed), len(clusters))
    for k, (r, cells) in enumerate(listed[:Cmax]):
        x, y = cells % W, cells // W
        out["slot"].ravel()[cells] = k
        out["rep"][k] = r
        out["csize"][k] = len(cells)
        out["cbox"][k] = (x.min(), y.min(), x.max(), y.max())
        out["csum"][k] = (x.sum(), y.sum())
    return out


def frontiers(d2, known, r2=0, min_size=1, Cmax=128):
    """d2, known [H,W] or [G,H,W] -> dict(label, slot shaped like d2, ncl [G,2], rep, csize [G,Cmax], cbox [G,Cmax,4],
    csum int64 [G,Cmax,2])."""
    d2, known = np.asarray(d2), np.asarray(known)
    if d2.ndim == 2:
        one = frontiers_one(d2, known, r2, min_size, Cmax)
        return {k: (v if k in ("label", "slot") else v[None]) for k, v in one.items()}
    outs = [frontiers_one(d, k, r2, min_size, Cmax) for d, k in zip(d2, known)]
    return {k: np.stack([o[k] for o in outs]) for k in KEYS}


def cost_matrix(g, slot, csize, Cmax, gain=0, size_cap=0, fgrid=None):
    """cost, cell int32 [F,Cmax] of fields g [F,H,W] against slot [H,W] or [G,H,W] and csize [G,Cmax] (or [Cmax])."""
    g = np.asarray(g)
    F = g.shape[0]
    slot = np.asarray(slot)
    slot = slot[None] if slot.ndim == 2 else slot
    G = slot.shape[0]
    csize = np.asarray(csize).reshape(G, Cmax)
    cost, cell = np.full((F, Cmax), INF, np.int32), np.full((F, Cmax), -1, np.int32)
    for f in range(F):
        gi = 0 if fgrid is None else int(fgrid[f])
        if not 0 <= gi < G:
            continue
        gf, sf = g[f].ravel().astype(np.int64), slot[gi].ravel()
        for k in range(Cmax):
            cells = np.flatnonzero(sf == k)
            if len(cells) == 0:
                continue
            m = int(gf[cells].min())
            if m == INF:
                continue
            cell[f, k] = int(cells[gf[cells] == m][0])
            s = int(csize[gi, k])
            cost[f, k] = min(m + int(gain) * (int(size_cap) - min(s, int(size_cap))), INF - 1)
    return cost, cell


def fleet_explore(d2, known, g, r2=0, min_size=1, Cmax=128, gain=0, size_cap=0):
    """The chain of sc_fleet_explore_batch on one grid: frontiers -> matrix -> assign_twin -> goal, gcost per robot."""
    g = np.asarray(g)
    F = g.shape[0]
    fr = frontiers(d2, known, r2, min_size, Cmax)
    out = {k: (v if k in ("label", "slot") else v[0]) for k, v in fr.items()}
    out["cost"], out["cell"] = cost_matrix(g, out["slot"], out["csize"], Cmax, gain, size_cap)
    a = assign_twin.assign_one(out["cost"])
    out.update(col_of=a["col_of"], row_of=a["row_of"], info=a["info"])
    goal, gcost = np.full(F, -1, np.int32), np.full(F, -1, np.int32)
    for r in range(F):
        if a["col_of"][r] >= 0:
            goal[r] = out["cell"][r, a["col_of"][r]]
            gcost[r] = g[r].ravel()[goal[r]]
    out.update(goal=goal, gcost=gcost)
    return out


# ---- the C reference ----
class Ref:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libfrontier_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i, i32 = C.c_void_p, C.c_int, C.c_int32
        self.lib.fx_known_from_discs.restype = None
        self.lib.fx_known_from_discs.argtypes = [vp, vp, i, i, i, vp]
        self.lib.fx_d2_known.restype = None
        self.lib.fx_d2_known.argtypes = [vp, vp, C.c_int64, vp]
        self.lib.fx_frontier.restype = i
        self.lib.fx_frontier.argtypes = [vp, vp, i, i, i32, i, i] + [vp] * 7
        self.lib.fx_cost_matrix.restype = None
        self.lib.fx_cost_matrix.argtypes = [vp, i, vp, vp, vp, i, i, i, i, i32, i32, vp, vp]

    def known_from_discs(self, base, discs, W, H):
        discs = np.ascontiguousarray(discs, dtype=np.int32).reshape(-1, 3)
        base = None if base is None else np.ascontiguousarray(base, dtype=np.uint8)
        known = np.empty((H, W), np.uint8)
        self.lib.fx_known_from_discs(None if base is None else base.ctypes.data, discs.ctypes.data, len(discs), W, H, known.ctypes.data)
        return known

    def d2_known(self, d2, known):
        d2, known = np.ascontiguousarray(d2, dtype=np.int32), np.ascontiguousarray(known, dtype=np.uint8)
        out = np.empty_like(d2)
        self.lib.fx_d2_known(d2.ctypes.data, known.ctypes.data, d2.size, out.ctypes.data)
        return out

    def frontiers(self, d2, known, r2=0, min_size=1, Cmax=128):
        d2, known = np.ascontiguousarray(d2, dtype=np.int32), np.ascontiguousarray(known, dtype=np.uint8)
        d3, k3 = (d2, known) if d2.ndim == 3 else (d2[None], known[None])
        G, H, W = d3.shape
        out = dict(label=np.empty_like(d3), slot=np.empty_like(d3), ncl=np.zeros((G, 2), np.int32), rep=np.zeros((G, Cmax), np.int32),
                   csize=np.zeros((G, Cmax), np.int32), cbox=np.zeros((G, Cmax, 4), np.int32), csum=np.zeros((G, Cmax, 2), np.int64))
        for gi in range(G):
            st = self.lib.fx_frontier(d3[gi].ctypes.data, k3[gi].ctypes.data, W, H, r2, min_size, Cmax, *(out[k][gi].ctypes.data for k in KEYS))
            assert st == 0
        out["label"], out["slot"] = out["label"].reshape(d2.shape), out["slot"].reshape(d2.shape)
        return out

    def cost_matrix(self, g, slot, csize, Cmax, gain=0, size_cap=0, fgrid=None):
        g, slot = np.ascontiguousarray(g, dtype=np.int32), np.ascontiguousarray(slot, dtype=np.int32)
        csize = np.ascontiguousarray(csize, dtype=np.int32)
        fgrid = None if fgrid is None else np.ascontiguousarray(fgrid, dtype=np.int32)
        F, H, W = g.shape
        G = 1 if slot.ndim == 2 else slot.shape[0]
        cost, cell = np.empty((F, Cmax), np.int32), np.empty((F, Cmax), np.int32)
        self.lib.fx_cost_matrix(g.ctypes.data, F, None if fgrid is None else fgrid.ctypes.data, slot.ctypes.data, csize.ctypes.data, G, W, H,
                                Cmax, gain, size_cap, cost.ctypes.data, cell.ctypes.data)
        return cost, cell


def labels_scipy(fr):
    """label and the cluster count of a boolean mask from scipy.ndimage.label with the 3 x 3 structure, relabelled to each
    cluster's smallest cell."""
    from scipy import ndimage
    H, W = fr.shape
    lab, k = ndimage.label(fr, structure=np.ones((3, 3), int))
    label = np.full((H, W), -1, np.int32)
    if k:
        idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
        mins = ndimage.minimum(idx, lab, index=np.arange(1, k + 1)).astype(np.int64)
        label[fr] = mins[lab[fr] - 1]
    return label, int(k)


def count_4connected(fr):
    from scipy import ndimage
    return int(ndimage.label(fr, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])[1])


# ---- maps: known masks (uint8 [H,W]) whose boundaries meet the tile edges of the kernel in every way ----
def _xy(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return xs, ys


def two_discs(W=200, H=150):
    """Two overlapping discs: the frontier is one closed ring, slanted nearly everywhere (on a free 200 x 150 grid 268 cells:
    one cluster 8-connected, 112 pieces 4-connected)."""
    return known_from_discs(None, [(93, 75, 40 * 40), (108, 75, 45 * 45)], W, H)


def ring(W, H, cx, cy, r_out, r_in):
    """Known between two circles: two concentric frontier rings."""
    xs, ys = _xy(W, H)
    q = (xs - cx) ** 2 + (ys - cy) ** 2
    return ((q <= r_out * r_out) & (q >= r_in * r_in)).astype(np.uint8)


def staircase(W, H, step=3, shift=0):
    """Known left of a staircase of `step` x `step` treads: horizontal and vertical runs joined at their corners."""
    xs, ys = _xy(W, H)
    return (xs < step * (ys // step + 1) + shift).astype(np.uint8)


def corner_diagonal(W, H):
    """Known on and below the main diagonal: the frontier is the diagonal itself, through (63,63)-(64,64), every link of it
    diagonal."""
    xs, ys = _xy(W, H)
    return (xs <= ys).astype(np.uint8)


def corner_antidiagonal(W, H, s=127):
    """Known up to the anti-diagonal x + y = s: for s = 127 it runs through (64,63)-(63,64)."""
    xs, ys = _xy(W, H)
    return (xs + ys <= s).astype(np.uint8)


def band(W, H, a=3, b=2, off=0, width=40):
    """A slanted band 0 <= a x - b y + off <= width: two long frontier curves that cross tile edges at changing offsets."""
    xs, ys = _xy(W, H)
    v = a * xs - b * ys + off
    return ((v >= 0) & (v <= width)).astype(np.uint8)


def three_discs(W, H):
    """The discs of the salt-map cases: three sensing discs in a row, (30, 35), (65, 35), (100, 35) of radius 20 at 130 x 70
    (with synth.salt_grid(130, 70, 0.2, seed=2): 204 frontier cells in 43 clusters, 23 of them of three cells or more)."""
    r = 2 * H // 7
    return np.array([(3 * W // 13, H // 2, r * r), (W // 2, H // 2, r * r), (10 * W // 13, H // 2, r * r)], np.int32)


# ---- the exploration loop ----
def explore_loop(occ, start, step, sense_r2=100):
    """The robot at `start` (cell) senses a disc, asks `step(occ_seen, known, pos)` for its next goal (a cell or -1), jumps
    there, senses again -- until no goal.  occ_seen = the obstacles inside the known mask.  Returns (goals visited, known).
    Every iteration reveals at least one cell (the goal touches an unknown cell, which the new disc covers), so W * H bounds
    the loop."""
    occ = np.asarray(occ)
    H, W = occ.shape
    pos = int(start)
    discs = [(pos % W, pos // W, sense_r2)]
    known = known_from_discs(None, discs, W, H)
    goals = []
    for _ in range(W * H):
        goal = int(step(np.where(known != 0, occ, 0).astype(np.uint8), known, pos))
        if goal < 0:
            return goals, known
        goals.append(goal)
        pos = goal
        known = known_from_discs(known, [(pos % W, pos // W, sense_r2)], W, H)
    raise AssertionError("exploration did not end within W * H iterations")


def true_component(occ, start):
    """The cells of start's 4-connected component of the free cells of the true map."""
    from scipy import ndimage
    lab, _ = ndimage.label(np.asarray(occ) == 0, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    return lab == lab.ravel()[start]


def twin_step(oracle, fields, Cmax=256):
    def step(occ_seen, known, pos):
        d2k = d2_known(oracle.edt(occ_seen), known)
        g = fields.field(d2k, pos)[0][None]
        return fleet_explore(d2k, known, g, Cmax=Cmax)["goal"][0]
    return step


def loop_maps():
    from sea_current_amd import synth
    return {"salt96x80": synth.salt_grid(96, 80, 0.2, seed=4), "blocks96x80": synth.block_grid(96, 80, 0.25, seed=4, smin=3, smax=16),
            "salt130x70": synth.salt_grid(130, 70, 0.35, seed=4)}


def loop_start(occ):
    """The free cell nearest the middle of the map."""
    H, W = occ.shape
    free = np.flatnonzero(occ.ravel() == 0)
    return int(free[np.argmin((free % W - W // 2) ** 2 + (free // W - H // 2) ** 2)])
