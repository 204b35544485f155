"""Checker for planning in poses, straight from the definition in include/sea_current_hip.h: the footprint mask by looping
over the offsets, the pose field as a heapq Dijkstra over the 8 W H states (for `toward` on the transposed graph, edge by
edge), the read-out by the stated rule on the toward = 0 numbering, the builder of the C statement (tests/cpp/pose_ref.c)
and the maps both are run on.  Checker only: the library never imports it."""
import ctypes as C
import heapq
import os
import subprocess

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "pose_ref.c")
INF = 2**31 - 1
Q_OK, Q_NO_PATH, Q_BAD_ENDPOINT, Q_TRUNCATED = 0, 1, 2, 3
HX = (1, 1, 0, -1, -1, -1, 0, 1)
HY = (0, 1, 1, 1, 0, -1, -1, -1)
ASTAR_MOVE = (0, 4, 2, 5, 1, 7, 3, 6)
FOOTPRINT_MAX = 32


def w_of(k):
    return 14 if k & 1 else 10


def covered(k, dx, dy, front, back, left, right):
    n = HX[k] ** 2 + HY[k] ** 2
    u, v = dx * HX[k] + dy * HY[k], -dx * HY[k] + dy * HX[k]
    return (u * u <= n * front * front if u >= 0 else u * u <= n * back * back) and \
           (v * v <= n * left * left if v >= 0 else v * v <= n * right * right)


def footprint_mask(d2, front, back, left, right, r2=0):
    """uint8 [H,W]: bit k set iff every covered offset that lands in the grid is traversable."""
    d2 = np.asarray(d2)
    H, W = d2.shape
    T = d2 >= max(r2, 1)
    out = np.zeros((H, W), np.uint8)
    R = 2 * max(front, back, left, right)
    for k in range(8):
        ok = np.ones((H, W), bool)
        for dy in range(-R, R + 1):
            if abs(dy) >= H:
                continue
            for dx in range(-R, R + 1):
                if abs(dx) >= W or not covered(k, dx, dy, front, back, left, right):
                    continue
                # cells c with c + (dx, dy) in the grid: ok &= T[c + o]
                ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
                yt, xt = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
                ok[ys, xs] &= T[yt, xt]
        out |= (ok.astype(np.uint8) << k).astype(np.uint8)
    return out


def args_ok(W, H, turn_cost, rev_cost, readout=False):
    if not (0 <= turn_cost <= 255 and -1 <= rev_cost <= 255):
        return False
    if readout and turn_cost == 0:
        return False
    return max(14 + max(rev_cost, 0), turn_cost) * (8 * W * H - 1) <= INF - 1


class Graph:
    """The pose graph of one grid."""

    def __init__(self, d2, r2, hmask, turn_cost, rev_cost):
        d2 = np.asarray(d2)
        self.H, self.W = d2.shape
        self.T = d2 >= max(r2, 1)
        hm = np.full(d2.shape, 0xFF, np.uint8) if hmask is None else np.asarray(hmask, np.uint8)
        self.V = [(self.T & (((hm >> k) & 1) != 0)) for k in range(8)]
        self.turn, self.rev = turn_cost, rev_cost

    def valid(self, x, y, k):
        return 0 <= x < self.W and 0 <= y < self.H and bool(self.V[k][y, x])

    def move(self, x, y, dx, dy):
        """A*'s rule for the move (x, y) -> (x + dx, y + dy)."""
        nx, ny = x + dx, y + dy
        if not (0 <= nx < self.W and 0 <= ny < self.H and self.T[y, x] and self.T[ny, nx]):
            return False
        return not (dx and dy) or bool(self.T[y, nx] and self.T[ny, x])

    def out_edges(self, x, y, k):
        """(x', y', k', cost) of every legal edge out of the valid pose (x, y, k)."""
        for s, c in ((1, w_of(k)), (-1, w_of(k) + self.rev)):
            if s < 0 and self.rev < 0:
                continue
            dx, dy = s * HX[k], s * HY[k]
            if self.move(x, y, dx, dy) and self.valid(x + dx, y + dy, k):
                yield x + dx, y + dy, k, c
        for kn in ((k + 1) & 7, (k + 7) & 7):
            if self.valid(x, y, kn):
                yield x, y, kn, self.turn

    def in_edges(self, x, y, k):
        """(x', y', k', cost) of every legal edge into the valid pose (x, y, k): the out-edges of the transposed graph."""
        for s, c in ((-1, w_of(k)), (1, w_of(k) + self.rev)):     # forward from c - h, reverse from c + h
            if s > 0 and self.rev < 0:
                continue
            px, py = x + s * HX[k], y + s * HY[k]
            if self.valid(px, py, k) and self.move(px, py, -s * HX[k], -s * HY[k]):
                yield px, py, k, c
        for kn in ((k + 1) & 7, (k + 7) & 7):
            if self.valid(x, y, kn):
                yield x, y, kn, self.turn

    def legal_edge(self, a, b):
        """The cost of the legal edge a -> b, or None."""
        for x, y, k, c in self.out_edges(*a):
            if (x, y, k) == b:
                return c
        return None


def seeds_of(gr, root, rhead):
    n = gr.W * gr.H
    if not (0 <= root < n and -1 <= rhead <= 7):
        return []
    x, y = root % gr.W, root // gr.W
    return [(x, y, k) for k in range(8) if (rhead == k or rhead == -1) and gr.valid(x, y, k)]


def pose_field(d2, root, rhead, turn_cost, rev_cost=-1, toward=False, r2=0, hmask=None):
    """(gp int32 [8,H,W], status) by Dijkstra; toward: on the transposed graph."""
    gr = Graph(d2, r2, hmask, turn_cost, rev_cost)
    assert args_ok(gr.W, gr.H, turn_cost, rev_cost)
    gp = np.full((8, gr.H, gr.W), INF, np.int64)
    seeds = seeds_of(gr, root, rhead)
    if not seeds:
        return gp.astype(np.int32), Q_BAD_ENDPOINT
    heap = []
    for x, y, k in seeds:
        gp[k, y, x] = 0
        heap.append((0, x, y, k))
    edges = gr.in_edges if toward else gr.out_edges
    while heap:
        g, x, y, k = heapq.heappop(heap)
        if g > gp[k, y, x]:
            continue
        for nx, ny, nk, c in edges(x, y, k):
            if g + c < gp[nk, ny, nx]:
                gp[nk, ny, nx] = g + c
                heapq.heappush(heap, (g + c, nx, ny, nk))
    return gp.astype(np.int32), Q_OK


def rot4(hmask):
    """The mask with its bits renamed k -> k + 4."""
    if hmask is None:
        return None
    hm = np.asarray(hmask, np.uint8)
    return ((hm << 4) | (hm >> 4)).astype(np.uint8)


def pose_field_by_identity(d2, root, rhead, turn_cost, rev_cost=-1, r2=0, hmask=None):
    """The toward field as the header defines it: the toward = 0 field of root heading rhead + 4, layers renamed k -> k + 4."""
    rh = rhead if rhead < 0 or rhead > 7 else (rhead + 4) & 7
    gp, st = pose_field(d2, root, rh, turn_cost, rev_cost, False, r2, rot4(hmask))
    return np.ascontiguousarray(np.roll(gp, 4, axis=0)), st


def pose_path(d2, gp, root, rhead, target, thead, turn_cost, rev_cost=-1, toward=False, r2=0, hmask=None, Lmax=4096, to_root=False,
              cells_only=False):
    """One read-out: (path list, head list, len, cost, status).  Truncated: the lists are empty (unspecified in the library)."""
    gp = np.asarray(gp)
    H, W = gp.shape[1:]
    assert args_ok(W, H, turn_cost, rev_cost, readout=True)
    n = W * H
    bad, nopath = ([], [], 0, -1, Q_BAD_ENDPOINT), ([], [], 0, -1, Q_NO_PATH)
    if not (0 <= root < n and -1 <= rhead <= 7 and 0 <= target < n and -1 <= thead <= 7):
        return bad
    auto = thead == -1
    if auto:             # the cheapest heading, smallest k of the caller's numbering
        if np.asarray(d2)[target // W, target % W] < max(r2, 1):
            return bad
        thead = int(np.argmin(gp[:, target // W, target % W]))
    if toward:           # rename to the toward = 0 numbering
        gp, hmask = np.roll(gp, 4, axis=0), rot4(hmask)
        rhead = rhead if rhead < 0 else (rhead + 4) & 7
        thead = (thead + 4) & 7
    gr = Graph(d2, r2, hmask, turn_cost, rev_cost)
    seeds = seeds_of(gr, root, rhead)
    tx, ty = target % W, target // W
    if not seeds or not (auto or gr.valid(tx, ty, thead)):
        return bad
    cost = int(gp[thead, ty, tx])
    if cost >= INF:
        return nopath
    walk = [(tx, ty, thead)]
    x, y, k, v = tx, ty, thead, cost
    while v > 0:
        cands = [(x - HX[k], y - HY[k], k)]
        if rev_cost >= 0:
            cands.append((x + HX[k], y + HY[k], k))
        cands += [(x, y, (k + 7) & 7), (x, y, (k + 1) & 7)]
        for px, py, pk in cands:
            if not gr.valid(px, py, pk):
                continue
            c = gr.legal_edge((px, py, pk), (x, y, k))
            if c is not None and gp[pk, py, px] < INF and int(gp[pk, py, px]) + c == v:
                x, y, k, v = px, py, pk, v - c
                break
        else:
            return nopath
        walk.append((x, y, k))
        if len(walk) > 8 * n:
            return nopath
    states = walk if to_root else walk[::-1]
    cells, heads = [], []
    for sx, sy, sk in states:
        c = sy * W + sx
        if cells_only and cells and cells[-1] == c:
            continue
        cells.append(c)
        heads.append((sk + 4) & 7 if toward else sk)
    if len(cells) > Lmax:
        return [], [], len(cells), cost, Q_TRUNCATED
    return cells, heads, len(cells), cost, Q_OK


def pose_paths(d2, gp, root, rhead, targets, thead, turn_cost, rev_cost=-1, toward=False, r2=0, hmask=None, Lmax=4096, to_root=False,
               cells_only=False):
    """The read-outs of one field as the library lays them out (path -1 and head 0 past len; truncated: nothing written)."""
    Q = len(targets)
    out = dict(path=np.full((Q, Lmax), -1, np.int32), head=np.zeros((Q, Lmax), np.uint8), len=np.zeros(Q, np.int32),
               cost=np.zeros(Q, np.int32), status=np.zeros(Q, np.int32))
    for q in range(Q):
        p, h, out["len"][q], out["cost"][q], out["status"][q] = pose_path(d2, gp, root, rhead, int(targets[q]), int(thead[q]), turn_cost,
                                                                          rev_cost, toward, r2, hmask, Lmax, to_root, cells_only)
        out["path"][q, :len(p)] = p
        out["head"][q, :len(h)] = h
    return out


class Ref:
    """The C statement, compiled on demand."""

    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libpose_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        self.lib.px_args_ok.restype = i
        self.lib.px_args_ok.argtypes = [i, i, i, i, i]
        self.lib.px_footprint_mask.restype = i
        self.lib.px_footprint_mask.argtypes = [vp, i, i, C.c_int32, i, i, i, i, vp]
        self.lib.px_pose_field.restype = i
        self.lib.px_pose_field.argtypes = [vp, vp, i, i, C.c_int32, i, i, i, i, i, vp]
        self.lib.px_pose_paths.restype = i
        self.lib.px_pose_paths.argtypes = [vp, vp, i, i, C.c_int32, i, i, i, vp, i, i, vp, vp, i, i, i, i, vp, vp, vp, vp, vp]

    def args_ok(self, W, H, turn_cost, rev_cost, readout=False):
        return bool(self.lib.px_args_ok(W, H, turn_cost, rev_cost, int(readout)))

    def footprint_mask(self, d2, front, back, left, right, r2=0):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        H, W = d2.shape
        out = np.empty((H, W), np.uint8)
        st = self.lib.px_footprint_mask(d2.ctypes.data, W, H, r2, front, back, left, right, out.ctypes.data)
        assert st == 0
        return out

    def pose_field(self, d2, root, rhead, turn_cost, rev_cost=-1, toward=False, r2=0, hmask=None):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        hm = None if hmask is None else np.ascontiguousarray(hmask, dtype=np.uint8)
        H, W = d2.shape
        gp = np.empty((8, H, W), np.int32)
        st = self.lib.px_pose_field(d2.ctypes.data, None if hm is None else hm.ctypes.data, W, H, r2, turn_cost, rev_cost, int(bool(toward)),
                                    int(root), int(rhead), gp.ctypes.data)
        assert st >= 0
        return gp, st

    def pose_paths(self, d2, gp, root, rhead, targets, thead, turn_cost, rev_cost=-1, toward=False, r2=0, hmask=None, Lmax=4096,
                   to_root=False, cells_only=False):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        gp = np.ascontiguousarray(gp, dtype=np.int32)
        hm = None if hmask is None else np.ascontiguousarray(hmask, dtype=np.uint8)
        targets, thead = np.ascontiguousarray(targets, dtype=np.int32), np.ascontiguousarray(thead, dtype=np.int32)
        H, W = d2.shape
        Q = len(targets)
        out = dict(path=np.full((Q, Lmax), -1, np.int32), head=np.zeros((Q, Lmax), np.uint8), len=np.zeros(Q, np.int32),
                   cost=np.zeros(Q, np.int32), status=np.zeros(Q, np.int32))
        st = self.lib.px_pose_paths(d2.ctypes.data, None if hm is None else hm.ctypes.data, W, H, r2, turn_cost, rev_cost, int(bool(toward)),
                                    gp.ctypes.data, int(root), int(rhead), targets.ctypes.data, thead.ctypes.data, Q, Lmax, int(bool(to_root)),
                                    int(bool(cells_only)), out["path"].ctypes.data, out["head"].ctypes.data, out["len"].ctypes.data,
                                    out["cost"].ctypes.data, out["status"].ctypes.data)
        assert st == 0
        return out


def same_readout(a, b):
    """Every output of two read-outs is equal; the entries of a path up to len where it is SC_Q_OK (past it, and truncated,
    they are unspecified)."""
    for key in ("len", "cost", "status"):
        if not np.array_equal(np.asarray(a[key]), np.asarray(b[key])):
            return False
    for q in range(len(a["len"])):
        if a["status"][q] == Q_OK:
            L = int(a["len"][q])
            if not (np.array_equal(a["path"][q, :L], b["path"][q, :L]) and np.array_equal(a["head"][q, :L], b["head"][q, :L])):
                return False
    return True


# ---- maps ----
def d2_of(occ):
    """A d2 stand-in: 0 on obstacles, 1 elsewhere."""
    return np.where(np.asarray(occ) != 0, 0, 1).astype(np.int32)


def salt(W, H, p, seed):
    from sea_current_amd import synth
    return synth.salt_grid(W, H, p, seed=seed)


def blocks(W=130, H=70, seed=10):
    from sea_current_amd import synth
    return synth.block_grid(W, H, 0.3, seed=seed, smin=3, smax=12)


def door_map(W=40, H=24, wall=(19, 21), door=(10, 12)):
    """Two rooms: a wall over columns wall[0] .. wall[1] with a door in rows door[0] .. door[1] (3 cells wide).  The wall is
    three cells thick, so that a long body cannot slip through at a diagonal heading either."""
    occ = np.zeros((H, W), np.uint8)
    occ[:, wall[0]:wall[1] + 1] = 1
    occ[door[0]:door[1] + 1, wall[0]:wall[1] + 1] = 0
    return occ


def turn_map():
    """13 x 12 (W x H): a one-cell staircase from (1, 1) to (9, 9) (16 moves, a quarter turn after almost every one; its
    diagonals are cut by the blocked side cells) and a corridor round it: along row 1, down column 11, back along row 9 (20
    moves, two quarter turns)."""
    occ = np.ones((12, 13), np.uint8)
    for k in range(1, 9):
        occ[k, k] = occ[k, k + 1] = 0
    occ[9, 9] = 0
    occ[1, 1:12] = 0
    occ[1:10, 11] = 0
    occ[9, 9:12] = 0
    return occ


def free_cells(d2, count, seed, r2=0):
    rng = np.random.default_rng(seed)
    free = np.flatnonzero(np.asarray(d2).ravel() >= max(r2, 1))
    return rng.choice(free, size=min(count, len(free)), replace=False).astype(np.int32)
