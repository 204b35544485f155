"""Checker for car-like pose planning, straight from the definition in include/sea_current_hip_car.h: the arc mask by walking
the 2n steps, the car field as a heapq Dijkstra over the 8 W H states (toward: over the edges INTO a state, edge by edge, no
renaming), the read-out by the stated rule, the builder of the C statement (tests/cpp/car_ref.c) and the maps both are run
on.  Checker only: the library never imports it."""
import ctypes as C
import heapq
import os
import subprocess

import numpy as np

from pose_twin import HX, HY, INF, Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED, w_of
from pose_twin import blocks, d2_of, door_map, free_cells, salt  # noqa: F401  (the maps the tests share)

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "car_ref.c")
ARC_MAX = 4


def arc_edge_cost(arc_n, arc_cost, rev_cost, reverse):
    return 24 * arc_n + arc_cost + (2 * arc_n * rev_cost if reverse else 0)


def args_ok(W, H, arc_n, arc_cost, rev_cost):
    if not (1 <= arc_n <= ARC_MAX and 0 <= arc_cost <= 255 and -1 <= rev_cost <= 255):
        return False
    return (24 * arc_n + arc_cost + 2 * arc_n * max(rev_cost, 0)) * (8 * W * H - 1) <= INF - 1


def arc_cells(x, y, k, s, n):
    """(the 2n + 1 cells p_0 .. p_2n of A((x, y), k, s), k')."""
    kn = (k + s) & 7
    cells = [(x + i * HX[k], y + i * HY[k]) for i in range(n + 1)]
    px, py = cells[-1]
    cells += [(px + j * HX[kn], py + j * HY[kn]) for j in range(1, n + 1)]
    return cells, kn


class Graph:
    """The car graph of one grid."""

    def __init__(self, d2, r2, hmask, arc_n, arc_cost, rev_cost):
        d2 = np.asarray(d2)
        self.H, self.W = d2.shape
        self.T = d2 >= max(r2, 1)
        hm = np.full(d2.shape, 0xFF, np.uint8) if hmask is None else np.asarray(hmask, np.uint8)
        self.V = [(self.T & (((hm >> k) & 1) != 0)) for k in range(8)]
        self.n, self.rev = arc_n, rev_cost
        self.ca, self.cr = arc_edge_cost(arc_n, arc_cost, rev_cost, False), arc_edge_cost(arc_n, arc_cost, rev_cost, True)

    def valid(self, x, y, k):
        return 0 <= x < self.W and 0 <= y < self.H and bool(self.V[k][y, x])

    def move(self, x, y, dx, dy):
        """A*'s rule for the move (x, y) -> (x + dx, y + dy)."""
        nx, ny = x + dx, y + dy
        if not (0 <= x < self.W and 0 <= y < self.H and 0 <= nx < self.W and 0 <= ny < self.H and self.T[y, x] and self.T[ny, nx]):
            return False
        return not (dx and dy) or bool(self.T[y, nx] and self.T[ny, x])

    def arc(self, x, y, k, s):
        """The end pose (x', y', k') of A((x, y), k, s) where it is legal, else None."""
        cells, kn = arc_cells(x, y, k, s, self.n)
        n = self.n
        for i in range(2 * n):
            (ax, ay), (bx, by) = cells[i], cells[i + 1]
            if not self.move(ax, ay, bx - ax, by - ay):
                return None
        if not all(self.valid(cx, cy, k) for cx, cy in cells[:n + 1]):
            return None
        if not all(self.valid(cx, cy, kn) for cx, cy in cells[n:]):
            return None
        return cells[-1] + (kn,)

    def out_edges(self, x, y, k):
        """(kind, x', y', k', cost) of every legal edge out of the valid pose (x, y, k), in the order of the definition."""
        n = self.n
        if self.move(x, y, HX[k], HY[k]) and self.valid(x + HX[k], y + HY[k], k):
            yield 1, x + HX[k], y + HY[k], k, w_of(k)
        if self.rev >= 0 and self.move(x, y, -HX[k], -HY[k]) and self.valid(x - HX[k], y - HY[k], k):
            yield 2, x - HX[k], y - HY[k], k, w_of(k) + self.rev
        for kind, s in ((3, 1), (4, -1)):
            end = self.arc(x, y, k, s)
            if end is not None:
                yield (kind,) + end + (self.ca,)
        if self.rev >= 0:
            for kind, s in ((5, 1), (6, -1)):      # the arcs of sense s that end in (x, y, k) started at heading k - s
                j = (k - s) & 7
                sx, sy = x - n * HX[k] - n * HX[j], y - n * HY[k] - n * HY[j]
                if self.arc(sx, sy, j, s) == (x, y, k):
                    yield kind, sx, sy, j, self.cr

    def in_edges(self, x, y, k):
        """(kind, x', y', k', cost) of every legal edge (x', y', k') -> (x, y, k), in the order of the definition."""
        n = self.n
        if self.valid(x, y, k) and self.valid(x - HX[k], y - HY[k], k) and self.move(x - HX[k], y - HY[k], HX[k], HY[k]):
            yield 1, x - HX[k], y - HY[k], k, w_of(k)
        if self.rev >= 0 and self.valid(x, y, k) and self.valid(x + HX[k], y + HY[k], k) and self.move(x + HX[k], y + HY[k], -HX[k], -HY[k]):
            yield 2, x + HX[k], y + HY[k], k, w_of(k) + self.rev
        for kind, s in ((3, 1), (4, -1)):          # a forward arc from (c', k - s) that ends here
            j = (k - s) & 7
            sx, sy = x - n * HX[k] - n * HX[j], y - n * HY[k] - n * HY[j]
            if self.arc(sx, sy, j, s) == (x, y, k):
                yield kind, sx, sy, j, self.ca
        if self.rev >= 0:
            for kind, s in ((5, 1), (6, -1)):      # the reverse arc that undoes A((x, y), k, s) leaves that arc's end
                end = self.arc(x, y, k, s)
                if end is not None:
                    yield (kind,) + end + (self.cr,)

    def legal_edge(self, a, b):
        """The cost of the cheapest legal edge a -> b, or None."""
        costs = [c for _, x, y, k, c in self.out_edges(*a) if (x, y, k) == b] if self.valid(*a) else []
        return min(costs) if costs else None


def arc_mask(d2, arc_n, r2=0, hmask=None):
    """uint16 [H,W]: bit 2k + (s < 0) set iff A(c, k, s) is legal."""
    gr = Graph(d2, r2, hmask, arc_n, 0, -1)
    out = np.zeros((gr.H, gr.W), np.uint16)
    for y in range(gr.H):
        for x in range(gr.W):
            if not gr.T[y, x]:
                continue
            m = 0
            for k in range(8):
                for si, s in enumerate((1, -1)):
                    if gr.arc(x, y, k, s) is not None:
                        m |= 1 << (2 * k + si)
            out[y, x] = m
    return out


def seeds_of(gr, root, rhead):
    n = gr.W * gr.H
    if not (0 <= root < n and -1 <= rhead <= 7):
        return []
    x, y = root % gr.W, root // gr.W
    return [(x, y, k) for k in range(8) if (rhead == k or rhead == -1) and gr.valid(x, y, k)]


def car_field(d2, root, rhead, arc_n, arc_cost, rev_cost=-1, toward=False, r2=0, hmask=None):
    """(gp int32 [8,H,W], status) by Dijkstra; toward: over the edges into a state."""
    gr = Graph(d2, r2, hmask, arc_n, arc_cost, rev_cost)
    assert args_ok(gr.W, gr.H, arc_n, arc_cost, rev_cost)
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
        for _, nx, ny, nk, c in edges(x, y, k):
            if g + c < gp[nk, ny, nx]:
                gp[nk, ny, nx] = g + c
                heapq.heappush(heap, (g + c, nx, ny, nk))
    return gp.astype(np.int32), Q_OK


def readout_candidates(gr, amask, x, y, k, toward):
    """The six candidates of a read-out step from (x, y, k), in order: (kind, far end, cost, legal, the 2n - 1 (cell, heading)
    entries between the two poses in walk order).  Straight moves are judged from d2 and hmask, arcs from amask with every
    index bounds-checked."""
    n, W, H = gr.n, gr.W, gr.H

    def bit(cx, cy, b):
        return 0 <= cx < W and 0 <= cy < H and bool((int(amask[cy, cx]) >> b) & 1)

    def between(cells, ka, kb, forward_driven):
        heads = [ka if (i < n or (i == n and forward_driven)) else kb for i in range(2 * n + 1)]
        return list(zip(cells, heads))[1:-1]

    out = []
    sg = -1 if toward else 1                       # toward = 0 walks against the edges, toward = 1 along them
    fx, fy = x - sg * HX[k], y - sg * HY[k]
    a, b = ((x, y, k), (fx, fy, k)) if toward else ((fx, fy, k), (x, y, k))
    out.append((1, (fx, fy, k), w_of(k), gr.valid(*a) and gr.valid(*b) and gr.move(a[0], a[1], b[0] - a[0], b[1] - a[1]), []))
    fx, fy = x + sg * HX[k], y + sg * HY[k]
    a, b = ((x, y, k), (fx, fy, k)) if toward else ((fx, fy, k), (x, y, k))
    out.append((2, (fx, fy, k), w_of(k) + gr.rev,
                gr.rev >= 0 and gr.valid(*a) and gr.valid(*b) and gr.move(a[0], a[1], b[0] - a[0], b[1] - a[1]), []))
    for kind, s in ((3, 1), (4, -1), (5, 1), (6, -1)):
        fwd = kind < 5
        # does the forward arc that the edge drives or undoes start at this state?  in-edges (toward = 0): kinds 5, 6;
        # out-edges (toward = 1): kinds 3, 4
        if fwd == bool(toward):
            cells, kn = arc_cells(x, y, k, s, n)
            legal = bit(x, y, 2 * k + (s < 0))
            far = cells[-1] + (kn,)
            mid = between(cells, k, kn, fwd)
        else:
            j = (k - s) & 7
            sx, sy = x - n * HX[k] - n * HX[j], y - n * HY[k] - n * HY[j]
            cells, kn = arc_cells(sx, sy, j, s, n)
            assert kn == k and cells[-1] == (x, y)
            legal = bit(sx, sy, 2 * j + (s < 0))
            far = (sx, sy, j)
            mid = between(cells, j, k, fwd)[::-1]
        legal = legal and (fwd or gr.rev >= 0) and 0 <= far[0] < W and 0 <= far[1] < H
        out.append((kind, far, gr.ca if fwd else gr.cr, legal, mid))
    return out


def car_path(d2, amask, gp, root, rhead, target, thead, arc_n, arc_cost, rev_cost=-1, toward=False, r2=0, hmask=None, Lmax=4096,
             to_root=False, kinds=None):
    """One read-out: (path list, head list, len, cost, status).  Truncated: the lists are empty (unspecified in the library).
    kinds (a list) receives (kind, near state, far state, cost) of every step."""
    gp = np.asarray(gp)
    H, W = gp.shape[1:]
    assert args_ok(W, H, arc_n, arc_cost, rev_cost)
    n = W * H
    bad, nopath = ([], [], 0, -1, Q_BAD_ENDPOINT), ([], [], 0, -1, Q_NO_PATH)
    if not (0 <= root < n and -1 <= rhead <= 7 and 0 <= target < n and -1 <= thead <= 7):
        return bad
    gr = Graph(d2, r2, hmask, arc_n, arc_cost, rev_cost)
    tx, ty = target % W, target // W
    if not seeds_of(gr, root, rhead):
        return bad
    if thead == -1:      # the cheapest heading, smallest k
        if not gr.T[ty, tx]:
            return bad
        thead = int(np.argmin(gp[:, ty, tx]))
    elif not gr.valid(tx, ty, thead):
        return bad
    cost = int(gp[thead, ty, tx])
    if cost >= INF:
        return nopath
    entries = [((tx, ty), thead)]
    x, y, k, v = tx, ty, thead, cost
    steps = 0
    while v > 0:
        for kind, far, c, legal, mid in readout_candidates(gr, amask, x, y, k, toward):
            if legal and gp[far[2], far[1], far[0]] < INF and int(gp[far[2], far[1], far[0]]) + c == v:
                if kinds is not None:
                    kinds.append((kind, (x, y, k), far, c))
                entries += mid
                entries.append(((far[0], far[1]), far[2]))
                x, y, k, v = far[0], far[1], far[2], v - c
                break
        else:
            return nopath
        steps += 1
        if steps > 8 * n:
            return nopath
    if not to_root:
        entries = entries[::-1]
    if len(entries) > Lmax:
        return [], [], len(entries), cost, Q_TRUNCATED
    return [cy * W + cx for (cx, cy), _ in entries], [h for _, h in entries], len(entries), cost, Q_OK


def car_paths(d2, amask, gp, root, rhead, targets, thead, arc_n, arc_cost, rev_cost=-1, toward=False, r2=0, hmask=None, Lmax=4096,
              to_root=False):
    """The read-outs of one field as the library lays them out (path -1 and head 0 past len; truncated: nothing written)."""
    Q = len(targets)
    out = dict(path=np.full((Q, Lmax), -1, np.int32), head=np.zeros((Q, Lmax), np.uint8), len=np.zeros(Q, np.int32),
               cost=np.zeros(Q, np.int32), status=np.zeros(Q, np.int32))
    for q in range(Q):
        p, h, out["len"][q], out["cost"][q], out["status"][q] = car_path(d2, amask, gp, root, rhead, int(targets[q]), int(thead[q]), arc_n,
                                                                         arc_cost, rev_cost, toward, r2, hmask, Lmax, to_root)
        out["path"][q, :len(p)] = p
        out["head"][q, :len(h)] = h
    return out


class Ref:
    """The C statement, compiled on demand."""

    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libcar_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        self.lib.cx_args_ok.restype = i
        self.lib.cx_args_ok.argtypes = [i, i, i, i, i]
        self.lib.cx_arc_mask.restype = i
        self.lib.cx_arc_mask.argtypes = [vp, vp, i, i, C.c_int32, i, vp]
        self.lib.cx_car_field.restype = i
        self.lib.cx_car_field.argtypes = [vp, vp, i, i, C.c_int32, i, i, i, i, i, i, vp]
        self.lib.cx_car_paths.restype = i
        self.lib.cx_car_paths.argtypes = [vp, vp, vp, i, i, C.c_int32, i, i, i, i, vp, i, i, vp, vp, i, i, i, vp, vp, vp, vp, vp]

    def args_ok(self, W, H, arc_n, arc_cost, rev_cost):
        return bool(self.lib.cx_args_ok(W, H, arc_n, arc_cost, rev_cost))

    def arc_mask(self, d2, arc_n, r2=0, hmask=None):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        hm = None if hmask is None else np.ascontiguousarray(hmask, dtype=np.uint8)
        H, W = d2.shape
        out = np.empty((H, W), np.uint16)
        st = self.lib.cx_arc_mask(d2.ctypes.data, None if hm is None else hm.ctypes.data, W, H, r2, arc_n, out.ctypes.data)
        assert st == 0
        return out

    def car_field(self, d2, root, rhead, arc_n, arc_cost, rev_cost=-1, toward=False, r2=0, hmask=None):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        hm = None if hmask is None else np.ascontiguousarray(hmask, dtype=np.uint8)
        H, W = d2.shape
        gp = np.empty((8, H, W), np.int32)
        st = self.lib.cx_car_field(d2.ctypes.data, None if hm is None else hm.ctypes.data, W, H, r2, arc_n, arc_cost, rev_cost,
                                   int(bool(toward)), int(root), int(rhead), gp.ctypes.data)
        assert st >= 0
        return gp, st

    def car_paths(self, d2, amask, gp, root, rhead, targets, thead, arc_n, arc_cost, rev_cost=-1, toward=False, r2=0, hmask=None,
                  Lmax=4096, to_root=False):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        am = np.ascontiguousarray(amask, dtype=np.uint16)
        gp = np.ascontiguousarray(gp, dtype=np.int32)
        hm = None if hmask is None else np.ascontiguousarray(hmask, dtype=np.uint8)
        targets, thead = np.ascontiguousarray(targets, dtype=np.int32), np.ascontiguousarray(thead, dtype=np.int32)
        H, W = d2.shape
        Q = len(targets)
        out = dict(path=np.full((Q, Lmax), -1, np.int32), head=np.zeros((Q, Lmax), np.uint8), len=np.zeros(Q, np.int32),
                   cost=np.zeros(Q, np.int32), status=np.zeros(Q, np.int32))
        st = self.lib.cx_car_paths(d2.ctypes.data, None if hm is None else hm.ctypes.data, am.ctypes.data, W, H, r2, arc_n, arc_cost,
                                   rev_cost, int(bool(toward)), gp.ctypes.data, int(root), int(rhead), targets.ctypes.data,
                                   thead.ctypes.data, Q, Lmax, int(bool(to_root)), out["path"].ctypes.data, out["head"].ctypes.data,
                                   out["len"].ctypes.data, out["cost"].ctypes.data, out["status"].ctypes.data)
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
def dead_end(W=30, H=9, width=3):
    """A corridor of `width` rows, closed at its right end and open into a room on the left."""
    occ = np.ones((H, W), np.uint8)
    occ[:, :8] = 0
    y0 = (H - width) // 2
    occ[y0:y0 + width, 8:W - 1] = 0
    return occ


def corridor(w, arc_len=40):
    """The issue's anchor map: (w + 2) x 42 (H x W); rows 1 .. w and columns 1 .. 40 are traversable."""
    occ = np.ones((w + 2, arc_len + 2), np.uint8)
    occ[1:w + 1, 1:arc_len + 1] = 0
    return occ

