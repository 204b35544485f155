"""Helpers of the waypoint tests: the CPU twin (tests/cpp/waypoints_ref.c, compiled on demand), a brute-force Visible,
an independent restatement of the greedy shortcut, the properties every output must have, and the edge cases both the
twin and the GPU are run on."""
import ctypes as C
import os
import subprocess

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "waypoints_ref.c")
Q_OK, Q_NO_PATH, Q_TRUNCATED, Q_BAD_PATH = 0, 1, 3, 5


class Twin:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libwaypoints_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        self.lib.wr_visible.restype = i
        self.lib.wr_visible.argtypes = [vp, i, i, C.c_int32, i, i]
        self.lib.wr_path_waypoints_batch.restype = i
        self.lib.wr_path_waypoints_batch.argtypes = [vp, i, i, C.c_int32, vp, vp, vp, i, i, i, vp, vp, vp]

    def visible(self, d2, r2, a, b):
        H, W = d2.shape
        return bool(self.lib.wr_visible(d2.ctypes.data, W, H, r2, int(a), int(b)))

    def waypoints(self, d2, path, lens, status=None, r2=0, Wmax=None):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        path = np.ascontiguousarray(path, dtype=np.int32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        H, W = d2.shape
        Q, Lmax = path.shape
        Wmax = Lmax if Wmax is None else Wmax
        out = dict(wp=np.full((Q, Wmax), -1, np.int32), n=np.zeros(Q, np.int32), status=np.zeros(Q, np.int32))
        assert self.lib.wr_path_waypoints_batch(d2.ctypes.data, W, H, r2, path.ctypes.data, lens.ctypes.data,
                                                None if status is None else status.ctypes.data, Q, Lmax, Wmax, out["wp"].ctypes.data,
                                                out["n"].ctypes.data, out["status"].ctypes.data) == 0
        return out


def visible_brute(d2, r2, a, b):
    """Visible(a, b) straight from the definition: every cell box (doubled coordinates) whose bounding box overlaps the
    segment's and whose four corners do not all lie strictly on one side of the segment's line must be traversable."""
    H, W = d2.shape
    thr = max(r2, 1)
    ax, ay, bx, by = 2 * (a % W), 2 * (a // W), 2 * (b % W), 2 * (b // W)
    cy, cx = np.mgrid[0:H, 0:W]
    x0, x1, y0, y1 = 2 * cx - 1, 2 * cx + 1, 2 * cy - 1, 2 * cy + 1
    meet = (x0 <= max(ax, bx)) & (x1 >= min(ax, bx)) & (y0 <= max(ay, by)) & (y1 >= min(ay, by))
    f = [(bx - ax) * (py - ay) - (by - ay) * (px - ax) for px, py in ((x0, y0), (x0, y1), (x1, y0), (x1, y1))]
    pos = (f[0] > 0) & (f[1] > 0) & (f[2] > 0) & (f[3] > 0)
    neg = (f[0] < 0) & (f[1] < 0) & (f[2] < 0) & (f[3] < 0)
    meet &= ~pos & ~neg
    return bool(np.all(d2[meet] >= thr))


def collinear(W, a, b, w):
    """1 same direction, -1 reverse, 0 not collinear."""
    ux, uy, vx, vy = b % W - a % W, b // W - a // W, w % W - b % W, w // W - b // W
    if ux * vy - uy * vx != 0:
        return 0
    d = ux * vx + uy * vy
    return 1 if d > 0 else (-1 if d < 0 else 0)


def greedy(vis, W, p):
    """The greedy prefix shortcut with the collinear merge and the reverse rule, restated from DESIGN.md over a
    Visible predicate.  Returns (output, anchors, reverse rule fired)."""
    L = len(p)
    out, anchors, fired = [int(p[0])], [], False
    a = 0
    while a < L - 1:
        anchors.append(a)
        j = a + 1
        while j + 1 < L and vis(p[a], p[j + 1]):
            j += 1
        if len(out) >= 2:
            while j > a + 1 and collinear(W, out[-2], p[a], p[j]) < 0:
                j -= 1
                fired = True
        while len(out) >= 2 and collinear(W, out[-2], out[-1], p[j]) > 0:
            out.pop()
        out.append(int(p[j]))
        a = j
    return out, anchors, fired


def check_output(vis, W, p, wp):
    """The output guarantees: endpoints, every leg Visible, a subsequence of the path in order, and no interior point
    collinear with its neighbours (neither direction)."""
    p = [int(c) for c in p]
    wp = [int(c) for c in wp]
    assert wp[0] == p[0] and wp[-1] == p[-1]
    pos = {c: i for i, c in enumerate(p)}
    idx = [pos[c] for c in wp]
    assert all(i < j for i, j in zip(idx, idx[1:])), "waypoints out of path order"
    for u, v in zip(wp, wp[1:]):
        assert vis(u, v), (u, v)
    for a, b, c in zip(wp, wp[1:], wp[2:]):
        ux, uy, vx, vy = b % W - a % W, b // W - a // W, c % W - b % W, c // W - b // W
        assert ux * vy - uy * vx != 0, ("collinear interior waypoint", a, b, c)


def edge_cases():
    """On a 12 x 9 grid with one obstacle cell: (d2, path [Q, Lmax], len [Q], input status [Q], expected [Q] dicts of n,
    status and wp, the cells of the last case, which needs 3 waypoints)."""
    W, H, Lmax = 12, 9, 40
    occ = np.zeros((H, W), np.uint8)
    occ[4, 6] = 1                       # one obstacle cell
    # only T matters here (r2 = 0: d2 >= 1), so d2 is 0 on the obstacle and large elsewhere
    d2 = np.where(occ == 1, 0, 100).astype(np.int32)
    c = lambda x, y: y * W + x
    rows, lens, sts, exp = [], [], [], []

    def add(cells, st=Q_OK, n=None, est=None, wp=None):
        r = np.full(Lmax, -1, np.int32)
        r[:len(cells)] = cells
        rows.append(r); lens.append(len(cells)); sts.append(st)
        exp.append(dict(n=n, status=est, wp=wp))

    add([c(3, 3)], n=1, est=Q_OK, wp=[c(3, 3)])                                       # len 1
    add([c(3, 3), c(4, 4)], n=2, est=Q_OK, wp=[c(3, 3), c(4, 4)])                      # len 2
    add([c(x, 0) for x in range(W)], n=2, est=Q_OK, wp=[c(0, 0), c(W - 1, 0)])      # along the grid border: first row
    add([c(W - 1, y) for y in range(H - 1, -1, -1)], n=2, est=Q_OK, wp=[c(W - 1, H - 1), c(W - 1, 0)])   # last column
    add([c(1, 1), c(2, 2)], st=Q_NO_PATH, n=0, est=Q_NO_PATH)                         # input status passed through
    add([c(3, 3), c(5, 3)], n=0, est=Q_BAD_PATH)                                     # not adjacent
    add([c(5, 3), c(5, 4), c(5, 5)], n=2, est=Q_OK, wp=[c(5, 3), c(5, 5)])           # straight run past the obstacle's side
    add([c(5, 5), c(6, 5), c(7, 4)], n=0, est=Q_BAD_PATH)                            # (6,5)->(7,4) cuts the corner of (6,4)
    add([c(6, 4)], n=0, est=Q_BAD_PATH)                                              # len 1 on an obstacle
    add([c(3, 3), c(200, 3)], n=0, est=Q_BAD_PATH)                                   # a cell outside the grid
    # around the obstacle: (4,4) -> (8,4) must turn at (6,5); with Wmax = 2 the needed count 3 comes back with TRUNCATED
    around = [c(4, 4), c(5, 5), c(6, 5), c(7, 5), c(8, 4)]
    add(around, n=3, est=Q_OK, wp=[c(4, 4), c(6, 5), c(8, 4)])
    return d2, np.stack(rows), np.array(lens, np.int32), np.array(sts, np.int32), exp, around
