"""Helpers of the weighted cost-field tests: the CPU twin (tests/cpp/field_w_ref.c, compiled on demand), the penalty
formula in NumPy, scipy's Dijkstra over the weighted graph and the wall map both the CPU and the GPU tests use."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from field_twin import INF

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "field_w_ref.c")


class TwinW:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libfield_w_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        self.lib.fw_cost_field.restype = i
        self.lib.fw_cost_field.argtypes = [vp, vp, i, i, i, C.c_int32, i, vp]
        self.lib.fw_field_paths.restype = None
        self.lib.fw_field_paths.argtypes = [vp, vp, i, i, i, C.c_int32, vp, i, vp, i, i, i, vp, vp, vp, vp]

    def field(self, d2, pen, root, r2=0, cap=255):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        pen = np.ascontiguousarray(pen, dtype=np.uint8)
        assert pen.shape == d2.shape
        H, W = d2.shape
        g = np.empty((H, W), np.int32)
        st = self.lib.fw_cost_field(d2.ctypes.data, pen.ctypes.data, int(cap), W, H, r2, int(root), g.ctypes.data)
        return g, st

    def paths(self, d2, pen, g, root, targets, r2=0, cap=255, Lmax=4096, to_root=False):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        pen = np.ascontiguousarray(pen, dtype=np.uint8)
        g = np.ascontiguousarray(g, dtype=np.int32)
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        H, W = d2.shape
        Q = targets.shape[0]
        out = dict(path=np.full((Q, Lmax), -1, np.int32), len=np.zeros(Q, np.int32), cost=np.zeros(Q, np.int32),
                   status=np.zeros(Q, np.int32))
        self.lib.fw_field_paths(d2.ctypes.data, pen.ctypes.data, int(cap), W, H, r2, g.ctypes.data, int(root), targets.ctypes.data, Q,
                                Lmax, int(bool(to_root)), out["path"].ctypes.data, out["len"].ctypes.data, out["cost"].ctypes.data,
                                out["status"].ctypes.data)
        return out


def penalty_numpy(d2, r2_clear, r2_soft, pen_max):
    """sc_clearance_penalty_u8 stated in integers: math.isqrt is the exact floor square root."""
    d2 = np.asarray(d2)
    thr = max(int(r2_clear), 1)
    s10 = math.isqrt(100 * int(r2_soft))
    table = {}
    out = np.zeros(d2.shape, np.uint8)
    flat, o = d2.ravel(), out.ravel()
    for i in np.flatnonzero((flat >= thr) & (flat < r2_soft)):
        v = int(flat[i])
        if v not in table:
            table[v] = (int(pen_max) * (s10 - math.isqrt(100 * v))) // s10
        o[i] = table[v]
    return out


def field_w_scipy(d2, pen, root, r2=0, cap=255):
    """g of one root from scipy's Dijkstra over the weighted graph (integer weights far below 2^53: exact)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    d2 = np.asarray(d2)
    pc = np.minimum(np.asarray(pen).astype(np.int64), int(cap))
    H, W = d2.shape
    T = d2 >= max(r2, 1)
    n = W * H
    rows, cols, wts = [], [], []
    ys, xs = np.mgrid[0:H, 0:W]
    for d, (dx, dy) in enumerate(zip((1, -1, 0, 0, 1, -1, 1, -1), (0, 0, 1, -1, 1, 1, -1, -1))):
        nx, ny = xs + dx, ys + dy
        ok = (nx >= 0) & (ny >= 0) & (nx < W) & (ny < H)
        nxc, nyc = np.clip(nx, 0, W - 1), np.clip(ny, 0, H - 1)
        ok &= T & T[nyc, nxc]
        if d >= 4:
            ok &= T[ys, nxc] & T[nyc, xs]
        rows.append((ys * W + xs)[ok])
        cols.append((nyc * W + nxc)[ok])
        wts.append(((10 if d < 4 else 14) + pc[nyc, nxc])[ok].astype(np.float64))
    A = csr_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    g = np.full(n, INF, np.int64)
    if 0 <= root < n and T.flat[root]:
        dist = dijkstra(A, directed=True, indices=int(root))
        fin = np.isfinite(dist)
        g[fin] = dist[fin].astype(np.int64)
    return g.reshape(H, W).astype(np.int32)


def path_weighted_cost(path, pen, cap=255):
    """Cost of a cell path (root first) in the weighted graph: 10 / 14 per step plus the capped penalty of every cell entered."""
    W = pen.shape[1]
    p = np.asarray(path, np.int64)
    dx, dy = np.abs(np.diff(p % W)), np.abs(np.diff(p // W))
    assert ((dx <= 1) & (dy <= 1) & (dx + dy >= 1)).all()
    return int(np.where(dx + dy == 2, 14, 10).sum() + np.minimum(pen.ravel()[p[1:]].astype(np.int64), cap).sum())


def wall_map():
    """130 x 70, a wall in columns 64..65 of rows 0..49; root cell (5, 10), target cell (124, 10)."""
    occ = np.zeros((70, 130), np.uint8)
    occ[0:50, 64:66] = 1
    return occ, 10 * 130 + 5, 10 * 130 + 124
