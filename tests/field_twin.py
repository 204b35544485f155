"""Helpers of the cost-field tests: the CPU twin (tests/cpp/field_ref.c, compiled on demand) and the maps both the twin
and the GPU are run on."""
import ctypes as C
import os
import subprocess

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "field_ref.c")
INF = 2**31 - 1
Q_OK, Q_NO_PATH, Q_BAD_ENDPOINT, Q_TRUNCATED = 0, 1, 2, 3


class Twin:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libfield_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        self.lib.fr_cost_field.restype = i
        self.lib.fr_cost_field.argtypes = [vp, i, i, C.c_int32, i, vp]
        self.lib.fr_field_paths.restype = None
        self.lib.fr_field_paths.argtypes = [vp, i, i, C.c_int32, vp, i, vp, i, i, i, vp, vp, vp, vp]

    def field(self, d2, root, r2=0):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        H, W = d2.shape
        g = np.empty((H, W), np.int32)
        st = self.lib.fr_cost_field(d2.ctypes.data, W, H, r2, int(root), g.ctypes.data)
        return g, st

    def paths(self, d2, g, root, targets, r2=0, Lmax=4096, to_root=False):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        g = np.ascontiguousarray(g, dtype=np.int32)
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        H, W = d2.shape
        Q = targets.shape[0]
        out = dict(path=np.full((Q, Lmax), -1, np.int32), len=np.zeros(Q, np.int32), cost=np.zeros(Q, np.int32),
                   status=np.zeros(Q, np.int32))
        self.lib.fr_field_paths(d2.ctypes.data, W, H, r2, g.ctypes.data, int(root), targets.ctypes.data, Q, Lmax, int(bool(to_root)),
                                out["path"].ctypes.data, out["len"].ctypes.data, out["cost"].ctypes.data, out["status"].ctypes.data)
        return out


def d2_of(occ):
    """A d2 stand-in for tests that only need traversability: 0 on obstacles, 1 elsewhere."""
    return np.where(np.asarray(occ) != 0, 0, 1).astype(np.int32)


def serpentine(n, wall=2, gap=2):
    """Horizontal walls every (wall + gap) rows, open at alternating ends: one corridor that winds through the map."""
    occ = np.zeros((n, n), np.uint8)
    k = 0
    for y in range(gap, n - 1, wall + gap):
        occ[y:y + wall, :] = 1
        if k % 2 == 0:
            occ[y:y + wall, n - gap:] = 0
        else:
            occ[y:y + wall, :gap] = 0
        k += 1
    return occ


def spiral(n, gap=2):
    """Concentric square walls, each with one opening, on alternate corners: the way from the centre to the border winds
    around every ring."""
    occ = np.zeros((n, n), np.uint8)
    lo, k = gap, 0
    while n - 1 - 2 * lo > 2 * gap:
        hi = n - 1 - lo
        occ[lo, lo:hi + 1] = 1
        occ[hi, lo:hi + 1] = 1
        occ[lo:hi + 1, lo] = 1
        occ[lo:hi + 1, hi] = 1
        if k % 2 == 0:
            occ[lo, lo + 1:lo + 1 + gap] = 0
        else:
            occ[hi, hi - gap:hi] = 0
        lo += gap + 1
        k += 1
    return occ


def field_scipy(d2, root, r2=0):
    """g of one root straight from scipy's Dijkstra over the same graph (integer weights, exact)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    d2 = np.asarray(d2)
    H, W = d2.shape
    thr = max(r2, 1)
    T = d2 >= thr
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
        wts.append(np.full(int(ok.sum()), 10 if d < 4 else 14, np.float64))
    A = csr_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    g = np.full(n, INF, np.int64)
    if 0 <= root < n and T.flat[root]:
        dist = dijkstra(A, directed=True, indices=int(root))
        fin = np.isfinite(dist)
        g[fin] = dist[fin].astype(np.int64)
    return g.reshape(H, W).astype(np.int32)
