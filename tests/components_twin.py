"""Helpers of the component tests: the CPU twin (tests/cpp/components_ref.c, compiled on demand), scipy's labelling in the
library's canonical form, and the maps both are run on."""
import ctypes as C
import os
import subprocess

import numpy as np

from field_twin import d2_of, serpentine, spiral  # noqa: F401  (the maps of the field tests, shared)

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "components_ref.c")
Q_OK, Q_NO_PATH, Q_BAD_ENDPOINT, Q_TRUNCATED = 0, 1, 2, 3


class Twin:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libcomponents_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        self.lib.cr_components.restype = i
        self.lib.cr_components.argtypes = [vp, i, i, C.c_int32, vp, vp, vp, vp]
        self.lib.cr_reachable.restype = None
        self.lib.cr_reachable.argtypes = [vp, i, vp, i, i, vp, vp, i, vp]

    def components(self, d2, r2=0):
        """d2 [H,W] or [G,H,W] -> dict(label, size shaped like d2, ncomp [G], largest [G])."""
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        d3 = d2 if d2.ndim == 3 else d2[None]
        G, H, W = d3.shape
        label, size = np.empty_like(d3), np.empty_like(d3)
        ncomp, largest = np.zeros(G, np.int32), np.zeros(G, np.int32)
        for g in range(G):
            st = self.lib.cr_components(d3[g].ctypes.data, W, H, r2, label[g].ctypes.data, size[g].ctypes.data,
                                        ncomp[g:].ctypes.data, largest[g:].ctypes.data)
            assert st == 0
        return dict(label=label.reshape(d2.shape), size=size.reshape(d2.shape), ncomp=ncomp, largest=largest)

    def reachable(self, label, start, goal, qgrid=None):
        label = np.ascontiguousarray(label, dtype=np.int32)
        start = np.ascontiguousarray(start, dtype=np.int32)
        goal = np.ascontiguousarray(goal, dtype=np.int32)
        qgrid = None if qgrid is None else np.ascontiguousarray(qgrid, dtype=np.int32)
        G, H, W = (1,) + label.shape if label.ndim == 2 else label.shape
        status = np.zeros(start.shape[0], np.int32)
        self.lib.cr_reachable(label.ctypes.data, G, None if qgrid is None else qgrid.ctypes.data, W, H, start.ctypes.data,
                              goal.ctypes.data, start.shape[0], status.ctypes.data)
        return status


def components_scipy(d2, r2=0):
    """The same four results of one grid from scipy.ndimage.label (4-connected), relabelled to each component's minimum."""
    from scipy import ndimage
    d2 = np.asarray(d2)
    H, W = d2.shape
    T = d2 >= max(r2, 1)
    lab, k = ndimage.label(T, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    label = np.full((H, W), -1, np.int32)
    size = np.zeros((H, W), np.int32)
    if k == 0:
        return dict(label=label, size=size, ncomp=0, largest=-1)
    mins = ndimage.minimum(idx, lab, index=np.arange(1, k + 1)).astype(np.int64)
    counts = np.bincount(lab.ravel(), minlength=k + 1)[1:]
    label[T] = mins[lab[T] - 1]
    size.flat[mins] = counts
    best = counts.max()
    return dict(label=label, size=size, ncomp=int(k), largest=int(mins[counts == best].min()))


def comb(n, tooth=8):
    """One-cell-wide teeth on every other column, joined along the bottom row: one component."""
    occ = np.ones((tooth + 1, n), np.uint8)
    occ[tooth, :] = 0
    occ[:, ::2] = 0
    return occ


def rings(n, gap=3):
    """Concentric closed square walls: every ring of free cells between two walls is a component of its own."""
    occ = np.zeros((n, n), np.uint8)
    lo = gap
    while n - 1 - 2 * lo > 0:
        hi = n - 1 - lo
        occ[lo, lo:hi + 1] = 1
        occ[hi, lo:hi + 1] = 1
        occ[lo:hi + 1, lo] = 1
        occ[lo:hi + 1, hi] = 1
        lo += gap + 1
    return occ


def cut_line(n, vertical):
    """A one-cell-wide line of n cells cut in three by two obstacles."""
    occ = np.zeros(n, np.uint8)
    occ[[n // 3, (2 * n) // 3 + 1]] = 1
    return occ.reshape(n, 1) if vertical else occ.reshape(1, n)
