"""Helpers of the multi-source cost-field tests: the CPU twin (tests/cpp/field_multi_ref.c, compiled on demand), scipy's
route to the same g (one Dijkstra per seed plus its cost, then the elementwise minimum) and the small maps both the CPU
and the GPU tests use."""
import ctypes as C
import os
import subprocess

import numpy as np

from field_twin import INF, d2_of, field_scipy
from field_w_twin import field_w_scipy

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "field_multi_ref.c")
SEED_COST_MAX = 1 << 24


class TwinM:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libfield_multi_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        self.lib.fm_cost_field.restype = i
        self.lib.fm_cost_field.argtypes = [vp, vp, i, i, i, C.c_int32, vp, vp, i, i, vp, vp]
        self.lib.fm_field_paths.restype = None
        self.lib.fm_field_paths.argtypes = [vp, vp, i, i, i, C.c_int32, vp, vp, vp, i, i, vp, i, i, i, vp, vp, vp, vp, vp]

    @staticmethod
    def _prep(d2, pen, seeds, seed_cost):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        pen = None if pen is None else np.ascontiguousarray(pen, dtype=np.uint8)
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        seed_cost = None if seed_cost is None else np.ascontiguousarray(seed_cost, dtype=np.int32)
        assert seed_cost is None or seed_cost.shape == seeds.shape
        return d2, pen, seeds, seed_cost

    def field(self, d2, seeds, seed_cost=None, r2=0, pen=None, cap=255, s0=0):
        """One field from `seeds` (the field's own list; s0 = where it starts in the call's array).  Returns g, owner, status."""
        d2, pen, seeds, seed_cost = self._prep(d2, pen, seeds, seed_cost)
        H, W = d2.shape
        g = np.empty((H, W), np.int32)
        owner = np.empty((H, W), np.int32)
        p = lambda a: None if a is None else a.ctypes.data
        st = self.lib.fm_cost_field(p(d2), p(pen), int(cap), W, H, r2, p(seeds), p(seed_cost), seeds.shape[0], int(s0), p(g), p(owner))
        return g, owner, st

    def paths(self, d2, g, seeds, targets, seed_cost=None, r2=0, pen=None, cap=255, s0=0, Lmax=4096, to_seed=False):
        d2, pen, seeds, seed_cost = self._prep(d2, pen, seeds, seed_cost)
        g = np.ascontiguousarray(g, dtype=np.int32)
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        H, W = d2.shape
        Q = targets.shape[0]
        out = dict(path=np.full((Q, Lmax), -1, np.int32), len=np.zeros(Q, np.int32), cost=np.zeros(Q, np.int32),
                   status=np.zeros(Q, np.int32), which=np.zeros(Q, np.int32))
        p = lambda a: None if a is None else a.ctypes.data
        self.lib.fm_field_paths(p(d2), p(pen), int(cap), W, H, r2, p(g), p(seeds), p(seed_cost), seeds.shape[0], int(s0), p(targets), Q, Lmax,
                                int(bool(to_seed)), p(out["path"]), p(out["len"]), p(out["cost"]), p(out["status"]), p(out["which"]))
        return out


def seed_valid(d2, seeds, seed_cost=None, r2=0):
    d2 = np.asarray(d2)
    seeds = np.asarray(seeds, np.int64)
    cost = np.zeros(seeds.shape, np.int64) if seed_cost is None else np.asarray(seed_cost, np.int64)
    ok = (seeds >= 0) & (seeds < d2.size) & (cost >= 0) & (cost <= SEED_COST_MAX)
    ok[ok] &= d2.ravel()[seeds[ok]] >= max(r2, 1)
    return ok


def field_multi_scipy(d2, seeds, seed_cost=None, r2=0, pen=None, cap=255):
    """g by the definition: one scipy Dijkstra per valid seed, plus its cost, then the elementwise minimum."""
    d2 = np.asarray(d2)
    g = np.full(d2.shape, INF, np.int64)
    ok = seed_valid(d2, seeds, seed_cost, r2)
    for k in np.flatnonzero(ok):
        one = (field_scipy(d2, int(seeds[k]), r2) if pen is None else field_w_scipy(d2, pen, int(seeds[k]), r2, cap)).astype(np.int64)
        one[one < INF] += 0 if seed_cost is None else int(seed_cost[k])
        g = np.minimum(g, one)
    return g.astype(np.int32)


def plug_map():
    """130 x 3; the seed (63, 1) is walled in on every side but the right, where the next 64-column tile begins: its only
    free neighbour is (64, 1).  Returns d2 and the seed's cell index."""
    occ = np.zeros((3, 130), np.uint8)
    for x, y in ((62, 0), (63, 0), (62, 1), (62, 2), (63, 2)):
        occ[y, x] = 1
    return d2_of(occ), 1 * 130 + 63


def mirror_map():
    """33 x 17 open, seeds (4, 8) and (28, 8): the 17 cells of column 16 are as far from one as from the other."""
    return np.ones((17, 33), np.int32), np.array([8 * 33 + 4, 8 * 33 + 28], np.int32)
