"""NumPy twin of wide-window scan matching (sc_scan_match_wide_batch) straight from the definition in
include/sea_current_hip.h: the pooled cost maps as direct window minima (not the doubling the kernels use), the bound of a
node, and the procedure level by level with its dives, whose counts are outputs; plus the loader of the C statement
(tests/cpp/match_wide_ref.c).  Checker only: the library never imports it."""
import ctypes as C
import os
import subprocess

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import match_twin as mt

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "match_wide_ref.c")
OVERFLOW, MAX_HALF, MAX_TOP, MIN_NODES, MAX_NODES, MAX_TOTAL = -2, 2048, 5, 64, 1 << 22, 1 << 26


class Invalid(ValueError):
    """Arguments outside the contract: the calls return SC_ERR_INVALID."""


# ---- the definition ----
def pooled(cost, m, unk):
    """P_m over x in -m .. W and y in -m .. H, int64 [H+m+1, W+m+1]: the minimum of cost over the m x m cells from (x, y) on,
    where a cell outside the grid costs unk.  A coordinate clipped to that range reads the right value."""
    H, W = cost.shape
    pad = np.full((H + 2 * m, W + 2 * m), unk, np.int16)               # x in -m .. W + m - 1: every window's cells
    pad[m:m + H, m:m + W] = cost
    rows = sliding_window_view(pad, m, axis=1).min(-1)                 # [H+2m, W+m+1]
    cols = sliding_window_view(np.ascontiguousarray(rows.T), m, axis=1).min(-1)
    return cols.T.astype(np.int64)


def children(nodes, q, wx, wy):
    """The children of size q of nodes int64 [n,3] = (r, dx0, dy0) of size 4q: those that begin inside the window."""
    a = np.arange(4) * q
    r = np.repeat(nodes[:, 0], 16)
    x = (nodes[:, 1, None, None] + a[None, None, :]).repeat(4, 1).ravel()
    y = (nodes[:, 2, None, None] + a[None, :, None]).repeat(4, 2).ravel()
    ok = (x <= wx) & (y <= wy)
    return np.stack([r[ok], x[ok], y[ok]], 1)


def _smallest(B, nodes):
    """Index of the smallest (B, dy0, dx0)."""
    return int(np.lexsort((nodes[:, 1], nodes[:, 2], B))[0])


def match_wide(d2, known, pts, centre, wx, wy, d2_cap, unk, top, max_nodes):
    """(best int32 [S,6], stats int32 [S,8]) of pts int [S,R,N,2] and centre int [S,2]; raises Invalid where the call
    returns SC_ERR_INVALID."""
    d2 = np.asarray(d2)
    H, W = d2.shape
    pts = np.asarray(pts, dtype=np.int64)
    S, R, N, _ = pts.shape
    centre = np.asarray(centre, dtype=np.int64).reshape(S, 2)
    if not (0 <= wx <= MAX_HALF and 0 <= wy <= MAX_HALF and 1 <= d2_cap <= 32767 and 0 <= unk <= d2_cap and 0 <= top <= MAX_TOP
            and MIN_NODES <= max_nodes <= MAX_NODES and S * max_nodes <= MAX_TOTAL and 1 <= N <= mt.MAX_POINTS and 1 <= R <= mt.MAX_ROT
            and R * (2 * wx + 1) * (2 * wy + 1) < 2**31):
        raise Invalid("range")
    m_top = 4 ** top
    xs, ys = np.arange(-wx, wx + 1, m_top), np.arange(-wy, wy + 1, m_top)
    if R * len(xs) * len(ys) > max_nodes:
        raise Invalid("too many top nodes")
    cost = mt.cost_map(d2, known, d2_cap, unk)
    P = [pooled(cost, 4 ** j, unk) for j in range(top + 1)]
    best, stats = np.zeros((S, 6), np.int32), np.zeros((S, 8), np.int32)

    for s in range(S):
        if not mt.centre_ok(centre[s]):
            best[s, 0] = mt.IGNORED
            continue
        cx, cy = centre[s]
        p = [pts[s, r][mt.present(pts[s, r])] for r in range(R)]
        if not any(len(q) for q in p):
            best[s, 5] = R * (2 * wx + 1) * (2 * wy + 1)
            continue

        def bound(j, nodes):
            """B of nodes [n,3] of size 4^j, int64 [n]."""
            m, B = 4 ** j, np.zeros(len(nodes), np.int64)
            for r in np.unique(nodes[:, 0]):
                sel = np.flatnonzero(nodes[:, 0] == r)
                for i in range(0, len(sel), 4096):                   # bounded temporaries
                    nd = nodes[sel[i:i + 4096]]
                    x = np.clip(cx + nd[:, 1, None] + p[r][None, :, 0], -m, W) + m
                    y = np.clip(cy + nd[:, 2, None] + p[r][None, :, 1], -m, H) + m
                    B[sel[i:i + 4096]] = P[j][y, x].sum(1)
            return B

        U = int(bound(0, np.array([(r, 0, 0) for r in range(R)], np.int64)).min())
        gx, gy = np.meshgrid(xs, ys)
        nodes = np.concatenate([np.stack([np.full(gx.size, r), gx.ravel(), gy.ravel()], 1) for r in range(R)]).astype(np.int64)
        n, n_dive, over = [0] * 6, 0, False
        for j in range(top, -1, -1):
            B = bound(j, nodes)
            n[j] = len(nodes)
            if j == 0:
                break
            v = []
            for r in range(R):
                sel = np.flatnonzero(nodes[:, 0] == r)
                if not len(sel):
                    continue
                i = sel[_smallest(B[sel], nodes[sel])]
                if B[i] > U:                                            # the U of the start of this level
                    continue
                cur = nodes[i:i + 1]
                for jj in range(j - 1, -1, -1):
                    kids = children(cur, 4 ** jj, wx, wy)
                    Bk = bound(jj, kids)
                    n_dive += len(kids)
                    k = _smallest(Bk, kids)
                    cur = kids[k:k + 1]
                v.append(int(Bk[k]))
            U = min([U] + v)
            nodes = children(nodes[B <= U], 4 ** (j - 1), wx, wy)
            if len(nodes) > max_nodes:
                over = True
                break
        stats[s] = n + [n_dive, U]
        if over:
            best[s, 0] = OVERFLOW
            continue
        smin = int(B.min())
        assert 0 <= smin < 2**31
        tie = nodes[B == smin]
        _, r, dy, dx = min((int(x * x + y * y), int(r), int(y), int(x)) for r, x, y in tie)
        best[s] = (r, dx, dy, smin, len(p[r]), len(tie))
    return best, stats


def work(stats):
    """Candidates bounded or scored: sum of n_j plus n_dive, per scan."""
    return np.asarray(stats, dtype=np.int64)[:, :7].sum(1)


# ---- the C statement ----
class Ref:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libmatch_wide_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i, i32 = C.c_void_p, C.c_int, C.c_int32
        self.lib.mwx_match.restype = i
        self.lib.mwx_match.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, i, i32, i32, i, i, vp, vp]

    def match(self, d2, known, pts, centre, wx, wy, d2_cap, unk, top, max_nodes, want_stats=True):
        """(best, stats or None); raises Invalid for status 1."""
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        H, W = d2.shape
        known = None if known is None else np.ascontiguousarray(known, dtype=np.uint8)
        pts = np.ascontiguousarray(pts, dtype=np.int32)
        S, R, N, _ = pts.shape
        centre = np.ascontiguousarray(centre, dtype=np.int32).reshape(S, 2)
        best = np.full((S, 6), -7, np.int32)
        stats = np.full((S, 8), -7, np.int32) if want_stats else None
        status = self.lib.mwx_match(d2.ctypes.data, None if known is None else known.ctypes.data, pts.ctypes.data, centre.ctypes.data, S, R, N,
                                    W, H, wx, wy, d2_cap, unk, top, max_nodes, best.ctypes.data, None if stats is None else stats.ctypes.data)
        if status == 1:
            raise Invalid("mwx_match")
        assert status == 0
        return best, stats
