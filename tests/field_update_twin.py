"""Helpers of the field-repair tests (sc_cost_field_update_batch): the definition in NumPy and heapq
(update_twin), the C statement (tests/cpp/field_update_ref.c, compiled on demand: TwinU) and the cases the CPU and the GPU
tests share (cases).

update_twin restates the header's definition: the unsupported set U as a least fixed point, grown from the cells that are
no longer traversable by a worklist over support counts, then Dijkstra seeded at the damage only."""
import ctypes as C
import heapq
import os
import subprocess

import numpy as np

from sea_current_amd import synth
from field_twin import INF, Q_BAD_ENDPOINT, Q_OK, d2_of, serpentine

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "field_update_ref.c")
DX = (1, -1, 0, 0, 1, -1, 1, -1)
DY = (0, 0, 1, -1, 1, 1, -1, -1)


def _legal(T, x, y, d):
    """The move from (x, y) in direction d is legal under T (the A* graph: no corner cutting, no move off the grid)."""
    H, W = T.shape
    nx, ny = x + DX[d], y + DY[d]
    if nx < 0 or ny < 0 or nx >= W or ny >= H or not T[y, x] or not T[ny, nx]:
        return False
    return d < 4 or (T[y, nx] and T[ny, x])


def update_twin(d2_old, d2_new, g, root, r2=0, pen_old=None, pen_new=None, cap=255):
    """(g', status, [changed cells, |U|]) of one field by the definition.  g is not modified."""
    d2_old, d2_new = np.asarray(d2_old), np.asarray(d2_new)
    H, W = d2_new.shape
    thr = max(int(r2), 1)
    T0, T1 = d2_old >= thr, d2_new >= thr
    weighted = pen_new is not None
    p0 = np.minimum(np.asarray(pen_old).astype(np.int64), cap) if weighted else np.zeros((H, W), np.int64)
    p1 = np.minimum(np.asarray(pen_new).astype(np.int64), cap) if weighted else np.zeros((H, W), np.int64)
    changed = (T0 != T1) | (T0 & T1 & (p0 != p1))
    g = np.array(g, dtype=np.int64).reshape(H, W)
    fin = g < INF
    has_root = 0 <= root < W * H
    rx, ry = (root % W, root // W) if has_root else (-1, -1)
    root_ok = has_root and bool(T1[ry, rx])

    # U: support counts, then a worklist from the cells that lost traversability
    def supports(x, y, d):
        """(x, y) supports its neighbour in direction d: legal under T', g finite, tight under w'"""
        nx, ny = x + DX[d], y + DY[d]
        return _legal(T1, x, y, d) and fin[y, x] and fin[ny, nx] and g[y, x] + (10 if d < 4 else 14) + p1[ny, nx] == g[ny, nx]

    count = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            if fin[y, x]:
                for d in range(8):
                    if supports(x, y, d):
                        count[y + DY[d], x + DX[d]] += 1
    inU = fin & ~T1
    work = [(int(x), int(y)) for y, x in zip(*np.nonzero(inU))]
    for y, x in zip(*np.nonzero(fin & T1 & (count == 0))):
        if not (root_ok and x == rx and y == ry):
            inU[y, x] = True
            work.append((int(x), int(y)))
    while work:
        x, y = work.pop()
        for d in range(8):
            if supports(x, y, d):
                nx, ny = x + DX[d], y + DY[d]
                count[ny, nx] -= 1
                if count[ny, nx] == 0 and not inU[ny, nx] and not (root_ok and nx == rx and ny == ry):
                    inU[ny, nx] = True
                    work.append((nx, ny))
    stats = [int(changed.sum()), int(inU.sum())]
    g[inU] = INF
    if not root_ok:
        # a field whose root is not traversable in the new map: the fresh build leaves SC_FIELD_INF everywhere
        g[:] = INF
        return g.astype(np.int32), Q_BAD_ENDPOINT, stats
    g[ry, rx] = 0
    # Dijkstra from the damage: the finite cells at or next to a changed or raised cell, and the root
    dmg = changed | inU
    dmg[ry, rx] = True
    near = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, xs = np.nonzero(dmg)
            ys, xs = ys + dy, xs + dx
            ok = (ys >= 0) & (xs >= 0) & (ys < H) & (xs < W)
            near[ys[ok], xs[ok]] = True
    heap = [(int(g[y, x]), int(x), int(y)) for y, x in zip(*np.nonzero(near & (g < INF)))]
    heapq.heapify(heap)
    while heap:
        gv, x, y = heapq.heappop(heap)
        if gv > g[y, x]:
            continue
        for d in range(8):
            if _legal(T1, x, y, d):
                nx, ny = x + DX[d], y + DY[d]
                v = gv + (10 if d < 4 else 14) + int(p1[ny, nx])
                if v < g[ny, nx]:
                    g[ny, nx] = v
                    heapq.heappush(heap, (v, nx, ny))
    return g.astype(np.int32), Q_OK, stats


class TwinU:
    """The C statement: fu_update(d2_old, pen_old, d2_new, pen_new, cap, W, H, r2, root, g in/out, stats[2]) -> status,
    -1 for arguments it refuses."""

    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libfield_update_ref.so")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
        self.lib = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        self.lib.fu_update.restype = i
        self.lib.fu_update.argtypes = [vp, vp, vp, vp, i, i, i, C.c_int32, i, vp, vp]

    def update(self, d2_old, d2_new, g, root, r2=0, pen_old=None, pen_new=None, cap=255):
        d2_old = np.ascontiguousarray(d2_old, dtype=np.int32)
        d2_new = np.ascontiguousarray(d2_new, dtype=np.int32)
        H, W = d2_new.shape
        g = np.array(g, dtype=np.int32).reshape(H, W)
        stats = np.zeros(2, np.int32)
        po = pn = None
        if pen_new is not None:
            po, pn = np.ascontiguousarray(pen_old, dtype=np.uint8), np.ascontiguousarray(pen_new, dtype=np.uint8)
        st = self.lib.fu_update(d2_old.ctypes.data, None if po is None else po.ctypes.data, d2_new.ctypes.data,
                                None if pn is None else pn.ctypes.data, int(cap), W, H, r2, int(root), g.ctypes.data, stats.ctypes.data)
        return g, st, [int(stats[0]), int(stats[1])]


# ---- the cases -------------------------------------------------------------------------------------------------------
def two_rooms(W=24, H=16, door=(7, 9)):
    """Two rooms split by a wall in column W // 2 with a door over rows door[0] .. door[1] - 1."""
    occ = np.zeros((H, W), np.uint8)
    occ[:, W // 2] = 1
    occ[door[0]:door[1], W // 2] = 0
    return occ


def _free_cell(d2, r2, seed):
    T = np.flatnonzero(np.asarray(d2).ravel() >= max(r2, 1))
    return int(T[np.random.default_rng(seed).integers(0, T.size)])


def _flip(occ, cells):
    out = occ.copy()
    for x, y in cells:
        out[y, x] ^= 1
    return out


def _block_and_free(occ, axis, v, rng):
    """(old, new): on line x = v (axis 0) or y = v (axis 1) one cell that is free in both becomes blocked and one cell that is
    blocked in `old` becomes free; `old` is occ with those two cells set so (a free and a blocked cell on the line)."""
    H, W = occ.shape
    n = H if axis == 0 else W
    a, b = (int(k) for k in rng.choice(n, size=2, replace=False)) if n > 1 else (0, 0)
    ca, cb = ((v, a), (v, b)) if axis == 0 else ((a, v), (b, v))
    old = occ.copy()
    old[ca[1], ca[0]] = 0
    new = old.copy()
    new[ca[1], ca[0]] = 1                                     # a free cell blocked
    if cb != ca:
        old[cb[1], cb[0]] = 1
        new[cb[1], cb[0]] = 0                                 # a blocked cell freed
    return old, new


def cases(oracle):
    """[(name, d2_old, d2_new, pen_old, pen_new, cap, r2, root)]: the maps and changes of the issue.  d2 comes from the
    oracle's EDT where clearance matters (r2 4) and from d2_of elsewhere."""
    out = []
    rng = np.random.default_rng(17)

    def add(name, occ0, occ1, r2=0, root=None, pens=None, cap=255, edt=False):
        d0, d1 = (oracle.edt(occ0), oracle.edt(occ1)) if edt else (d2_of(occ0), d2_of(occ1))
        if root is None:
            root = _free_cell(np.minimum(d0, d1), r2, len(out))
        po, pn = pens if pens is not None else (None, None)
        out.append((name, d0, d1, po, pn, cap, r2, root))

    maps = [("salt64x64", synth.salt_grid(64, 64, 0.15, seed=2)), ("salt65x63", synth.salt_grid(65, 63, 0.15, seed=3)),
            ("blocks130x70", synth.block_grid(130, 70, 0.2, seed=7, smin=3, smax=12)),
            ("salt130x70", synth.salt_grid(130, 70, 0.2, seed=5)), ("blocks64x64", synth.block_grid(64, 64, 0.2, seed=9, smin=3, smax=10))]
    # one cell blocked and one freed at x or y of 0, 63, 64 and the last index
    for name, occ in maps:
        H, W = occ.shape
        for v in sorted({0, 63, 64, W - 1} & set(range(W))):
            add(f"{name}/x{v}", *_block_and_free(occ, 0, v, rng))
        for v in sorted({0, 63, 64, H - 1} & set(range(H))):
            add(f"{name}/y{v}", *_block_and_free(occ, 1, v, rng))
    # thin maps
    for name, (W, H) in (("1x200", (1, 200)), ("200x1", (200, 1))):
        occ = np.zeros((H, W), np.uint8)
        occ1 = occ.copy()
        occ1.ravel()[[64, 150]] = 1
        add(f"{name}/block", occ, occ1, root=10)
        add(f"{name}/free", occ1, occ, root=10)
        add(f"{name}/root_side", occ, occ1, root=100)
    # a rectangle moved by one cell across a tile corner
    occ = np.zeros((70, 130), np.uint8)
    occ0, occ1 = occ.copy(), occ.copy()
    occ0[60:66, 60:66] = 1
    occ1[61:67, 61:67] = 1
    add("rect_across_corner", occ0, occ1, root=0)
    add("rect_across_corner/far_root", occ1, occ0, root=69 * 130 + 129)
    # serpentine: the corridor closed (everything beyond is in U), a wall opened (everything falls, U empty)
    s = serpentine(64)
    closed = s.copy()
    closed[2:4, 62:64] = 1
    add("serpentine/closed", s, closed, root=0)
    add("serpentine/reopened", closed, s, root=0)
    opened = s.copy()
    opened[:, 0:2] = 0
    add("serpentine/wall_opened", s, opened, root=0)
    # root blocked, root freed, no change, every cell changed
    occ = maps[0][1]
    r = _free_cell(d2_of(occ), 0, 5)
    blocked = _flip(occ, [(r % 64, r // 64)])
    add("root_blocked", occ, blocked, root=r)
    add("root_freed", blocked, occ, root=r)
    add("no_change", occ, occ)
    add("every_cell_changed", occ, 1 - occ, root=r)
    add("root_out_of_range", occ, _flip(occ, [(3, 3)]), root=64 * 64)
    # weighted: penalties raised, lowered and both, with the map fixed; and with the map changing too
    occ = maps[2][1]
    H, W = occ.shape
    pen = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    up, dn, both = pen.copy(), pen.copy(), pen.copy()
    up[20:40, 50:80] = np.minimum(up[20:40, 50:80].astype(np.int32) + 40, 255).astype(np.uint8)
    dn[20:40, 50:80] //= 2
    both[10:30, 60:70] //= 3
    both[40:60, 60:70] = 255
    for nm, pn, cap in (("raised", up, 255), ("lowered", dn, 255), ("both", both, 255), ("both_cap7", both, 7), ("same", pen, 255)):
        add(f"weighted/{nm}", occ, occ, pens=(pen, pn), cap=cap)
    add("weighted/map_too", occ, _flip(occ, [(63, 20), (64, 21), (10, 64)]), pens=(pen, both))
    # clearance: r2_clear 4 over the oracle's EDT
    occ = synth.block_grid(130, 70, 0.1, seed=11, smin=3, smax=8)
    occ1 = occ.copy()
    occ1[30:34, 62:66] ^= 1
    add("r2_4", occ, occ1, r2=4, edt=True)
    return out


def hand_case():
    """A 5 x 5 map with U computed by hand.  Root (0, 0), a wall in row 2 open at x = 4; cell (4, 2) closes.
    Everything below the wall lost its only way in: U = the door and rows 3, 4 = 1 + 10 cells; one cell changed."""
    occ0 = np.zeros((5, 5), np.uint8)
    occ0[2, 0:4] = 1
    occ1 = occ0.copy()
    occ1[2, 4] = 1
    return d2_of(occ0), d2_of(occ1), 0, [1, 11]
