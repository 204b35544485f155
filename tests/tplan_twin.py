"""NumPy twin of the space-time re-planning (sc_traj_reserve_batch, sc_tplan_batch, sc_fleet_replan_batch): the definition of
include/sea_current_hip.h, one operation per line, fp64 without fused multiply-adds.  The reference of the GPU tests (bit
for bit) and of tests/cpp/tplan_ref.c."""
import numpy as np

TP_OK, TP_NO_PATH, TP_BAD_ENDPOINT, TP_START_BLOCKED = 0, 1, 2, 3
TRAJ_OK, TRAJ_BAD = 0, 2
DX = (1, -1, 0, 0, 1, -1, 1, -1)
DY = (0, 0, 1, -1, 1, 1, -1, -1)


def centres(W, H, frame):
    """The cell centres sc_cells_to_points_batch writes, widened: (cx fp64 [W], cy fp64 [H])."""
    x_min, y_min, res_x, res_y = (np.float32(v) for v in frame)
    half = np.float32(0.5)
    ix = np.arange(W, dtype=np.float32) + half
    iy = np.arange(H, dtype=np.float32) + half
    cx = x_min + ix * res_x
    cy = y_min + iy * res_y
    assert cx.dtype == np.float32 and cy.dtype == np.float32
    return cx.astype(np.float64), cy.astype(np.float64)


def pack(bits):
    """bool [..., H, W] -> uint32 [..., H, ceil(W/32)]: cell x is bit x & 31 of word x >> 5."""
    bits = np.asarray(bits, bool)
    W = bits.shape[-1]
    Wq = (W + 31) // 32
    full = np.zeros(bits.shape[:-1] + (Wq * 32,), np.uint64)
    full[..., :W] = bits
    words = (full.reshape(bits.shape[:-1] + (Wq, 32)) << np.arange(32, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)
    return words.astype(np.uint32)


def unpack(words, W):
    """uint32 [..., H, Wq] -> bool [..., H, W]."""
    words = np.asarray(words, np.uint32)
    b = (words[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return b.reshape(words.shape[:-1] + (-1,))[..., :W].astype(bool)


def _clamp(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def reserve(knots, tstatus, radius, select, pad, W, H, frame, res=None):
    """ORs the reservations of the knot rows into res (bool [L, H, W], None = all clear).  -> (res bool [L, H, W], tstatus)."""
    kn = np.asarray(knots, np.float64)
    P, L, _ = kn.shape
    K = L - 1
    radius = np.asarray(radius, np.float64)
    ts = np.zeros(P, np.int32) if tstatus is None else np.asarray(tstatus, np.int32).copy()
    bad_r = ~(np.isfinite(radius) & (radius >= 0))
    ts[(ts == TRAJ_OK) & bad_r] = TRAJ_BAD
    res = np.zeros((L, H, W), bool) if res is None else np.asarray(res, bool).copy()
    cx, cy = centres(W, H, frame)
    cxg = cx[None, None, :]
    cyg = cy[None, :, None]
    for q in range(P):
        if ts[q] != TRAJ_OK or (select is not None and select[q] == 0):
            continue
        R = radius[q] + pad
        RR = R * R
        ax = kn[q, :-1, 0][:, None, None]
        ay = kn[q, :-1, 1][:, None, None]
        bx = kn[q, 1:, 0][:, None, None]
        by = kn[q, 1:, 1][:, None, None]
        d0x = ax - cxg
        d0y = ay - cyg
        d1x = bx - cxg
        d1y = by - cyg
        ex = d1x - d0x
        ey = d1y - d0y
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            a = ex * ex + ey * ey
            b = d0x * ex + d0y * ey
            qq = -b / a
            lam = np.where(a > 0, _clamp(qq, 0.0, 1.0), 0.0)
            px = d0x + lam * ex
            py = d0y + lam * ey
            m2 = px * px + py * py
            hit = m2 < RR                       # false where a knot is absent (NaN)
        res[:K] |= hit
        res[1:] |= hit
    return res, ts


def moves(d2, r2):
    """sc_moves_i32_u8: uint8 [H, W], bit d set where the step in direction d is allowed (no corner cutting)."""
    d2 = np.asarray(d2)
    H, W = d2.shape
    t = np.zeros((H + 2, W + 2), bool)
    t[1:-1, 1:-1] = d2 >= max(int(r2), 1)
    at = lambda dx, dy: t[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    c = at(0, 0)
    m = np.zeros((H, W), np.uint8)
    for d in range(8):
        ok = c & at(DX[d], DY[d])
        if DX[d] and DY[d]:
            ok = ok & at(DX[d], 0) & at(0, DY[d])
        m |= ok.astype(np.uint8) << d
    return m


def _shift(a, dx, dy):
    """out[y + dy, x + dx] = a[y, x]; what leaves the grid is dropped."""
    H, W = a.shape
    out = np.zeros_like(a)
    out[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = a[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    return out


def plan_one(mv, free, res, L, start, goal, t_start, hold):
    """One query.  -> (status, arrive, path list, reach bool [L, H, W] (layers outside t_start .. arrive / L-1 are zero))."""
    H, W = mv.shape
    reach = np.zeros((L, H, W), bool)
    cells = W * H
    if not (0 <= start < cells and 0 <= goal < cells and 0 <= t_start < L):
        return TP_BAD_ENDPOINT, -1, [], reach
    sy, sx = divmod(int(start), W)
    gy, gx = divmod(int(goal), W)
    if not (free[sy, sx] and free[gy, gx]):
        return TP_BAD_ENDPOINT, -1, [], reach
    if res is not None and res[t_start, sy, sx]:
        return TP_START_BLOCKED, -1, [], reach
    t_hold = 0
    if hold and res is not None:
        at_goal = np.nonzero(res[:, gy, gx])[0]
        if len(at_goal):
            t_hold = int(at_goal[-1]) + 1
    t_min = max(t_start, t_hold)
    reach[t_start, sy, sx] = True
    can = [(mv >> d & 1).astype(bool) for d in range(8)]
    arrive = -1
    t = t_start
    while True:
        if t >= t_min and reach[t, gy, gx]:
            arrive = t
            break
        if t == L - 1:
            break
        nxt = reach[t].copy()                                   # a wait
        for d in range(8):
            leaving = reach[t] & can[d]
            nxt |= _shift(leaving, DX[d], DY[d])
        if res is not None:
            nxt &= ~res[t + 1]
        reach[t + 1] = nxt
        t += 1
    if arrive < 0:
        return TP_NO_PATH, -1, [], reach
    x, y = gx, gy
    path = [y * W + x]
    for t in range(arrive, t_start, -1):
        prev = reach[t - 1]
        if not prev[y, x]:
            for d in range(8):
                px, py = x - DX[d], y - DY[d]
                if 0 <= px < W and 0 <= py < H and prev[py, px] and (mv[py, px] >> d & 1):
                    x, y = px, py
                    break
            else:
                raise AssertionError("a reached cell has a predecessor")
        path.append(y * W + x)
    return TP_OK, arrive, path[::-1], reach


def plan(d2, r2, res, L, start, goal, t_start, hold, frame=None, want_reach=False):
    """The search.  res: bool [L, H, W] or None.  -> dict(status, arrive, len int32 [B]; path int32 [B, L], -1 where not written;
    knots_out fp64 [B, L, 2] with a frame; reach bool [B, L, H, W] with want_reach)."""
    d2 = np.asarray(d2)
    H, W = d2.shape
    mv = moves(d2, r2)
    free = d2 >= max(int(r2), 1)
    B = len(start)
    out = dict(status=np.zeros(B, np.int32), arrive=np.full(B, -1, np.int32), len=np.zeros(B, np.int32), path=np.full((B, L), -1, np.int32))
    if frame is not None:
        out["knots_out"] = np.full((B, L, 2), np.nan)
        cx, cy = centres(W, H, frame)
    if want_reach:
        out["reach"] = np.zeros((B, L, H, W), bool)
    for b in range(B):
        ts = 0 if t_start is None else int(t_start[b])
        st, arr, path, reach = plan_one(mv, free, res, L, int(start[b]), int(goal[b]), ts, hold)
        out["status"][b] = st
        if want_reach:
            out["reach"][b] = reach
        if st != TP_OK:
            continue
        out["arrive"][b] = arr
        out["len"][b] = len(path)
        out["path"][b, :len(path)] = path
        if frame is not None:
            cells = np.asarray(path + ([int(goal[b])] * (L - 1 - arr) if hold else []))
            out["knots_out"][b, ts:ts + len(cells), 0] = cx[cells % W]
            out["knots_out"][b, ts:ts + len(cells), 1] = cy[cells // W]
    return out


def fleet_replan(knots, tstatus, radius, select, pad, W, H, frame, res, d2, r2, start, goal, t_start, hold, r_new=None, sequential=False,
                 want_reach=False):
    """Reserve the selected fleet paths into res (bool [L, H, W], None = all clear), then plan: all robots at once, or one by one
    with each robot's row reserved (radius r_new[i], the same pad) before the next.  -> plan's dict plus res and tstatus."""
    L = np.asarray(knots).shape[1]
    res, ts = reserve(knots, tstatus, radius, select, pad, W, H, frame, res)
    if not sequential:
        out = plan(d2, r2, res, L, start, goal, t_start, hold, frame, want_reach)
    else:
        outs = []
        for i in range(len(start)):
            o = plan(d2, r2, res, L, start[i:i + 1], goal[i:i + 1], None if t_start is None else t_start[i:i + 1], hold, frame, want_reach)
            res, _ = reserve(o["knots_out"], None, np.asarray(r_new, np.float64)[i:i + 1], None, pad, W, H, frame, res)
            outs.append(o)
        out = {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}
    out["res"] = res
    out["tstatus"] = ts
    return out
