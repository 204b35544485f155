"""NumPy twin of the delay schedules (sc_traj_shift_table_batch, sc_traj_schedule_batch, sc_traj_shift_knots_batch,
sc_fleet_schedule_batch): the definition of include/sea_current_hip.h.  The predicate is traj_twin's m2 < R*R, the same
operations in the same order; everything else is integers.  The reference of the GPU tests (exactly) and of
tests/cpp/traj_sched_ref.c."""
import numpy as np

import traj_twin as tw

SLOT_UNRESOLVED, SLOT_NOT_OK, SLOT_UNNAMED = -1, -2, -3
BOX_SLACK = 2.0 ** -48


def path_ok(tstatus, radius):
    """-> (ok bool [P], tstatus with SC_TRAJ_BAD for a radius outside the contract)."""
    radius = np.asarray(radius, np.float64)
    ts = np.asarray(tstatus, np.int32).copy()
    ts[(ts == tw.TRAJ_OK) & ~(np.isfinite(radius) & (radius >= 0))] = tw.TRAJ_BAD
    return ts == tw.TRAJ_OK, ts


def boxes(kn):
    """[P, 4] x0, x1, y0, y1 of every path's present knots; +inf, -inf where there is none."""
    kn = np.asarray(kn, np.float64)
    pres = ~np.isnan(kn).any(axis=2)
    x, y = kn[:, :, 0], kn[:, :, 1]
    return np.stack([np.where(pres, x, np.inf).min(axis=1), np.where(pres, x, -np.inf).max(axis=1),
                     np.where(pres, y, np.inf).min(axis=1), np.where(pres, y, -np.inf).max(axis=1)], axis=1)


def gap2(a, b):
    """The squared gap between boxes a and b [..., 4], each axis shrunk by 2^-48 of the span (see csrc/traj_sched.hip)."""
    with np.errstate(invalid="ignore", over="ignore"):
        gx = (np.maximum(a[..., 0], b[..., 0]) - np.minimum(a[..., 1], b[..., 1])) - \
            BOX_SLACK * (np.maximum(a[..., 1], b[..., 1]) - np.minimum(a[..., 0], b[..., 0]))
        gy = (np.maximum(a[..., 2], b[..., 2]) - np.minimum(a[..., 3], b[..., 3])) - \
            BOX_SLACK * (np.maximum(a[..., 3], b[..., 3]) - np.minimum(a[..., 2], b[..., 2]))
        gx = np.where(gx > 0, gx, 0.0)
        gy = np.where(gy > 0, gy, 0.0)
        return gx * gx + gy * gy


def any_conflict(klo, khi, RR):
    """Does some interval of the rows klo, khi [..., K+1, 2] conflict (traj_twin.conflicts' m2 < RR)? -> bool [...]."""
    d0x = khi[..., :-1, 0] - klo[..., :-1, 0]
    d0y = khi[..., :-1, 1] - klo[..., :-1, 1]
    d1x = khi[..., 1:, 0] - klo[..., 1:, 0]
    d1y = khi[..., 1:, 1] - klo[..., 1:, 1]
    ex = d1x - d0x
    ey = d1y - d0y
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = ex * ex + ey * ey
        b = d0x * ex + d0y * ey
        q = -b / a
        lam = np.where(a > 0, tw._clamp(q, 0.0, 1.0), 0.0)
        px = d0x + lam * ex
        py = d0y + lam * ey
        m2 = px * px + py * py
        return (m2 < RR).any(axis=-1)


def shifted(row, s):
    """row [K+1, 2] shifted by every s of the int array s -> [len(s), K+1, 2]: knot_s[k] = row[max(k - s, 0)]."""
    k = np.arange(row.shape[0])
    return row[np.maximum(k[None, :] - np.asarray(s)[:, None], 0)]


def shift_table(kn, tstatus, radius, group, D, stride, skip=True, stats=None):
    """-> (table uint64 [P, P], tstatus).  skip=False evaluates the pairs the box test drops (the result is the same).  stats
    (a dict) receives the numbers of pairs compared, skipped by the box, with all 2D-1 bits set (full) and with some but not
    all (some)."""
    kn = np.asarray(kn, np.float64)
    P = kn.shape[0]
    radius = np.asarray(radius, np.float64)
    ok, ts = path_ok(tstatus, radius)
    nb = 2 * D - 1
    r = np.arange(nb) - (D - 1)
    s_lo = np.maximum(r, 0) * stride
    s_hi = np.maximum(-r, 0) * stride
    bx = boxes(kn)
    weight = np.uint64(1) << np.arange(nb, dtype=np.uint64)
    table = np.zeros((P, P), np.uint64)
    st = dict(compared=0, skipped=0, full=0, some=0)
    for lo in range(P - 1):
        if not ok[lo]:
            continue
        for hi in range(lo + 1, P):
            if not ok[hi] or (group is not None and group[lo] >= 0 and group[lo] == group[hi]):
                continue
            st["compared"] += 1
            R = radius[lo] + radius[hi]
            RR = R * R
            if not gap2(bx[lo], bx[hi]) < RR:
                st["skipped"] += 1
                if skip:
                    continue
            bits = any_conflict(shifted(kn[lo], s_lo), shifted(kn[hi], s_hi), RR)
            n = int(bits.sum())
            st["full"] += n == nb
            st["some"] += 0 < n < nb
            table[lo, hi] = (weight * bits.astype(np.uint64)).sum(dtype=np.uint64)
            table[hi, lo] = (weight * bits[::-1].astype(np.uint64)).sum(dtype=np.uint64)
    if stats is not None:
        stats.update({k: int(v) for k, v in st.items()})
    return table, ts


def schedule(table, tstatus, D, order=None, jmax=None):
    """-> (slot int32 [P], counts int32 [4]); tstatus as shift_table returned it."""
    P = table.shape[0]
    slot = np.full(P, SLOT_UNNAMED, np.int32)
    mask = (1 << D) - 1
    for p in (range(P) if order is None else order):
        p = int(p)
        if p < 0 or p >= P or slot[p] != SLOT_UNNAMED:
            continue
        jm = D - 1 if jmax is None else int(jmax[p])
        if tstatus[p] != tw.TRAJ_OK:
            slot[p] = SLOT_NOT_OK
        elif jm < 0:
            slot[p] = 0
        else:
            busy = 0
            for q in np.nonzero(slot >= 0)[0]:
                busy |= (int(table[p, q]) >> (D - 1 - int(slot[q]))) & mask
            free = [j for j in range(min(jm, D - 1) + 1) if not (busy >> j) & 1]
            slot[p] = free[0] if free else SLOT_UNRESOLVED
    counts = np.array([(slot == 0).sum(), (slot > 0).sum(), (slot == SLOT_UNRESOLVED).sum(), (slot < SLOT_UNRESOLVED).sum()], np.int32)
    return slot, counts


def shift_knots(kn, slot, stride):
    kn = np.asarray(kn, np.float64)
    out = np.full(kn.shape, np.nan)
    k = np.arange(kn.shape[1])
    for p in range(kn.shape[0]):
        if slot[p] >= 0:
            out[p] = kn[p][np.maximum(k - int(slot[p]) * stride, 0)]
    return out


def at_rest(kn, D, stride):
    """bool [P]: the path is at rest or absent from tick K - (D-1) * stride onward (the condition of the equivalence note)."""
    kn = np.asarray(kn, np.float64)
    tail = kn[:, kn.shape[1] - 1 - (D - 1) * stride:]
    same = (tail == tail[:, :1]) | (np.isnan(tail) & np.isnan(tail[:, :1]))
    return same.all(axis=(1, 2))


def fleet_schedule(time, pts, offsets, length, status, t0, flags, T0, dt_c, K, radius, group=None, D=8, stride=1, order=None, jmax=None,
                   skip=True, stats=None, **_):
    kn, ts = tw.knots(time, pts, offsets, length, status, t0, flags, T0, dt_c, K)
    table, ts = shift_table(kn, ts, radius, group, D, stride, skip, stats)
    slot, counts = schedule(table, ts, D, order, jmax)
    with np.errstate(invalid="ignore"):
        delay = np.where(slot >= 0, slot * stride * dt_c, np.nan)
    return dict(knots=kn, tstatus=ts, table=table, slot=slot, counts=counts, delay=delay, knots_out=shift_knots(kn, slot, stride))
