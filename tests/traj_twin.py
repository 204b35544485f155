"""NumPy twin of the timed-path conflicts (sc_traj_knots_batch, sc_traj_conflicts_batch, sc_fleet_conflicts_batch): the
definition of include/sea_current_hip.h in fp64, one operation per line, no fused multiply-adds.  The reference of the
GPU tests (bit for bit) and of tests/cpp/traj_ref.c."""
import numpy as np

TRAJ_OK, TRAJ_SKIPPED, TRAJ_BAD = 0, 1, 2
SMOOTH_OK = 0


def _clamp(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def knots(time, pts, offsets, length, status, t0, flags, T0, dt_c, K):
    """-> (knots fp64 [P, K+1, 2], tstatus int32 [P])."""
    time = np.asarray(time, np.float64)
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    P = len(length)
    kn = np.full((P, K + 1, 2), np.nan)
    ts = np.zeros(P, np.int32)
    k = np.arange(K + 1, dtype=np.float64)
    tau = T0 + k * dt_c
    for p in range(P):
        n = int(length[p])
        if (status is not None and status[p] != SMOOTH_OK) or n < 1:
            ts[p] = TRAJ_SKIPPED
            continue
        o = int(offsets[p])
        t = time[o:o + n]
        xy = pts[o:o + n].astype(np.float64)
        d = 0.0 if t0 is None else float(t0[p])
        if not (np.isfinite(t).all() and np.isfinite(xy).all() and np.isfinite(d)) or (t[1:] < t[:-1]).any():
            ts[p] = TRAJ_BAD
            continue
        fl = 3 if flags is None else int(flags[p])
        u = tau - d
        before = u < t[0]
        after = u > t[-1]
        if n == 1:
            out = np.broadcast_to(xy[0], (K + 1, 2)).copy()
        else:
            j = np.searchsorted(t, u, side="right") - 1      # the last index with time[j] <= u
            j = np.minimum(np.maximum(j, 0), n - 2)
            den = t[j + 1] - t[j]
            num = u - t[j]
            with np.errstate(divide="ignore", invalid="ignore"):
                f = np.where(den > 0, num / den, 0.0)
            a = xy[j]
            b = xy[j + 1]
            diff = b - a
            step = f[:, None] * diff
            out = a + step
        out[before] = xy[0] if fl & 1 else np.nan
        out[after] = xy[-1] if fl & 2 else np.nan
        kn[p] = out
    return kn, ts


def conflicts(kn, tstatus, T0, dt_c, radius, group=None, sep_cap=np.inf, stats=None):
    """-> dict(first_t, first_with, min_sep, min_with, n_conf, conflict uint32 [P, ceil(P/32)], tstatus).  stats (a dict) receives
    the counts the tests assert on the random fleet."""
    kn = np.asarray(kn, np.float64)
    P, K1, _ = kn.shape
    K = K1 - 1
    radius = np.asarray(radius, np.float64)
    ts = np.asarray(tstatus, np.int32).copy()
    bad_r = ~(np.isfinite(radius) & (radius >= 0))
    ts[(ts == TRAJ_OK) & bad_r] = TRAJ_BAD
    ok = ts == TRAJ_OK
    kn = np.where(ok[:, None, None], kn, np.nan)
    tau = T0 + np.arange(K, dtype=np.float64) * dt_c
    first = np.full((P, P), np.inf)
    sep2 = np.full((P, P), np.inf)
    st = dict(conf_pairs=0, clear_pairs=0, root=0, inside=0, never=0)
    for lo in range(P - 1):
        hi = np.arange(lo + 1, P)
        cmp_ = ok[lo] & ok[hi]
        if group is not None:
            cmp_ &= ~((group[hi] == group[lo]) & (group[lo] >= 0))
        if not cmp_.any():
            continue
        hi = hi[cmp_]
        d0x = kn[hi, :-1, 0] - kn[lo, :-1, 0]
        d0y = kn[hi, :-1, 1] - kn[lo, :-1, 1]
        d1x = kn[hi, 1:, 0] - kn[lo, 1:, 0]
        d1y = kn[hi, 1:, 1] - kn[lo, 1:, 1]
        ex = d1x - d0x
        ey = d1y - d0y
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            a = ex * ex + ey * ey
            b = d0x * ex + d0y * ey
            c = d0x * d0x + d0y * d0y
            q = -b / a
            lam = np.where(a > 0, _clamp(q, 0.0, 1.0), 0.0)
            px = d0x + lam * ex
            py = d0y + lam * ey
            m2 = px * px + py * py
            R = radius[lo] + radius[hi]
            RR = (R * R)[:, None]
            conf = m2 < RR                                   # false where a knot is absent (NaN)
            disc = b * b - a * (c - RR)
            disc = np.where(disc > 0, disc, 0.0)
            r = (-b - np.sqrt(disc)) / a
            lc = np.where(c < RR, 0.0, _clamp(r, 0.0, lam))
            t = tau[None, :] + lc * dt_c
        t = np.where(conf, t, np.inf)
        first[lo, hi] = first[hi, lo] = t.min(axis=1)
        s2 = np.where(m2 == m2, m2, np.inf).min(axis=1)
        sep2[lo, hi] = sep2[hi, lo] = s2
        anyc = conf.any(axis=1)
        st["conf_pairs"] += int(anyc.sum())
        st["clear_pairs"] += int((~anyc).sum())
        st["root"] += int((conf & ~(c < RR)).sum())
        st["inside"] += int((conf & (c < RR)).sum())
        st["never"] += int(np.isinf(s2).sum())
    if stats is not None:
        stats.update(st)
    first_t = first.min(axis=1) if P else np.zeros(0)
    has = np.isfinite(first).any(axis=1)
    first_with = np.where(has, first.argmin(axis=1), -1).astype(np.int32)   # argmin: the smallest index attaining it
    s2min = sep2.min(axis=1)
    with np.errstate(invalid="ignore"):
        ms = np.sqrt(s2min)
    rep = ms < sep_cap
    min_sep = np.where(rep, ms, np.inf)
    min_with = np.where(rep, sep2.argmin(axis=1), -1).astype(np.int32)
    cm = np.isfinite(first)
    n_conf = cm.sum(axis=1).astype(np.int32)
    nw = (P + 31) // 32
    bits = np.zeros((P, nw * 32), np.uint32)
    bits[:, :P] = cm
    conflict = (bits.reshape(P, nw, 32) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint64).astype(np.uint32)
    return dict(first_t=first_t, first_with=first_with, min_sep=min_sep, min_with=min_with, n_conf=n_conf, conflict=conflict, tstatus=ts)


def fleet(time, pts, offsets, length, status, t0, flags, T0, dt_c, K, radius, group=None, sep_cap=np.inf, stats=None):
    kn, ts = knots(time, pts, offsets, length, status, t0, flags, T0, dt_c, K)
    out = conflicts(kn, ts, T0, dt_c, radius, group, sep_cap, stats)
    out["knots"] = kn
    return out
