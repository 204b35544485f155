"""CPU twin of sc_speed_limits_batch for ONE path: the definition of include/sea_current_hip.h (per-stage speed limits
from curvature and clearance) restated in NumPy fp64, with the curve derivatives from oracle.bezier_eval.  Test
infrastructure only."""
import numpy as np


def gridpoints(AL, N):
    """a_i = AL * (3 s^2 - 2 s^3) at s = i / N: the TOPP-RA path of gen_vel_prof<1>(AL, 0, 0, 0, ..) at its gridpoints."""
    s = np.arange(N + 1, dtype=np.float64) / N
    return float(AL) * (3 * s * s - 2 * s * s * s)


def window_samples(AL, N, J):
    """x [N+1, 2J+1]: the arclength positions stage i answers for, half way to its neighbours."""
    a = gridpoints(AL, N)
    lo = np.concatenate([a[:1], (a[:-1] + a[1:]) / 2])
    hi = np.concatenate([(a[:-1] + a[1:]) / 2, a[-1:]])
    j = np.arange(-J, J + 1, dtype=np.float64) / J
    x = np.where(j[None, :] < 0, a[:, None] + j[None, :] * (a - lo)[:, None], a[:, None] + j[None, :] * (hi - a)[:, None])
    return np.clip(x, 0.0, float(AL))


def locate(x, cum):
    """arclength positions x (any shape) -> (leg, t, B): cum float32 [ns, nsub+1]."""
    cum = np.asarray(cum, np.float32)
    ns, nsub = cum.shape[0], cum.shape[1] - 1
    seg_len = cum[:, nsub].astype(np.float64)
    B = np.concatenate([[0.0], np.cumsum(seg_len)])
    leg = np.clip(np.searchsorted(B, x, side="right") - 1, 0, ns - 1)
    r = np.clip(x - B[leg], 0.0, seg_len[leg])
    k = np.zeros(x.shape, np.int64)
    for j in np.unique(leg):
        m = leg == j
        k[m] = np.searchsorted(cum[j].astype(np.float64), r[m], side="right") - 1
    k = np.clip(k, 0, nsub - 1)
    ck = cum[leg, k].astype(np.float64)
    den = cum[leg, k + 1].astype(np.float64) - ck
    f = np.where(den > 0, (r - ck) / np.where(den > 0, den, 1.0), 0.0)
    return leg, np.clip((k + f) / nsub, 0.0, 1.0), B


def clearance(px, py, d2, frame):
    """Bilinear interpolation of min(res) * sqrt(d2) over the cell centres; frame = (x_min, y_min, res_x, res_y) float32."""
    H, W = d2.shape
    x_min, y_min, res_x, res_y = (float(np.float32(v)) for v in frame)
    fx = np.clip((px - x_min) / res_x - 0.5, 0.0, W - 1)
    fy = np.clip((py - y_min) / res_y - 0.5, 0.0, H - 1)
    ix = np.minimum(fx.astype(np.int64), max(W - 2, 0))
    iy = np.minimum(fy.astype(np.int64), max(H - 2, 0))
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    ux, uy = fx - ix, fy - iy
    d = float(min(np.float32(res_x), np.float32(res_y))) * np.sqrt(np.maximum(d2, 0).astype(np.float64))
    e0 = d[iy, ix] * (1.0 - ux) + d[iy, ix1] * ux
    e1 = d[iy1, ix] * (1.0 - ux) + d[iy1, ix1] * ux
    return e0 * (1.0 - uy) + e1 * uy


def speed_limits(ctrl, cum, AL, limits, dyn, N=100, J=4, d2=None, frame=None):
    """ctrl float32 [ns,4,2], cum float32 [ns,nsub+1], AL the path's float32 arclength, limits (vel_min, vel_max, ..), dyn
    (omega_max, alat_max, clear_floor, clear_gain).  Returns dict(vlo, vhi [N+1], min_clear, flagged bool [N+1]: a sample
    of the stage lies within 1e-9 AL of an interior leg joint, where the curvature jumps)."""
    from oracle import oracle
    ctrl = np.ascontiguousarray(ctrl, np.float32).reshape(-1, 4, 2)
    om, alat, cf, cg = (float(v) for v in dyn)
    vel_min, vel_max = float(limits[0]), float(limits[1])
    x = window_samples(AL, N, J)
    leg, t, B = locate(x, cum)
    sh = x.shape
    d1 = oracle.bezier_eval(ctrl, leg.ravel().astype(np.int32), t.ravel(), 1)
    dd = oracle.bezier_eval(ctrl, leg.ravel().astype(np.int32), t.ravel(), 2)
    ax, ay, bx, by = d1[:, 0], d1[:, 1], dd[:, 0], dd[:, 1]
    with np.errstate(all="ignore"):
        q = ax * ax + ay * ay
        kappa = np.abs(ax * by - ay * bx) / (q * np.sqrt(q))
        kappa = np.where(np.isfinite(kappa), kappa, 0.0)
        pos = kappa > 0
        ks = np.where(pos, kappa, 1.0)
        v = np.full(kappa.shape, vel_max)
        v = np.where(pos, np.minimum(v, np.minimum(om / ks, np.sqrt(alat / ks))), v)
    min_clear = np.inf
    if d2 is not None and np.isfinite(cf):
        p = oracle.bezier_eval(ctrl, leg.ravel().astype(np.int32), t.ravel(), 0)
        c = clearance(p[:, 0], p[:, 1], np.asarray(d2), frame)
        v = np.minimum(v, cf + cg * c)
        min_clear = float(c.min())
    joints = B[1:-1]
    near = np.zeros(sh, bool) if joints.size == 0 else (np.abs(x[..., None] - joints).min(axis=-1) <= 1e-9 * float(AL))
    return dict(vlo=np.full(N + 1, vel_min), vhi=v.reshape(sh).min(axis=1), min_clear=min_clear, flagged=near.any(axis=1), x=x)
