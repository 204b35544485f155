"""Inputs shared by the timed-path conflict tests (no GPU needed to build them): the hand cases with exact answers and the
seeded random fleet.  Every case is a dict of the arguments of traj_twin.fleet."""
import numpy as np

FLEET_SEED = 7          # chosen on the CPU: the twin's counts on this fleet are asserted in tests/test_traj_twin.py
FLEET_P, FLEET_K, FLEET_T0, FLEET_DT = 130, 300, -1.0, 0.25


def bits(a):
    """The bit patterns of fp64 values, every NaN the same one (an absent knot has no payload to compare)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.nan, a).view(np.uint64)


def pack(paths, radius, t0=None, flags=None, group=None, status=None, T0=0.0, dt_c=0.5, K=None, sep_cap=np.inf):
    """paths: a list of (time [n], pts [n][2]) -> the packed layout sc_smooth_paths_batch writes."""
    length = np.array([len(t) for t, _ in paths], np.int32)
    offsets = np.zeros(len(paths) + 1, np.int32)
    offsets[1:] = np.cumsum(length)
    M = max(int(offsets[-1]), 1)
    time = np.zeros(M)
    pts = np.zeros((M, 2), np.float32)
    for p, (t, xy) in enumerate(paths):
        time[offsets[p]:offsets[p + 1]] = t
        pts[offsets[p]:offsets[p + 1]] = np.asarray(xy, np.float32).reshape(-1, 2)
    P = len(paths)
    opt = lambda v, dt: None if v is None else np.ascontiguousarray(v, dtype=dt)
    if K is None:
        end = max((t[-1] + (0.0 if t0 is None else t0[p])) for p, (t, _) in enumerate(paths) if len(t))
        K = max(1, int(np.ceil((end - T0) / dt_c)))
    return dict(time=time, pts=pts, offsets=offsets, length=length, status=opt(status, np.int32), t0=opt(t0, np.float64),
                flags=opt(flags, np.int32), T0=float(T0), dt_c=float(dt_c), K=int(K),
                radius=np.array(np.broadcast_to(np.asarray(radius, np.float64), (P,))), group=opt(group, np.int32),
                sep_cap=float(sep_cap))


def line(x0, y0, x1, y1, n=9, dt=1.0):
    """n samples dt apart, uniformly from (x0, y0) to (x1, y1)."""
    s = np.arange(n) / (n - 1)
    return np.arange(n) * dt, np.stack([x0 + s * (x1 - x0), y0 + s * (y1 - y0)], axis=1)


def head_on(dt_c=0.5):
    return pack([line(0, 0, 8, 0), line(8, 0, 0, 0)], 0.5, dt_c=dt_c)


def crossing(delay=0.0):
    return pack([line(0, 0, 8, 0), line(4, -4, 4, 4)], 0.5, t0=[0.0, delay], flags=[0, 0], dt_c=0.5, K=22)


def parked(hold=True):
    return pack([line(0, 0, 8, 0), line(8, 8, 8, 0)], 0.5, t0=[0.0, 10.0], flags=[3 if hold else 1, 3], dt_c=0.5, K=40)


def mirror_tie():
    """Path 1 meets its mirror images 2 and 0 (about y = 0) at the same instant and the same distance."""
    return pack([line(8, 4, 8, 0), line(0, 0, 8, 0), line(8, -4, 8, 0)], 0.5, group=[5, -1, 5], dt_c=0.5)


def random_fleet(seed=FLEET_SEED, P=FLEET_P, K=FLEET_K, T0=FLEET_T0, dt_c=FLEET_DT, lens=(1, 2, 70), box=40.0, broken=True):
    """P paths in a box: lengths `lens` first, then 3 .. 40 samples, uneven time steps (some zero), random delay, flags,
    group and radius; with `broken` a few paths skipped or outside the contract."""
    rng = np.random.default_rng(seed)
    paths = []
    for p in range(P):
        n = lens[p] if p < len(lens) else int(rng.integers(3, 41))
        dt = rng.uniform(0.1, 1.0, n)
        dt[rng.random(n) < 0.05] = 0.0
        t = np.cumsum(dt) - dt[0] + rng.uniform(0.0, 2.0)
        start = rng.uniform(0.0, box, 2)
        head = rng.uniform(0.0, 2 * np.pi)
        turn = rng.normal(0.0, 0.15, n).cumsum()
        step = np.stack([np.cos(head + turn), np.sin(head + turn)], axis=1) * (dt * rng.uniform(0.5, 2.0))[:, None]
        xy = start + np.cumsum(step, axis=0) - step[0]
        paths.append((t, xy.astype(np.float32)))
    t0 = rng.uniform(-2.0, 30.0, P)
    flags = rng.integers(0, 4, P)
    group = rng.integers(-2, 6, P)
    radius = rng.uniform(0.3, 1.5, P)
    status = np.zeros(P, np.int32)
    case = pack(paths, radius, t0=t0, flags=flags, group=group, status=status, T0=T0, dt_c=dt_c, K=K)
    if broken and P >= 16:
        o = case["offsets"]
        case["status"][5] = 3                                   # skipped
        case["length"][7] = 0                                   # skipped: no sample
        case["pts"][o[9] + 1, 0] = np.nan                       # bad: a sample
        case["time"][o[10] + 2] = case["time"][o[10] + 1] - 0.5  # bad: time decreases
        case["t0"][11] = np.inf                                 # bad: delay
        case["radius"][12] = -0.1                               # bad: radius
        case["radius"][13] = np.nan
    return case
