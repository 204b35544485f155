"""An exact, stage-local certificate for TOPP-RA solutions, and a dense-solve reference for the sampled spline.

Test infrastructure (no test in here).  Nothing below calls into oracle/toppra_oracle.c or shares its method: the rows of
every stage are built in rational arithmetic from the definition in that file's header comment, and a stage's two-variable
linear programme is solved by VERTEX ENUMERATION (every pair of boundary lines is intersected, the feasible intersections are
kept, the extreme x is read off), not by the Fourier-Motzkin elimination of u that the oracle and the kernels use.

A claimed solution (K, x, u, t) is certified stage by stage:
  backward, stage i : with the claimed K[i+1] taken as exact input, the exact minimum and maximum of x over the stage polygon
                      {(u, x): acceleration rows, K_lo[i+1] <= x + 2 D_i u <= K_hi[i+1], xlo_i <= x <= xhi_i} against K[i];
  forward, stage i  : with the claimed x[i] and K[i+1] taken as exact input, the exact greatest u over the rows with a positive
                      u coefficient against u[i], and x[i] + 2 D_i u clamped into K[i+1] against x[i+1];
  knot times        : t[i] = sum_{j<i} D_j / mean(sqrt x_j, sqrt x_{j+1}) (5.0 where the mean is below 1e-8), math.fsum.
Each check uses only the claimed values of the neighbouring stage, so the rationals do not grow along a plan and any subset
of stages can be certified on its own (`stages=`).  Status-0 plans only.

All values are exact: floats convert to fractions.Fraction without loss, the gridpoints are the doubles i / N and D_i is
their exact difference.  Inside the vertex enumeration the rows are scaled to integers (a row multiplied by a positive
number is the same half-plane), so that intersections and feasibility are integer cross-multiplications with no gcd.
"""
import math
from fractions import Fraction as Fr

import numpy as np

MAXSD = 10 ** 8
NEARLY_ZERO = 1e-8


def _frs(a):
    return [Fr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()]


class Plan:
    """The inputs of one plan as exact rationals, and the rows of its stages."""

    def __init__(self, p0, p1, v0, v1, vlim_lo, vlim_hi, alim_lo, alim_hi, N, sd_start=0.0, sd_end=0.0):
        p0, p1, v0, v1 = _frs(p0), _frs(p1), _frs(v0), _frs(v1)
        self.dof, self.N = len(p0), int(N)
        self.c1 = v0
        self.c2 = [3 * (b - a) - 2 * s - e for a, b, s, e in zip(p0, p1, v0, v1)]
        self.c3 = [-2 * (b - a) + s + e for a, b, s, e in zip(p0, p1, v0, v1)]
        f = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (self.N + 1, self.dof))
        self.vlo, self.vhi = f(vlim_lo), f(vlim_hi)
        self.alo, self.ahi = _frs(alim_lo), _frs(alim_hi)
        self.s = [Fr(i / self.N) for i in range(self.N + 1)]          # the doubles i / N
        self.x0, self.xN = Fr(float(sd_start)) ** 2, Fr(float(sd_end)) ** 2

    def D(self, i):
        return self.s[i + 1] - self.s[i]

    def qs(self, k, s):
        return self.c1[k] + s * (2 * self.c2[k] + s * 3 * self.c3[k])

    def qss(self, k, s):
        return 2 * self.c2[k] + 6 * self.c3[k] * s

    def xbounds(self, i):
        """xlo, xhi of the velocity constraint at gridpoint i: xhi = min(1e8, min_k vlim_k / q'_k)^2, xlo likewise."""
        sdmin, sdmax = Fr(-MAXSD), Fr(MAXSD)
        for k in range(self.dof):
            v = self.qs(k, self.s[i])
            lo, hi = Fr(float(self.vlo[i, k])), Fr(float(self.vhi[i, k]))
            if v > 0:
                sdmax, sdmin = min(hi / v, sdmax), max(lo / v, sdmin)
            elif v < 0:
                sdmax, sdmin = min(lo / v, sdmax), max(hi / v, sdmin)
        return (sdmin * sdmin if sdmin > 0 else Fr(0)), sdmax * sdmax

    def accel_rows(self, i):
        """Rows (alpha, beta, gamma), alpha u + beta x <= gamma: collocation at i and interpolation (at N: collocation twice)."""
        R = []
        for k in range(self.dof):
            a, b = self.qs(k, self.s[i]), self.qss(k, self.s[i])
            a2, b2 = a, b
            if i < self.N:
                bn = self.qss(k, self.s[i + 1])
                a2, b2 = self.qs(k, self.s[i + 1]) + 2 * self.D(i) * bn, bn
            R += [(a, b, self.ahi[k]), (-a, -b, -self.alo[k]), (a2, b2, self.ahi[k]), (-a2, -b2, -self.alo[k])]
        return R

    def next_rows(self, i, klo, khi):
        return [(2 * self.D(i), Fr(1), khi), (-2 * self.D(i), Fr(-1), -klo)]


def _int_rows(rows):
    out = []
    for al, be, ga in rows:
        m = math.lcm(al.denominator, be.denominator, ga.denominator)
        out.append((int(al * m), int(be * m), int(ga * m)))
    return out


def x_range_by_vertices(rows):
    """Exact (min x, max x) over the polygon {(u, x): alpha u + beta x <= gamma for every row}, or None if it is empty.
    The polygon must be bounded (the next-set rows and the x bounds make it so).  Every pair of boundary lines is intersected;
    an intersection whose x lies inside the range found so far cannot move either end and is not tested for feasibility."""
    for al, be, ga in rows:
        if al == 0 and be == 0 and ga < 0:
            return None
    R = [r for r in _int_rows(rows) if r[0] != 0 or r[1] != 0]
    lo = hi = None                 # (numerator, denominator > 0)
    n = len(R)
    for i in range(n):
        ai, bi, gi = R[i]
        for j in range(i + 1, n):
            aj, bj, gj = R[j]
            det = ai * bj - aj * bi
            if det == 0:
                continue
            un, xn = gi * bj - gj * bi, ai * gj - aj * gi
            if det < 0:
                det, un, xn = -det, -un, -xn
            if lo is not None and xn * lo[1] >= lo[0] * det and xn * hi[1] <= hi[0] * det:
                continue
            if all(a * un + b * xn <= g * det for a, b, g in R):
                if lo is None or xn * lo[1] < lo[0] * det:
                    lo = (xn, det)
                if hi is None or xn * hi[1] > hi[0] * det:
                    hi = (xn, det)
    if lo is None:
        return None
    return Fr(*lo), Fr(*hi)


def backward_exact(plan, i, klo_next, khi_next):
    """Exact controllable set of stage i given the next one: (lo clamped at 0, hi), or None if the stage polygon is empty."""
    xlo, xhi = plan.xbounds(i)
    rows = plan.accel_rows(i) + plan.next_rows(i, klo_next, khi_next) + [(Fr(0), Fr(1), xhi), (Fr(0), Fr(-1), -xlo)]
    r = x_range_by_vertices(rows)
    return None if r is None else (max(r[0], Fr(0)), r[1])


def forward_exact(plan, i, xi, klo_next, khi_next):
    """Exact greedy step from x[i]: (greatest u, least u, x[i+1] clamped into K[i+1])."""
    umax = umin = None
    for al, be, ga in plan.accel_rows(i) + plan.next_rows(i, klo_next, khi_next):
        if al > 0:
            q = (ga - be * xi) / al
            umax = q if umax is None else min(umax, q)
        elif al < 0:
            q = (ga - be * xi) / al
            umin = q if umin is None else max(umin, q)
    return umax, umin, min(max(xi + 2 * plan.D(i) * umax, klo_next), khi_next)


def knot_times(x, N):
    """t from x by the definition, correctly rounded sums (math.fsum) of the double terms."""
    x = np.asarray(x, dtype=np.float64)
    terms = []
    for i in range(1, N + 1):
        D = i / N - (i - 1) / N
        sda = 0.5 * (math.sqrt(max(x[i - 1], 0.0)) + math.sqrt(max(x[i], 0.0)))
        terms.append(D / sda if sda > NEARLY_ZERO else 5.0)
    return np.array([math.fsum(terms[:i]) for i in range(N + 1)])


def certify(p0, p1, v0, v1, vlim_lo, vlim_hi, alim_lo, alim_hi, N, sd_start, sd_end, K, x, u, t, stages=None, detail=False):
    """Worst relative residual of the claimed solution (K [N+1, 2], x [N+1], u [N], t [N+1]) against the definition, over the
    stages in `stages` (default: all of 0 .. N-1).  Residuals, each relative to the largest exact magnitude of its quantity
    over the certified stages: K[i] (both ends) against the exact set; u[i] and x[i+1] against the exact step; how far the
    exact least u exceeds the exact greatest u (a state outside the controllable set); x[0] and K[N] against sd^2; t.
    An empty stage polygon gives inf.  detail=True returns the per-stage residuals as a dict with the worst under "worst"."""
    plan = Plan(p0, p1, v0, v1, vlim_lo, vlim_hi, alim_lo, alim_hi, N, sd_start, sd_end)
    K = np.asarray(K, dtype=np.float64); x = np.asarray(x, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64); t = np.asarray(t, dtype=np.float64)
    assert K.shape == (N + 1, 2) and x.shape == (N + 1,) and u.shape == (N,) and t.shape == (N + 1,)
    stages = list(range(N)) if stages is None else sorted(set(int(i) for i in stages))
    assert all(0 <= i < N for i in stages)
    dK, du, dx, feas = {}, {}, {}, {}
    sK, su, sx = plan.xN, Fr(0), plan.x0
    for i in stages:
        klo, khi = Fr(float(K[i + 1, 0])), Fr(float(K[i + 1, 1]))
        b = backward_exact(plan, i, klo, khi)
        if b is None:
            dK[i] = math.inf
        else:
            dK[i] = max(abs(Fr(float(K[i, 0])) - b[0]), abs(Fr(float(K[i, 1])) - b[1]))
            sK = max(sK, abs(b[1]))
        umax, umin, xn = forward_exact(plan, i, Fr(float(x[i])), klo, khi)
        du[i], dx[i] = abs(Fr(float(u[i])) - umax), abs(Fr(float(x[i + 1])) - xn)
        feas[i] = max(umin - umax, Fr(0)) if umin is not None else Fr(0)
        su, sx = max(su, abs(umax)), max(sx, abs(xn))
    rel = lambda d, s: {i: (float(v / s) if s else (0.0 if v == 0 else math.inf)) for i, v in d.items()}
    out = dict(K=rel(dK, sK), u=rel(du, su), x=rel(dx, sx), feasible=rel(feas, su))
    ends = max(abs(Fr(float(x[0])) - plan.x0) / (sx if sx else 1), abs(Fr(float(K[N, 0])) - plan.xN) / (sK if sK else 1),
               abs(Fr(float(K[N, 1])) - plan.xN) / (sK if sK else 1))
    tt = knot_times(x, N)
    out["t"] = float(np.max(np.abs(t - tt)) / np.max(np.abs(tt)))
    out["ends"] = float(ends)
    out["worst"] = max([out["t"], out["ends"]] + [v for k in ("K", "u", "x", "feasible") for v in out[k].values()])
    return out if detail else out["worst"]


def edge_stages(N, rng, most=12):
    """At most `most` stages of a long plan: 0, 1, N-2, N-1, the stages on either side of each multiple of 32 (thinned evenly
    if there are too many), the rest drawn from `rng`."""
    ends = sorted({i for i in (0, 1, N - 2, N - 1) if 0 <= i < N})
    sides = sorted({i for m in range(32, N, 32) for i in (m - 1, m) if 0 <= i < N} - set(ends))
    room = most - len(ends)
    if len(sides) > room:
        sides = [sides[(j * len(sides)) // room] for j in range(room)]
    got = set(ends) | set(sides)
    rest = [i for i in range(N) if i not in got]
    while len(got) < min(most, N):
        got.add(rest.pop(int(rng.integers(len(rest)))))
    return sorted(got)


def property_checks(r, p0, p1, v0, v1, vl, al, N):
    """The constraint-satisfaction properties of tests/test_oracle_toppra.py::test_toppra_constraints_hold_6dof on one
    solution r (K, x, u, t): limits kept, x inside K, knot times increasing.  They do not see time-optimality."""
    x, u, K = r["x"], r["u"], r["K"]
    assert np.all(x >= -1e-12) and np.all(x <= K[:, 1] + 1e-9) and np.all(x >= K[:, 0] - 1e-9)
    s = np.arange(N + 1) / N
    d = p1 - p0
    c2 = 3 * d - 2 * v0 - v1; c3 = -2 * d + v0 + v1
    qs = v0[None] + s[:, None] * (2 * c2[None] + 3 * c3[None] * s[:, None])
    qss = 2 * c2[None] + 6 * c3[None] * s[:, None]
    # velocity limits at every gridpoint
    assert np.all(np.abs(qs) * np.sqrt(np.maximum(x, 0))[:, None] <= vl[None] * (1 + 1e-9) + 1e-9)
    # acceleration limits at collocation points i < N
    a = qs[:-1] * u[:, None] + qss[:-1] * x[:-1, None]
    assert np.all(np.abs(a) <= al[None] * (1 + 1e-9) + 1e-9)
    # time-optimality signature: forward pass saturates some constraint or the K bound
    assert np.all(np.diff(r["t"]) > 0)


# ---- sampling -------------------------------------------------------------------------------------------------------------

def spline_reference(p0, p1, v0, v1, x, t, times):
    """pos, vel, acc [dof, len(times)] (float64) of the clamped cubic spline through (t_i, q_k(i / N)) with end slopes
    q'_k(0) sqrt(x_0) and q'_k(1) sqrt(x_N): one dense solve for the second derivatives, no knot is dropped."""
    p0, p1, v0, v1, x, t, times = (np.asarray(a, dtype=np.float64) for a in (p0, p1, v0, v1, x, t, times))
    n = t.shape[0]
    h = np.diff(t)
    assert np.all(h >= NEARLY_ZERO), "knot times must differ by at least 1e-8"
    s = np.arange(n) / (n - 1)
    c2, c3 = 3 * (p1 - p0) - 2 * v0 - v1, -2 * (p1 - p0) + v0 + v1
    y = p0[:, None] + s * (v0[:, None] + s * (c2[:, None] + s * c3[:, None]))
    d0, d1 = v0 * np.sqrt(max(x[0], 0.0)), (v0 + 2 * c2 + 3 * c3) * np.sqrt(max(x[-1], 0.0))
    sl = np.diff(y, axis=1) / h
    A = np.zeros((n, n)); rhs = np.zeros((y.shape[0], n))
    A[0, 0], A[0, 1], rhs[:, 0] = 2 * h[0], h[0], 6 * (sl[:, 0] - d0)
    A[-1, -1], A[-1, -2], rhs[:, -1] = 2 * h[-1], h[-1], 6 * (d1 - sl[:, -1])
    for j in range(1, n - 1):
        A[j, j - 1], A[j, j], A[j, j + 1] = h[j - 1], 2 * (h[j - 1] + h[j]), h[j]
        rhs[:, j] = 6 * (sl[:, j] - sl[:, j - 1])
    M = np.linalg.solve(A, rhs.T).T
    g = np.clip(np.searchsorted(t, times, side="left") - 1, 0, n - 2)
    hg, a, b = h[g], t[g + 1] - times, times - t[g]
    m0, m1 = M[:, g], M[:, g + 1]
    ca, cb = y[:, g] / hg - m0 * hg / 6, y[:, g + 1] / hg - m1 * hg / 6
    pos = (m0 * a ** 3 + m1 * b ** 3) / (6 * hg) + ca * a + cb * b
    vel = (m1 * b ** 2 - m0 * a ** 2) / (2 * hg) - ca + cb
    acc = (m0 * a + m1 * b) / hg
    return pos, vel, acc


def sample_times(T, dt):
    """The sample times of parametrizer::Spline's uniform sampling: ceil(T / dt) of them, the last one T itself."""
    n = int(math.ceil(T / dt))
    tt = np.array([(T * j) / (n - 1) for j in range(n)]) if n > 1 else np.zeros(n)
    if n > 1:
        tt[-1] = T
    return tt


def sample_residual(got, ref):
    """Worst |got - ref| over a [dof, n] block, relative to the reference's largest magnitude of each joint."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref), axis=1)))


# ---- inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------

def random_plan(rng, dof, N, per_stage):
    """One plan's inputs: non-zero end velocities, asymmetric acceleration limits, constant or per-stage velocity limits.
    Generous enough that plans are usually solvable; the tests assert status 0."""
    p0 = rng.uniform(-2, 2, dof); p1 = p0 + rng.uniform(0.5, 3, dof) * rng.choice([-1.0, 1.0], dof)
    v0 = rng.uniform(-0.5, 0.5, dof); v1 = rng.uniform(-0.5, 0.5, dof)
    al = rng.uniform(2.0, 6.0, dof)
    alo, ahi = -al, al * rng.uniform(0.5, 1.5, dof)
    vhi = rng.uniform(1.0, 3.0, dof)
    if per_stage:
        vhi = vhi[None, :] * (0.6 + 0.4 * np.abs(np.sin(rng.uniform(1, 6) * np.arange(N + 1) / N)))[:, None]
    return dict(p0=p0, p1=p1, v0=v0, v1=v1, vlo=-vhi, vhi=vhi, alo=alo, ahi=ahi)


def random_plans(seed, dof, N, per_stage, P):
    rng = np.random.default_rng(seed)
    return [random_plan(rng, dof, N, per_stage) for _ in range(P)]


IDLE = None     # a joint that does not move: p0 = p1, zero end velocities (every row of it has a zero u coefficient)

# name -> (scale c_k of each joint, or IDLE; index of a joint whose limits are multiplied by 1000, or None; exact)
# exact: every c_k is a signed power of two, so every row is the 1-dof row times a power of two or a row the 1-dof problem has
# with the other sign, every bound is the same double, and K, x, u, t are bit-equal to the 1-dof result; a slack joint's bounds
# are never the least or the greatest, which changes no minimum.  Otherwise the scaled inputs are rounded: agreement to 1e-12.
REPLICAS = {
    "dof2": ((1.0, 3.0), None, False),
    "dof3_idle": ((1.0, IDLE, -0.5), None, True),
    "dof6_pow2": ((1.0, 0.5, 2.0, -1.0, 4.0, -0.25), None, True),
    "dof6_general": ((1.0, 3.0, 0.3, -7.0, 1.7, 0.01), None, False),
    "dof7_slack": ((1.0, 0.5, 2.0, -1.0, 4.0, -0.25, 1.0), 6, True),
    "dof8_idle": ((1.0, 3.0, 0.3, IDLE, -7.0, 1.7, 0.01, -2.0), None, False),
    "dof16_pow2": (tuple((-2.0) ** (k - 8) for k in range(16)), None, True),
}


def scaled_replica(p1, v0, v1, vlo, vhi, alo, ahi, c, slack=None):
    """A multi-joint plan whose joint k is the 1-dof plan (p0 = 0, p1, v0, v1, limits) times c[k]; limits swap where c[k] < 0.
    It has the same s(t) as the 1-dof plan."""
    out = {k: np.zeros(len(c)) for k in ("p0", "p1", "v0", "v1", "vlo", "vhi", "alo", "ahi")}
    for k, ck in enumerate(c):
        if ck is IDLE:
            out["vlo"][k], out["vhi"][k], out["alo"][k], out["ahi"][k] = -1.0, 1.0, -1.0, 1.0
            continue
        m = 1000.0 if k == slack else 1.0
        out["p1"][k], out["v0"][k], out["v1"][k] = ck * p1, ck * v0, ck * v1
        lim = lambda lo, hi: (m * ck * lo, m * ck * hi) if ck > 0 else (m * ck * hi, m * ck * lo)
        out["vlo"][k], out["vhi"][k] = lim(vlo, vhi)
        out["alo"][k], out["ahi"][k] = lim(alo, ahi)
    return out


# the four 1-dof plans of test_toppra_zero_divisor_pair (N = 4, sd_start = sd_end = 0.5): at s = 0.25 the collocation slot has
# alpha = 1 = 2 Delta beta, a row pair whose divisor is exactly zero
ZERO_DIVISOR = dict(N=4, sd=0.5, p1=1.5, v0=0.5, v1=2.5, vl=50.0, alo=(-4.0, 0.5, 1.0, -40.0), ahi=(4.0, 4.0, 4.0, 40.0))
ZERO_DIVISOR_SCALES = {     # signed powers of two keep the exact zero exact
    3: (1.0, IDLE, -2.0),
    7: (1.0, -0.5, IDLE, 4.0, -1.0, 0.25, 2.0),
    8: (-1.0, 0.5, 2.0, IDLE, -4.0, 1.0, 0.125, -8.0),
    16: tuple(IDLE if k == 5 else (-2.0) ** (k - 8) for k in range(16)),
}


# (dof, N) of the certified random plans.  Fast kernel (dof <= 7, every stage certified): every template instance and every
# residue of N modulo its chunk of 4 stages.  Wide kernel (edge_stages): around its chunks of 32 stages.
FAST_SHAPES = [(1, 5), (2, 9), (3, 4), (4, 7), (5, 8), (6, 13), (7, 9), (6, 32), (2, 1), (7, 2)]
WIDE_SHAPES = [(8, 31), (8, 33), (12, 32), (16, 65)]
# per-stage limits at 16 joints: staged in LDS while 8 (35 (N + 1) + 2049) <= 65536 bytes, that is up to N = 174; from N = 175
# on the kernel reads them from global memory
WIDE_PER_STAGE_SHAPES = [(16, 150), (16, 174), (16, 175), (16, 200)]
SAMPLE_SHAPES = [(3, 33), (7, 31), (8, 32), (16, 65)]
# the same plans started and ended in motion (path speeds sd_start, sd_end), per-stage limits
MOVING_ENDS_SHAPES = [(2, 9), (5, 8), (6, 13), (7, 9), (8, 33), (16, 65)]
MOVING_ENDS = (0.3, 0.2)
PLANS_PER_SHAPE = 3


def shape_plans(dof, N, per_stage, P=PLANS_PER_SHAPE):
    """The plans of one shape (the same on the CPU, where the oracle is certified on them, and on the GPU) and the stages to certify."""
    seed = 1000 * dof + 10 * N + int(per_stage)
    plans = random_plans(seed, dof, N, per_stage, P)
    rng = np.random.default_rng(seed + 5)
    stages = [None if dof <= 7 else edge_stages(N, rng) for _ in plans]
    return plans, stages


def certify_plan(pl, N, r, stages=None, sd_start=0.0, sd_end=0.0, detail=False):
    return certify(pl["p0"], pl["p1"], pl["v0"], pl["v1"], pl["vlo"], pl["vhi"], pl["alo"], pl["ahi"], N, sd_start, sd_end,
                   r["K"], r["x"], r["u"], r["t"], stages=stages, detail=detail)


def stack(plans):
    """A list of plans as one batch: arrays [P, dof] (velocity limits [P, N+1, dof] where they are per stage)."""
    return {k: np.ascontiguousarray(np.stack([pl[k] for pl in plans]), dtype=np.float64) for k in plans[0]}
