"""The TOPP-RA oracle beyond one joint, held to something that is not itself: the exact stage certificate of
tests/toppra_cert.py (vertex enumeration in rational arithmetic), scaled replicas of the reference's recorded 1-dof run, and a
dense-solve spline.  The plans certified here are the ones tests/test_gpu_toppra_cert.py runs through the kernels: the kernels'
1e-9 there rests on the oracle's 1e-10 here."""
import os

import numpy as np
import pytest

import toppra_cert as tc

ORACLE_TOL = 1e-10     # the oracle against the certificate; measured: 1.4e-14 at worst on these plans


def _solve(oracle, pl, N, sd_start=0.0, sd_end=0.0):
    return oracle.toppra(pl["p0"], pl["p1"], pl["v0"], pl["v1"], pl["vlo"], pl["vhi"], pl["alo"], pl["ahi"], N=N,
                         sd_start=sd_start, sd_end=sd_end)


SHAPES = ([(d, n, ps) for d, n in tc.FAST_SHAPES + tc.WIDE_SHAPES for ps in (0, 1)] +
          [(d, n, 1) for d, n in tc.WIDE_PER_STAGE_SHAPES] + [(d, n, ps) for d, n in tc.SAMPLE_SHAPES for ps in (0, 1)])


@pytest.mark.parametrize("dof,N,per_stage", sorted(set(SHAPES)))
def test_oracle_passes_certificate(oracle, dof, N, per_stage):
    """Constant and per-stage velocity limits, asymmetric acceleration limits, 1 .. 16 joints: every stage up to 7 joints, at
    most 12 stages (the ends, the sides of the multiples of 32, a few at random) beyond."""
    plans, stages = tc.shape_plans(dof, N, per_stage)
    for pl, st in zip(plans, stages):
        assert st is None or len(st) <= 12
        r = _solve(oracle, pl, N)
        assert r["status"] == 0
        res = tc.certify_plan(pl, N, r, stages=st)
        print(f"oracle certificate dof={dof} N={N} per_stage={per_stage}: {res:.2e}")
        assert res <= ORACLE_TOL


@pytest.mark.parametrize("dof,N", tc.MOVING_ENDS_SHAPES)
def test_oracle_passes_certificate_moving_ends(oracle, dof, N):
    """Plans that start and end in motion: x[0] = sd_start^2 inside K[0], K[N] = sd_end^2."""
    plans, stages = tc.shape_plans(dof, N, 1)
    for pl, st in zip(plans, stages):
        r = _solve(oracle, pl, N, *tc.MOVING_ENDS)
        assert r["status"] == 0
        assert tc.certify_plan(pl, N, r, st, *tc.MOVING_ENDS) <= ORACLE_TOL


def test_certificate_rejects_what_the_property_test_accepts(oracle):
    """A controllable set slightly too small, a lower end slightly too high, a forward u slightly below the maximum: each keeps
    every limit (the assertions of test_toppra_constraints_hold_6dof pass on it) and each is reported by the certificate, at
    the stage it was made in and nowhere else."""
    rng = np.random.default_rng(7)
    dof, N = 6, 200
    vl = np.array([2, 2, 2, 3, 3, 3.0]); al = np.array([5, 5, 5, 8, 8, 8.0])
    p0 = rng.uniform(-np.pi, np.pi, dof); p1 = rng.uniform(-np.pi, np.pi, dof)
    v0 = rng.uniform(-1, 1, dof); v1 = rng.uniform(-1, 1, dof)
    pl = dict(p0=p0, p1=p1, v0=v0, v1=v1, vlo=-vl, vhi=vl, alo=-al, ahi=al)
    r = _solve(oracle, pl, N)
    assert r["status"] == 0
    tc.property_checks(r, p0, p1, v0, v1, vl, al, N)
    # a stage where the state is well inside its controllable set and the step is not small
    inside = np.flatnonzero((r["x"][:N] < r["K"][:N, 1] * (1 - 1e-3)) & (r["x"][:N] > r["K"][:N, 0] + 1e-3 * r["K"][:N, 1]))
    i = int(inside[np.argmax(np.abs(r["u"][inside]))])
    near = [i - 1, i, i + 1]
    assert tc.certify_plan(pl, N, r, stages=near) <= ORACLE_TOL
    copy = lambda: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    small = copy(); small["K"][i, 1] *= 1 - 1e-6
    high = copy(); high["K"][i, 0] += 1e-6 * r["K"][i, 1]
    slow = copy(); slow["u"][i] -= 1e-6 * abs(r["u"][i])
    for bad, key in ((small, "K"), (high, "K"), (slow, "u")):
        tc.property_checks(bad, p0, p1, v0, v1, vl, al, N)          # the old test does not see it
        d = tc.certify_plan(pl, N, bad, stages=near, detail=True)
        assert d[key][i] >= 1e-7, (key, d[key])
        assert d["worst"] >= 1e-7
    # stage i - 1 takes the claimed K[i] as its input: the certificate's verdicts are local
    d = tc.certify_plan(pl, N, slow, stages=near, detail=True)
    assert max(d["K"].values()) <= ORACLE_TOL and d["u"][i - 1] <= ORACLE_TOL and d["u"][i + 1] <= ORACLE_TOL


def test_vertex_enumeration_on_known_polygons():
    """The certificate's own linear-programme solver on polygons whose answer is plain: a square, a triangle, a segment (two
    rows that meet in equality), an empty set."""
    from fractions import Fraction as F
    row = lambda a, b, g: (F(a), F(b), F(g))
    square = [row(1, 0, 2), row(-1, 0, 1), row(0, 1, 5), row(0, -1, -3)]                 # -1 <= u <= 2, 3 <= x <= 5
    assert tc.x_range_by_vertices(square) == (3, 5)
    tri = [row(1, 1, 4), row(-1, 1, 0), row(0, -1, 0)]                                    # x <= 4 - u, x <= u, x >= 0
    assert tc.x_range_by_vertices(tri) == (0, 2)
    seg = [row(2, 1, 1), row(-2, -1, -1), row(0, 1, F(3, 4)), row(0, -1, F(-1, 4))]      # x + 2 u = 1, 1/4 <= x <= 3/4
    assert tc.x_range_by_vertices(seg) == (F(1, 4), F(3, 4))
    assert tc.x_range_by_vertices(square + [row(0, 1, 2)]) is None                        # x <= 2 and x >= 3
    assert tc.x_range_by_vertices(square + [row(0, 0, -1)]) is None                       # 0 <= -1
    assert tc.x_range_by_vertices(square + [row(0, 0, 1)]) == (3, 5)


@pytest.mark.parametrize("dof,N", tc.SAMPLE_SHAPES)
def test_oracle_sampling_matches_dense_spline(oracle, dof, N):
    """sco_toppra_sample (Thomas sweep, knot dropping) against one dense solve of the same clamped spline."""
    plans, _ = tc.shape_plans(dof, N, 0)
    for pl in plans:
        r = _solve(oracle, pl, N)
        assert r["status"] == 0
        s = oracle.toppra_sample(pl["p0"], pl["p1"], pl["v0"], pl["v1"], r["x"], r["t"], 0.02)
        assert s["length"] == int(np.ceil(r["t"][-1] / 0.02)) and s["length"] > 20
        assert np.array_equal(s["time"], tc.sample_times(r["t"][-1], 0.02))
        ref = tc.spline_reference(pl["p0"], pl["p1"], pl["v0"], pl["v1"], r["x"], r["t"], s["time"])
        for k, q in zip(("pos", "vel", "acc"), ref):
            res = tc.sample_residual(s[k], q)
            print(f"oracle sampling dof={dof} N={N} {k}: {res:.2e}")
            assert res < 1e-5
            assert res < 2e-7


@pytest.mark.parametrize("dof,N", tc.SAMPLE_SHAPES)
def test_dense_spline_matches_scipy(oracle, dof, N):
    """The NumPy reference against scipy's clamped CubicSpline, both in fp64.  The second-derivative system is tridiagonal and
    diagonally dominant, its condition number at most 3 max h / min h (below 1e3 on these knots), so the two agree to about
    1e3 * 2^-53 * (N + 1) < 1e-11 of each quantity's largest magnitude; 1e-10 is asserted."""
    CubicSpline = pytest.importorskip("scipy.interpolate").CubicSpline
    plans, _ = tc.shape_plans(dof, N, 0)
    for pl in plans:
        r = _solve(oracle, pl, N)
        h = np.diff(r["t"])
        assert h.min() >= 1e-8 and 3 * h.max() / h.min() < 1e3
        times = tc.sample_times(r["t"][-1], 0.02)
        ref = tc.spline_reference(pl["p0"], pl["p1"], pl["v0"], pl["v1"], r["x"], r["t"], times)
        s = np.arange(N + 1) / N
        d = pl["p1"] - pl["p0"]
        c2, c3 = 3 * d - 2 * pl["v0"] - pl["v1"], -2 * d + pl["v0"] + pl["v1"]
        for k in range(dof):
            y = pl["p0"][k] + s * (pl["v0"][k] + s * (c2[k] + s * c3[k]))
            d0, d1 = pl["v0"][k] * np.sqrt(r["x"][0]), pl["v1"][k] * np.sqrt(r["x"][-1])
            cs = CubicSpline(r["t"], y, bc_type=((1, d0), (1, d1)))
            for nu, q in enumerate(ref):
                want = cs(times, nu)
                assert np.max(np.abs(q[k] - want)) <= 1e-10 * np.max(np.abs(want)), (k, nu)


# ---- scaled replicas of the recorded run -----------------------------------------------------------------------------------

def _fixture(golden_dir):
    fx = np.load(os.path.join(golden_dir, "toppra_1dof_output.npz"))
    one = dict(p1=float(fx["arclength"]), v0=0.0, v1=0.0, vlo=float(fx["vel_lim"][0]), vhi=float(fx["vel_lim"][1]),
               alo=float(fx["acc_lim"][0]), ahi=float(fx["acc_lim"][1]))
    return fx, one


@pytest.mark.parametrize("name", sorted(tc.REPLICAS))
def test_oracle_scaled_replicas_of_the_recording(oracle, golden_dir, name):
    """Joint k = the recorded 1-dof problem times c_k: the same s(t), so the recorded duration, sample times and (divided by
    c_k) profiles must come out of the multi-joint code path, and K, x, u, t must be those of the 1-dof plan."""
    c, slack, exact = tc.REPLICAS[name]
    fx, one = _fixture(golden_dir)
    N = 100
    r1 = oracle.toppra([0.0], [one["p1"]], [0.0], [0.0], [one["vlo"]], [one["vhi"]], [one["alo"]], [one["ahi"]], N=N)
    pl = tc.scaled_replica(c=c, slack=slack, **one)
    r = _solve(oracle, pl, N)
    assert r["status"] == r1["status"] == 0
    for k in ("K", "x", "u", "t"):
        if exact:
            assert np.array_equal(r[k], r1[k]), k
        else:
            assert np.max(np.abs(r[k] - r1[k])) <= 1e-12 * np.max(np.abs(r1[k])), k
    assert np.float32(r["t"][-1]) == fx["time"][-1]
    dt = float(np.float32(0.02))
    s = oracle.toppra_sample(pl["p0"], pl["p1"], pl["v0"], pl["v1"], r["x"], r["t"], dt)
    assert s["length"] == 4328
    assert np.array_equal(s["time"].astype(np.float32), fx["time"])
    rel = lambda a, b: np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b))
    for k, ck in enumerate(c):
        if ck is tc.IDLE:
            assert not s["vel"][k].any() and not s["acc"][k].any() and not s["pos"][k].any()
            continue
        assert rel(s["vel"][k].astype(np.float64) / ck, fx["vel"]) < 2e-7, k
        assert rel(s["acc"][k].astype(np.float64) / ck, fx["acc"]) < 2e-7, k
    assert tc.certify_plan(pl, N, r, stages=tc.edge_stages(N, np.random.default_rng(3))) <= ORACLE_TOL


@pytest.mark.parametrize("dof", sorted(tc.ZERO_DIVISOR_SCALES))
def test_oracle_zero_divisor_pair_beyond_one_joint(oracle, dof):
    """The four plans of test_toppra_zero_divisor_pair as power-of-two scaled, sign-flipped copies of that joint plus an idle
    joint: the exact zero divisor stays exact, statuses and (bit for bit) solutions are the 1-dof ones."""
    z = tc.ZERO_DIVISOR
    seen = set()
    for alo, ahi in zip(z["alo"], z["ahi"]):
        r1 = oracle.toppra([0.0], [z["p1"]], [z["v0"]], [z["v1"]], [-z["vl"]], [z["vl"]], [alo], [ahi], N=z["N"],
                           sd_start=z["sd"], sd_end=z["sd"])
        pl = tc.scaled_replica(z["p1"], z["v0"], z["v1"], -z["vl"], z["vl"], alo, ahi, tc.ZERO_DIVISOR_SCALES[dof])
        r = _solve(oracle, pl, z["N"], z["sd"], z["sd"])
        assert r["status"] == r1["status"]
        seen.add(r["status"])
        if r["status"] == 0:
            for k in ("K", "x", "u", "t"):
                assert np.array_equal(r[k], r1[k]), k
            assert tc.certify_plan(pl, z["N"], r, sd_start=z["sd"], sd_end=z["sd"]) <= ORACLE_TOL
    assert 0 in seen and len(seen) > 1
