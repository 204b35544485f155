"""The CPU twin of the per-stage speed limits (tests/speed_twin.py) on the recorded example path: with every term off it
is the constant limit and oracle.toppra reproduces the recording's duration; with curvature and clearance terms on the
profile is feasible, slower, and respects the limit at every interior knot; and the window and clamp rules at their edges
(N = 1, J = 1, one leg, one-column and one-row grids, a curve leaving the frame).  No GPU."""
import os

import numpy as np
import pytest

import speed_twin

INF = float("inf")


@pytest.fixture(scope="module")
def example(oracle, golden_dir):
    fx = np.load(os.path.join(golden_dir, "toppra_1dof_output.npz"))
    ctrl = oracle.bezier_from_path(fx["waypoints"])
    _, cum = oracle.bezier_arclength(ctrl, 100)
    cum = cum.astype(np.float32)
    AL = np.float32(0.0)
    for v in cum[:, -1]:
        AL = np.float32(AL + v)
    lim = (float(fx["vel_lim"][0]), float(fx["vel_lim"][1]), float(fx["acc_lim"][0]), float(fx["acc_lim"][1]))
    return dict(fx=fx, ctrl=ctrl, cum=cum, AL=AL, lim=lim)


def _toppra(oracle, e, tw, N=100):
    lim = e["lim"]
    return oracle.toppra([0.0], [float(e["AL"])], [0.0], [0.0], tw["vlo"][:, None], tw["vhi"][:, None], [lim[2]], [lim[3]], N=N)


def _grid():
    """A 64 x 48 grid over the example path with an obstacle block beside its corner."""
    from oracle import oracle
    occ = np.zeros((48, 64), np.uint8)
    occ[2:6, 56:60] = 1
    return oracle.edt(occ), (np.float32(-1.0), np.float32(-1.0), np.float32(0.2), np.float32(0.25))


def test_terms_off_is_the_constant_limit(oracle, example):
    tw = speed_twin.speed_limits(example["ctrl"], example["cum"], example["AL"], example["lim"], (INF, INF, INF, 0.0))
    assert np.array_equal(tw["vhi"], np.full(101, example["lim"][1])) and np.array_equal(tw["vlo"], np.full(101, example["lim"][0]))
    assert tw["min_clear"] == INF
    r = _toppra(oracle, example, tw)
    assert r["status"] == 0
    T = float(example["fx"]["time"][-1])
    assert abs(r["t"][-1] - T) < 2e-5, (r["t"][-1], T)


def test_limits_slow_the_profile_and_hold_at_the_knots(oracle, example):
    d2, frame = _grid()
    off = _toppra(oracle, example, speed_twin.speed_limits(example["ctrl"], example["cum"], example["AL"], example["lim"], (INF, INF, INF, 0.0)))
    tw = speed_twin.speed_limits(example["ctrl"], example["cum"], example["AL"], example["lim"], (0.05, 0.02, 0.05, 0.5), d2=d2, frame=frame)
    assert tw["vhi"].min() < example["lim"][1] and (tw["vhi"] > 0).all() and (tw["vhi"] <= example["lim"][1]).all()
    assert np.isfinite(tw["min_clear"]) and tw["min_clear"] >= 0
    r = _toppra(oracle, example, tw)
    assert r["status"] == 0
    assert np.isfinite(r["t"][-1]) and r["t"][-1] > off["t"][-1]
    s = np.arange(101) / 100
    dq = float(example["AL"]) * (6 * s - 6 * s * s)             # q'(s_i) of the Hermite path
    i = np.arange(1, 100)
    assert (r["x"][i] <= (tw["vhi"][i] / dq[i]) ** 2 * (1 + 1e-9)).all()


def test_curvature_term_alone_matches_its_formula(example):
    """omega only: at a stage the limit is omega / (the largest curvature in its window), never above vel_max."""
    tw = speed_twin.speed_limits(example["ctrl"], example["cum"], example["AL"], example["lim"], (0.05, INF, INF, 0.0), J=4)
    x = tw["x"]
    leg, t, _ = speed_twin.locate(x, example["cum"])
    from oracle import oracle
    d1 = oracle.bezier_eval(example["ctrl"], leg.ravel().astype(np.int32), t.ravel(), 1)
    dd = oracle.bezier_eval(example["ctrl"], leg.ravel().astype(np.int32), t.ravel(), 2)
    kap = np.abs(d1[:, 0] * dd[:, 1] - d1[:, 1] * dd[:, 0]) / (d1[:, 0] ** 2 + d1[:, 1] ** 2) ** 1.5
    kmax = kap.reshape(x.shape).max(axis=1)
    with np.errstate(divide="ignore"):
        exp = np.minimum(example["lim"][1], 0.05 / kmax)
    assert np.allclose(tw["vhi"], exp, rtol=1e-12, atol=0)
    assert tw["vhi"].argmin() in range(40, 61)                   # the corner of the example lies mid-way


def test_window_edges():
    # N = 1: two stages that share the whole curve between them; J = 1: the gridpoint and the two window ends
    x = speed_twin.window_samples(8.0, 1, 1)
    assert np.array_equal(x, np.array([[0.0, 0.0, 4.0], [4.0, 8.0, 8.0]]))
    x = speed_twin.window_samples(3.0, 7, 32)
    a = speed_twin.gridpoints(3.0, 7)
    assert x.shape == (8, 65) and np.array_equal(x[:, 32], a) and x.min() == 0.0 and x.max() == 3.0
    assert (np.diff(x, axis=1) >= 0).all() and np.allclose(x[1:, 0], x[:-1, -1], rtol=0, atol=1e-15)   # windows tile [0, AL]


def test_locate_one_leg_and_table_ends(oracle):
    ctrl = oracle.bezier_from_path(np.array([[0, 0], [2, 1]], np.float32))
    assert ctrl.shape[0] == 1
    for nsub in (1, 10):
        _, cum = oracle.bezier_arclength(ctrl, nsub)
        cum = cum.astype(np.float32)
        AL = float(cum[0, -1])
        leg, t, B = speed_twin.locate(np.array([0.0, AL / 2, AL]), cum)
        assert (leg == 0).all() and t[0] == 0.0 and t[2] == 1.0 and 0.0 < t[1] < 1.0 and np.array_equal(B, [0.0, AL])
        tw = speed_twin.speed_limits(ctrl, cum, np.float32(AL), (-1.0, 1.0, -1.0, 1.0), (0.5, 0.5, INF, 0.0), N=1, J=1)
        assert tw["vhi"].shape == (2,) and not tw["flagged"].any()


def test_clearance_clamps():
    d2 = np.arange(40, dtype=np.int32)[:, None] ** 2            # 40 x 1: one column, clearance = row * res
    fr = (np.float32(0.0), np.float32(0.0), np.float32(0.5), np.float32(0.5))
    c = speed_twin.clearance(np.array([0.25, -9.0, 77.0]), np.array([0.25 + 0.5 * 3.5, 5.25, 5.25]), d2, fr)
    assert np.allclose(c, [0.5 * 3.5, 0.5 * 10, 0.5 * 10], rtol=1e-15)          # x is ignored: the second column is the first
    c = speed_twin.clearance(np.array([5.25, 5.25]), np.array([-3.0, 99.0]), d2.T.copy(), fr)   # 1 x 40, leaving it in y
    assert np.allclose(c, [0.5 * 10, 0.5 * 10], rtol=1e-15)
    d2 = np.zeros((4, 5), np.int32)
    d2[:, 4] = 9
    c = speed_twin.clearance(np.array([-50.0, 50.0, 2.0]), np.array([50.0, -50.0, 1.0]), d2, fr)  # outside: the border centres
    assert np.allclose(c, [0.0, 1.5, 0.5 * 1.5], rtol=1e-15)
    inf = np.full((3, 3), 2**31 - 1, np.int32)                  # no obstacle: finite, large
    assert np.isfinite(speed_twin.clearance(np.array([0.7]), np.array([0.7]), inf, fr)).all()
