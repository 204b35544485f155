"""The CPU twin of the weighted cost fields (tests/cpp/field_w_ref.c): its g against scipy's Dijkstra over the weighted
graph, its anchor (pen_cap = 0) against the unweighted twin, the wall map on which the weighted path keeps its distance,
and the edge cases of the read-out.  No GPU."""
import numpy as np
import pytest

from sea_current_amd import synth
from field_twin import INF, Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED, Twin, d2_of, serpentine
from field_w_twin import TwinW, field_w_scipy, path_weighted_cost, penalty_numpy, wall_map


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return TwinW(tmp_path_factory.mktemp("field_w_ref"))


@pytest.fixture(scope="module")
def twin0(tmp_path_factory):
    return Twin(tmp_path_factory.mktemp("field_ref_for_w"))


def _maps(oracle):
    out = [("salt97x61", oracle.edt(synth.salt_grid(97, 61, 0.15, seed=1)), 0),
           ("salt64x64", oracle.edt(synth.salt_grid(64, 64, 0.15, seed=2)), 0),
           ("serpentine", d2_of(serpentine(64)), 0),
           ("1x90", oracle.edt(synth.salt_grid(1, 90, 0.0, seed=3)), 0),
           ("90x1", oracle.edt(synth.salt_grid(90, 1, 0.0, seed=4)), 0)]
    return out


def _pen(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _roots(d2, r2, k, seed):
    rng = np.random.default_rng(seed)
    T = np.flatnonzero(d2.ravel() >= max(r2, 1))
    return [int(x) for x in rng.choice(T, size=min(k, T.size), replace=False)]


def test_twin_field_equals_scipy(twin, oracle):
    for i, (name, d2, r2) in enumerate(_maps(oracle)):
        pen = _pen(d2.shape, 20 + i)
        for cap in (255, 7):
            for root in _roots(d2, r2, 2, 11):
                g, st = twin.field(d2, pen, root, r2, cap)
                assert st == Q_OK, name
                np.testing.assert_array_equal(g, field_w_scipy(d2, pen, root, r2, cap), err_msg=f"{name} cap {cap}")


def test_penalty_formula_small_values():
    d2 = np.array([[0, 1, 2, 4, 9, 25, 35, 36, 37, 2**31 - 1]], np.int32)
    # s10 = 60: 40 * (60 - isqrt(100 d2)) // 60
    np.testing.assert_array_equal(penalty_numpy(d2, 0, 36, 40), [[0, 33, 30, 26, 20, 6, 0, 0, 0, 0]])
    np.testing.assert_array_equal(penalty_numpy(d2, 4, 36, 40), [[0, 0, 0, 26, 20, 6, 0, 0, 0, 0]])
    assert not penalty_numpy(d2, 0, 36, 0).any()


def test_cap_zero_equals_unweighted_twin(twin, twin0, oracle):
    maps = _maps(oracle) + [("blocks_r2", oracle.edt(synth.block_grid(128, 96, 0.2, seed=7, smin=3, smax=16)), 4)]
    for i, (name, d2, r2) in enumerate(maps):
        H, W = d2.shape
        pen = _pen(d2.shape, 40 + i)
        tg = np.random.default_rng(5).integers(0, W * H, size=100).astype(np.int32)
        for root in _roots(d2, r2, 2, 13):
            g, st = twin.field(d2, pen, root, r2, 0)
            g0, st0 = twin0.field(d2, root, r2)
            assert st == st0
            np.testing.assert_array_equal(g, g0, err_msg=name)
            for Lmax in (4096, 8):
                for to_root in (False, True):
                    a = twin.paths(d2, pen, g, root, tg, r2=r2, cap=0, Lmax=Lmax, to_root=to_root)
                    b = twin0.paths(d2, g0, root, tg, r2=r2, Lmax=Lmax, to_root=to_root)
                    for k in ("status", "len", "cost"):
                        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
                    for q in np.flatnonzero(b["status"] == Q_OK):
                        np.testing.assert_array_equal(a["path"][q, :b["len"][q]], b["path"][q, :b["len"][q]], err_msg=name)


def test_wall_map_weighted_path_keeps_its_distance(twin, twin0, oracle):
    occ, root, target = wall_map()
    d2 = oracle.edt(occ)
    pen = penalty_numpy(d2, 0, 36, 40)
    gw, _ = twin.field(d2, pen, root)
    g0, _ = twin0.field(d2, root)
    np.testing.assert_array_equal(gw, field_w_scipy(d2, pen, root))
    tg = np.array([target], np.int32)
    pw = twin.paths(d2, pen, gw, root, tg)
    p0 = twin0.paths(d2, g0, root, tg)
    assert pw["status"][0] == Q_OK and p0["status"][0] == Q_OK
    path_w, path_0 = pw["path"][0, :pw["len"][0]], p0["path"][0, :p0["len"][0]]
    assert path_w[0] == root and path_w[-1] == target and path_0[0] == root and path_0[-1] == target
    assert path_weighted_cost(path_w, pen) == gw.flat[target] == pw["cost"][0]
    assert d2.ravel()[path_w].min() > d2.ravel()[path_0].min()
    assert gw.flat[target] < path_weighted_cost(path_0, pen)
    assert gw.flat[target] > g0.flat[target]


def test_twin_edge_cases(twin):
    occ = np.zeros((20, 30), np.uint8)
    occ[5:15, 10] = occ[5:15, 20] = 1
    occ[5, 10:21] = occ[14, 10:21] = 1          # an enclosed pocket (rows 6..13, columns 11..19)
    occ[2, 2] = 1
    d2 = d2_of(occ)
    H, W = d2.shape
    pen = _pen(d2.shape, 3)
    root = 0
    g, st = twin.field(d2, pen, root)
    assert st == Q_OK and g[0, 0] == 0           # the root's own penalty is never paid
    assert np.all(g[6:14, 11:20] == INF) and g[2, 2] == INF
    tg = np.array([0, 2 * W + 2, 9 * W + 15, -1, W * H, W * H - 1, 3], np.int32)
    out = twin.paths(d2, pen, g, root, tg)
    np.testing.assert_array_equal(out["status"], [Q_OK, Q_BAD_ENDPOINT, Q_NO_PATH, Q_BAD_ENDPOINT, Q_BAD_ENDPOINT, Q_OK, Q_OK])
    assert out["len"][0] == 1 and out["cost"][0] == 0 and out["path"][0, 0] == 0      # r == t
    assert out["len"][2] == 0 and out["cost"][2] == -1
    assert out["cost"][6] == g[0, 3] <= 30 + int(pen[0, 1]) + int(pen[0, 2]) + int(pen[0, 3])
    # Lmax 8: the needed count, and both orders
    full = twin.paths(d2, pen, g, root, tg)
    short = twin.paths(d2, pen, g, root, tg, Lmax=8)
    assert short["status"][5] == Q_TRUNCATED and short["len"][5] == full["len"][5] > 8 and short["cost"][5] == full["cost"][5]
    back = twin.paths(d2, pen, g, root, tg, to_root=True)
    L = full["len"][5]
    np.testing.assert_array_equal(back["path"][5, :L], full["path"][5, :L][::-1])
    assert path_weighted_cost(full["path"][5, :L], pen) == full["cost"][5]
    # a blocked root: every cell INF, every read-out SC_Q_BAD_ENDPOINT
    g, st = twin.field(d2, pen, 2 * W + 2)
    assert st == Q_BAD_ENDPOINT and np.all(g == INF)
    assert np.all(twin.paths(d2, pen, g, 2 * W + 2, tg)["status"] == Q_BAD_ENDPOINT)
    g, st = twin.field(d2, pen, -1)
    assert st == Q_BAD_ENDPOINT and np.all(g == INF)
