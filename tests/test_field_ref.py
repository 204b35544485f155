"""The CPU twin of the cost fields (tests/cpp/field_ref.c): its g against scipy's Dijkstra, its read-out against the A*
oracle.  No GPU."""
import numpy as np
import pytest

from sea_current_amd import synth
from field_twin import INF, Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED, Twin, d2_of, field_scipy, serpentine, spiral


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return Twin(tmp_path_factory.mktemp("field_ref"))


def _maps(oracle):
    out = []
    for W, H, p, seed in ((96, 80, 0.20, 1), (64, 64, 0.05, 2), (1, 200, 0.1, 3), (200, 1, 0.1, 4), (37, 121, 0.3, 5)):
        out.append((f"salt{W}x{H}", oracle.edt(synth.salt_grid(W, H, p, seed=seed)), 0))
    out.append(("blocks_r2", oracle.edt(synth.block_grid(128, 96, 0.2, seed=7, smin=3, smax=16)), 4))
    out.append(("serpentine", d2_of(serpentine(64)), 0))
    out.append(("spiral", d2_of(spiral(65)), 0))
    return out


def _roots(d2, r2, k, seed):
    rng = np.random.default_rng(seed)
    T = np.flatnonzero(d2.ravel() >= max(r2, 1))
    return [int(x) for x in rng.choice(T, size=min(k, T.size), replace=False)]


def test_twin_field_equals_scipy(twin, oracle):
    for name, d2, r2 in _maps(oracle):
        for root in _roots(d2, r2, 3, 11):
            g, st = twin.field(d2, root, r2)
            assert st == Q_OK, name
            np.testing.assert_array_equal(g, field_scipy(d2, root, r2), err_msg=name)


def test_twin_paths_equal_astar_oracle(twin, oracle):
    for name, d2, r2 in _maps(oracle):
        H, W = d2.shape
        rng = np.random.default_rng(5)
        for root in _roots(d2, r2, 2, 13):
            g, _ = twin.field(d2, root, r2)
            tg = rng.integers(0, W * H, size=200).astype(np.int32)
            for Lmax in (4096, 8):
                ref = oracle.astar_batch(d2, np.full(tg.size, root, np.int32), tg, r2=r2, Lmax=Lmax)
                for to_root in (False, True):
                    out = twin.paths(d2, g, root, tg, r2=r2, Lmax=Lmax, to_root=to_root)
                    for k in ("status", "len", "cost"):
                        np.testing.assert_array_equal(out[k], ref[k], err_msg=f"{name} {k} Lmax={Lmax}")
                    for q in np.flatnonzero(ref["status"] == Q_OK):
                        p = ref["path"][q, :ref["len"][q]]
                        np.testing.assert_array_equal(out["path"][q, :ref["len"][q]], p[::-1] if to_root else p, err_msg=name)
                if Lmax == 8:
                    assert np.any(ref["status"] == Q_TRUNCATED), name


def test_twin_edge_cases(twin, oracle):
    occ = np.zeros((20, 30), np.uint8)
    occ[5:15, 10] = occ[5:15, 20] = 1
    occ[5, 10:21] = occ[14, 10:21] = 1          # an enclosed pocket (rows 6..13, columns 11..19)
    occ[2, 2] = 1
    d2 = d2_of(occ)
    H, W = d2.shape
    root = 0
    g, st = twin.field(d2, root)
    assert st == Q_OK and g[0, 0] == 0
    assert np.all(g[6:14, 11:20] == INF) and g[2, 2] == INF
    tg = np.array([0, 2 * W + 2, 9 * W + 15, -1, W * H, W * H - 1, 3], np.int32)
    out = twin.paths(d2, g, root, tg)
    np.testing.assert_array_equal(out["status"], [Q_OK, Q_BAD_ENDPOINT, Q_NO_PATH, Q_BAD_ENDPOINT, Q_BAD_ENDPOINT, Q_OK, Q_OK])
    assert out["len"][0] == 1 and out["cost"][0] == 0 and out["path"][0, 0] == 0      # r == t
    assert out["len"][2] == 0 and out["cost"][2] == -1
    ref = oracle.astar_batch(d2, np.zeros(tg.size, np.int32), tg)
    for k in ("status", "len", "cost"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    # a blocked root: every cell INF, every read-out SC_Q_BAD_ENDPOINT
    g, st = twin.field(d2, 2 * W + 2)
    assert st == Q_BAD_ENDPOINT and np.all(g == INF)
    assert np.all(twin.paths(d2, g, 2 * W + 2, tg)["status"] == Q_BAD_ENDPOINT)
    g, st = twin.field(d2, -1)
    assert st == Q_BAD_ENDPOINT and np.all(g == INF)


def test_twin_maze_lengths(twin, oracle):
    """The serpentine and the spiral force long detours: the read-out has to follow them cell by cell."""
    for occ, centre in ((serpentine(48), False), (spiral(49), True)):
        d2 = d2_of(occ)
        H, W = d2.shape
        T = np.flatnonzero(d2.ravel() >= 1)
        root = (H // 2) * W + W // 2 if centre else int(T[0])
        assert d2.flat[root] >= 1
        g, _ = twin.field(d2, root)
        tg = T[-50:].astype(np.int32)
        out = twin.paths(d2, g, root, tg)
        ref = oracle.astar_batch(d2, np.full(tg.size, root, np.int32), tg)
        np.testing.assert_array_equal(out["status"], ref["status"])
        np.testing.assert_array_equal(out["len"], ref["len"])
        assert out["len"].max() > 4 * max(W, H)
