"""The CPU twin of the multi-source cost fields (tests/cpp/field_multi_ref.c): its g against scipy (one Dijkstra per seed
plus the seed cost, then the minimum), against the single-root twins for one seed, its read-out against the A* oracle
from the owning seed, and the cases the definition singles out.  No GPU."""
import numpy as np
import pytest

from sea_current_amd import synth
from field_twin import INF, Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED, Twin, d2_of, serpentine
from field_w_twin import TwinW
from field_multi_twin import SEED_COST_MAX, TwinM, field_multi_scipy, mirror_map, plug_map


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return TwinM(tmp_path_factory.mktemp("field_multi_ref"))


@pytest.fixture(scope="module")
def twin1(tmp_path_factory):
    return Twin(tmp_path_factory.mktemp("field_multi_ref_1"))


@pytest.fixture(scope="module")
def twinw(tmp_path_factory):
    return TwinW(tmp_path_factory.mktemp("field_multi_ref_w"))


def _maps(oracle):
    out = []
    for W, H, p, seed in ((96, 80, 0.20, 1), (1, 200, 0.1, 3), (200, 1, 0.1, 4)):
        out.append((f"salt{W}x{H}", oracle.edt(synth.salt_grid(W, H, p, seed=seed)), 0))
    out.append(("blocks_r2", oracle.edt(synth.block_grid(128, 96, 0.2, seed=7, smin=3, smax=16)), 4))
    out.append(("serpentine", d2_of(serpentine(64)), 0))
    return out


def _seeds(d2, r2, k, seed):
    rng = np.random.default_rng(seed)
    T = np.flatnonzero(d2.ravel() >= max(r2, 1))
    s = np.array(rng.choice(T, size=min(k, T.size), replace=False), np.int32)
    return s, rng.integers(0, 400, size=s.size).astype(np.int32)


def _check_owner_by_walk(d2, g, owner, seeds, cost, r2=0):
    """owner at a seed that holds its own cost is the smallest such seed; elsewhere it is finite exactly where g is."""
    assert np.array_equal(owner >= 0, g < INF)
    c = np.zeros(len(seeds), np.int32) if cost is None else cost
    for s in range(len(seeds)):
        if 0 <= seeds[s] < g.size and g.flat[seeds[s]] == c[s] and d2.flat[seeds[s]] >= max(r2, 1) and 0 <= c[s] <= SEED_COST_MAX:
            same = [k for k in range(len(seeds)) if seeds[k] == seeds[s] and c[k] == c[s]]
            assert owner.flat[seeds[s]] == min(same)


def test_twin_g_equals_scipy_minimum(twin, oracle):
    for name, d2, r2 in _maps(oracle):
        seeds, cost = _seeds(d2, r2, 5, 11)
        for sc in (None, cost):
            g, owner, st = twin.field(d2, seeds, sc, r2)
            assert st == Q_OK, name
            np.testing.assert_array_equal(g, field_multi_scipy(d2, seeds, sc, r2), err_msg=name)
            _check_owner_by_walk(d2, g, owner, seeds, sc, r2)


def test_twin_weighted_g_equals_scipy_minimum(twin, oracle):
    d2 = oracle.edt(synth.salt_grid(64, 48, 0.15, seed=5))
    pen = np.random.default_rng(2).integers(0, 256, size=d2.shape).astype(np.uint8)
    seeds, cost = _seeds(d2, 0, 4, 3)
    for cap in (255, 40):
        g, owner, st = twin.field(d2, seeds, cost, pen=pen, cap=cap)
        np.testing.assert_array_equal(g, field_multi_scipy(d2, seeds, cost, pen=pen, cap=cap))
        _check_owner_by_walk(d2, g, owner, seeds, cost)


def test_one_seed_equals_the_single_root_twins(twin, twin1, twinw, oracle):
    for name, d2, r2 in _maps(oracle):
        seeds, _ = _seeds(d2, r2, 1, 13)
        g, owner, st = twin.field(d2, seeds, None, r2)
        ref, rs = twin1.field(d2, int(seeds[0]), r2)
        assert st == rs == Q_OK
        np.testing.assert_array_equal(g, ref, err_msg=name)
        assert np.array_equal(owner, np.where(ref < INF, 0, -1)), name
        H, W = d2.shape
        tg = np.random.default_rng(1).integers(0, W * H, size=100).astype(np.int32)
        for to in (False, True):
            a = twin.paths(d2, g, seeds, tg, r2=r2, Lmax=64, to_seed=to)
            b = twin1.paths(d2, ref, int(seeds[0]), tg, r2=r2, Lmax=64, to_root=to)
            for k in ("status", "len", "cost"):
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
            for q in np.flatnonzero(b["status"] == Q_OK):
                np.testing.assert_array_equal(a["path"][q, :b["len"][q]], b["path"][q, :b["len"][q]])
    d2 = oracle.edt(synth.salt_grid(64, 48, 0.15, seed=5))
    pen = np.random.default_rng(2).integers(0, 256, size=d2.shape).astype(np.uint8)
    seeds, _ = _seeds(d2, 0, 1, 3)
    g, _, _ = twin.field(d2, seeds, pen=pen, cap=90)
    ref, _ = twinw.field(d2, pen, int(seeds[0]), cap=90)
    np.testing.assert_array_equal(g, ref)


def test_twin_paths_equal_astar_oracle_from_the_owner(twin, oracle):
    for name, d2, r2 in _maps(oracle):
        H, W = d2.shape
        seeds, cost = _seeds(d2, r2, 5, 17)
        for sc in (None, cost):
            c = np.zeros(seeds.size, np.int32) if sc is None else sc
            g, owner, _ = twin.field(d2, seeds, sc, r2)
            tg = np.random.default_rng(5).integers(0, W * H, size=200).astype(np.int32)
            for Lmax in (4096, 8):
                for to in (False, True):
                    out = twin.paths(d2, g, seeds, tg, sc, r2=r2, Lmax=Lmax, to_seed=to)
                    has = np.isin(out["status"], (Q_OK, Q_TRUNCATED))
                    assert np.array_equal(out["which"] >= 0, has) and (out["which"][~has] == -1).all()
                    np.testing.assert_array_equal(out["which"][has], owner.ravel()[tg[has]], err_msg=name)
                    w = np.where(has, out["which"], 0)
                    ref = oracle.astar_batch(d2, seeds[w], tg, r2=r2, Lmax=Lmax)
                    for q in range(tg.size):
                        if not has[q]:
                            t = tg[q]
                            bad = d2.flat[t] < max(r2, 1)
                            assert out["status"][q] == (Q_BAD_ENDPOINT if bad else Q_NO_PATH) and out["len"][q] == 0 and out["cost"][q] == -1
                            continue
                        assert out["status"][q] == ref["status"][q] and out["len"][q] == ref["len"][q], (name, q)
                        assert out["cost"][q] - c[w[q]] == ref["cost"][q], (name, q)
                        if out["status"][q] == Q_OK:
                            p = ref["path"][q, :ref["len"][q]]
                            np.testing.assert_array_equal(out["path"][q, :ref["len"][q]], p[::-1] if to else p, err_msg=f"{name} {q}")


def test_plug_map(twin, twin1):
    d2, seed = plug_map()
    g, owner, st = twin.field(d2, [seed])
    assert st == Q_OK and (g < INF).sum() == 199 and g[1, 63] == 0 and g[1, 64] == 10
    np.testing.assert_array_equal(g, twin1.field(d2, seed)[0])
    np.testing.assert_array_equal(g, field_multi_scipy(d2, [seed]))
    gt, _, _ = twin.field(d2.T.copy(), [63 * 3 + 1])
    np.testing.assert_array_equal(gt, g.T)


def test_duplicates_dominated_and_exact_tie(twin):
    d2 = np.ones((9, 40), np.int32)
    a, b = 4 * 40 + 5, 4 * 40 + 25                       # 20 cells apart on one row: dist 200
    # duplicates: the smaller index owns
    g, owner, _ = twin.field(d2, [a, b, a], [7, 0, 7])
    assert g.flat[a] == 7 and owner.flat[a] == 0
    # a dominated seed: b costs 300 itself but is reached from a at 0 + 200; it is not terminal
    g, owner, _ = twin.field(d2, [a, b], [0, 300])
    assert g.flat[b] == 200 and (owner == 0).all()
    out = twin.paths(d2, g, [a, b], [b], [0, 300])
    assert out["which"][0] == 0 and out["len"][0] == 21 and out["cost"][0] == 200
    # a seed whose cost equals the cost from the other seed stays terminal although a parent satisfies the equality
    g, owner, _ = twin.field(d2, [a, b], [0, 200])
    assert g.flat[b] == 200 and owner.flat[b] == 1 and owner.flat[b - 1] == 0
    out = twin.paths(d2, g, [a, b], [b, b + 1], [0, 200])
    assert list(out["which"]) == [1, 1] and list(out["len"]) == [1, 2] and list(out["cost"]) == [200, 210]


def test_mirror_map(twin, oracle):
    d2, seeds = mirror_map()
    g, owner, _ = twin.field(d2, seeds)
    col = np.arange(17) * 33 + 16
    one = [field_multi_scipy(d2, seeds[k:k + 1]) for k in (0, 1)]
    assert np.array_equal(one[0].ravel()[col], one[1].ravel()[col])              # 17 exact ties
    out = twin.paths(d2, g, seeds, col, Lmax=64)
    np.testing.assert_array_equal(out["which"], owner.ravel()[col])
    ref = oracle.astar_batch(d2, seeds[out["which"]], col.astype(np.int32), Lmax=64)
    for q in range(17):
        assert out["len"][q] == ref["len"][q] and out["cost"][q] == ref["cost"][q]
        np.testing.assert_array_equal(out["path"][q, :ref["len"][q]], ref["path"][q, :ref["len"][q]])


def test_invalid_and_empty_seed_lists(twin):
    d2 = np.ones((8, 12), np.int32)
    d2[3, 3] = 0
    tg = np.array([0, 3 * 12 + 3, -1, 96, 50], np.int32)
    for seeds, cost in (([], None), ([-1, 96, 3 * 12 + 3], None), ([5, 6], [-1, SEED_COST_MAX + 1])):
        g, owner, st = twin.field(d2, np.array(seeds, np.int32), cost)
        assert st == Q_BAD_ENDPOINT and (g == INF).all() and (owner == -1).all()
        out = twin.paths(d2, g, np.array(seeds, np.int32), tg, cost)
        assert list(out["status"]) == [Q_NO_PATH, Q_BAD_ENDPOINT, Q_BAD_ENDPOINT, Q_BAD_ENDPOINT, Q_NO_PATH]
        assert (out["which"] == -1).all() and (out["len"] == 0).all() and (out["cost"] == -1).all()
    # invalid seeds are skipped, indices keep counting them; the largest allowed cost is valid
    g, owner, st = twin.field(d2, [-5, 3 * 12 + 3, 7, 1000], [0, 0, SEED_COST_MAX, 0], s0=10)
    assert st == Q_OK and g.flat[7] == SEED_COST_MAX and set(np.unique(owner)) == {-1, 12} and owner[3, 3] == -1
