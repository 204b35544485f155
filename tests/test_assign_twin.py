"""The NumPy twin of sc_assign_batch (tests/assign_twin.py) against an exhaustive search over all matchings, its certificate,
and the hand cases of the definition in include/sea_current_hip.h.  No GPU."""
import re

import numpy as np
import pytest

import assign_twin as tw
import sea_current_amd as sc

KINDS = ("tie", "small", "octile", "full")
FORBIDDEN = (0.0, 0.1, 0.5, 0.9, 1.0)


def test_the_header_states_the_procedure_the_twin_runs():
    src = " ".join(open(sc.HEADER_PATH).read().split())
    for quote in ("lowest j among equals", "most pairs", "smallest sum of costs", "SC_ASSIGN_BIG", "n (n + 1) / 2",
                  "u[r] + v[c] <= a[r][c]", "way[j] = j0"):
        assert quote in src, quote
    assert re.search(r"#define\s+SC_ASSIGN_MAX_DIM\s+1024\b", src) and tw.MAX_DIM == 1024
    assert re.search(r"#define\s+SC_ASSIGN_BIG\s+\(1ll << 42\)", src) and tw.BIG == 1 << 42
    assert tw.BIG > 1024 * 2**31 and 1024 * tw.BIG <= 2**52


@pytest.mark.parametrize("R", range(1, 7))
@pytest.mark.parametrize("C", range(1, 8))
def test_twin_is_optimal_on_every_small_shape(R, C):
    rng = np.random.default_rng(100 * R + C)
    for kind in KINDS:
        for fb in FORBIDDEN:
            cost = tw.random_cost(rng, R, C, kind, fb)
            out = tw.assign_one(cost)
            k, s = tw.brute_force(cost)
            assert (int(out["info"][0]), int(out["info"][1])) == (k, s), (kind, fb, cost.tolist())
            tw.certificate(cost, out)


def test_the_unique_optimum():
    out = tw.assign_one(np.array([[4, 1, 3], [2, 0, 5], [3, 2, 2]], np.int32))
    assert out["col_of"].tolist() == [1, 0, 2] and out["row_of"].tolist() == [1, 0, 2]
    assert out["info"][[0, 1, 3]].tolist() == [3, 5, tw.OK]


def test_forbidden_row_column_and_matrix():
    rng = np.random.default_rng(5)
    cost = tw.random_cost(rng, 5, 5, "small")
    row = cost.copy()
    row[2, :] = tw.INF
    out = tw.assign_one(row)
    assert out["col_of"][2] == -1 and out["info"][0] == 4 and (out["row_of"] == -1).sum() == 1
    tw.certificate(row, out)
    col = cost.copy()
    col[:, 3] = tw.INF
    out = tw.assign_one(col)
    assert out["row_of"][3] == -1 and out["info"][0] == 4 and (out["col_of"] == -1).sum() == 1
    tw.certificate(col, out)
    none = np.full((4, 6), tw.INF, np.int32)
    out = tw.assign_one(none)
    assert out["info"].tolist()[:2] == [0, 0] and (out["col_of"] == -1).all() and (out["row_of"] == -1).all()
    tw.certificate(none, out)


@pytest.mark.parametrize("kind", KINDS)
def test_more_rows_than_columns_is_the_transpose(kind):
    rng = np.random.default_rng(11)
    cost = tw.random_cost(rng, 9, 5, kind, 0.2)
    a, b = tw.assign_one(cost), tw.assign_one(np.ascontiguousarray(cost.T))
    assert np.array_equal(a["col_of"], b["row_of"]) and np.array_equal(a["row_of"], b["col_of"])
    assert np.array_equal(a["u"], b["v"]) and np.array_equal(a["v"], b["u"]) and np.array_equal(a["info"], b["info"])
    tw.certificate(cost, a)


def test_negative_entry_is_bad_and_alone():
    rng = np.random.default_rng(3)
    cost = tw.random_cost(rng, 3, 4, "small")[None].repeat(3, 0)
    cost[1, 2, 1] = -1
    out = tw.assign(cost)
    assert out["info"][:, 3].tolist() == [tw.OK, tw.BAD, tw.OK]
    assert (out["col_of"][1] == -1).all() and (out["row_of"][1] == -1).all() and not out["u"][1].any() and not out["v"][1].any()
    assert out["info"][1].tolist() == [0, 0, 0, tw.BAD]
    for k in out:
        assert np.array_equal(out[k][0], out[k][2])


def test_steps_stay_within_the_bound_and_ties_take_the_lowest_index():
    out = tw.assign_one(np.zeros((1, 5), np.int32))
    assert out["col_of"].tolist() == [0] and out["info"].tolist() == [1, 0, 1, tw.OK]
    out = tw.assign_one(np.array([[5, 3, 3], [3, 3, 9]], np.int32))               # line 0 takes post 1, not 2; line 1 post 0, not 1
    assert out["col_of"].tolist() == [1, 0] and out["info"].tolist() == [2, 6, 2, tw.OK]
    i, j = np.mgrid[0:40, 0:40]
    out = tw.assign_one((i * j).astype(np.int32))
    assert out["info"][2] == 40 * 41 // 2                                         # the bound is attained
    tw.certificate((i * j).astype(np.int32), out)


def test_field_cost_matrix_twin():
    g = np.arange(24, dtype=np.int32).reshape(2, 3, 4)
    g[1, 2, 3] = tw.INF
    cells = np.array([0, 11, -1, 12, 5], np.int32)
    m = tw.field_cost_matrix(g, cells)
    assert m.tolist() == [[0, 12], [11, tw.INF], [tw.INF, tw.INF], [tw.INF, tw.INF], [5, 17]]
    m = tw.field_cost_matrix(g, cells, np.array([7, tw.INF - 3], np.int64))
    assert m.tolist() == [[7, tw.INF - 1], [18, tw.INF], [tw.INF, tw.INF], [tw.INF, tw.INF], [12, tw.INF - 1]]
