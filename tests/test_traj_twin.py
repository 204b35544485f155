"""The NumPy twin of the timed-path conflicts (tests/traj_twin.py) on the hand cases with exact answers, and the counts that
keep the random fleet of the GPU tests from being vacuous.  No GPU."""
import numpy as np
import pytest

import traj_cases as tc
import traj_twin as tw

INF = np.inf


@pytest.mark.parametrize("dt_c", [0.25, 0.5, 1.0, 3.0])
def test_head_on(dt_c):
    o = tw.fleet(**tc.head_on(dt_c))
    assert o["first_t"].tolist() == [3.5, 3.5] and o["min_sep"].tolist() == [0.0, 0.0]
    assert o["first_with"].tolist() == [1, 0] and o["min_with"].tolist() == [1, 0] and o["n_conf"].tolist() == [1, 1]
    assert o["conflict"].tolist() == [[2], [1]]


def test_crossing_and_delays():
    o = tw.fleet(**tc.crossing(0.0))
    assert np.abs(o["first_t"] - (4.0 - np.sqrt(0.5))).max() <= 1e-12 and o["min_sep"].tolist() == [0.0, 0.0]
    o = tw.fleet(**tc.crossing(1.0))
    assert o["first_t"].tolist() == [4.0, 4.0] and np.abs(o["min_sep"] - np.sqrt(0.5)).max() <= 1e-12
    o = tw.fleet(**tc.crossing(2.0))
    assert o["first_t"].tolist() == [INF, INF] and np.abs(o["min_sep"] - np.sqrt(2.0)).max() <= 1e-12
    assert o["first_with"].tolist() == [-1, -1] and o["min_with"].tolist() == [1, 0] and o["n_conf"].tolist() == [0, 0]


def test_parked_and_vanishing():
    o = tw.fleet(**tc.parked(hold=True))
    assert o["first_t"].tolist() == [17.0, 17.0]
    o = tw.fleet(**tc.parked(hold=False))
    assert o["first_t"].tolist() == [INF, INF] and o["min_sep"].tolist() == [8.0, 8.0]


def test_same_group_is_never_compared():
    c = tc.head_on()
    c["group"] = np.array([4, 4], np.int32)
    o = tw.fleet(**c)
    assert o["first_t"].tolist() == [INF, INF] and o["min_sep"].tolist() == [INF, INF] and o["min_with"].tolist() == [-1, -1]
    assert not o["conflict"].any()
    c["group"] = np.array([-1, -1], np.int32)          # a negative group equals nobody
    assert tw.fleet(**c)["first_t"].tolist() == [3.5, 3.5]
    c["group"] = np.array([0, 1], np.int32)
    assert tw.fleet(**c)["first_t"].tolist() == [3.5, 3.5]


def test_skipped_and_bad_paths_are_invisible():
    """Four paths along the head-on line: 0 and 3 are the head-on pair, 1 is skipped, 2 has a NaN sample."""
    a, b = tc.line(0, 0, 8, 0), tc.line(8, 0, 0, 0)
    bad = (b[0], b[1].copy())
    bad[1][3, 1] = np.nan
    c = tc.pack([a, b, bad, b], 0.5, status=[0, 2, 0, 0])
    o = tw.fleet(**c)
    assert o["tstatus"].tolist() == [tw.TRAJ_OK, tw.TRAJ_SKIPPED, tw.TRAJ_BAD, tw.TRAJ_OK]
    assert o["first_t"].tolist() == [3.5, INF, INF, 3.5] and o["first_with"].tolist() == [3, -1, -1, 0]
    assert o["min_sep"].tolist() == [0.0, INF, INF, 0.0] and o["min_with"].tolist() == [3, -1, -1, 0]
    assert o["n_conf"].tolist() == [1, 0, 0, 1] and o["conflict"].ravel().tolist() == [8, 0, 0, 1]
    assert np.isnan(o["knots"][1:3]).all()
    for key, val in (("radius", -1.0), ("radius", np.nan), ("t0", np.inf)):
        c2 = tc.pack([a, b, b], 0.5, t0=[0.0, 0.0, 0.0])
        c2[key][1] = val
        o = tw.fleet(**c2)
        assert o["tstatus"].tolist() == [0, tw.TRAJ_BAD, 0] and o["first_with"].tolist() == [2, -1, 0], key
    c3 = tc.pack([a, b], 0.5)
    c3["time"][12] = c3["time"][11] - 0.25
    assert tw.fleet(**c3)["tstatus"].tolist() == [0, tw.TRAJ_BAD]


def test_one_sample_path_and_one_interval():
    a = tc.line(0, 0, 8, 0)
    dot = (np.array([2.0]), np.array([[4.0, 0.25]]))
    o = tw.fleet(**tc.pack([a, dot], 0.5))                 # stands at its point before and after (flags 3)
    assert o["first_t"].tolist() == [4.0 - np.sqrt(1.0 - 0.0625)] * 2 and o["min_sep"].tolist() == [0.25, 0.25]
    o = tw.fleet(**tc.pack([a, dot], 0.5, flags=[3, 0]))   # there at t = 2 only: never on both ends of an interval
    assert o["first_t"].tolist() == [INF, INF] and o["min_sep"].tolist() == [INF, INF]
    o = tw.fleet(**tc.pack([a, tc.line(8, 0, 0, 0)], 0.5, dt_c=8.0, K=1))
    assert o["first_t"].tolist() == [3.5, 3.5] and o["knots"].shape == (2, 2, 2)


def test_sep_cap_below_and_above():
    c = tc.crossing(2.0)                                   # true separation sqrt(2)
    c["sep_cap"] = 1.0
    o = tw.fleet(**c)
    assert o["min_sep"].tolist() == [INF, INF] and o["min_with"].tolist() == [-1, -1]
    c["sep_cap"] = 1.5
    o = tw.fleet(**c)
    assert np.abs(o["min_sep"] - np.sqrt(2.0)).max() <= 1e-12 and o["min_with"].tolist() == [1, 0]


def test_exact_tie_takes_the_smaller_index():
    o = tw.fleet(**tc.mirror_tie())
    assert o["first_t"][1] == o["first_t"][0] == o["first_t"][2] < INF
    assert o["first_with"].tolist() == [1, 0, 1] and o["min_with"].tolist() == [1, 0, 1]
    assert o["n_conf"].tolist() == [1, 2, 1] and o["conflict"].ravel().tolist() == [2, 5, 2]


def test_random_fleet_is_not_vacuous():
    st = {}
    c = tc.random_fleet()
    o = tw.fleet(**c, stats=st)
    assert st["conf_pairs"] >= 10 and st["clear_pairs"] >= 10, st
    assert st["root"] >= 1 and st["inside"] >= 1 and st["never"] >= 1, st
    assert (st["conf_pairs"], st["clear_pairs"], st["root"], st["inside"], st["never"]) == (140, 6582, 118, 1951, 1020)
    assert np.bincount(o["tstatus"]).tolist() == [123, 2, 5]
    P = tc.FLEET_P
    m = ((o["conflict"][:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(P, -1)[:, :P]
    assert np.array_equal(m, m.T) and not m.diagonal().any() and np.array_equal(m.sum(1), o["n_conf"])
    assert int(m.sum()) == 2 * st["conf_pairs"]
    capped = tw.fleet(**{**c, "sep_cap": 2.0})
    far = o["min_sep"] >= 2.0
    assert far.any() and (~far).any()
    assert np.isinf(capped["min_sep"][far]).all() and (capped["min_with"][far] == -1).all()
    assert np.array_equal(capped["min_sep"][~far], o["min_sep"][~far]) and np.array_equal(capped["first_t"], o["first_t"])
