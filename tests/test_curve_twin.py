"""The CPU twin of the curve check and repair (tests/curve_twin.py) on the legs the CPU oracle's from_path lays through
hand-made and random waypoints: the two 32 x 32 cases of DESIGN.md section 21 with their exact levels, minima and round
counts, the corridor that shrinking cannot fix, a leg that leaves the frame, the bits of level 0, a 64 times denser
sampling, and a random sweep.  No GPU."""
import numpy as np
import pytest

import curve_twin as tw

FRAME = (0.0, 0.0, 1.0, 1.0)
CASE_A = [(4, 4), (16, 6), (18, 21), (28, 21)]
CASE_B = [(10, 12), (10, 21), (15, 21), (15, 12)]


def wall_map():
    occ = np.zeros((32, 32), np.uint8)
    occ[8:20, 12:14] = 1
    occ[22:24, 0:20] = 1
    return occ


def centres(cells):
    return (np.array(cells, np.float32) + np.float32(0.5)).astype(np.float32)


@pytest.fixture(scope="module")
def world(oracle):
    d2 = tw.edt(wall_map())
    assert np.array_equal(d2, oracle.edt(wall_map()))
    legs = {k: oracle.bezier_from_path(centres(v)) for k, v in (("a", CASE_A), ("b", CASE_B))}
    return d2, legs


SO3 = np.array([0, 3], np.int32)


@pytest.mark.parametrize("case,lvl0,levels,mins,rounds", [("a", [13, 0, 0], [0, 1, 2, 2], [9, 1, 1], 2),
                                                          ("b", [1, 0, 1], [0, 2, 2, 0], [1, 1, 1], 2)])
def test_wall_cases_resolve_as_recorded(world, case, lvl0, levels, mins, rounds):
    d2, legs = world
    chk = tw.clearance(legs[case], SO3, d2, FRAME, 1)
    assert list(chk["leg_min"]) == lvl0
    assert chk["hit_legs"][0] == sum(v < 1 for v in lvl0) and chk["hit_leg"][0] == 1 and 0.0 < chk["hit_t"][0] < 1.0
    o = tw.clear(legs[case], SO3, d2, FRAME, 1, 6)
    assert list(o["level"]) == levels and list(o["leg_min"]) == mins and o["rounds"][0] == rounds and o["status"][0] == tw.OK
    # the repaired curve passes the check, its ends and the legs at level 0 keep their bits
    again = tw.clearance(o["ctrl"], SO3, d2, FRAME, 1)
    assert again["hit_legs"][0] == 0 and again["hit_leg"][0] == -1 and again["hit_t"][0] == -1.0 and list(again["leg_min"]) == mins
    assert o["ctrl"][:, [0, 3]].tobytes() == legs[case][:, [0, 3]].tobytes()
    if case == "a":
        assert o["ctrl"][0, 1].tobytes() == legs[case][0, 1].tobytes() and o["ctrl"][0, 2].tobytes() != legs[case][0, 2].tobytes()


@pytest.mark.parametrize("case", ["a", "b"])
def test_corridor_cannot_be_fixed_by_shrinking(world, case):
    """Row 21 is a corridor of d2 = 1: with r2_clear = 4 the straight legs are not clear either."""
    d2, legs = world
    for max_level in (1, 6, 30):
        o = tw.clear(legs[case], SO3, d2, FRAME, 4, max_level)
        assert o["status"][0] == tw.COLLIDES and o["level"].max() == max_level and (o["leg_min"] < 4).any()
        assert o["rounds"][0] <= max_level * 4


def test_leaving_the_frame_hits(world):
    d2, _ = world
    free = np.full((32, 32), tw.INT_MAX, np.int32)
    c = np.array([[[30.5, 5.5], [31.5, 5.5], [32.5, 5.5], [33.5, 5.5]]], np.float32)
    chk = tw.clearance(c, np.array([0, 1], np.int32), free, FRAME, 0)
    assert chk["leg_min"][0] == 0 and chk["hit_leg"][0] == 0 and chk["hit_t"][0] == np.float32(0.5)   # x = 32 at t = 1/2
    inside = np.array([[[3.5, 5.5], [5.5, 9.5], [8.5, 9.5], [10.5, 5.5]]], np.float32)
    chk = tw.clearance(inside, np.array([0, 1], np.int32), free, FRAME, 0)
    assert chk["leg_min"][0] == tw.INT_MAX and chk["hit_legs"][0] == 0
    nan = inside.copy()
    nan[0, 1, 0] = np.nan
    chk = tw.clearance(nan, np.array([0, 1], np.int32), free, FRAME, 0)
    assert chk["leg_min"][0] == 0 and chk["hit_t"][0] == 0.0
    o = tw.clear(c, np.array([0, 1], np.int32), free, FRAME, 0, 3)   # its end point lies outside: unresolved
    assert o["status"][0] == tw.COLLIDES and list(o["level"]) == [3, 3] and o["rounds"][0] == 3


def test_level_zero_returns_the_input_bits(world):
    d2, legs = world
    free = np.full((32, 32), tw.INT_MAX, np.int32)
    for case in ("a", "b"):
        o = tw.clear(legs[case], SO3, free, FRAME, 1, 6)
        assert o["ctrl"].tobytes() == legs[case].tobytes() and not o["level"].any() and o["rounds"][0] == 0 and o["status"][0] == tw.OK
        for i in range(3):
            assert tw.leg_ctrl(legs[case][i], 0, 0).tobytes() == legs[case][i].tobytes()
    # a skipped path in the middle keeps everything
    two = np.concatenate([legs["a"], legs["b"]])
    o = tw.clear(two, np.array([0, 3, 6], np.int32), d2, FRAME, 1, 6, status=np.array([0, 2], np.int32))
    assert list(o["status"]) == [0, 2] and o["ctrl"][3:].tobytes() == legs["b"].tobytes() and list(o["leg_min"][3:]) == [-1] * 3


def test_denser_sampling_can_only_be_lower(world):
    d2, legs = world
    lower = 0
    for case in ("a", "b"):
        for lv in (0, 1, 3):
            for i in range(3):
                c = tw.leg_ctrl(legs[case][i], lv, lv)
                mn, _, _, n = tw.leg_eval(c, d2, FRAME, 1)
                dn, _, _, _ = tw.leg_eval(c, d2, FRAME, 1, dense=64)
                assert dn <= mn and 6 <= n
                lower += dn < mn
                # samples at most half a cell apart: the bound the guarantee rests on
                pts = tw.leg_samples(c, n)
                assert np.sqrt((np.diff(pts, axis=0) ** 2).sum(1)).max() <= 0.5
    assert lower <= 6


def test_random_sweep():
    """240 paths of three to six waypoints whose straight legs are clear, on a 32 x 32 and a 48 x 48 block map.  The twin
    gives: 32 x 32 (seed 5) 71 of 120 paths hit at level 0 (59 %) and 68 of those resolve (96 %); 48 x 48 (seed 6) 81 of 120
    (68 %) and 77 (95 %).  The shares asserted below only keep the sweep from being vacuous."""
    from oracle import oracle
    total = hit0 = resolved = 0
    for W, seed in ((32, 5), (48, 6)):
        occ, d2, wp, npts = tw.sweep_paths(W, W, seed, 120)
        assert np.array_equal(d2, oracle.edt(occ))
        for p in range(len(npts)):
            c = oracle.bezier_from_path(wp[p, :npts[p]])
            so = np.array([0, npts[p] - 1], np.int32)
            chk = tw.clearance(c, so, d2, (0.0, 0.0, 1.0, 1.0), 1)
            o = tw.clear(c, so, d2, (0.0, 0.0, 1.0, 1.0), 1, 6)
            total += 1
            if chk["hit_legs"][0]:
                hit0 += 1
                resolved += o["status"][0] == tw.OK
                assert o["rounds"][0] >= 1 and o["level"].any()
            else:
                assert o["status"][0] == tw.OK and o["rounds"][0] == 0 and not o["level"].any() and o["ctrl"].tobytes() == c.tobytes()
            if o["status"][0] == tw.OK:
                assert tw.clearance(o["ctrl"], so, d2, (0.0, 0.0, 1.0, 1.0), 1)["hit_legs"][0] == 0
    assert total >= 200 and hit0 > total / 4 and resolved > hit0 / 2, (total, hit0, resolved)
