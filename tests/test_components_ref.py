"""The CPU twin of the component labelling (tests/cpp/components_ref.c) against scipy.ndimage.label relabelled to each
component's minimum, and its reachability statuses against the A* oracle.  No GPU."""
import numpy as np
import pytest

from components_twin import Q_OK, Q_TRUNCATED, Twin, comb, components_scipy, d2_of, serpentine, spiral


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return Twin(tmp_path_factory.mktemp("components_ref"))


def _line(n, p, seed):
    return (np.random.default_rng(seed).random(n) < p).astype(np.uint8)


def _maps(oracle):
    from sea_current_amd import synth
    return {
        "salt97x61": (oracle.edt(synth.salt_grid(97, 61, 0.41, seed=5)), 0),
        "salt64": (oracle.edt(synth.salt_grid(64, 64, 0.2, seed=6)), 0),
        "row200": (d2_of(_line(200, 0.1, 7).reshape(1, 200)), 0),     # salt_grid frees the border, which is all of a line
        "col200": (d2_of(_line(200, 0.1, 8).reshape(200, 1)), 0),
        "salt37x121": (oracle.edt(synth.salt_grid(37, 121, 0.5, seed=9)), 0),
        "blocks128x96": (oracle.edt(synth.block_grid(128, 96, 0.35, seed=10, smin=3, smax=24)), 4),
        "serpentine64": (d2_of(serpentine(64)), 0),
        "spiral65": (d2_of(spiral(65)), 0),
        "free": (np.full((40, 70), 9, np.int32), 0),
        "blocked": (np.zeros((40, 70), np.int32), 0),
        "comb": (d2_of(comb(41)), 0),
    }


NAMES = ["salt97x61", "salt64", "row200", "col200", "salt37x121", "blocks128x96", "serpentine64", "spiral65", "free", "blocked", "comb"]


@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_scipy(twin, oracle, name):
    d2, r2 = _maps(oracle)[name]
    got, ref = twin.components(d2, r2), components_scipy(d2, r2)
    assert np.array_equal(got["label"], ref["label"])
    assert np.array_equal(got["size"], ref["size"])
    assert int(got["ncomp"][0]) == ref["ncomp"] and int(got["largest"][0]) == ref["largest"]
    T = d2 >= max(r2, 1)
    assert ((got["label"] >= 0) == T).all()
    assert int(got["size"].sum()) == int(T.sum())
    if name == "blocked":
        assert ref["ncomp"] == 0 and ref["largest"] == -1
    if name in ("free", "serpentine64", "spiral65", "comb"):
        assert ref["ncomp"] == 1 and ref["largest"] == int(np.flatnonzero(T.ravel())[0])
    if name in ("row200", "col200"):
        assert ref["ncomp"] >= 3


def test_largest_tie_goes_to_the_smaller_index(twin):
    """Two components of 12 cells and one of 5: the first of the equal ones wins, wherever it lies."""
    d2 = np.zeros((9, 20), np.int32)
    d2[1:4, 12:16] = 1       # 12 cells, representative 1 * 20 + 12
    d2[5:8, 2:6] = 1         # 12 cells, representative 5 * 20 + 2
    d2[8, 10:15] = 1         # 5 cells
    got = twin.components(d2)
    assert int(got["ncomp"][0]) == 3 and int(got["largest"][0]) == 32
    assert got["size"].ravel()[[32, 102, 170]].tolist() == [12, 12, 5]
    assert components_scipy(d2)["largest"] == 32
    got = twin.components(d2[::-1].copy())
    assert int(got["largest"][0]) == 1 * 20 + 2


def test_reachability_is_the_status_of_astar(twin, oracle):
    d2, _ = _maps(oracle)["salt97x61"]
    free = np.flatnonzero(d2.ravel() >= 1)
    rng = np.random.default_rng(11)
    s = rng.choice(free, 300).astype(np.int32)
    g = rng.choice(free, 300).astype(np.int32)
    st = twin.reachable(twin.components(d2)["label"], s, g)
    ref = oracle.astar_batch(d2, s, g, Lmax=64)["status"].copy()
    assert (ref == Q_TRUNCATED).any()
    ref[ref == Q_TRUNCATED] = Q_OK
    assert np.array_equal(st, ref)
    assert 30 < int((st != Q_OK).sum()) < 300
