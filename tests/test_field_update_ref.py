"""The repair of a cost field after a map change on the CPU: the definition in NumPy (field_update_twin.update_twin) ==
the C statement (tests/cpp/field_update_ref.c) == a fresh field of the new map from the field twins, in g, status and both
stats.  The cases are those the GPU test runs (field_update_twin.cases).  No GPU."""
import numpy as np
import pytest

from sea_current_amd import synth
from field_twin import INF, Q_BAD_ENDPOINT, Q_OK, Twin, d2_of
from field_w_twin import TwinW
from field_update_twin import TwinU, cases, hand_case, update_twin


@pytest.fixture(scope="module")
def twin0(tmp_path_factory):
    return Twin(tmp_path_factory.mktemp("field_ref_for_update"))


@pytest.fixture(scope="module")
def twinw(tmp_path_factory):
    return TwinW(tmp_path_factory.mktemp("field_w_ref_for_update"))


@pytest.fixture(scope="module")
def twinu(tmp_path_factory):
    return TwinU(tmp_path_factory.mktemp("field_update_ref"))


def fresh(twin0, twinw, d2, pen, cap, r2, root):
    """(g, status) of a fresh build on the CPU."""
    H, W = d2.shape
    if not 0 <= root < W * H:
        return np.full((H, W), INF, np.int32), Q_BAD_ENDPOINT
    return twin0.field(d2, root, r2) if pen is None else twinw.field(d2, pen, root, r2, cap)


def test_every_case_three_ways(twin0, twinw, twinu, oracle):
    all_cases = cases(oracle)
    assert len(all_cases) >= 50
    for name, d0, d1, p0, p1, cap, r2, root in all_cases:
        g0, _ = fresh(twin0, twinw, d0, p0, cap, r2, root)
        want, wst = fresh(twin0, twinw, d1, p1, cap, r2, root)
        a, ast, astats = update_twin(d0, d1, g0, root, r2, p0, p1, cap)
        b, bst, bstats = twinu.update(d0, d1, g0, root, r2, p0, p1, cap)
        np.testing.assert_array_equal(a, want, err_msg=name)
        np.testing.assert_array_equal(b, want, err_msg=name)
        assert ast == bst == wst, name
        assert astats == bstats, name
        thr = max(r2, 1)
        T0, T1 = d0 >= thr, d1 >= thr
        changed = T0 != T1
        if p1 is not None:
            changed |= T0 & T1 & (np.minimum(p0, cap) != np.minimum(p1, cap))
        assert astats[0] == int(changed.sum()), name
        # U holds at least every cell that turned INF or rose, at most every finite cell
        assert int(((g0 < INF) & (want > g0)).sum()) <= astats[1] <= int((g0 < INF).sum()), name


def test_named_cases_say_what_they_claim(twin0, twinw, twinu, oracle):
    by_name = {c[0]: c for c in cases(oracle)}
    def run(name):
        _, d0, d1, p0, p1, cap, r2, root = by_name[name]
        g0, _ = fresh(twin0, twinw, d0, p0, cap, r2, root)
        g, st, stats = twinu.update(d0, d1, g0, root, r2, p0, p1, cap)
        return g0, g, st, stats
    g0, g, st, stats = run("no_change")
    assert stats == [0, 0] and st == Q_OK
    np.testing.assert_array_equal(g, g0)
    g0, g, st, stats = run("weighted/same")
    assert stats == [0, 0]
    np.testing.assert_array_equal(g, g0)
    g0, g, st, stats = run("root_blocked")
    assert st == Q_BAD_ENDPOINT and np.all(g == INF) and stats == [1, int((g0 < INF).sum())]
    g0, g, st, stats = run("root_freed")
    assert st == Q_OK and np.all(g0 == INF) and stats == [1, 0] and (g < INF).sum() > 1000
    g0, g, st, stats = run("every_cell_changed")
    assert stats[0] == 64 * 64 and stats[1] == int((g0 < INF).sum()) and st == Q_BAD_ENDPOINT
    # the corridor closed two rows below the root's: everything beyond it is in U; the wall opened: U is empty
    g0, g, st, stats = run("serpentine/closed")
    assert stats[0] == 4 and stats[1] == int((g0 < INF).sum()) - int((g < INF).sum()) > 1500
    g0, g, st, stats = run("serpentine/wall_opened")
    assert stats[1] == 0 and (g < g0).sum() > 1000
    g0, g, st, stats = run("weighted/lowered")
    assert stats[0] > 0 and not (g > g0).any()
    g0, g, st, stats = run("weighted/raised")
    assert stats[1] > 0 and not (g < g0).any()


def test_hand_computed_U(twin0, twinu):
    d0, d1, root, want_stats = hand_case()
    g0, _ = twin0.field(d0, root)
    assert g0[4, 0] == 14 + 30 + 10 + 10 + 14 + 30               # to (4, 1), through the door (4, 2) to (4, 3), back to (0, 4)
    for g, st, stats in (update_twin(d0, d1, g0, root), twinu.update(d0, d1, g0, root)):
        assert st == Q_OK and stats == want_stats
        assert np.all(g[2:] == INF)
        np.testing.assert_array_equal(g[:2], g0[:2])


def test_chained_frames(twin0, twinu):
    """8 frames of the dynamic-obstacle stream, each fed the previous repair."""
    W, H, K = 130, 100, 6
    rects = synth.block_rects(W, H, 0.15, seed=21, smin=3, smax=14)
    d_prev = d2_of(synth.raster_rects(rects, W, H))
    root = int(np.flatnonzero(d_prev.ravel() >= 1)[0])
    g, _ = twin0.field(d_prev, root)
    raised = 0
    for frame in range(8):
        rects = synth.move_rects(rects, frame, W, H, K=K, step=2, seed=21)
        d_new = d2_of(synth.raster_rects(rects, W, H))
        d_new[root // W, root % W] = 1
        g2, st, stats = twinu.update(d_prev, d_new, g, root)
        want, wst = twin0.field(d_new, root)
        assert st == wst == Q_OK
        np.testing.assert_array_equal(g2, want, err_msg=f"frame {frame}")
        a, ast, astats = update_twin(d_prev, d_new, g, root)
        np.testing.assert_array_equal(a, want, err_msg=f"frame {frame}")
        assert ast == st and astats == stats
        raised += stats[1]
        g, d_prev = g2, d_new
    assert raised > 0


def test_argument_errors(twinu):
    d = np.ones((4, 4), np.int32)
    g = np.full((4, 4), INF, np.int32)
    pen = np.zeros((4, 4), np.uint8)
    neg = g.copy()
    neg[1, 1] = -5
    assert twinu.update(d, d, neg, 0)[1] == -1
    assert twinu.update(d, d, g, 0, pen_old=pen, pen_new=pen, cap=256)[1] == -1
    assert twinu.lib.fu_update(d.ctypes.data, pen.ctypes.data, d.ctypes.data, None, 255, 4, 4, 0, 0, g.ctypes.data, None) == -1
    assert twinu.lib.fu_update(d.ctypes.data, None, d.ctypes.data, None, 0, 0, 4, 0, 0, g.ctypes.data, None) == -1
    assert twinu.lib.fu_update(None, None, d.ctypes.data, None, 0, 4, 4, 0, 0, g.ctypes.data, None) == -1
    assert twinu.update(d, d, g, 0)[1] == Q_OK
