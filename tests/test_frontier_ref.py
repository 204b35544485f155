"""The two CPU statements of the exploration frontiers against each other and against scipy: the NumPy twin
(tests/frontier_twin.py) == the C reference (tests/cpp/frontier_ref.c) in every output; labels == scipy.ndimage.label with the
3 x 3 structure relabelled to each cluster's minimum; the two-disc ring is one cluster where a 4-connected labelling gives 112;
the rank order, the Cmax cut and min_size; the matrix against a brute-force loop; the exploration loop's invariant on the twin
alone; the C reference under AddressSanitizer and UBSan as a program of its own.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import frontier_twin as ft
from field_twin import Twin as FieldTwin, d2_of

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = os.path.join(HERE, "cpp", "frontier_ref_check.c")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ft.Ref(tmp_path_factory.mktemp("frontier_ref"))


@pytest.fixture(scope="module")
def fields(tmp_path_factory):
    return FieldTwin(tmp_path_factory.mktemp("field_ref"))


def _salt(W=130, H=70, p=0.2, seed=2):
    from sea_current_amd import synth
    return d2_of(synth.salt_grid(W, H, p, seed=seed)), ft.known_from_discs(None, ft.three_discs(W, H), W, H)


def _cases(oracle):
    from sea_current_amd import synth
    free = lambda k: np.full(k.shape, 9, np.int32)
    blocks = synth.block_grid(128, 96, 0.3, seed=10, smin=3, smax=24)
    return {
        "salt130x70": _salt() + (0,),
        "two_discs": (free(ft.two_discs()), ft.two_discs(), 0),
        "ring": (free(ft.ring(200, 150, 100, 75, 60, 30)), ft.ring(200, 150, 100, 75, 60, 30), 0),
        "staircase": (free(ft.staircase(130, 70)), ft.staircase(130, 70), 0),
        "corner": (free(ft.corner_diagonal(130, 130)), ft.corner_diagonal(130, 130), 0),
        "anticorner": (free(ft.corner_antidiagonal(130, 130)), ft.corner_antidiagonal(130, 130), 0),
        "band": (free(ft.band(200, 200)), ft.band(200, 200), 0),
        "blocks_r2_4": (oracle.edt(blocks), ft.known_from_discs(None, ft.three_discs(128, 96), 128, 96), 4),
        "row": (np.ones((1, 200), np.int32), ft.known_from_discs(None, [(50, 0, 100), (120, 0, 25)], 200, 1), 0),
        "column": (np.ones((200, 1), np.int32), ft.known_from_discs(None, [(0, 50, 100), (0, 120, 25)], 1, 200), 0),
    }


NAMES = ["salt130x70", "two_discs", "ring", "staircase", "corner", "anticorner", "band", "blocks_r2_4", "row", "column"]


@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_c_reference_and_scipy(ref, oracle, name):
    d2, known, r2 = _cases(oracle)[name]
    got, want = ft.frontiers(d2, known, r2), ref.frontiers(d2, known, r2)
    for k in ft.KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    fr = ft.frontier_mask(d2, known, r2)
    label, n = ft.labels_scipy(fr)
    assert np.array_equal(got["label"], label) and int(got["ncl"][0, 1]) == n
    assert ((got["label"] >= 0) == fr).all() and fr.any()
    # the listed rows against the labels
    L = min(int(got["ncl"][0, 0]), 128)
    for k in range(L):
        cells = np.flatnonzero(got["label"].ravel() == got["rep"][0, k])
        x, y = cells % d2.shape[1], cells // d2.shape[1]
        assert got["csize"][0, k] == len(cells) and cells[0] == got["rep"][0, k]
        assert got["cbox"][0, k].tolist() == [x.min(), y.min(), x.max(), y.max()] and got["csum"][0, k].tolist() == [x.sum(), y.sum()]
        assert (got["slot"].ravel()[cells] == k).all()
    assert (np.diff(got["rep"][0, :L]) > 0).all() and (got["rep"][0, L:] == -1).all() and not got["cbox"][0, L:].any()


def test_known_and_d2_known(ref):
    rng = np.random.default_rng(1)
    base = (rng.random((70, 130)) < 0.1).astype(np.uint8) * 7
    discs = np.array([(10, 10, 30), (64, 35, 0), (129, 69, 100), (-5, 20, 64), (40, 40, -1), (300, 300, 2**31 - 1)], np.int32)
    for b in (None, base):
        k = ft.known_from_discs(b, discs, 130, 70)
        assert np.array_equal(k, ref.known_from_discs(b, discs, 130, 70)) and set(np.unique(k)) <= {0, 1}
    assert k.all()                                                                # the last disc covers everything
    k = ft.known_from_discs(base, discs[:5], 130, 70)
    assert k[35, 64] == 1 and k[35, 65] == base[35, 65] // 7 and k[40, 40] == base[40, 40] // 7 and not k.all()
    assert np.array_equal(ft.known_from_discs(base, np.zeros((0, 3), np.int32), 130, 70), (base != 0).astype(np.uint8))
    d2 = rng.integers(0, 50, (70, 130)).astype(np.int32)
    k = ft.known_from_discs(None, discs[:4], 130, 70)
    assert np.array_equal(ft.d2_known(d2, k), ref.d2_known(d2, k)) and np.array_equal(ft.d2_known(d2, k) != 0, (d2 != 0) & (k != 0))


def test_two_disc_ring_is_one_cluster_only_with_diagonal_links():
    known = ft.two_discs()
    fr = ft.frontier_mask(np.full((150, 200), 9, np.int32), known)
    out = ft.frontiers(np.full((150, 200), 9, np.int32), known)
    assert int(fr.sum()) == 268 and out["ncl"].tolist() == [[1, 1]] and out["csize"][0, 0] == 268
    assert ft.count_4connected(fr) == 112


def test_all_known_has_no_frontier(ref):
    d2 = _salt()[0]
    known = np.ones_like(d2, dtype=np.uint8)
    for impl in (ft, ref):
        out = impl.frontiers(d2, known)
        assert out["ncl"].tolist() == [[0, 0]] and (out["label"] == -1).all() and (out["slot"] == -1).all() and (out["rep"] == -1).all()
        cost, cell = impl.cost_matrix(np.zeros((3,) + d2.shape, np.int32), out["slot"], out["csize"], 128)
        assert (cost == ft.INF).all() and (cell == -1).all()
    # nothing known: no frontier either
    assert ft.frontiers(d2, np.zeros_like(known))["ncl"].tolist() == [[0, 0]]


def test_rank_order_cmax_cut_and_min_size(ref):
    d2, known = _salt()
    full = ft.frontiers(d2, known, Cmax=64)
    assert full["ncl"].tolist() == [[43, 43]] and int((full["label"] >= 0).sum()) == 204
    reps = np.unique(full["label"][full["label"] >= 0])
    assert np.array_equal(full["rep"][0, :43], reps) and (full["slot"] >= 0).sum() == 204
    for impl in (ft, ref):
        cut = impl.frontiers(d2, known, Cmax=8)
        assert cut["ncl"].tolist() == [[43, 43]] and np.array_equal(cut["rep"][0], reps[:8])
        assert np.array_equal(cut["csize"][0], full["csize"][0, :8]) and np.array_equal(cut["label"], full["label"])
        assert np.array_equal(cut["slot"], np.where(full["slot"] < 8, full["slot"], -1))
        big = impl.frontiers(d2, known, min_size=3, Cmax=64)
        keep = np.flatnonzero(full["csize"][0, :43] >= 3)
        assert big["ncl"].tolist() == [[23, 43]] and len(keep) == 23
        assert np.array_equal(big["rep"][0, :23], full["rep"][0, keep]) and np.array_equal(big["csize"][0, :23], full["csize"][0, keep])
        assert ((big["slot"] >= 0) == np.isin(full["slot"], keep)).all()


def test_matrix_against_brute_force(ref, fields):
    d2, known = _salt()
    d2k = ft.d2_known(d2, known)
    fr = ft.frontiers(d2k, known, Cmax=64)
    free = np.flatnonzero(d2k.ravel() >= 1)
    roots = free[np.random.default_rng(3).choice(len(free), 6, replace=False)]
    g = np.stack([fields.field(d2k, r)[0] for r in roots])
    g[5] = ft.INF                                                  # a robot that reaches nothing
    g[4] = np.where(g[4] != ft.INF, ft.INF - 10, ft.INF)           # and one whose costs sit just below the clamp
    slot, csize = fr["slot"], fr["csize"][0]
    for gain, cap in ((0, 0), (7, 5), (3, 1000), (2**20, 2**10)):
        cost, cell = ft.cost_matrix(g, slot, fr["csize"], 64, gain, cap)
        c2, l2 = ref.cost_matrix(g, slot, fr["csize"], 64, gain, cap)
        assert np.array_equal(cost, c2) and np.array_equal(cell, l2)
        for f in range(6):
            for k in range(64):
                best = None
                for c in np.flatnonzero(slot.ravel() == k).tolist():          # ascending: the first to attain the minimum stays
                    v = int(g[f].ravel()[c])
                    if v != ft.INF and (best is None or v < best[0]):
                        best = (v, c)
                if best is None:
                    assert cost[f, k] == ft.INF and cell[f, k] == -1
                else:
                    assert cell[f, k] == best[1]
                    assert cost[f, k] == min(best[0] + gain * (cap - min(int(csize[k]), cap)), ft.INF - 1)
        assert (cost[5] == ft.INF).all() and (cost[:5, :43] != ft.INF).any() and (cost >= 0).all()
    assert (cost == ft.INF - 1).any()                              # the clamp of the last pair
    # the tie goes to the smaller cell: a constant field
    cost, cell = ft.cost_matrix(np.full((1,) + d2.shape, 5, np.int32), slot, fr["csize"], 64)
    assert np.array_equal(cell[0, :43], fr["rep"][0, :43]) and (cost[0, :43] == 5).all()
    # a field on a grid that does not exist
    cost, cell = ft.cost_matrix(g[:2], slot, fr["csize"], 64, fgrid=[0, 3])
    c2, l2 = ref.cost_matrix(g[:2], slot, fr["csize"], 64, fgrid=[0, 3])
    assert np.array_equal(cost, c2) and np.array_equal(cell, l2) and (cost[1] == ft.INF).all() and (cost[0] != ft.INF).any()


@pytest.mark.parametrize("name", ["salt96x80", "blocks96x80", "salt130x70"])
def test_exploration_ends_with_the_component_known(oracle, fields, name):
    occ = ft.loop_maps()[name]
    start = ft.loop_start(occ)
    goals, known = ft.explore_loop(occ, start, ft.twin_step(oracle, fields))
    comp = ft.true_component(occ, start)
    assert len(goals) >= 10 and len(set(goals)) == len(goals)
    assert (known[comp] != 0).all()
    assert comp.ravel()[goals].all()


def test_check_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "frontier_ref_check")
    subprocess.check_call(["cc", "-g", "-O1", "-std=c11", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           CHECK, ft.SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("frontier_ref OK") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
