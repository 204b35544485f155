"""The CPU side of tests/test_gpu_limit.py, without a GPU: conditions on the reference alone that keep the comparison at the
8192-cell limit from being empty.  With uniform draws almost every query on a strip ends Q_TRUNCATED and no path comes near
the last line; tests/limit_cases.py places and pins its inputs, and here the oracle and the twins say that the placement
works: the queries find paths, paths reach the last line and cross 4095 | 4096, fields cover the strip, views and rays
change the last line, the matcher moves off its prior, and the two input sets differ in every compared array.  Every figure
is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

import limit_cases as lc
import stream_cases as sc_cases
from limit_cases import MID, Q_OK


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    return sc_cases.Twins(tmp_path_factory.mktemp("limit_cases"))


def test_the_limit_chains_cover_every_grid_entry():
    """Every device entry of the header that takes a W and an H runs in a limit chain or in the space-time strips."""
    want = sc_cases.device_entries() - lc.NO_GRID
    assert lc.NO_GRID <= sc_cases.device_entries()
    have = lc.covered_symbols()
    assert have - {"sc_smooth_paths_batch", "sc_bezier_arclength_batch"} <= want and want <= have, \
        f"not at the limit: {sorted(want - have)}; not grid entries: {sorted(have - want)}"
    assert not any(isinstance(c, lc.Limit) for c in sc_cases.CHAINS)


def _shares(name, status, ok_min, nopath_min=None):
    valid, ok, nopath, trunc = lc.counts(status)
    print(f"{name}: {valid} valid, {ok} Q_OK, {nopath} Q_NO_PATH, {trunc} Q_TRUNCATED")
    assert ok_min[1] * ok >= ok_min[0] * valid, (name, "Q_OK", ok, valid)
    if nopath_min is None:
        assert 8 * trunc <= valid, (name, "Q_TRUNCATED", trunc, valid)
    else:
        assert nopath_min[1] * nopath >= nopath_min[0] * valid, (name, "Q_NO_PATH", nopath, valid)


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_reference_conditions(twins, case):
    family, shape = case
    chain = lc.chain(family, shape)
    st = chain.strip
    form = lambda which: {k: (v.shape, v.dtype) for k, v in chain.inputs(which).items()}
    assert form("A") == form("B")
    assert set(chain.symbols) <= sc_cases.device_entries()
    for which in ("A", "B"):
        o = chain.expected_view(which, twins)
        edge = cross = False
        for pre, (status, ln, path) in chain.queries(o).items():
            name = f"{chain.name} {which} {pre}"
            if family is lc.Components:
                _shares(name, status, (1, 4), (1, 8))
            elif family in (lc.Fields, lc.Pose):
                _shares(name, status, (3, 4))
            else:
                print(name, lc.counts(status))
            e, c = lc.path_reach(st, status, ln, path, chain.edge_margin)
            print(f"{name}: a path on the last line {e}, across 4096 {c}, longest {int(np.max(np.where(status == Q_OK, ln, 0)))}")
            edge, cross = edge | e, cross | c
        if chain.readouts:
            assert edge, (chain.name, which, "no Q_OK path reaches the last line")
            assert cross or not st.mid, (chain.name, which, "no Q_OK path crosses 4095 | 4096")
        last = (lambda a: a[..., :, -1]) if st.xlong else (lambda a: a[..., -1, :])
        if family in (lc.Fields, lc.Explore, lc.Pose):
            inp = chain.inputs(which)
            key, fstat = ("pf_gp", "pf_status") if family is lc.Pose else ("f_g", "f_status")
            for f in np.flatnonzero(o[fstat] == Q_OK):
                g = o[key][f].reshape(-1, chain.H, chain.W)          # a pose field: one layer per heading
                if family is lc.Explore:                             # known free space only: the field is held to what the discs uncovered
                    free = (o["d2k"] > 0)
                    n = int(free.sum())
                    print(f"{chain.name} {which} field {f}: finite on {int(((g[0] >= 0) & (g[0] < 2 ** 30) & free).sum())} of {n} known free cells")
                    continue
                # a pose field: the cells where the footprint fits at every heading (a pose turns on the spot there, so what is
                # reachable is reachable cell by cell, as in a plain field)
                free = o["d2"] > 0 if family is lc.Fields else (o["hmask"] == 0xFF)
                finite = ((g >= 0) & (g < 2 ** 30)).any(0) & free
                print(f"{chain.name} {which} field {f}: finite on {int(finite.sum())} of {int(free.sum())} free cells")
                assert finite.sum() > 0.99 * free.sum(), (chain.name, which, f)
        if family is lc.Views:
            assert last(o["known"]).any() and last(o["known_s"]).any(), "no applied view changes the last line"
            assert (o["known"][:, MID - 1] if st.xlong else o["known"][MID - 1]).any() or not st.mid
        if family is lc.Explore:
            assert last(o["known"]).any(), "no disc reaches the last line"
        if family is lc.Scan:
            inp = chain.inputs(which)
            hit = o["hit"]
            assert (st.long(hit[hit >= 0]) == st.L - 1).any() or last(o["known"]).any(), "no cast ray changes the last line"
            assert last(o["known"]).any() and last(o["L2"]).any()
            rays = inp["rays"]
            assert ((rays[:, 2] >= chain.W) | (rays[:, 3] >= chain.H)).any(), "no ray leaves the grid"
            assert ((rays[:, 2 if st.xlong else 3]) == st.L - 1).any(), "no ray ends on the last line"
            centre_l = inp["centre"][:, 0 if st.xlong else 1]
            assert (centre_l + (40 if st.xlong else 30) > st.L - 1).any(), "the wide window stays inside the grid"
            print(f"{chain.name} {which}: best {o['best'].tolist()} wide {o['wide'].tolist()}")
            assert (o["best"][:, 1:3] != 0).any() and (o["wide"].reshape(chain.S, -1)[:, 1:3] != 0).any(), "the matcher stays on its prior"
    chain.differs(twins)


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_astar_rounds_find_paths(oracle, shape):
    st = lc.Strip(*shape)
    rng = lc.astar_rng(*shape)
    for r in range(2):
        c = lc.astar_limit_case(oracle, rng, *shape, fam=r)
        ref = c["ref"]
        name = f"A* {shape[0]}x{shape[1]} map {r} family {c['fam']} r2 {c['r2']}"
        _shares(name, ref["status"], (3, 4))
        e, x = lc.path_reach(st, ref["status"], ref["len"], ref["path"])
        print(f"{name}: a path on the last line {e}, across 4096 {x}, longest {int(ref['len'][ref['status'] == Q_OK].max())}, "
              f"expanded {int(ref['expanded'].sum())}")
        assert e and (x or not st.mid)
        assert ref["status"][0] == Q_OK and ref["path"][0, ref["len"][0] - 1] == st.corner


@pytest.mark.parametrize("shape", lc.TPLAN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tplan_strips_reserve_the_last_cell(shape):
    import tplan_twin as tw
    from test_gpu_tplan import twin
    W, H = shape
    c = lc.tplan_case(W, H)
    st = lc.Strip(W, H)
    ref = twin(c)
    print(f"tplan {W}x{H}: status {ref['status'].tolist()} arrive {ref['arrive'].tolist()}")
    assert ref["res"].reshape(c["L"], -1)[:, st.corner].all(), "the last cell is reserved in every layer"
    assert ref["res"].reshape(c["L"], -1)[:, :st.corner].any()
    assert (ref["status"] == tw.TP_OK).sum() >= 3 and ref["status"][0] == tw.TP_OK and ref["status"][2] == tw.TP_OK
    assert (st.long(c["start"]) >= st.L - lc.FAR).sum() >= len(c["start"]) - 1
