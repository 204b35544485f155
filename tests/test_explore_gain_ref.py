"""Coordinated exploration goals by gain without a GPU: the NumPy twin (tests/explore_gain_twin.py) equals the C statement
(tests/cpp/explore_gain_ref.c) on random small cases, the identities of the definition hold on the twin, the arguments the
definition refuses are refused by both, and the behavioural fixture separates the travel-cost matching from the picks by
gain."""
import numpy as np
import pytest

import explore_gain_twin as et
import frontier_twin as ft
import sectors_twin as st
import views_twin as vt

INF = et.INF


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return et.Ref(tmp_path_factory.mktemp("explore_gain_ref"))


def _case(seed, W=28, H=22, R=3, N=6, p_occ=0.12):
    """A salted map, a known disc in the middle, breadth-first fields of R robots through the known free cells, N candidates of
    which some are dead (outside the grid, on an obstacle) and two share a cell."""
    rng = np.random.default_rng(seed)
    occ = (rng.random((H, W)) < p_occ).astype(np.uint8)
    known = ft.known_from_discs(None, [(W // 2, H // 2, 49)], W, H)
    occ_seen = np.where(known != 0, occ, 0).astype(np.uint8)
    free = (known != 0) & (occ == 0)
    cells = np.flatnonzero(free.ravel())
    robots = rng.choice(cells, R, replace=len(cells) < R)
    g = np.stack([et.bfs_field(free, int(r)) for r in robots])
    cand = rng.choice(cells, N).astype(np.int32)
    if N >= 4:
        cand[1] = cand[0]
        cand[2] = -1 if seed % 2 else W * H
        blocked = np.flatnonzero(occ_seen.ravel() != 0)
        if len(blocked):
            cand[3] = blocked[0]
    return dict(occ=occ_seen, known=known, g=g, cand=cand, W=W, H=H)


def _same(a, b):
    assert (a is None) == (b is None)
    if a is not None:
        for k in et.OUT_KEYS:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("seed", range(6))
def test_twin_equals_c_statement_full_circle(ref, seed):
    c = _case(seed)
    kw = dict(r2=(16, 25, 36)[seed % 3], wg=(1, 3, 0)[seed % 3], wc=(1, 2)[seed % 2], min_gain=seed % 2)
    _same(et.explore_gain(c["occ"], c["known"], c["g"], c["cand"], **kw), ref.explore_gain(c["occ"], c["known"], c["g"], c["cand"], **kw))


@pytest.mark.parametrize("B,span", [(3, 1), (3, 2), (8, 1), (8, 4), (8, 7), (16, 8)])
def test_twin_equals_c_statement_with_a_table(ref, B, span):
    c = _case(10 + B + span, R=2, N=5)
    d = st.heading_dirs(B)
    a = et.explore_gain(c["occ"], c["known"], c["g"], c["cand"], 25, d, span, wg=2)
    _same(a, ref.explore_gain(c["occ"], c["known"], c["g"], c["cand"], 25, d, span, wg=2))
    picked = a["goal"] >= 0
    assert ((a["head"][picked] >= 0) & (a["head"][picked] < B)).all() and (a["head"][~picked] == -1).all()


def test_refusals(ref):
    c = _case(3)
    d = st.heading_dirs(8)
    bad = [dict(r2=-1), dict(r2=9, wg=(1 << 20) + 1), dict(r2=9, wc=-1), dict(r2=9, min_gain=-1), dict(r2=9, rounds=-1),
           dict(r2=9, rounds=1025), dict(r2=9, dirs=d, span=8), dict(r2=9, dirs=d, span=0), dict(r2=9, dirs=d[::-1].copy(), span=2)]
    for kw in bad:
        assert et.explore_gain(c["occ"], c["known"], c["g"], c["cand"], **kw) is None, kw
        assert ref.explore_gain(c["occ"], c["known"], c["g"], c["cand"], **kw) is None, kw
    g = c["g"].copy()
    g[0, 0, 0] = -1
    assert et.explore_gain(c["occ"], c["known"], g, c["cand"], 9) is None and ref.explore_gain(c["occ"], c["known"], g, c["cand"], 9) is None
    ok = et.explore_gain(c["occ"], c["known"], c["g"], c["cand"], 9, dirs=d, span=7)      # span == B - 1 is the widest sensor
    assert ok is not None


def test_no_candidates_and_no_rounds(ref):
    c = _case(4)
    for kw in (dict(cand=np.zeros(0, np.int32)), dict(cand=c["cand"], rounds=0)):
        a = et.explore_gain(c["occ"], c["known"], c["g"], kw["cand"], 25, rounds=kw.get("rounds"))
        _same(a, ref.explore_gain(c["occ"], c["known"], c["g"], kw["cand"], 25, rounds=kw.get("rounds")))
        assert (a["goal"] == -1).all() and (a["gcost"] == -1).all() and (a["ggain"] == 0).all() and a["npick"][0] == 0
        assert np.array_equal(a["known_out"], c["known"]) and np.array_equal(a["gain0"], a["gain_end"])


@pytest.mark.parametrize("seed", range(4))
def test_identities(seed):
    c = _case(20 + seed, R=3, N=7)
    occ, known, g, cand = c["occ"], c["known"], c["g"], c["cand"]
    a = et.explore_gain(occ, known, g, cand, 25, wg=2)
    # (a) the gains of the picks add up to the free cells newly known
    assert int(a["ggain"].sum()) == int(((occ == 0) & (a["known_out"] != 0) & (known == 0)).sum())
    # (b) gains only fall, and a taken candidate has nothing left to see in the full-circle form
    assert (a["gain_end"] <= a["gain0"]).all()
    taken = a["cand_of"][a["cand_of"] >= 0]
    assert (a["gain_end"][taken] == 0).all()
    # (c) without a gain term the picks are the greedy nearest pairs
    b = et.explore_gain(occ, known, g, cand, 25, wg=0, min_gain=0)
    live = et.alive(occ, cand)
    cost = np.where(live[None, :], g.reshape(len(g), -1)[:, np.where(live, cand, 0)].astype(np.int64), INF)
    free_r, free_n = np.ones(len(g), bool), np.ones(len(cand), bool)
    for t in range(int(b["npick"][0])):
        m = np.where(free_r[:, None] & free_n[None, :], cost, INF)
        r, n = np.unravel_index(np.argmin(m), m.shape)                 # the first minimum: smallest r, then smallest n
        assert b["pick"][r] == t and b["cand_of"][r] == n and b["gcost"][r] == m[r, n]
        free_r[r], free_n[n] = False, False
    touched = np.zeros(len(cand), bool)
    for n in b["cand_of"][b["cand_of"] >= 0]:
        vis_n = vt.seen(occ, st.views_from_cells(cand[n:n + 1], c["W"], c["H"], 25))
        for k in range(len(cand)):
            touched[k] |= bool((vt.seen(occ, st.views_from_cells(cand[k:k + 1], c["W"], c["H"], 25)) & vis_n).any())
    assert np.array_equal(b["gain_end"][~touched], b["gain0"][~touched])
    # (d) one robot, no travel term: the argmax of gain0 with the smallest n
    d = et.explore_gain(occ, known, g[:1], cand, 25, wc=0)
    elig = live & (cost[0] != INF) & (d["gain0"] >= 1)
    if elig.any():
        assert d["cand_of"][0] == int(np.argmax(np.where(elig, d["gain0"], -1)))
    else:
        assert d["npick"][0] == 0


def test_frontier_centres_twin_equals_c_statement(ref):
    for known in (ft.two_discs(), ft.ring(130, 70, 64, 35, 30, 12), ft.staircase(65, 63), ft.band(130, 70)):
        d2 = np.full(known.shape, 100, np.int32)
        for Cmax, min_size in ((4, 1), (64, 2)):
            fr = ft.frontiers(d2, known, 0, min_size, Cmax)
            a = et.frontier_centres(fr["slot"], fr["csize"], fr["csum"], Cmax)
            assert np.array_equal(a, ref.frontier_centres(fr["slot"], fr["csize"], fr["csum"], Cmax))
            L = min(int(fr["ncl"][0, 0]), Cmax)
            assert (a[0, L:] == -1).all() and (a[0, :L] >= 0).all()
            assert (fr["slot"].ravel()[a[0, :L]] == np.arange(L)).all()   # a centre is a cell of its cluster


def test_fixture_separates_cost_matching_from_picks_by_gain(ref):
    f = et.two_doorways()
    W, r2 = f["W"], et.SENSE_R2
    room_a = lambda c: c >= 0 and (c // W) <= 32
    room_b = lambda c: c >= 0 and (c // W) >= 47
    # 1. travel cost and cluster size alone send both robots to room A's doorways
    old = ft.fleet_explore(f["d2k"], f["known"], f["g"], Cmax=8)
    assert int(old["ncl"][0]) == 3
    assert all(room_a(int(c)) for c in old["goal"])
    # 2. with a gain term one robot goes to room B
    new = et.fleet_explore_gain(f["d2k"], f["known"], f["occ_seen"], f["g"], r2, Cmax=8, wg=2, wc=1, min_gain=1)
    assert int(new["npick"][0]) == 2
    assert sorted((room_a(int(c)), room_b(int(c))) for c in new["goal"]) == [(False, True), (True, False)]
    c_new = ref.explore_gain(f["occ_seen"], f["known"], f["g"], new["centre"], r2, wg=2, wc=1, min_gain=1, rounds=2)
    for k in et.OUT_KEYS:
        assert np.array_equal(new[k], c_new[k]), k
    # the second doorway of A lost most of its gain to the first pick
    a2 = [n for n in range(3) if room_a(int(new["centre"][n])) and n not in new["cand_of"]][0]
    assert new["gain_end"][a2] < new["gain0"][a2] // 2
    # 3. the two goals by gain reveal strictly more free cells of the true map
    assert et.revealed(f["occ"], f["known"], new["goal"], r2) > et.revealed(f["occ"], f["known"], old["goal"], r2)
