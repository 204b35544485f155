"""CPU checks of the waypoint definition through its C twin tests/cpp/waypoints_ref.c: Visible
against a brute-force corner-sign test, the shortcut of oracle A* paths against an independent restatement of the greedy
rule and against the output guarantees, and the edge cases.  No GPU needed."""
import numpy as np
import pytest

from sea_current_amd import synth
from waypoints_twin import (Q_BAD_PATH, Q_NO_PATH, Q_OK, Q_TRUNCATED, Twin, check_output, collinear, edge_cases, greedy,
                            visible_brute)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return Twin(tmp_path_factory.mktemp("waypoints_ref"))


@pytest.mark.parametrize("W,H,kind,dens,r2", [(40, 30, "salt", 0.08, 0), (40, 30, "salt", 0.25, 0), (40, 30, "block", 0.2, 0),
                                              (17, 53, "salt", 0.15, 0), (17, 53, "block", 0.3, 0), (40, 30, "block", 0.1, 2)])
def test_visible_matches_brute_force(twin, oracle, W, H, kind, dens, r2):
    occ = synth.salt_grid(W, H, dens, seed=W * H + 7) if kind == "salt" else synth.block_grid(W, H, dens, seed=W + H, smin=2, smax=8)
    d2 = oracle.edt(occ)
    free = np.flatnonzero(d2.ravel() >= max(r2, 1))
    rng = np.random.default_rng(W * 1000 + H)
    pairs = rng.choice(free, size=(2000, 2))
    seen = [0, 0]
    for a, b in pairs:
        want = visible_brute(d2, r2, int(a), int(b))
        assert twin.visible(d2, r2, a, b) == want, (int(a), int(b))
        assert twin.visible(d2, r2, b, a) == want
        seen[want] += 1
    assert min(seen) > 50, seen          # both outcomes are exercised


@pytest.mark.parametrize("r2", [0, 4])
def test_shortcut_of_astar_paths(twin, oracle, r2):
    W = H = 256
    d2 = oracle.edt(synth.block_grid(W, H, 0.20))
    s, g = synth.queries(d2 >= max(r2, 1), 200, seed=17 + r2)
    res = oracle.astar_batch(d2, s, g, r2=r2, Lmax=2048)
    assert (res["status"] == Q_OK).sum() > 150
    out = twin.waypoints(d2, res["path"], res["len"], res["status"], r2=r2)
    vis = lambda u, v: twin.visible(d2, r2, u, v)
    shortened = 0
    for q in range(200):
        if res["status"][q] != Q_OK:
            assert out["status"][q] == res["status"][q] and out["n"][q] == 0
            continue
        assert out["status"][q] == Q_OK
        p = res["path"][q, :res["len"][q]]
        wp = out["wp"][q, :out["n"][q]]
        check_output(vis, W, p, wp)
        want, anchors, fired = greedy(vis, W, p)
        assert not fired                              # the reverse rule does not fire on these A* paths
        assert wp.tolist() == want
        for a in anchors:                             # maximality: the anchor cannot see one cell further
            nxt = [k for k in range(a + 1, len(p)) if not vis(p[a], p[k])]
            if nxt:
                j = nxt[0] - 1
                assert not vis(p[a], p[j + 1])
        shortened += len(wp) < len(p)
    assert shortened > 100


def test_edge_cases(twin):
    d2, path, lens, st, exp, around = edge_cases()
    out = twin.waypoints(d2, path, lens, st)
    for q, e in enumerate(exp):
        assert out["status"][q] == e["status"], q
        assert out["n"][q] == e["n"], q
        if e["wp"] is not None:
            assert out["wp"][q, :e["n"]].tolist() == e["wp"], q
    assert set(out["status"].tolist()) == {Q_OK, Q_NO_PATH, Q_BAD_PATH}
    # Wmax too small: TRUNCATED with the needed count, the first Wmax points written
    tr = twin.waypoints(d2, path[-1:], lens[-1:], None, Wmax=2)
    assert tr["status"][0] == Q_TRUNCATED and tr["n"][0] == 3 and tr["wp"][0].tolist() == around[:1] + [around[2]]
    # no input status: every path is taken as planned
    nost = twin.waypoints(d2, path, lens, None)
    assert nost["status"][4] == Q_OK and nost["n"][4] == 2


def test_collinear_helper():
    W = 10
    assert collinear(W, 0, 2, 4) == 1 and collinear(W, 4, 2, 3) == -1 and collinear(W, 0, 11, 12) == 0
