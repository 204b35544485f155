"""sc_components_batch / sc_reachable_batch / sc_astar_batch_screened (Context.components, reachable, astar_batch(label=)):
labels, sizes, counts and the largest component bit-exact against the CPU twin (tests/cpp/components_ref.c) on maps chosen
for tile edges, winding corridors and critical clusters; reachability equal to the twin; the screened search equal to the
unscreened one with fewer expansions; the device chain without a host hop; host forms; argument errors."""
import numpy as np
import pytest

from components_twin import Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED, Twin, comb, cut_line, d2_of, rings, serpentine, spiral

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return Twin(tmp_path_factory.mktemp("components_ref_gpu"))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _salt(W, H, p, seed):
    from sea_current_amd import synth
    return d2_of(synth.salt_grid(W, H, p, seed=seed))


def _check(ctx, twin, d2, r2=0):
    ref = twin.components(d2, r2)
    o = ctx.components(_t(d2), r2=r2, want_size=True)
    ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    if not np.array_equal(got["label"], ref["label"]):
        bad = np.argwhere(got["label"] != ref["label"])
        raise AssertionError(f"{len(bad)} labels differ, first at {tuple(bad[0])}: gpu {got['label'][tuple(bad[0])]} "
                             f"ref {ref['label'][tuple(bad[0])]}")
    assert np.array_equal(got["size"], ref["size"])
    assert np.array_equal(got["ncomp"], ref["ncomp"]) and np.array_equal(got["largest"], ref["largest"])
    # without sizes: the same labels, counts and largest component (the sizes then live in scratch)
    o = ctx.components(_t(d2), r2=r2)
    ctx.synchronize()
    assert o["size"] is None
    assert np.array_equal(o["label"].cpu().numpy(), ref["label"])
    assert np.array_equal(o["ncomp"].cpu().numpy(), ref["ncomp"]) and np.array_equal(o["largest"].cpu().numpy(), ref["largest"])
    return ref


@pytest.mark.parametrize("W,H", [(256, 256), (130, 70), (65, 63), (64, 64), (1000, 700)])
def test_salt41_bit_exact(ctx, twin, W, H):
    ref = _check(ctx, twin, _salt(W, H, 0.41, 21))
    assert int(ref["ncomp"][0]) > 10


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_salt_256_bit_exact(ctx, twin, p):
    _check(ctx, twin, _salt(256, 256, p, 22))


@pytest.mark.parametrize("vertical", [False, True])
def test_lines_cut_in_three(ctx, twin, vertical):
    ref = _check(ctx, twin, d2_of(cut_line(129, vertical)))
    assert int(ref["ncomp"][0]) == 3


@pytest.mark.parametrize("name", ["serpentine", "spiral", "comb", "rings"])
def test_mazes(ctx, twin, name):
    occ = {"serpentine": lambda: serpentine(256), "spiral": lambda: spiral(255), "comb": lambda: comb(200, tooth=70),
           "rings": lambda: rings(200)}[name]()
    ref = _check(ctx, twin, d2_of(occ))
    if name == "rings":
        assert int(ref["ncomp"][0]) == 25                   # the outside and 24 rings: nested components do not leak
    else:
        assert int(ref["ncomp"][0]) == 1                      # one corridor through every tile


def test_blocks_with_clearance(ctx, twin, oracle):
    from sea_current_amd import synth
    d2 = oracle.edt(synth.block_grid(300, 200, 0.35))
    ref = _check(ctx, twin, d2, r2=4)
    assert int(ref["ncomp"][0]) > 1


@pytest.mark.parametrize("p", [0.41, 0.20])
def test_salt_1024_bit_exact(ctx, twin, p):
    _check(ctx, twin, _salt(1024, 1024, p, 23))


def test_several_grids_in_one_call(ctx, twin):
    d2 = np.stack([_salt(130, 70, 0.41, 24), np.zeros((70, 130), np.int32), d2_of(serpentine(130)[:70])])
    ref = _check(ctx, twin, d2)
    assert ref["ncomp"][1] == 0 and ref["largest"][1] == -1


@pytest.fixture(scope="module")
def world(twin):
    """256^2 salt at p 0.41 with 1024 random pairs of free cells: more than half of them have no path."""
    d2 = _salt(256, 256, 0.41, 34)
    free = np.flatnonzero(d2.ravel() >= 1)
    rng = np.random.default_rng(26)
    s, g = rng.choice(free, 1024).astype(np.int32), rng.choice(free, 1024).astype(np.int32)
    s[:8] = g[:8]                                             # start == goal
    label = twin.components(d2)["label"]
    return d2, label, s, g, twin.reachable(label, s, g)


def test_reachable_equals_twin(ctx, twin):
    d2 = np.stack([_salt(130, 70, 0.41, 27), _salt(130, 70, 0.5, 28)])
    label = twin.components(d2)["label"]
    rng = np.random.default_rng(29)
    n = 130 * 70
    s, g = rng.integers(-5, n + 5, 4096).astype(np.int32), rng.integers(-5, n + 5, 4096).astype(np.int32)   # some out of range, many blocked
    qg = rng.integers(0, 2, 4096).astype(np.int32)
    qg[:16] = [-1, 2] * 8                                     # a bad grid
    s[16:48] = g[16:48]                                       # start == goal
    ref = twin.reachable(label, s, g, qg)
    for st in (Q_OK, Q_NO_PATH, Q_BAD_ENDPOINT):
        assert (ref == st).sum() > 30
    dev_label = ctx.components(_t(d2))["label"]
    got = ctx.reachable(dev_label, _t(s), _t(g), _t(qg))
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy(), ref)
    # one grid, qgrid None
    got = ctx.reachable(dev_label[0], _t(s), _t(g))
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy(), twin.reachable(label[0], s, g))


def _same_results(a, b):
    a = {k: v.cpu().numpy() for k, v in a.items()}
    b = {k: v.cpu().numpy() for k, v in b.items()}
    for k in ("status", "len", "cost"):
        assert np.array_equal(a[k], b[k]), k
    for q in np.flatnonzero(a["status"] == Q_OK):
        assert np.array_equal(a["path"][q, :a["len"][q]], b["path"][q, :b["len"][q]]), q
    return a


@pytest.mark.parametrize("Lmax", [2048, 8])
def test_screened_equals_unscreened(ctx, oracle, world, Lmax):
    d2, _, s, g, reach = world
    assert 0.5 < (reach == Q_NO_PATH).mean() < 0.7
    dd, ds, dg = _t(d2), _t(s), _t(g)
    label = ctx.components(dd)["label"]
    plain = ctx.astar_batch(dd, ds, dg, Lmax=Lmax)
    n_plain = ctx.astar_last_expansions()
    plain = {k: v.clone() for k, v in plain.items()}
    scr = ctx.astar_batch(dd, ds, dg, Lmax=Lmax, label=label)
    n_scr = ctx.astar_last_expansions()
    a = _same_results(scr, plain)
    st = a["status"].copy()
    if Lmax == 8:
        assert (st == Q_TRUNCATED).any()
    st[st == Q_TRUNCATED] = Q_OK
    assert np.array_equal(st, reach)
    ref = oracle.astar_batch(d2, s, g, Lmax=Lmax, nthreads=8)
    assert np.array_equal(ref["status"], a["status"])
    assert n_scr < n_plain
    assert n_scr == int(ref["expanded"][ref["status"] != Q_NO_PATH].sum())


def test_screened_multi_equals_unscreened(ctx, world):
    d2a, _, s, g, _ = world
    d2 = np.stack([d2a, _salt(256, 256, 0.35, 30)])
    free_b = d2[1].ravel() >= 1
    qg = (np.arange(1024) % 2).astype(np.int32)
    dd, ds, dg, dq = _t(d2), _t(s), _t(g), _t(qg)
    label = ctx.components(dd)["label"]
    plain = {k: v.clone() for k, v in ctx.astar_batch_multi(dd, dq, ds, dg, Lmax=2048).items()}
    scr = ctx.astar_batch_multi(dd, dq, ds, dg, Lmax=2048, label=label)
    ctx.synchronize()
    a = _same_results(scr, plain)
    odd = qg == 1
    assert (a["status"][odd & ~(free_b[s] & free_b[g])] == Q_BAD_ENDPOINT).all()      # blocked on the second grid
    for st in (Q_OK, Q_NO_PATH, Q_BAD_ENDPOINT):
        assert (a["status"][odd] == st).any()


def test_one_stream_chain(ctx, world):
    """components -> screened A* -> path_waypoints with no synchronisation in between."""
    d2, _, s, g, _ = world
    dd, ds, dg = _t(d2), _t(s), _t(g)
    ctx.synchronize()
    wr = ctx.path_waypoints(dd, ctx.astar_batch(dd, ds, dg, Lmax=2048, label=ctx.components(dd)["label"]))
    ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in wr.items()}
    ref = ctx.path_waypoints(dd, ctx.astar_batch(dd, ds, dg, Lmax=2048))
    ctx.synchronize()
    ref = {k: v.cpu().numpy() for k, v in ref.items()}
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["n"], ref["n"])
    assert (got["status"] == Q_OK).sum() > 100 and (got["status"] == Q_NO_PATH).sum() > 100
    for q in np.flatnonzero(got["status"] == Q_OK):
        assert np.array_equal(got["wp"][q, :got["n"][q]], ref["wp"][q, :ref["n"][q]]), q


def test_host_forms_equal_device_forms(ctx, twin):
    d2 = np.stack([_salt(130, 70, 0.41, 31), d2_of(rings(130)[:70])])
    ref = twin.components(d2)
    got = ctx.components_host(d2, want_size=True)
    for k in ("label", "size", "ncomp", "largest"):
        assert np.array_equal(got[k], ref[k]), k
    got = ctx.components_host(d2[0])
    assert got["size"] is None and np.array_equal(got["label"], ref["label"][0]) and got["largest"][0] == ref["largest"][0]
    rng = np.random.default_rng(32)
    s, g = rng.integers(-2, 130 * 70 + 2, 500).astype(np.int32), rng.integers(-2, 130 * 70 + 2, 500).astype(np.int32)
    qg = rng.integers(-1, 3, 500).astype(np.int32)
    assert np.array_equal(ctx.reachable_host(ref["label"], s, g, qg), twin.reachable(ref["label"], s, g, qg))
    assert np.array_equal(ctx.reachable_host(ref["label"][0], s, g), twin.reachable(ref["label"][0], s, g))


def test_argument_errors(ctx):
    import torch
    l, h = ctx._l, ctx._h
    d2 = torch.ones((8, 8), dtype=torch.int32, device="cuda")
    lab = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    q = torch.zeros(4, dtype=torch.int32, device="cuda")
    path = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()
    INVALID = 1
    assert l.sc_components_batch(h, None, 1, 8, 8, 0, p(lab), None, None, None) == INVALID
    assert l.sc_components_batch(h, p(d2), 1, 8, 8, 0, None, None, None, None) == INVALID
    assert l.sc_components_batch(h, p(d2), 0, 8, 8, 0, p(lab), None, None, None) == INVALID
    assert l.sc_components_batch(h, p(d2), 1, 0, 8, 0, p(lab), None, None, None) == INVALID
    assert l.sc_components_batch(h, p(d2), 1, 8, 8193, 0, p(lab), None, None, None) == INVALID
    assert l.sc_components_batch(h, p(d2), 1, 8, 8, 0, p(lab), None, None, None) == 0        # every optional output left out
    assert l.sc_reachable_batch(h, None, 1, None, 8, 8, p(q), p(q), 4, p(q)) == INVALID
    assert l.sc_reachable_batch(h, p(lab), 1, None, 8, 8, p(q), p(q), 4, None) == INVALID
    assert l.sc_reachable_batch(h, p(lab), 2, None, 8, 8, p(q), p(q), 4, p(q)) == INVALID       # qgrid NULL needs G == 1
    assert l.sc_reachable_batch(h, p(lab), 1, None, 8, 8, p(q), p(q), -1, p(q)) == INVALID
    assert l.sc_reachable_batch(h, p(lab), 1, None, 8, 8, p(q), p(q), 0, p(q)) == 0             # Q == 0: a no-op
    scr = lambda **kw: l.sc_astar_batch_screened(h, kw.get("d2", p(d2)), kw.get("label", p(lab)), kw.get("G", 1), None, kw.get("W", 8), 8,
                                                 0, p(q), p(q), kw.get("Q", 4), kw.get("Lmax", 8), p(path), p(q), p(q), kw.get("status", p(q)))
    for bad in (dict(d2=None), dict(label=None), dict(G=0), dict(G=2), dict(W=0), dict(W=8193), dict(Q=-1), dict(Lmax=0), dict(status=None)):
        assert scr(**bad) == INVALID, bad
    assert scr(Q=0) == 0
    ctx.synchronize()
