"""sc_explore_gain_batch / sc_frontier_centres / sc_fleet_explore_gain_batch on the GPU: every output bit-equal to the C
statement (tests/cpp/explore_gain_ref.c) and, where the naive NumPy form is quick enough, to the twin
(tests/explore_gain_twin.py) -- on 64 x 64, 65 x 63 and 130 x 70, blocks and salt, radii 15, 16, 17 and 33, R in {1, 3, 17},
N in {1, 5, 64, 300}; candidates on the tile edges (x or y = 63, 64) and in the grid corners, two on one cell, discs that do not
meet, dead candidates of each kind among live ones; a robot with an all-infinite row; ties in the score; min_gain, rounds and
N = 0 stopping the loop; the full circle and tables of 3, 8, 16 and 64 bins with span 1, B/2 and B - 1; every optional output
NULL and given; known_out aliasing known; argument errors; host forms; frontier_centres on the shapes of the frontier tests
with G = 1 and 2; the chain on one stream followed by field_paths and, for 8 bins, pose_fields; the behavioural fixture;
identity (a) on device outputs; a second call against the first one's known_out."""
import numpy as np
import pytest

import explore_gain_twin as et
import frontier_twin as ft
import sectors_twin as st

pytestmark = pytest.mark.gpu
INF = et.INF


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return et.Ref(tmp_path_factory.mktemp("explore_gain_ref"))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _eq(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{name}: {len(bad)} differ, first at {bad[0].tolist()}: gpu {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def _map(kind, W, H):
    from sea_current_amd import synth
    return synth.block_grid(W, H, 0.3, seed=10, smin=3, smax=24) if kind == "blocks" else synth.salt_grid(W, H, 0.05, seed=2)


def _scene(kind, W, H, R, N, seed=0):
    """The observed map of three sensing discs, Manhattan fields of R robots over its free cells (the last robot's row all
    infinite when R > 1) and N candidates: tile edges, grid corners, a pair on one cell, dead ones of each kind, then frontier
    cells and random free cells."""
    rng = np.random.default_rng(seed)
    true = _map(kind, W, H)
    known = ft.known_from_discs(None, ft.three_discs(W, H), W, H)
    occ = np.where(known != 0, true, 0).astype(np.uint8)
    free = np.flatnonzero(occ.ravel() == 0)
    robots = rng.choice(np.flatnonzero((occ.ravel() == 0) & (known.ravel() != 0)), R)
    ys, xs = np.mgrid[0:H, 0:W]
    g = np.stack([np.where(occ == 0, 10 * (np.abs(xs - r % W) + np.abs(ys - r // W)), INF) for r in robots]).astype(np.int32)
    if R > 1:
        g[-1] = INF
    fr = np.flatnonzero(ft.frontier_mask(np.where(occ == 0, 100, 0), known).ravel())
    edge = [y * W + x for x, y in ((63, 31), (min(64, W - 1), 32), (20, 63 if H > 63 else H - 1), (21, min(64, H - 1)))]
    special = edge + [0, W - 1, (H - 1) * W, W * H - 1, edge[0], -1, W * H, int(np.flatnonzero(occ.ravel() != 0)[0]), -(2**31)]
    pool = np.concatenate([rng.permutation(fr), rng.permutation(free)])
    cand = np.array((special + pool.tolist())[:N] if N >= 5 else pool[:N], np.int64)
    return dict(occ=occ, known=known, g=g, cand=cand.astype(np.int32), W=W, H=H)


def _check(ctx, ref, s, r2, dirs=None, span=0, twin=False, known_out="new", **kw):
    """Every output of the GPU == the C statement's (and the twin's); returns them."""
    tk = _t(s["known"])
    out = ctx.explore_gain(_t(s["occ"]), tk, _t(s["g"]), _t(s["cand"]), r2, dirs, span, known_out=tk if known_out == "alias" else None, **kw)
    ctx.synchronize()
    kw.pop("want_all", None)
    want = ref.explore_gain(s["occ"], s["known"], s["g"], s["cand"], r2, dirs, span, **kw)
    for k in out:
        _eq(k, out[k].cpu().numpy(), want[k])
    if twin:
        tw = et.explore_gain(s["occ"], s["known"], s["g"], s["cand"], r2, dirs, span, **kw)
        for k in et.OUT_KEYS:
            _eq("twin " + k, want[k], tw[k])
    return want, out


@pytest.mark.parametrize("W,H,kind,r", [(64, 64, "blocks", 15), (64, 64, "salt", 16), (65, 63, "blocks", 17), (65, 63, "salt", 33),
                                        (130, 70, "blocks", 16), (130, 70, "salt", 33)])
@pytest.mark.parametrize("R,N", [(1, 5), (3, 1), (3, 64), (17, 5), (17, 64)])
def test_full_circle_equals_the_statements(ctx, ref, W, H, kind, r, R, N):
    s = _scene(kind, W, H, R, N, seed=R + N)
    want, _ = _check(ctx, ref, s, r * r, twin=N <= 5, wg=3, wc=1)
    assert want["npick"][0] <= min(R, N)
    # identity (a) on what the device returned
    assert int(want["ggain"].sum()) == int(((s["occ"] == 0) & (want["known_out"] != 0) & (s["known"] == 0)).sum())


@pytest.mark.parametrize("R", [3, 17])
def test_three_hundred_candidates(ctx, ref, R):
    s = _scene("salt", 130, 70, R, 300, seed=R)
    want, _ = _check(ctx, ref, s, 17 * 17, wg=2)
    assert want["npick"][0] == R - 1                                   # every robot but the one with the infinite row
    _check(ctx, ref, s, 15 * 15, dirs=st.heading_dirs(16), span=8, wg=2)


@pytest.mark.parametrize("B", [3, 8, 16, 64])
def test_tables(ctx, ref, B):
    d = st.heading_dirs(B, 0.25 if B == 16 else 0.0)
    for i, span in enumerate(sorted({1, B // 2, B - 1})):
        s = _scene(("blocks", "salt")[i % 2], *((65, 63), (130, 70))[i % 2], 3, 20, seed=B + span)
        want, _ = _check(ctx, ref, s, (16, 17, 33)[i] ** 2, dirs=d, span=span, twin=(B == 8 and span == 4), wg=2)
        picked = want["goal"] >= 0
        assert picked.any() and (want["head"][picked] >= 0).all() and (want["head"][picked] < B).all()


def test_same_cell_disjoint_discs_and_ties(ctx, ref):
    W, H = 130, 70
    occ, known = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    known[:, :8] = 1
    ys, xs = np.mgrid[0:H, 0:W]
    # two candidates on one cell, one far away whose disc meets neither, two whole discs in the unknown at one distance from
    # robots 0 and 1 (equal gain, equal cost)
    cand = np.array([35 * W + 20, 35 * W + 20, 35 * W + 100, 19 * W + 64, 51 * W + 64], np.int32)
    robots = [35 * W + 64, 35 * W + 64, 35 * W + 20]
    g = np.stack([10 * (np.abs(xs - r % W) + np.abs(ys - r // W)) for r in robots]).astype(np.int32)
    s = dict(occ=occ, known=known, g=g, cand=cand)
    want, _ = _check(ctx, ref, s, 15 * 15, twin=True, wg=1, wc=1)
    assert want["gain0"][0] == want["gain0"][1] > 0 and want["gain_end"][1] == 0      # the twin cell's gain fell to 0
    assert want["gain0"][3] == want["gain0"][4]
    one = _check(ctx, ref, s, 15 * 15, wg=1, wc=1, rounds=1)[0]
    assert one["gain_end"][2] == one["gain0"][2] and one["gain_end"][3] == one["gain0"][3]   # discs that do not meet the pick's
    # equal scores: robots 0 and 1 stand on one cell, candidates 3 and 4 mirror each other: r first, then n
    tie = _check(ctx, ref, s, 15 * 15, twin=True, wg=0, wc=1, min_gain=0)[0]
    assert tie["pick"][2] == 0 and tie["cand_of"][2] == 0              # distance 0 wins the first round
    assert tie["cand_of"][0] == 3 and tie["cand_of"][1] == 4 and tie["pick"][0] < tie["pick"][1]


def test_stopping(ctx, ref):
    s = _scene("salt", 65, 63, 3, 20, seed=5)
    full = _check(ctx, ref, s, 256, wg=2)[0]
    assert full["npick"][0] == 2
    top = int(np.sort(full["ggain"])[-1])
    early = _check(ctx, ref, s, 256, wg=2, min_gain=top)[0]           # the second pick no longer reaches min_gain
    assert early["npick"][0] == 1
    assert _check(ctx, ref, s, 256, wg=2, rounds=1)[0]["npick"][0] == 1
    none = _check(ctx, ref, s, 256, wg=2, rounds=0)[0]
    assert none["npick"][0] == 0 and (none["goal"] == -1).all() and np.array_equal(none["gain0"], none["gain_end"])
    assert np.array_equal(none["known_out"], s["known"])
    s0 = dict(s, cand=np.zeros(0, np.int32))
    empty = _check(ctx, ref, s0, 256)[0]
    assert empty["npick"][0] == 0 and (empty["goal"] == -1).all() and (empty["gcost"] == -1).all()
    assert _check(ctx, ref, s, 256, wg=2, min_gain=10**6)[0]["npick"][0] == 0


def test_optional_outputs_and_aliasing(ctx, ref):
    s = _scene("blocks", 65, 63, 3, 20, seed=7)
    d = st.heading_dirs(8)
    for dirs, span in ((None, 0), (d, 3)):
        want, out = _check(ctx, ref, s, 17 * 17, dirs, span, wg=2, want_all=False)
        assert sorted(out) == ["gcost", "goal", "npick"]
        _check(ctx, ref, s, 17 * 17, dirs, span, wg=2, known_out="alias")


def test_second_call_against_its_own_known_out(ctx, ref):
    """Scratch is reused and the done word of the first call (which ran out of eligible pairs) is cleared."""
    s = _scene("salt", 130, 70, 17, 64, seed=9)
    first = _check(ctx, ref, s, 16 * 16, wg=2, min_gain=200)[0]
    assert first["npick"][0] < 16                                      # stopped early: the done word was set
    s2 = dict(s, known=first["known_out"])
    second = _check(ctx, ref, s2, 16 * 16, wg=2, min_gain=1)[0]
    assert second["npick"][0] > 0 and np.array_equal(second["gain0"], first["gain_end"])
    _check(ctx, ref, s, 16 * 16, dirs=st.heading_dirs(16), span=5, wg=2)   # a table after the full circle, smaller after larger
    _check(ctx, ref, _scene("salt", 64, 64, 3, 5, seed=9), 15 * 15, wg=2)


def test_host_forms(ctx, ref):
    s = _scene("salt", 65, 63, 3, 20, seed=11)
    d = st.heading_dirs(8)
    for dirs, span in ((None, 0), (d, 4)):
        out = ctx.explore_gain_host(s["occ"], s["known"], s["g"], s["cand"], 256, dirs, span, wg=2)
        want = ref.explore_gain(s["occ"], s["known"], s["g"], s["cand"], 256, dirs, span, wg=2)
        for k in et.OUT_KEYS:
            _eq(k, out[k], want[k])
    few = ctx.explore_gain_host(s["occ"], s["known"], s["g"], s["cand"], 256, d, 4, wg=2, want_all=False)
    assert sorted(few) == ["gcost", "goal", "npick"] and np.array_equal(few["goal"], want["goal"])
    import sea_current_amd as sc
    bad = s["g"].copy()
    bad[0, 0, 0] = -1
    with pytest.raises(sc.SeaCurrentError):
        ctx.explore_gain_host(s["occ"], s["known"], bad, s["cand"], 256)


def test_argument_errors(ctx):
    import sea_current_amd as sc
    l, h, p = ctx._l, ctx._h, sc._ptr
    occ, known, kout = (_t(np.zeros((8, 8), np.uint8)) for _ in range(3))
    g, cand = _t(np.zeros((2, 8, 8), np.int32)), _t(np.array([5, 9, 60], np.int32))
    goal, gcost, npick = _t(np.zeros(2, np.int32)), _t(np.zeros(2, np.int32)), _t(np.zeros(1, np.int32))
    good = st.heading_dirs(8)
    INV = 1

    def eg(W=8, H=8, R=2, N=3, o=occ, k=known, gg=g, c=cand, r2=9, d=None, B=None, span=0, wg=1, wc=1, mg=1, rounds=2, go=goal, gc=gcost,
           npk=npick, ko=None):
        d = None if d is None else np.ascontiguousarray(d, dtype=np.int32)
        return l.sc_explore_gain_batch(h, p(o), p(k), p(gg), R, p(c), N, W, H, r2, p(d), (0 if d is None else len(d)) if B is None else B, span,
                                       wg, wc, mg, rounds, p(go), p(gc), None, None, None, None, p(npk), None, None, p(ko))

    assert eg() == 0 and eg(ko=kout) == 0 and eg(ko=known) == 0 and eg(N=0, c=None) == 0 and eg(rounds=0) == 0 and eg(d=good, span=7) == 0
    assert eg(wg=1 << 20, wc=1 << 20, mg=0, rounds=1024) == 0
    assert [eg(W=0), eg(H=0), eg(W=8193), eg(H=8193), eg(R=0), eg(R=1025), eg(N=-1), eg(N=65537), eg(o=None), eg(k=None), eg(gg=None),
            eg(c=None), eg(go=None), eg(gc=None), eg(npk=None), eg(ko=occ)] == [INV] * 16
    assert [eg(r2=-1), eg(wg=-1), eg(wg=(1 << 20) + 1), eg(wc=-1), eg(wc=(1 << 20) + 1), eg(mg=-1), eg(rounds=-1), eg(rounds=1025)] == [INV] * 8
    assert eg(R=1024, N=65537) == INV                                  # refused before anything is touched
    assert [eg(d=good, span=8), eg(d=good, span=0), eg(d=good[::-1], span=2), eg(d=good, B=2, span=1), eg(d=st.heading_dirs(64), B=65, span=2)] == [INV] * 5
    slot, csize, csum, centre = _t(np.full((8, 8), -1, np.int32)), _t(np.zeros(4, np.int32)), _t(np.zeros((4, 2), np.int64)), _t(np.zeros(4, np.int32))
    fc = lambda G=1, W=8, H=8, C=4, s=slot, z=csize, m=csum, ce=centre: l.sc_frontier_centres(h, p(s), p(z), p(m), G, W, H, C, p(ce))
    assert fc() == 0
    assert [fc(G=0), fc(W=0), fc(H=8193), fc(C=0), fc(C=65537), fc(s=None), fc(z=None), fc(m=None), fc(ce=None)] == [INV] * 9
    d2, unk = _t(np.full((8, 8), 100, np.int32)), _t(np.zeros((8, 8), np.uint8))   # `known` was written through its alias above

    def fl(W=8, H=8, ms=1, C=4, dd=d2, R=2, r2=9, rounds=2, go=goal):
        return l.sc_fleet_explore_gain_batch(h, p(dd), p(unk), W, H, 0, ms, C, p(occ), p(g), R, r2, None, 0, 0, 1, 1, 1, rounds, None, None, None,
                                             None, None, None, None, None, p(go), p(gcost), None, None, None, None, p(npick), None, None, None)

    assert fl() == 0
    assert [fl(W=0), fl(ms=0), fl(C=0), fl(C=65537), fl(dd=None), fl(R=0), fl(r2=-1), fl(rounds=1025), fl(go=None)] == [INV] * 9
    ctx.synchronize()
    assert goal.cpu().numpy().tolist() == [-1, -1]                     # nothing is known: no frontier, no pick


@pytest.mark.parametrize("G", [1, 2])
def test_frontier_centres(ctx, ref, G):
    shapes = [ft.two_discs(), ft.ring(200, 150, 100, 75, 60, 25), ft.staircase(200, 150), ft.band(200, 150)]
    for i in range(0, len(shapes), G):
        known = np.stack(shapes[i:i + G]) if G > 1 else shapes[i]
        d2 = np.full(known.shape, 100, np.int32)
        for Cmax, min_size in ((3, 1), (64, 2)):
            fr = ctx.frontiers(_t(d2), _t(known), min_size=min_size, Cmax=Cmax)
            centre = ctx.frontier_centres(fr, 200, 150)
            ctx.synchronize()
            tw = ft.frontiers(d2, known, 0, min_size, Cmax)
            want = et.frontier_centres(tw["slot"], tw["csize"], tw["csum"], Cmax)
            _eq("centre", centre.cpu().numpy(), want)
            _eq("centre (C)", ref.frontier_centres(tw["slot"], tw["csize"], tw["csum"], Cmax), want)
            host = ctx.frontier_centres_host({k: v.cpu().numpy() for k, v in fr.items() if k in ("slot", "csize", "csum")}, 200, 150)
            _eq("centre (host)", host, want)
            assert (want >= 0).any()


def test_the_chain_on_one_stream(ctx, ref, oracle):
    """known_from_views -> edt -> d2_known -> cost_fields -> fleet_explore_gain -> field_paths (and pose_fields for 8 bins), one
    synchronise at the end."""
    import torch
    W, H = 130, 70
    occ = _map("salt", W, H).copy()
    robots = np.array([35 * W + 30, 35 * W + 65, 35 * W + 100, 30 * W + 60], np.int32)
    occ[robots // W, robots % W] = 0
    views = np.stack([robots % W, robots // W, np.full(4, 400)], 1).astype(np.int32)
    d8 = st.heading_dirs(8)
    known, occ_seen = ctx.known_from_views(_t(views), _t(occ), occ_seen=True)
    d2k = ctx.d2_known(ctx.edt(occ_seen), known)
    g = ctx.cost_fields(d2k, _t(robots))["g"]
    a = ctx.fleet_explore_gain(d2k, known, occ_seen, g, 16 * 16, Cmax=64, wg=2, want_all=True)
    b = ctx.fleet_explore_gain(d2k, known, occ_seen, g, 16 * 16, Cmax=64, dirs=d8, span=2, wg=2)
    paths = ctx.field_paths(d2k, g, _t(robots), torch.arange(4, dtype=torch.int32, device="cuda"), a["goal"], Lmax=512)
    rhead = torch.where(b["head"] >= 0, (b["head"] + 1) % 8, -1).to(torch.int32)      # the axis of a sensor of two bins of eight
    pf = ctx.pose_fields(d2k, b["goal"], rhead, 5, toward=True)
    ctx.synchronize()
    kn, seen = known.cpu().numpy(), occ_seen.cpu().numpy()
    wd2k, gh = ft.d2_known(oracle.edt(seen), kn), g.cpu().numpy()
    _eq("d2k", d2k.cpu().numpy(), wd2k)
    wa = et.fleet_explore_gain(wd2k, kn, seen, gh, 16 * 16, Cmax=64, wg=2)
    for k in et.OUT_KEYS + ("label", "slot", "ncl", "rep", "csize", "cbox", "csum", "centre"):
        _eq(k, a[k].cpu().numpy(), wa[k])
    wb = ref.explore_gain(seen, kn, gh, wa["centre"], 16 * 16, d8, 2, wg=2, rounds=4)
    for k in et.OUT_KEYS:
        _eq("table " + k, b[k].cpu().numpy(), wb[k])
    assert (wa["goal"] >= 0).all() and len(set(wa["goal"].tolist())) == 4
    st_, ln, pth = paths["status"].cpu().numpy(), paths["len"].cpu().numpy(), paths["path"].cpu().numpy()
    assert (st_ == 0).all() and all(pth[r, ln[r] - 1] == wa["goal"][r] for r in range(4))
    _eq("path cost", paths["cost"].cpu().numpy(), wa["gcost"])
    assert (pf["status"].cpu().numpy() == 0).all()
    host = ctx.fleet_explore_gain_host(wd2k, kn, seen, gh, 16 * 16, Cmax=64, wg=2, want_all=True)
    for k in et.OUT_KEYS + ("slot", "ncl", "centre"):
        _eq("host " + k, host[k], wa[k])


def test_behavioural_fixture(ctx):
    f = et.two_doorways()
    r2 = et.SENSE_R2
    old = ctx.fleet_explore(_t(f["d2k"]), _t(f["known"]), _t(f["g"]), Cmax=8)
    new = ctx.fleet_explore_gain(_t(f["d2k"]), _t(f["known"]), _t(f["occ_seen"]), _t(f["g"]), r2, Cmax=8, wg=2, wc=1, min_gain=1)
    ctx.synchronize()
    want = et.fleet_explore_gain(f["d2k"], f["known"], f["occ_seen"], f["g"], r2, Cmax=8, wg=2, wc=1, min_gain=1)
    for k in et.OUT_KEYS:
        _eq(k, new[k].cpu().numpy(), want[k])
    _eq("old goal", old["goal"].cpu().numpy(), ft.fleet_explore(f["d2k"], f["known"], f["g"], Cmax=8)["goal"])
    rows = sorted(int(c) // f["W"] for c in new["goal"].cpu().numpy())
    assert rows[0] <= 32 and rows[1] >= 47                             # one robot to room A, one to room B
    assert et.revealed(f["occ"], f["known"], new["goal"].cpu().numpy(), r2) > et.revealed(f["occ"], f["known"], old["goal"].cpu().numpy(), r2)
