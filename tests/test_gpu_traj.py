"""Conflicts between timed paths on the GPU (sc_traj_knots_batch, sc_traj_conflicts_batch, sc_fleet_conflicts_batch): every
output against the NumPy twin bit for bit (fp64 values as bit patterns, integers, tstatus, the matrix) on the seeded random
fleet and the hand cases, the entry points against each other, argument errors, host forms, and the device chain behind
smooth_paths without a host hop.  The pair kernel works on tiles of 64 row paths x 32 column paths x chunks of 16 ticks:
P = 1, 2, 3, 64, 65, 130 and K = 1, 2, 15, 16, 17, 63, 64, 65, 300 walk around those sizes; path lengths 1, 2 and 70.  A launch
splits column tiles and tick chunks over about 4096 workgroups, so at these sizes a workgroup sees one tile and one chunk:
P = 65 with K = 11000 gives every workgroup two chunks at that default, and contexts created with SC_TRAJ_WORKGROUPS lowered
make the 130-path fleet walk up to 5 tiles and 19 chunks inside one workgroup."""
import numpy as np
import pytest

import traj_cases as tc
import traj_twin as tw

pytestmark = pytest.mark.gpu

INF = float("inf")
FLOATS = ("first_t", "min_sep")
INTS = ("first_with", "min_with", "n_conf", "tstatus")
PATH_KEYS = ("time", "pts", "offsets", "length", "status")


@pytest.fixture(scope="module")
def ctx():
    import sea_current_amd as sc
    c = sc.Context(0)
    yield c
    c.close()


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(o):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in o.items()}


def _sm(c):
    return {k: _t(c[k]) for k in PATH_KEYS if c[k] is not None}


def _fleet(ctx, c, **kw):
    o = ctx.fleet_conflicts(_sm(c), _t(c["radius"]), t0=_t(c["t0"]), flags=_t(c["flags"]), group=_t(c["group"]), T0=c["T0"], dt_c=c["dt_c"],
                            K=c["K"], sep_cap=c["sep_cap"], want_matrix=True, want_knots=True, **kw)
    ctx.synchronize()
    return _np(o)


def _same(got, ref, keys=FLOATS + INTS + ("knots", "conflict")):
    for k in keys:
        if k in FLOATS or k == "knots":
            assert np.array_equal(tc.bits(got[k]), tc.bits(ref[k])), k
        elif k == "conflict":
            assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k   # torch holds the words as int32
        else:
            assert np.array_equal(got[k], ref[k]), k


_twin_cache = {}


def _twin(name, make):
    """The twin's answer to a named case, computed once."""
    if name not in _twin_cache:
        c = make()
        _twin_cache[name] = (c, tw.fleet(**c))
    return _twin_cache[name]


def _sub(P, K):
    """The random fleet's generator at another size (its first three paths have 1, 2 and 70 samples), the clock stretched so that
    its K ticks cover the same 75 s."""
    return lambda: tc.random_fleet(seed=tc.FLEET_SEED + P + K, P=P, K=K, dt_c=75.0 / K, box=12.0 if P < 64 else 40.0)


@pytest.mark.parametrize("P,K", [(130, 300), (1, 17), (2, 17), (3, 17), (64, 17), (65, 17), (65, 1), (65, 2), (65, 15), (65, 16), (65, 63),
                                 (65, 64), (65, 65), (65, 11000)])
def test_random_fleet_against_twin(ctx, P, K):
    c, ref = _twin(("fleet", P, K), (lambda: tc.random_fleet()) if (P, K) == (130, 300) else _sub(P, K))
    got = _fleet(ctx, c)
    _same(got, ref)
    if P >= 64:
        assert (ref["n_conf"] > 0).any() and (ref["tstatus"] != 0).sum() == 7


@pytest.mark.parametrize("target", [1, 6, 30])
def test_several_tiles_and_chunks_per_workgroup(target):
    """The 130-path fleet (3 row tiles, 5 column tiles, 19 tick chunks) with the launch aiming for `target` workgroups:
    1: one workgroup per row tile walks all 5 tiles in each of the 19 chunks; 6: two column shares (tiles 0, 2, 4 and 1, 3), 19
    chunks each; 30: one tile per workgroup, two tick splits of 10 and 9 chunks.  The barrier before a tile is staged again,
    the row knots' reload, the carry of the minima across both loops and the matrix word of a later tile all show in the
    outputs, which equal the twin's (and so the default launch's) bit for bit, with and without the caller's matrix."""
    import os
    import sea_current_amd as sc
    os.environ["SC_TRAJ_WORKGROUPS"] = str(target)
    try:
        low = sc.Context(0)
    finally:
        del os.environ["SC_TRAJ_WORKGROUPS"]
    try:
        c, ref = _twin(("fleet", 130, 300), tc.random_fleet)
        _same(_fleet(low, c), ref)
        bare = _np(low.fleet_conflicts(_sm(c), _t(c["radius"]), t0=_t(c["t0"]), flags=_t(c["flags"]), group=_t(c["group"]), T0=c["T0"],
                                       dt_c=c["dt_c"], K=c["K"]))
        _same(bare, ref, FLOATS + INTS)
        h, href = _twin(("hand", "tie"), HAND["tie"])
        _same(_fleet(low, h), href)
    finally:
        low.close()


HAND = {
    "head_on": lambda: tc.head_on(0.25), "head_on_3s": lambda: tc.head_on(3.0), "crossing": lambda: tc.crossing(0.0),
    "crossing_1s": lambda: tc.crossing(1.0), "crossing_2s": lambda: tc.crossing(2.0), "parked": lambda: tc.parked(True),
    "vanishing": lambda: tc.parked(False), "tie": tc.mirror_tie,
    "one_interval": lambda: tc.pack([tc.line(0, 0, 8, 0), tc.line(8, 0, 0, 0)], 0.5, dt_c=8.0, K=1),
    "one_sample": lambda: tc.pack([tc.line(0, 0, 8, 0), (np.array([2.0]), np.array([[4.0, 0.25]]))], 0.5),
    "capped": lambda: {**tc.crossing(2.0), "sep_cap": 1.0},
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases_against_twin(ctx, name):
    c, ref = _twin(("hand", name), HAND[name])
    got = _fleet(ctx, c)
    _same(got, ref)
    if name.startswith("head_on") or name == "one_interval":
        assert got["first_t"].tolist() == [3.5, 3.5] and got["min_sep"].tolist() == [0.0, 0.0]
    if name == "parked":
        assert got["first_t"].tolist() == [17.0, 17.0]
    if name == "vanishing":
        assert got["first_t"].tolist() == [INF, INF] and got["min_sep"].tolist() == [8.0, 8.0]
    if name == "tie":
        assert got["first_with"].tolist() == [1, 0, 1] and got["min_with"].tolist() == [1, 0, 1]


def test_entry_points_agree(ctx):
    """knots of the separate and the combined call, the combined call with and without the caller's buffers, a call that
    asks for one output only, and sep_cap: equal wherever the definition says so."""
    c, ref = _twin(("fleet", 130, 300), tc.random_fleet)
    full = _fleet(ctx, c)
    sm = _sm(c)
    kn = ctx.traj_knots(sm, t0=_t(c["t0"]), flags=_t(c["flags"]), T0=c["T0"], dt_c=c["dt_c"], K=c["K"])
    assert np.array_equal(tc.bits(kn["knots"].cpu().numpy()), tc.bits(full["knots"]))
    sep = _np(ctx.traj_conflicts(kn["knots"], kn["tstatus"], _t(c["radius"]), group=_t(c["group"]), T0=c["T0"], dt_c=c["dt_c"], want_matrix=True))
    ctx.synchronize()
    _same(sep, full, FLOATS + INTS + ("conflict",))
    bare = _np(ctx.fleet_conflicts(sm, _t(c["radius"]), t0=_t(c["t0"]), flags=_t(c["flags"]), group=_t(c["group"]), T0=c["T0"], dt_c=c["dt_c"],
                                   K=c["K"]))                     # knots in the context's scratch, n_conf without the matrix
    assert bare["conflict"] is None and "knots" not in bare
    _same(bare, full, FLOATS + INTS)
    import sea_current_amd as sc
    import torch
    only = torch.full((130,), -7, dtype=torch.int32, device="cuda")
    p = sc._ptr
    assert sc.lib().sc_fleet_conflicts_batch(ctx._h, p(sm["time"]), p(sm["pts"]), p(sm["offsets"]), p(sm["length"]), p(sm["status"]), 130,
                                             p(_t(c["t0"])), p(_t(c["flags"])), c["T0"], c["dt_c"], c["K"], None, None, p(_t(c["radius"])),
                                             p(_t(c["group"])), INF, None, None, None, None, p(only), None) == 0
    ctx.synchronize()
    assert np.array_equal(only.cpu().numpy(), full["n_conf"])
    capped = _fleet(ctx, {**c, "sep_cap": 2.0})
    _same(capped, tw.fleet(**{**c, "sep_cap": 2.0}))
    far = full["min_sep"] >= 2.0
    assert far.any() and (~far).any() and np.isinf(capped["min_sep"][far]).all() and (capped["min_with"][far] == -1).all()
    _same({k: (v[~far] if k in ("min_sep", "min_with") else v) for k, v in capped.items()},
          {k: (v[~far] if k in ("min_sep", "min_with") else v) for k, v in full.items()}, FLOATS + INTS + ("conflict", "knots"))


def test_default_arguments_and_ticks(ctx):
    """t0, flags, group and status NULL; K=None covers the longest path plus its delay."""
    c = {**tc.random_fleet(seed=3, P=40, K=65, broken=False), "t0": None, "flags": None, "group": None, "status": None}
    _same(_fleet(ctx, c), tw.fleet(**c))
    h = tc.parked(True)
    o = ctx.fleet_conflicts(_sm(h), 0.5, t0=_t(h["t0"]), dt_c=0.5, want_matrix=True)
    assert o["K"] == 36                                            # the second path ends at 10 + 8 s
    assert _np(o)["first_t"].tolist() == [17.0, 17.0]


def test_argument_errors(ctx):
    import sea_current_amd as sc
    c = tc.head_on()
    sm = _sm(c)
    p = sc._ptr
    import torch
    kn = torch.zeros((2, 17, 2), dtype=torch.float64, device="cuda")
    ts = torch.zeros(2, dtype=torch.int32, device="cuda")
    rad = _t(c["radius"])
    f = torch.zeros(2, dtype=torch.float64, device="cuda")

    def knots(P=2, K=16, T0=0.0, dt_c=0.5, time=sm["time"], out=kn, st=ts):
        return sc.lib().sc_traj_knots_batch(ctx._h, p(time), p(sm["pts"]), p(sm["offsets"]), p(sm["length"]), None, P, None, None, T0, dt_c, K,
                                            p(out), p(st))

    def conf(P=2, K=16, T0=0.0, dt_c=0.5, sep_cap=INF, knp=kn, st=ts, r=rad):
        return sc.lib().sc_traj_conflicts_batch(ctx._h, p(knp), p(st), P, K, T0, dt_c, p(r), None, sep_cap, p(f), None, None, None, None, None)

    def fleet(P=2, K=16, dt_c=0.5, sep_cap=INF, r=rad, off=sm["offsets"]):
        return sc.lib().sc_fleet_conflicts_batch(ctx._h, p(sm["time"]), p(sm["pts"]), p(off), p(sm["length"]), None, P, None, None, 0.0, dt_c, K,
                                                 None, None, p(r), None, sep_cap, p(f), None, None, None, None, None)

    assert knots() == 0 and conf() == 0 and fleet() == 0
    for kw in (dict(P=0), dict(P=16385), dict(K=0), dict(K=65536), dict(P=16384, K=4096), dict(dt_c=0.0), dict(dt_c=-1.0), dict(dt_c=INF),
               dict(dt_c=float("nan")), dict(T0=INF), dict(T0=float("nan"))):
        assert knots(**kw) == 1 and conf(**kw) == 1, kw
    assert knots(time=None) == 1 and knots(out=None) == 1 and knots(st=None) == 1
    assert conf(knp=None) == 1 and conf(st=None) == 1 and conf(r=None) == 1
    for cap in (0.0, -1.0, float("nan")):
        assert conf(sep_cap=cap) == 1 and fleet(sep_cap=cap) == 1
    assert fleet(P=0) == 1 and fleet(K=0) == 1 and fleet(dt_c=0.0) == 1 and fleet(r=None) == 1 and fleet(off=None) == 1
    ctx.synchronize()
    with pytest.raises(sc.SeaCurrentError):
        ctx.fleet_conflicts(sm, 0.5, dt_c=-0.1, K=4)


def test_host_forms_equal_device_forms(ctx):
    import sea_current_amd as sc
    c = tc.random_fleet()
    c["radius"][[12, 13]] = 0.5                                    # the host forms refuse a t0 or radius outside the contract
    c["t0"][11] = 1.0
    ref = tw.fleet(**c)
    dev = _fleet(ctx, c)
    _same(dev, ref)
    sm = {k: c[k] for k in PATH_KEYS}
    kw = dict(T0=c["T0"], dt_c=c["dt_c"])
    host = ctx.fleet_conflicts_host(sm, c["radius"], t0=c["t0"], flags=c["flags"], group=c["group"], K=c["K"], want_matrix=True, want_knots=True, **kw)
    _same(host, dev)
    kn = ctx.traj_knots_host(sm, t0=c["t0"], flags=c["flags"], K=c["K"], **kw)
    assert np.array_equal(tc.bits(kn["knots"]), tc.bits(dev["knots"])) and np.array_equal(kn["tstatus"], dev["tstatus"])
    sep = ctx.traj_conflicts_host(kn["knots"], kn["tstatus"], c["radius"], group=c["group"], want_matrix=True, **kw)
    _same(sep, dev, FLOATS + INTS + ("conflict",))
    few = ctx.fleet_conflicts_host(sm, c["radius"], t0=c["t0"], flags=c["flags"], group=c["group"], K=c["K"], **kw)
    _same(few, dev, FLOATS + INTS)
    for key, val in (("radius", -0.5), ("radius", float("nan")), ("t0", INF)):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        bad[key][20] = val
        with pytest.raises(sc.SeaCurrentError):
            ctx.fleet_conflicts_host(sm, bad["radius"], t0=bad["t0"], flags=c["flags"], group=c["group"], K=c["K"], **kw)
    off = c["offsets"].copy()
    off[4] = off[3] - 1
    with pytest.raises(sc.SeaCurrentError):
        ctx.traj_knots_host({**sm, "offsets": off}, K=c["K"], **kw)
    with pytest.raises(sc.SeaCurrentError):
        ctx.traj_conflicts_host(kn["knots"], kn["tstatus"], np.full(130, -1.0), **kw)


def test_device_chain_without_host_hop(ctx):
    """astar_batch -> path_waypoints -> cells_to_points -> smooth_paths -> fleet_conflicts on one stream, a dozen queries that
    cross on the 64 x 48 map of the speed-limit tests: equal to the same calls fed from host copies, and to the twin on the
    smoother's outputs."""
    import torch
    occ = np.zeros((48, 64), np.uint8)
    occ[4:9, 6:12] = 1
    occ[30:40, 22:30] = 1
    occ[10:14, 50:64] = 1
    occ[44:48, 0:64:3] = 1
    res = float(np.float32(np.float32(7.7) / np.float32(300)))
    x0 = float(np.float32(-3.3))
    d2 = ctx.edt(_t(occ))
    cell = lambda x, y: y * 64 + x
    ys = (16, 20, 24, 27, 18, 22)
    s = [cell(2, y) for y in ys] + [cell(60, y) for y in ys]       # six left to right, six right to left on the same rows
    g = [cell(60, y) for y in reversed(ys)] + [cell(2, y) for y in reversed(ys)]
    s, g = _t(np.array(s, np.int32)), _t(np.array(g, np.int32))
    Q = 12
    radius, t0 = 0.5 * res, _t(np.linspace(0.0, 1.1, Q))

    def chain(hop):
        def h(x):
            if not hop:
                return x
            ctx.synchronize()
            return {k: (v.cpu().cuda() if hasattr(v, "cpu") else v) for k, v in x.items()} if isinstance(x, dict) else x.cpu().cuda()
        r = h(ctx.astar_batch(d2, s, g, r2=1, Lmax=512))
        wr = h(ctx.path_waypoints(d2, r, r2=1, Wmax=64))
        path, npts = ctx.cells_to_points(wr, 64, x0, x0, res, res)
        sm = h(ctx.smooth_paths(h(path), h(npts), (-1.0, 1.0, -0.5, 0.5), capacity=Q * 2000))
        o = ctx.fleet_conflicts(sm, radius, t0=t0, dt_c=0.1, K=80, want_matrix=True, want_knots=True)
        ctx.synchronize()
        return _np(sm), _np(o)

    (sm, a), (_, b) = chain(False), chain(True)
    assert (sm["status"] == 0).all() and int(sm["needed"][0]) <= Q * 2000
    end = (sm["time"][sm["offsets"][:-1] + sm["length"] - 1] + np.linspace(0.0, 1.1, Q)).max()
    assert end <= 8.0                                              # K = 80 covers every path
    _same(a, b)
    ref = tw.fleet(sm["time"], sm["pts"], sm["offsets"], sm["length"], sm["status"], np.linspace(0.0, 1.1, Q), None, 0.0, 0.1, 80,
                   np.full(Q, radius))
    _same(a, ref)
    assert (a["n_conf"] > 0).sum() >= 4 and (a["tstatus"] == 0).all()
