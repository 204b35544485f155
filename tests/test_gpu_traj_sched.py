"""Delay schedules on the GPU (sc_traj_shift_table_batch, sc_traj_schedule_batch, sc_traj_shift_knots_batch,
sc_fleet_schedule_batch): table, slot, counts, tstatus and the bit patterns of knots_out against the NumPy twin exactly, on
the seeded fleet and on sizes around the kernel's tiles.  The table kernel gives a wavefront one pair (two when 2D-1 <= 31, four when 2D-1 <= 15:
D = 8, 9 and D = 16, 17 sit on either side), streams the rows through LDS in chunks of 64 ticks behind a halo of (D-1) * stride ticks (K = 63,
64, 65, 128, 129 walk around the chunks; (D-1) * stride = 512 is the largest halo LDS takes, 700 reads global memory), and
skips pairs whose boxes are too far apart (SC_TRAJ_SCHED_NOSKIP=1 evaluates them: the same table).  Then the entry points
against each other, host forms, argument errors, the residual report of traj_conflicts and the device chain behind
smooth_paths."""
import numpy as np
import pytest

import traj_cases as tc
import traj_sched_twin as sw

pytestmark = pytest.mark.gpu

PATH_KEYS = ("time", "pts", "offsets", "length", "status")
INTS = ("table", "slot", "counts", "tstatus")


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


def _fleet(ctx, c, D, stride, order=None, jmax=None, **kw):
    kw = {"want_table": True, "want_knots": True, **kw}
    o = ctx.fleet_schedule(_sm(c), _t(c["radius"]), t0=_t(c["t0"]), flags=_t(c["flags"]), group=_t(c["group"]), T0=c["T0"], dt_c=c["dt_c"],
                           K=c["K"], D=D, stride=stride, order=None if order is None else _t(np.asarray(order, np.int32)),
                           jmax=None if jmax is None else _t(np.asarray(jmax, np.int32)), **kw)
    ctx.synchronize()
    return _np(o)


def _same(got, ref, keys=INTS + ("knots", "knots_out", "delay")):
    for k in keys:
        if k in INTS:
            a = got[k].view(np.uint64) if k == "table" else got[k]            # torch holds the table's words as int64
            assert np.array_equal(a, ref[k]), k
        else:
            assert np.array_equal(tc.bits(got[k]), tc.bits(ref[k])), k


_twin_cache = {}


def _twin(name, make, D, stride, **kw):
    """The twin's answer to a named case, computed once."""
    if name not in _twin_cache:
        c = make()
        _twin_cache[name] = (c, sw.fleet_schedule(**c, D=D, stride=stride, **kw))
    return _twin_cache[name]


def _big(D=8, stride=1, K=300):
    return _twin(("fleet", D, stride, K), lambda: tc.random_fleet(K=K), D, stride)


def _sub(P, K):
    """The random fleet's generator at another size, the clock stretched so that its K ticks cover the same 75 s; the few paths of
    a small fleet share a small box, so that they meet."""
    return lambda: tc.random_fleet(seed=tc.FLEET_SEED + P + K, P=P, K=K, dt_c=75.0 / K, box=3.0 if P < 64 else 40.0)


@pytest.mark.parametrize("D,stride,K", [(8, 1, 300), (8, 4, 300), (32, 2, 400), (1, 1, 300), (17, 1, 300), (16, 1, 300), (9, 1, 300)])
def test_fleet_against_twin(ctx, D, stride, K):
    c, ref = _big(D, stride, K)
    _same(_fleet(ctx, c, D, stride), ref)
    assert (ref["tstatus"] != 0).sum() == 7 and ref["counts"][0] > 0 and ref["counts"][2] > 0 and (D == 1 or ref["counts"][1] > 0)


@pytest.mark.parametrize("P", [1, 2, 3, 64, 65])
def test_small_fleets(ctx, P):
    c, ref = _twin(("sub", P, 17), _sub(P, 17), 8, 1)
    _same(_fleet(ctx, c, 8, 1), ref)
    assert P == 1 or (ref["table"] != 0).any()


@pytest.mark.parametrize("K", [1, 2, 15, 16, 17, 63, 64, 65, 128, 129])
def test_chunk_and_halo_edges(ctx, K):
    """P = 65 with D = min(K + 1, 8): one below, at and one above one and two chunks of 64 intervals; K = 1 has (D-1) * stride == K."""
    D = min(K + 1, 8)
    c, ref = _twin(("sub", 65, K), _sub(65, K), D, 1)
    _same(_fleet(ctx, c, D, 1), ref)


@pytest.mark.parametrize("D,stride,K", [(5, 128, 512), (8, 100, 700), (3, 150, 300)])
def test_shifts_as_long_as_the_horizon(ctx, D, stride, K):
    """(D-1) * stride == K: 512 is the largest halo the LDS build takes (and D = 5 would pack four pairs per wavefront if their
    rows fitted: two), 700 goes through the build that reads global memory, and 2 * 150 ticks of 300 with an even stride."""
    c, ref = _twin(("long", D, stride, K), _sub(65, K), D, stride)
    _same(_fleet(ctx, c, D, stride), ref)
    assert (ref["table"] != 0).any()


@pytest.mark.parametrize("flag", [0, 3])
def test_uniform_flags(ctx, flag):
    c, ref = _twin(("flags", flag), lambda: {**tc.random_fleet(), "flags": np.full(tc.FLEET_P, flag, np.int32)}, 8, 2)
    _same(_fleet(ctx, c, 8, 2), ref)


def test_order_pins_and_limits(ctx):
    c, base = _big()
    rng = np.random.default_rng(2)
    P = tc.FLEET_P
    order = rng.permutation(P)
    _same(_fleet(ctx, c, 8, 1, order=order), sw.fleet_schedule(**c, D=8, stride=1, order=order))
    order[[3, 17]] = order[0]                                      # repeats: two paths are never named
    order[[5, 6, 7]] = -1, P, 2 ** 31 - 1
    jmax = rng.integers(0, 11, P)                                  # 8, 9, 10: clamped
    jmax[rng.random(P) < 0.2] = -1                                 # pinned
    ref = sw.fleet_schedule(**c, D=8, stride=1, order=order, jmax=jmax)
    _same(_fleet(ctx, c, 8, 1, order=order, jmax=jmax), ref)
    assert (ref["slot"] == -3).sum() == 5 and (ref["slot"] > 0).any() and (ref["slot"] == -1).any() and not np.array_equal(ref["slot"], base["slot"])
    _same(_fleet(ctx, c, 8, 1, jmax=0), sw.fleet_schedule(**c, D=8, stride=1, jmax=np.zeros(P, np.int32)))


def test_box_skip_changes_no_bit():
    """A context created with SC_TRAJ_SCHED_NOSKIP=1 evaluates the 5678 pairs of the fleet that the box test drops."""
    import os
    import sea_current_amd as sc
    os.environ["SC_TRAJ_SCHED_NOSKIP"] = "1"
    try:
        dense = sc.Context(0)
    finally:
        del os.environ["SC_TRAJ_SCHED_NOSKIP"]
    try:
        for cfg in ((8, 1, 300), (32, 2, 400)):
            c, ref = _big(*cfg)
            _same(_fleet(dense, c, cfg[0], cfg[1]), ref)
    finally:
        dense.close()


def test_entry_points_agree(ctx):
    """The three separate calls against the combined one, and the combined call with the context's scratch for knots, tstatus
    and table."""
    import torch
    c, ref = _big(8, 4, 300)
    full = _fleet(ctx, c, 8, 4)
    kn = ctx.traj_knots(_sm(c), t0=_t(c["t0"]), flags=_t(c["flags"]), T0=c["T0"], dt_c=c["dt_c"], K=c["K"])
    tb = ctx.traj_shift_table(kn["knots"], kn["tstatus"], _t(c["radius"]), group=_t(c["group"]), D=8, stride=4)
    sd = ctx.traj_schedule(tb["table"], tb["tstatus"], D=8)
    out = ctx.traj_shift_knots(kn["knots"], sd["slot"], stride=4)
    ctx.synchronize()
    sep = _np(dict(table=tb["table"], tstatus=tb["tstatus"], slot=sd["slot"], counts=sd["counts"], knots_out=out))
    _same(sep, ref, INTS + ("knots_out",))
    bare = _fleet(ctx, c, 8, 4, want_table=False, want_knots=False)
    assert "table" not in bare and "knots" not in bare and "knots_out" not in bare
    _same(bare, full, ("slot", "counts", "tstatus", "delay"))
    prefilled = torch.full((tc.FLEET_P, tc.FLEET_P), -1, dtype=torch.int64, device="cuda")   # every entry is written
    import sea_current_amd as sc
    assert sc.lib().sc_traj_shift_table_batch(ctx._h, sc._ptr(kn["knots"]), sc._ptr(kn["tstatus"]), tc.FLEET_P, c["K"], sc._ptr(_t(c["radius"])),
                                              sc._ptr(_t(c["group"])), 8, 4, sc._ptr(prefilled)) == 0
    ctx.synchronize()
    assert np.array_equal(prefilled.cpu().numpy().view(np.uint64), ref["table"])


@pytest.mark.parametrize("P,K,box,D,stride", [(70, 70, 12.0, 4, 3), (33, 17, 6.0, 8, 1)])
def test_unshifted_bit_is_the_conflict_matrix(ctx, P, K, box, D, stride):
    """The table kernel and the pair kernel evaluate one predicate (sc_traj_closest): on the same knots, tstatus, radius and
    group, bit D-1 of table[p][q] (nobody shifted) is bit q % 32 of word q // 32 of traj_conflicts' matrix, and both calls leave
    the same tstatus.  The smallest sizes that cross the pair kernel's 64-row and 32-column tiles and 16-tick chunks and the
    table kernel's 64-tick chunk; D = 4 packs four pairs into a wavefront, D = 8 two.  On the two twins the identity holds with
    328 of 4900 and 130 of 1089 bits set and 5 paths BAD."""
    c = tc.random_fleet(seed=tc.FLEET_SEED + P + K, P=P, K=K, dt_c=75.0 / K, box=box)
    kn = ctx.traj_knots(_sm(c), t0=_t(c["t0"]), flags=_t(c["flags"]), T0=c["T0"], dt_c=c["dt_c"], K=K)
    tb = ctx.traj_shift_table(kn["knots"], kn["tstatus"].clone(), _t(c["radius"]), group=_t(c["group"]), D=D, stride=stride)
    cf = ctx.traj_conflicts(kn["knots"], kn["tstatus"].clone(), _t(c["radius"]), group=_t(c["group"]), T0=c["T0"], dt_c=c["dt_c"],
                            want_matrix=True)
    ctx.synchronize()
    tb, cf = _np(tb), _np(cf)
    q = np.arange(P)
    unshifted = (tb["table"].view(np.uint64) >> np.uint64(D - 1)) & np.uint64(1)
    matrix = (cf["conflict"].view(np.uint32)[:, q // 32] >> (q % 32).astype(np.uint32)) & np.uint32(1)
    print("bits set: table", int(unshifted.sum()), "matrix", int(matrix.sum()), "of", P * P, "BAD", int((tb["tstatus"] == 2).sum()))
    assert np.array_equal(unshifted, matrix)
    assert np.array_equal(tb["tstatus"], cf["tstatus"])
    assert matrix.any() and not matrix.all()


def test_residual_report_is_empty(ctx):
    """traj_conflicts on knots_out: no conflict among the scheduled paths (every path rests where the shifts end), and the
    unscheduled ones are absent."""
    for cfg in ((8, 1, 300), (32, 2, 400)):
        c, ref = _big(*cfg)
        got = ctx.fleet_schedule(_sm(c), _t(c["radius"]), t0=_t(c["t0"]), flags=_t(c["flags"]), group=_t(c["group"]), T0=c["T0"], dt_c=c["dt_c"],
                                 K=c["K"], D=cfg[0], stride=cfg[1], want_knots=True)
        before = _np(ctx.traj_conflicts(got["knots"], got["tstatus"].clone(), _t(c["radius"]), group=_t(c["group"]), T0=c["T0"], dt_c=c["dt_c"]))
        after = _np(ctx.traj_conflicts(got["knots_out"], got["tstatus"].clone(), _t(c["radius"]), group=_t(c["group"]), T0=c["T0"], dt_c=c["dt_c"]))
        ctx.synchronize()
        assert before["n_conf"].sum() == 280 and (after["n_conf"] == 0).all() and np.isinf(after["first_t"]).all()
        assert sw.at_rest(ref["knots"], cfg[0], cfg[1])[ref["tstatus"] == 0].all()


def test_default_ticks_cover_the_shifts(ctx):
    h = tc.parked(True)
    o = ctx.fleet_schedule(_sm(h), 0.5, t0=_t(h["t0"]), dt_c=0.5, D=6, stride=2)
    assert o["K"] == 36 + 10                                       # the second path ends at 10 + 8 s, then (D-1) * stride ticks
    o = _np(o)
    assert o["slot"].tolist() == [0, -1] and o["counts"].tolist() == [1, 0, 1, 0] and o["delay"][0] == 0.0 and np.isnan(o["delay"][1])
    x = tc.crossing()
    o = _np(ctx.fleet_schedule(_sm(x), 0.5, flags=_t(x["flags"]), dt_c=0.5))
    assert o["K"] == 16 + 7 and o["slot"].tolist() == [0, 3] and o["delay"].tolist() == [0.0, 1.5]


def test_argument_errors(ctx):
    import torch
    import sea_current_amd as sc
    c = tc.head_on()
    sm = _sm(c)
    p = sc._ptr
    L = sc.lib()
    kn = torch.zeros((2, 17, 2), dtype=torch.float64, device="cuda")
    ts = torch.zeros(2, dtype=torch.int32, device="cuda")
    rad = _t(c["radius"])
    tab = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    slot = torch.zeros(2, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")

    def table(P=2, K=16, D=8, stride=1, knp=kn, st=ts, r=rad, t=tab):
        return L.sc_traj_shift_table_batch(ctx._h, p(knp), p(st), P, K, p(r), None, D, stride, p(t))

    def sched(P=2, D=8, t=tab, st=ts, s=slot, n=cnt):
        return L.sc_traj_schedule_batch(ctx._h, p(t), p(st), P, D, None, None, p(s), p(n))

    def shift(P=2, K=16, stride=1, knp=kn, s=slot, out=kn.clone()):
        return L.sc_traj_shift_knots_batch(ctx._h, p(knp), P, K, p(s), stride, p(out))

    def fleet(P=2, K=16, D=8, stride=1, dt_c=0.5, r=rad, s=slot, n=cnt, off=sm["offsets"]):
        return L.sc_fleet_schedule_batch(ctx._h, p(sm["time"]), p(sm["pts"]), p(off), p(sm["length"]), None, P, None, None, 0.0, dt_c, K,
                                         None, None, p(r), None, D, stride, None, None, None, p(s), p(n), None)

    assert table() == 0 and sched() == 0 and shift() == 0 and fleet() == 0
    for kw in (dict(P=0), dict(P=8193), dict(K=0), dict(K=65536), dict(P=8192, K=8192), dict(D=0), dict(D=33), dict(stride=0),
               dict(D=8, stride=3), dict(D=2, stride=17)):
        assert table(**kw) == 1 and fleet(**kw) == 1, kw
    assert table(D=2, stride=16) == 0 and table(D=1, stride=10 ** 9) == 0 and fleet(D=2, stride=16) == 0
    assert table(knp=None) == 1 and table(st=None) == 1 and table(r=None) == 1 and table(t=None) == 1
    for kw in (dict(P=0), dict(P=8193), dict(D=0), dict(D=33), dict(t=None), dict(st=None), dict(s=None), dict(n=None)):
        assert sched(**kw) == 1, kw
    for kw in (dict(P=0), dict(P=8193), dict(K=0), dict(K=65536), dict(stride=0), dict(knp=None), dict(s=None), dict(out=None)):
        assert shift(**kw) == 1, kw
    for kw in (dict(dt_c=0.0), dict(dt_c=float("nan")), dict(r=None), dict(s=None), dict(n=None), dict(off=None)):
        assert fleet(**kw) == 1, kw
    ctx.synchronize()
    with pytest.raises(sc.SeaCurrentError):
        ctx.fleet_schedule(sm, 0.5, dt_c=0.5, K=16, D=40)


def test_host_forms_equal_device_forms(ctx):
    import sea_current_amd as sc
    c = tc.random_fleet()
    c["radius"][[12, 13]] = 0.5                                    # the host forms refuse a t0 or radius outside the contract
    c["t0"][11] = 1.0
    rng = np.random.default_rng(4)
    order, jmax = rng.permutation(tc.FLEET_P).astype(np.int32), rng.integers(-1, 9, tc.FLEET_P).astype(np.int32)
    ref = sw.fleet_schedule(**c, D=8, stride=2, order=order, jmax=jmax)
    _same(_fleet(ctx, c, 8, 2, order=order, jmax=jmax), ref)
    sm = {k: c[k] for k in PATH_KEYS}
    kw = dict(T0=c["T0"], dt_c=c["dt_c"], K=c["K"])
    host = ctx.fleet_schedule_host(sm, c["radius"], t0=c["t0"], flags=c["flags"], group=c["group"], D=8, stride=2, order=order, jmax=jmax,
                                   want_table=True, want_knots=True, **kw)
    _same(host, ref)
    few = ctx.fleet_schedule_host(sm, c["radius"], t0=c["t0"], flags=c["flags"], group=c["group"], D=8, stride=2, order=order, jmax=jmax, **kw)
    assert "table" not in few and "knots_out" not in few
    _same(few, ref, ("slot", "counts", "tstatus", "delay"))
    kn = ctx.traj_knots_host(sm, t0=c["t0"], flags=c["flags"], **kw)
    tb = ctx.traj_shift_table_host(kn["knots"], kn["tstatus"], c["radius"], group=c["group"], D=8, stride=2)
    sd = ctx.traj_schedule_host(tb["table"], tb["tstatus"], D=8, order=order, jmax=jmax)
    out = ctx.traj_shift_knots_host(kn["knots"], sd["slot"], stride=2)
    _same(dict(table=tb["table"], tstatus=tb["tstatus"], slot=sd["slot"], counts=sd["counts"], knots_out=out), ref, INTS + ("knots_out",))
    bad = c["radius"].copy()
    for val in (-0.5, float("nan"), float("inf")):
        bad[20] = val
        with pytest.raises(sc.SeaCurrentError):
            ctx.fleet_schedule_host(sm, bad, t0=c["t0"], flags=c["flags"], group=c["group"], **kw)
        with pytest.raises(sc.SeaCurrentError):
            ctx.traj_shift_table_host(kn["knots"], kn["tstatus"], bad)
    t0 = c["t0"].copy()
    t0[20] = np.inf
    with pytest.raises(sc.SeaCurrentError):
        ctx.fleet_schedule_host(sm, c["radius"], t0=t0, **kw)
    with pytest.raises(sc.SeaCurrentError):
        ctx.traj_shift_table_host(kn["knots"], kn["tstatus"], c["radius"], D=8, stride=50)   # 7 * 50 > K


def test_device_chain_without_host_hop(ctx):
    """astar_batch -> path_waypoints -> cells_to_points -> smooth_paths -> fleet_schedule on one stream, a dozen queries that
    cross on the 64 x 48 map of test_gpu_traj.py: equal to the twin on the smoother's outputs, some paths wait, and the
    residual report is empty."""
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
    Q, D, stride = 12, 16, 5
    K = 80 + (D - 1) * stride
    radius, t0, flags = 0.5 * res, np.linspace(0.0, 1.1, Q), np.zeros(Q, np.int32)
    r = ctx.astar_batch(d2, s, g, r2=1, Lmax=512)
    wr = ctx.path_waypoints(d2, r, r2=1, Wmax=64)
    path, npts = ctx.cells_to_points(wr, 64, x0, x0, res, res)
    sm = ctx.smooth_paths(path, npts, (-1.0, 1.0, -0.5, 0.5), capacity=Q * 2000)
    o = ctx.fleet_schedule(sm, radius, t0=_t(t0), flags=_t(flags), dt_c=0.1, K=K, D=D, stride=stride, want_table=True, want_knots=True)
    left = ctx.traj_conflicts(o["knots_out"], o["tstatus"].clone(), radius, dt_c=0.1)
    ctx.synchronize()
    sm, a, left = _np(sm), _np(o), _np(left)
    assert (sm["status"] == 0).all() and int(sm["needed"][0]) <= Q * 2000
    assert (sm["time"][sm["offsets"][:-1] + sm["length"] - 1] + t0).max() <= 8.0   # tick 80 is past every path: all absent where the shifts end
    ref = sw.fleet_schedule(sm["time"], sm["pts"], sm["offsets"], sm["length"], sm["status"], t0, flags, 0.0, 0.1, K, np.full(Q, radius),
                            D=D, stride=stride)
    _same(a, ref)
    assert (a["slot"] > 0).sum() >= 1 and (a["tstatus"] == 0).all() and (left["n_conf"] == 0).all()
