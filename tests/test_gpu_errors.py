"""Error behaviour of the C ABI on a GPU box: bad arguments come back as status codes (nothing exits, nothing faults),
empty batches are no-ops, and a context survives a rejected call."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_invalid_arguments_are_status_codes():
    import torch
    import sea_current_amd as sc
    ctx = sc.Context(0)
    l, h = ctx._l, ctx._h
    occ = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    d2 = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    INVALID = 1
    assert l.sc_edt_u8_i32(h, None, 8, 8, 1, p(d2)) == INVALID
    assert l.sc_edt_u8_i32(h, p(occ), 0, 8, 1, p(d2)) == INVALID
    assert l.sc_edt_u8_i32(h, p(occ), 8, 1 << 20, 1, p(d2)) == INVALID          # beyond SC_MAX_DIM
    assert l.sc_edt_u8_i32(None, p(occ), 8, 8, 1, p(d2)) == INVALID
    q = torch.zeros(4, dtype=torch.int32, device="cuda")
    path = torch.zeros((4, 16), dtype=torch.int32, device="cuda")
    assert l.sc_astar_batch(h, p(d2), 8, 8, 0, p(q), p(q), 4, 0, p(path), p(q), p(q), p(q)) == INVALID   # Lmax 0
    assert l.sc_astar_batch(h, p(d2), 8, 8, 0, p(q), p(q), -1, 16, p(path), p(q), p(q), p(q)) == INVALID
    assert l.sc_astar_batch(h, p(d2), 8, 8, 0, p(q), p(q), 0, 16, p(path), p(q), p(q), p(q)) == 0          # empty batch: no-op
    assert l.sc_bezier_resample_batch(h, p(d2), p(d2), p(d2), p(q), 1, 1, 100000, p(d2), p(q), 0, None, None, None, None, p(q)) == INVALID
    assert l.sc_fmt_star_batch(h, p(d2), 5000, p(d2), p(d2), 1, C.c_float(1.0), None, 0, 8, p(d2), p(q), p(d2), p(q)) == INVALID
    assert l.sc_occ_from_rects(h, None, None, 3, 8, 8, 1, p(occ)) == INVALID                                  # R > 0 without rects
    assert l.sc_status_string(INVALID)
    # the context still works
    occ[3, 3] = 1
    out = ctx.edt(occ)
    torch.cuda.synchronize()
    assert int(out[3, 3]) == 0 and int(out[0, 0]) == 18
    # per-query statuses: out-of-range / blocked endpoints do not fail the batch
    res = ctx.astar_batch(out, torch.tensor([-5, 27, 0], dtype=torch.int32, device="cuda"), torch.tensor([1, 1, 64], dtype=torch.int32, device="cuda"), Lmax=16)
    torch.cuda.synchronize()
    assert res["status"].tolist() == [2, 2, 2]
    ctx.close()


def test_host_forms_allocate_nothing_in_steady_state():
    """The header promises no allocation in steady state: a fixed sequence of _host calls (one staging buffer serves them all)
    run twice leaves scratch_bytes() where the first pass left it."""
    import sea_current_amd as sc
    from sea_current_amd import synth
    ctx = sc.Context(0)
    occ = synth.salt_grid(192, 128, 0.1, seed=3)
    wp = np.cumsum(np.full((8, 6, 2), 0.7, np.float32), axis=1)
    T = np.ones((50, 2), np.float32)

    def one_pass():
        d2 = ctx.edt_host(occ)
        s, g = synth.queries(d2 >= 1, 24, seed=3)
        res = ctx.astar_batch_host(d2, s, g, Lmax=1024)
        ctx.path_waypoints_host(d2, res["path"], res["len"], res["status"])
        f = ctx.cost_fields_host(d2, s[:3])
        ctx.field_paths_host(d2, f["g"], s[:3], np.zeros(8, np.int32), g[:8])
        out = np.empty((50, 2), np.float32)
        assert ctx._l.sc_bezier_shrink_tangent_batch_host(ctx._h, sc._ptr(T), sc._ptr(T), 50, 0.5, None, 0, sc._ptr(out)) == 0
        ctx.smooth_paths_host(wp, np.full(8, 6, np.int32), (-1.0, 1.0, -0.5, 0.5), 4096)

    one_pass()
    b1 = ctx.scratch_bytes()
    one_pass()
    assert ctx.scratch_bytes() == b1 > 0
    ctx.close()


# -- the argument contract of the cost-field family (single-root, weighted, multi-source; device and _host forms)
_FIELD_ENTRIES = dict(
    cf=("sc_cost_field_batch", "d2 G fgrid W H r2 root F rounds g fstatus"),
    cfw=("sc_cost_field_weighted_batch", "d2 pen pen_cap G fgrid W H r2 root F rounds g fstatus"),
    cfm=("sc_cost_field_multi_batch", "d2 pen pen_cap G fgrid W H r2 seed seed_cost seed_off n_seed F rounds g owner fstatus"),
    fp=("sc_field_paths_batch", "d2 G fgrid W H r2 g root F qfield target Q Lmax to_end path len cost status"),
    fpw=("sc_field_paths_weighted_batch", "d2 pen pen_cap G fgrid W H r2 g root F qfield target Q Lmax to_end path len cost status"),
    fpm=("sc_field_paths_multi_batch",
         "d2 pen pen_cap G fgrid W H r2 g owner seed n_seed F qfield target Q Lmax to_end path len cost status which"),
)
_BUILDS, _READS, _PEN, _MULTI = ("cf", "cfw", "cfm"), ("fp", "fpw", "fpm"), ("cfw", "cfm", "fpw", "fpm"), ("cfm", "fpm")
_DEV, _HOST = ("dev",), ("host",)
_BOTH = _DEV + _HOST


def _field_rows():
    """(entry, forms, overrides of the valid call, expected return code, what to check in the outputs).  A string among the
    overrides names an array of the pool in test_field_family_argument_contract."""
    rows = []

    def row(entries, expect, check=None, forms=_BOTH, **over):
        rows.extend((e, forms, over, expect, check) for e in entries)

    every = _BUILDS + _READS
    # the accepted calls: g of the open 8 x 8 map in closed form, the path to cell 61 read from it
    row(("cf", "cfm"), 0, "g10")
    row(("cfw",), 0, "g13")
    row(("fp", "fpm"), 0, "path90")
    row(("fpw",), 0, "path111")
    # every entry: ctx, d2, G, F, W, H, fgrid
    for bad in (dict(ctx=None), dict(d2=None), dict(G=0), dict(F=0), dict(W=0), dict(H=0), dict(W=8193), dict(H=8193), dict(G=2)):
        row(every, 1, **bad)
    # builds: the pointers each contract requires, the optional ones, the tile bound (checked before scratch or launch)
    row(("cf", "cfw"), 1, root=None)
    row(_BUILDS, 1, g=None)
    row(("cf", "cfm"), 0, "g10", fstatus=None)
    row(("cfw",), 0, "g13", fstatus=None)
    row(("cfm",), 0, "g10", owner=None)
    row(("cfm",), 0, "g10", seed_cost="cost0")
    row(("cf", "cfm"), 1, forms=_DEV, W=8192, H=8192, F=65536)
    row(("cfw",), 1, forms=_DEV, W=8192, H=8192, F=65536, pen_cap=0)
    # weighted: pen, pen_cap, (14 + pen_cap) * (W H - 1) <= INT32_MAX - 1
    row(("cfw", "fpw"), 1, pen=None)
    row(("cfw", "fpw"), 1, pen_cap=-1)
    row(("cfw", "fpw"), 1, pen_cap=256)
    row(("cfw", "fpw"), 1, W=4096, H=4096, pen_cap=255)
    # multi: seed_off, n_seed, seed, pen_cap only with pen, the bound with a seed cost on top
    row(("cfm",), 1, seed_off=None)
    row(_MULTI, 1, n_seed=-1)
    row(_MULTI, 1, seed=None)
    row(("cfm",), 0, "inf", seed=None, n_seed=0, seed_off="off0")
    row(("fpm",), 0, "nopath", seed=None, n_seed=0)
    row(_MULTI, 1, pen="pen0", pen_cap=-1)
    row(_MULTI, 1, pen="pen0", pen_cap=256)
    row(("cfm",), 0, "g10", pen_cap=999)
    row(("fpm",), 0, "path90", pen_cap=999)
    row(("cfm",), 0, "g10", pen="pen0", pen_cap=255)
    row(("fpm",), 0, "path90", pen="pen0", pen_cap=255)
    row(_MULTI, 1, pen="pen0", pen_cap=255, W=4096, H=4096)
    # read-outs: pointers, Q, Lmax
    for name in ("g", "qfield", "target", "path", "len", "cost", "status"):
        row(_READS, 1, **{name: None})
    row(("fp", "fpw"), 1, root=None)
    row(("fpm",), 1, owner=None)
    row(("fpm",), 0, "path90", which=None)
    row(_READS, 1, Lmax=0)
    row(_READS, 1, Q=-1)
    row(_READS, 0, Q=0)
    row(_READS, 1, Q=0, Lmax=0)                 # the checks precede the empty-batch return
    # the data checks of the _host forms
    for bad in ("off_dec", "off_over", "off_neg"):
        row(("cfm",), 1, forms=_HOST, seed_off=bad)
    for bad in ("cost_neg", "cost_big"):
        row(("cfm",), 1, forms=_HOST, seed_cost=bad)
    row(("cfm",), 0, "g10", forms=_HOST, seed_cost="cost_max")
    row(_READS, 1, forms=_HOST, g="gneg")
    row(_READS, 0, forms=_HOST, g="gneg", Q=0)  # ... and the scan of g follows it
    return rows


def test_field_family_argument_contract():
    """Every rule of the argument contract of the twelve cost-field entries, one row each: what is rejected comes back as
    SC_ERR_INVALID before anything is staged or launched (the 4096 x 4096 and 8192 x 8192 rows pass 64-element buffers),
    what is accepted computes the closed-form field of the open 8 x 8 map, and the context survives all of it."""
    import torch
    import sea_current_amd as sc
    ctx = sc.Context(0)
    i = np.arange(8)
    mx, mn = np.maximum(i[:, None], i[None]), np.minimum(i[:, None], i[None])
    g10, g13 = (10 * mx + 4 * mn).astype(np.int32)[None], (13 * mx + 4 * mn).astype(np.int32)[None]
    i32 = lambda *v: np.array(v, np.int32)
    host = dict(
        d2=np.ones((8, 8), np.int32), pen0=np.zeros((8, 8), np.uint8), pen3=np.full((8, 8), 3, np.uint8),
        root=i32(0), seed=i32(0, 0), off=i32(0, 2), off0=i32(0, 0), off_dec=i32(2, 1), off_over=i32(0, 3), off_neg=i32(-1, 2),
        cost0=i32(0, 0), cost_neg=i32(0, -1), cost_big=i32(sc.FIELD_SEED_COST_MAX + 1, 0), cost_max=i32(0, sc.FIELD_SEED_COST_MAX),
        g10=g10, g13=g13, gneg=g10 - 1, own0=np.zeros((1, 8, 8), np.int32), qfield=i32(0), target=i32(61),
        gout=np.zeros((1, 8, 8), np.int32), ownout=np.zeros((1, 8, 8), np.int32), fstatus=i32(0),
        path=np.zeros((1, 16), np.int32), len=i32(0), cost=i32(0), status=i32(0), which=i32(0))
    pools = dict(host=host, dev={k: torch.from_numpy(v).cuda() for k, v in host.items()})
    outs = ("gout", "ownout", "fstatus", "path", "len", "cost", "status", "which")
    base = dict(ctx=ctx._h, d2="d2", pen_cap=255, G=1, fgrid=None, W=8, H=8, r2=0, root="root", F=1, rounds=-1, fstatus="fstatus",
                seed="seed", seed_cost=None, seed_off="off", n_seed=2, owner="ownout", qfield="qfield", target="target", Q=1, Lmax=16,
                to_end=0, path="path", len="len", cost="cost", status="status", which="which")
    per_entry = dict(cf=dict(g="gout"), cfw=dict(g="gout", pen="pen3"), cfm=dict(g="gout", pen=None), fp=dict(g="g10"),
                     fpw=dict(g="g13", pen="pen3"), fpm=dict(g="g10", pen=None, owner="own0"))
    seen = set()
    for entry, forms, over, expect, check in _field_rows():
        sym, names = _FIELD_ENTRIES[entry]
        for form in forms:
            pool = pools[form]
            fn = getattr(ctx._l, sym + ("_host" if form == "host" else ""))
            vals = {**base, **per_entry[entry], **over}
            args = [sc._ptr(pool[v]) if isinstance(v, str) else v for v in (vals[n] for n in ["ctx"] + names.split())]
            for k in outs:
                pool[k][...] = -7
            what = f"{sym} {form} {over}"
            assert fn(*args) == expect, what
            seen.add((entry, form, expect))
            if check is None:
                continue
            o = {k: (pool[k].cpu().numpy() if form == "dev" else pool[k]) for k in outs}
            if check in ("g10", "g13"):
                assert (o["gout"] == host[check]).all(), what
                assert o["fstatus"][0] == (sc.Q_OK if vals["fstatus"] else -7), what
                if entry == "cfm":
                    assert (o["ownout"] == (0 if vals["owner"] else -7)).all(), what
            elif check == "inf":
                assert (o["gout"] == sc.FIELD_INF).all() and (o["ownout"] == -1).all() and o["fstatus"][0] == sc.Q_BAD_ENDPOINT, what
            elif check == "nopath":
                assert (o["status"][0], o["len"][0], o["cost"][0], o["which"][0]) == (sc.Q_NO_PATH, 0, -1, -1), what
            else:
                cost = int(check[4:])
                assert (o["status"][0], o["len"][0], o["cost"][0]) == (sc.Q_OK, 8, cost), what
                assert o["path"][0, 0] == 0 and o["path"][0, 7] == 61, what
                if entry == "fpm":
                    assert o["which"][0] == (0 if vals["which"] else -7), what
    assert seen >= {(e, f, r) for e in _FIELD_ENTRIES for f in _BOTH for r in (0, 1)}
    # the context still works
    res = ctx.cost_fields_host(host["d2"], host["root"])
    assert (res["g"] == g10).all() and res["status"][0] == sc.Q_OK
    ctx.close()
