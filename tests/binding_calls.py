"""What the Python binding hands to the C library, recorded without a library or a GPU.

A Context is made without sc_ctx_create; its library is a stand-in whose every function notes (name, arguments) and returns 0,
and sc._ptr is replaced by a function that describes the array instead of taking its address.  Every _host method is called with
small numpy inputs and its device twin with the same values as torch CPU tensors, each optional branch once.  record() returns
the cases as a list of JSON-ready dicts; `python tests/binding_calls.py --record FILE` writes them.  The recorder uses only the
public method names and sc._ptr, so the same file records any commit: tests/golden/binding_calls.json was taken from the commit
before the binding's device / host pairs became one body each, and tests/test_binding_calls.py compares the tree against it.

While recording, numpy.empty, torch.empty and torch.empty_like return zeros: an uninitialised output would make the digests
(and the `needed` that smooth_paths(capacity=None) reads back) depend on the allocator."""
import ctypes
import hashlib
import json
import math
import sys

import numpy as np


def _digest(raw):
    return hashlib.sha1(raw).hexdigest()[:8]


def _shape(t):
    return "x".join(str(n) for n in t.shape) or "scalar"


def _describe(t):
    """The stand-in for sc._ptr: kind, dtype, shape, contiguity and a digest of the bytes; None stays None."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        c = t.flags["C_CONTIGUOUS"]
        return "np %s %s %s %s" % (t.dtype, _shape(t), "c" if c else "nc", _digest(np.ascontiguousarray(t).tobytes()))
    c = t.is_contiguous()
    return "torch.%s %s %s %s %s" % (t.device.type, str(t.dtype)[6:], _shape(t), "c" if c else "nc",
                                     _digest(t.contiguous().view(-1).numpy().tobytes() if t.numel() else b""))


def _scalar(v):
    if isinstance(v, float) and not math.isfinite(v):
        return "float:" + ("nan" if v != v else "inf" if v > 0 else "-inf")
    return "%s:%r" % (type(v).__name__, v)


def _arg(v):
    if v is None or (isinstance(v, str) and v[:3] in ("np ", "tor")):
        return v                                                      # a pointer, already described
    if isinstance(v, ctypes.c_void_p):
        return "ctx"
    return _scalar(v)


def _result(v, args):
    """A returned value; an array that the last C call took is "@" and its place among that call's arguments."""
    import torch
    if isinstance(v, dict):
        return {k: _result(x, args) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return [_result(x, args) for x in v]
    if isinstance(v, np.ndarray) or torch.is_tensor(v):
        d = _describe(v)
        return "@%d" % args.index(d) if d in args else d
    return None if v is None else _scalar(v)


class _Lib:
    """Every attribute is a C function that notes its call and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append([name] + [_arg(a) for a in args])
            return 0
        return fn


def _t(v):
    """The torch CPU form of a numpy argument (bit words as the signed type torch computes with); dicts by value."""
    import torch
    if isinstance(v, dict):
        return {k: _t(x) for k, x in v.items()}
    if isinstance(v, np.ndarray):
        signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(v.dtype)
        return torch.from_numpy((v.view(signed) if signed else v).copy())
    return v


def record():
    import torch
    import sea_current_amd as sc

    ctx = object.__new__(sc.Context)
    ctx._l, ctx._h = _Lib(), ctypes.c_void_p(1)
    cases = []

    def call(case, method, *a, **kw):
        ctx._l.calls = []
        try:
            res = getattr(ctx, method)(*a, **kw)
            res = _result(res, ctx._l.calls[-1] if ctx._l.calls else [])
        except (ValueError, AssertionError) as e:
            res = "raises %s: %s" % (type(e).__name__, e)
        cases.append(dict(case="%s %s" % (method, case), calls=ctx._l.calls, result=res))

    def both(case, method, *a, dev=None, **kw):
        """method_host with the numpy arguments, method with their torch forms (plus the device-only keywords in dev)."""
        call(case, method + "_host", *a, **kw)
        call(case, method, *[_t(x) for x in a], **{k: _t(x) for k, x in kw.items()}, **(dev or {}))

    i32 = lambda *v: np.array(v, np.int32)
    H = W = 8
    P, Q, K, N = 3, 4, 5, 4
    d2 = ((np.arange(H * W, dtype=np.int32) * 7) % 23).reshape(H, W)
    d2s = np.stack([d2, d2[::-1]])
    known = (d2 % 3 > 0).astype(np.uint8)
    occ = (d2 % 5 == 0).astype(np.uint8)
    pen = (d2 * 3 % 256).astype(np.uint8)
    frame = (-1.0, -2.0, 0.5, 0.25)
    start, goal, qgrid = i32(1, 10, 20, 63), i32(62, 5, 44, 0), i32(0, 1, 1, 0)

    saved = np.empty, torch.empty, torch.empty_like, sc._ptr
    np.empty, torch.empty, torch.empty_like, sc._ptr = np.zeros, torch.zeros, torch.zeros_like, _describe
    try:
        # -- grids
        call("2d", "edt_host", occ)
        call("3d list", "edt_host", np.stack([occ, 1 - occ]).tolist())
        lines = np.arange(24, dtype=np.float32).reshape(6, 4) / 4
        both("plain", "occ_from_polygons", lines, i32(0, 2, 6), W, H, -1.0, -2.0, 0.5, 0.25)
        both("all", "occ_from_polygons", lines, i32(0, 2, 6), W, H, -1.0, -2.0, 0.5, 0.25, closed=np.array([1, 0], np.uint8),
             box=np.arange(8, dtype=np.float32).reshape(2, 4), grid_off=i32(0, 1, 2), base=np.stack([occ, occ]))
        both("no lines", "occ_from_polygons", np.zeros((0, 4), np.float32), i32(0), W, H, 0.0, 0.0, 1.0, 1.0)
        call("out", "occ_from_polygons", _t(lines), _t(i32(0, 2, 6)), W, H, -1.0, -2.0, 0.5, 0.25, out=_t(occ))
        call("coerced", "occ_from_polygons_host", lines.astype(np.float64).ravel(), [0, 2, 6], W, H, -1.0, -2.0, 0.5, 0.25)
        both("plain", "astar_batch", d2, start, goal)
        both("r2 Lmax", "astar_batch", d2, start, goal, r2=2, Lmax=16)
        call("coerced", "astar_batch_host", np.asfortranarray(d2.astype(np.int64)), start.tolist(), goal[::-1][::-1], Lmax=16)
        call("not contiguous", "astar_batch", _t(d2).t(), _t(start), _t(goal), Lmax=16)
        call("label", "astar_batch", _t(d2), _t(start), _t(goal), Lmax=16, label=_t(d2))
        call("out", "astar_batch", _t(d2), _t(start), _t(goal), Lmax=16,
             out={k: _t(np.zeros((Q, 16) if k == "path" else Q, np.int32)) for k in ("path", "len", "cost", "status")})
        both("2d", "components", d2)
        both("3d size", "components", d2s, r2=2, want_size=True)
        both("2d", "reachable", d2, start, goal)
        both("3d", "reachable", d2s, start, goal, qgrid=qgrid)
        both("2d", "clearance_penalty", d2)
        both("3d", "clearance_penalty", d2s, r2=1, r2_soft=25, pen_max=30)

        # -- cost fields
        roots, fgrid = i32(9, 54), i32(1, 0)
        g = np.stack([d2, d2 + 1])
        qfield, targets = i32(0, 1, 1, 0), i32(3, 12, 33, 60)
        both("plain", "cost_fields", d2, roots)
        both("pen", "cost_fields", d2, roots, r2=1, pen=pen, pen_cap=100)
        both("grids", "cost_fields", d2s, roots, fgrid=fgrid, rounds=2)
        both("plain", "field_paths", d2, g, roots, qfield, targets, Lmax=16)
        both("pen to_root", "field_paths", d2s, g, roots, qfield, targets, r2=1, Lmax=16, to_root=True, fgrid=fgrid, pen=np.stack([pen, pen]),
             pen_cap=9)
        seeds, seed_off, seed_cost = i32(9, 10, 54, 55, 56), i32(0, 2, 5), i32(0, 3, 1, 0, 2)
        both("plain", "cost_fields_multi", d2, seeds, seed_off)
        both("all", "cost_fields_multi", d2s, seeds, seed_off, seed_cost=seed_cost, r2=1, fgrid=fgrid, rounds=3, want_owner=False,
             pen=np.stack([pen, pen]), pen_cap=7)
        fields = dict(g=g, owner=g % 5, status=i32(0, 0))
        both("plain", "field_paths_multi", d2, fields, seeds, qfield, targets, Lmax=16)
        both("all", "field_paths_multi", d2s, fields, seeds, qfield, targets, r2=1, Lmax=16, to_seed=True, fgrid=fgrid,
             pen=np.stack([pen, pen]), pen_cap=7)
        path = (np.arange(Q * 16, dtype=np.int32) % 64).reshape(Q, 16)
        lens, qstatus = i32(16, 3, 0, 7), i32(0, 0, 1, 3)
        call("plain", "path_waypoints_host", d2, path, lens)
        call("plain", "path_waypoints", _t(d2), _t(dict(path=path, len=lens)))
        call("status Wmax", "path_waypoints_host", d2, path, lens, qstatus, r2=1, Wmax=6)
        call("status Wmax", "path_waypoints", _t(d2), _t(dict(path=path, len=lens, status=qstatus)), r2=1, Wmax=6)

        # -- smoothing
        n_max, nsub = 3, 4
        S = P * (n_max - 1)
        wp = (np.arange(P * n_max * 2, dtype=np.float32).reshape(P, n_max, 2) % 5) * 0.5
        npts = i32(3, 2, 3)
        ctrl = np.arange(S * 8, dtype=np.float32).reshape(S, 4, 2) / 8
        cum = np.cumsum(np.ones((S, nsub + 1), np.float32), axis=1)
        seg_off, arcl = i32(0, 2, 3, 5), np.array([2.0, 1.0, 3.0], np.float32)
        limits, dyn = (0.0, 1.0, -2.0, 2.0), (1.5, 2.0, 0.1, 0.5)
        limits_a = np.tile(np.array(limits), (P, 1)) + np.arange(P)[:, None]
        dyn_a = np.tile(np.array(dyn), (P, 1)) + np.arange(P)[:, None]
        pstatus = i32(0, 1, 0)
        both("numbers", "speed_limits", ctrl, cum, seg_off, arcl, limits, dyn, N=N)
        both("arrays grid", "speed_limits", ctrl, cum, seg_off, arcl, limits_a, dyn_a, N=N, J=2, status=pstatus, d2=d2, frame=frame)
        both("no frame", "speed_limits", ctrl, cum, seg_off, arcl, limits, dyn, N=N, d2=d2)
        both("plain", "curve_clearance", ctrl, seg_off, d2, frame)
        both("r2 status", "curve_clearance", ctrl, seg_off, d2, frame, r2_clear=2, status=pstatus)
        both("plain", "curve_clear", ctrl, seg_off, d2, frame)
        both("all", "curve_clear", ctrl, seg_off, d2, frame, r2_clear=2, max_level=3, status=pstatus, dev=dict(inplace=True))
        sp = dict(dt=0.1, N=N, nsub=nsub)
        for case, kw in (("plain", {}), ("lines angle", dict(start_angle=0.5, lines=lines)), ("no lines", dict(lines=np.zeros((0, 4), np.float32))),
                         ("dyn", dict(dyn=dyn, J=2)), ("dyn grid", dict(dyn=dyn_a, d2=d2, frame=frame)),
                         ("clear", dict(d2=d2, frame=frame, r2_clear=2, max_level=3)),
                         ("clear dyn", dict(dyn=dyn, d2=d2, frame=frame, r2_clear=0)), ("clear no grid", dict(r2_clear=2)),
                         ("grid no dyn", dict(d2=d2, frame=frame)), ("dyn grid no frame", dict(dyn=dyn, d2=d2))):
            call(case, "smooth_paths_host", wp, npts, limits, 10, **sp, **kw)
            call(case, "smooth_paths", _t(wp), _t(npts), limits, capacity=10, **sp, **{k: _t(v) for k, v in kw.items()})
        call("limits array", "smooth_paths_host", wp.tolist(), npts.tolist(), limits_a, 10, **sp)
        call("limits array", "smooth_paths", _t(wp), _t(npts), _t(limits_a), capacity=10, **sp)
        call("estimate", "smooth_paths", _t(wp), _t(npts), limits, **sp)
        call("estimate clear", "smooth_paths", _t(wp), _t(npts), limits, **sp, d2=_t(d2), frame=frame, r2_clear=1)
        for kw in ({}, dict(dyn=dyn), dict(d2=_t(d2), frame=frame, r2_clear=1)):
            first = ctx.smooth_paths(_t(wp), _t(npts), limits, capacity=10, **sp, **kw)
            call("out reused %s" % sorted(kw), "smooth_paths", _t(wp), _t(npts), limits, capacity=10, out=first, **sp, **kw)
        call("out of another capacity", "smooth_paths", _t(wp), _t(npts), limits, capacity=12, out=first, **sp, **kw)

        # -- timed paths
        sm = dict(time=np.array([0.0, 0.1, 0.2, 0.0, 0.1, 0.0, 0.3]), pts=np.arange(14, dtype=np.float32).reshape(7, 2) / 2,
                  offsets=i32(0, 3, 5, 7), length=i32(3, 2, 2), status=i32(0, 0, 1))
        sm_nostatus = {k: v for k, v in sm.items() if k != "status"}
        sm_empty = dict(sm, length=i32(0, 0, 0))
        t0, flags, radius, group = np.array([0.0, 0.5, 0.25]), i32(3, 1, 2), np.array([0.3, 0.2, 0.1]), i32(0, 0, 1)
        knots = np.arange(P * (K + 1) * 2, dtype=np.float64).reshape(P, K + 1, 2) / 3
        tstatus = i32(0, 1, 0)
        both("plain", "traj_knots", sm)
        both("no status", "traj_knots", sm_nostatus, t0=0.5, flags=1)
        both("no samples", "traj_knots", sm_empty, t0=t0)
        both("all", "traj_knots", sm, t0=t0, flags=flags, T0=-0.1, dt_c=0.05, K=K)
        both("number", "traj_conflicts", knots, tstatus, 0.25)
        both("all", "traj_conflicts", knots, tstatus, radius, group=group, T0=-0.1, dt_c=0.05, sep_cap=2.0, want_matrix=True)
        call("lists", "traj_conflicts_host", knots.tolist(), tstatus.tolist(), radius.tolist(), group=1)
        both("plain", "fleet_conflicts", sm, 0.25)
        both("all", "fleet_conflicts", sm, radius, t0=t0, flags=flags, group=group, T0=-0.1, dt_c=0.05, K=K, sep_cap=2.0, want_matrix=True,
             want_knots=True)
        both("number", "traj_shift_table", knots, tstatus, 0.25)
        both("all", "traj_shift_table", knots, tstatus, radius, group=group, D=4, stride=2)
        table = (np.arange(P * P, dtype=np.uint64).reshape(P, P) * np.uint64(0x0123456789ABCDEF))
        both("plain", "traj_schedule", table, tstatus)
        both("all", "traj_schedule", table, tstatus, D=4, order=i32(2, 0, 1), jmax=i32(3, -1, 2))
        both("order list", "traj_schedule", table, tstatus, order=[2, 0, 1], jmax=2)
        both("short order", "traj_schedule", table, tstatus, order=[2, 0])
        call("signed table", "traj_schedule_host", table.view(np.int64), tstatus)
        slot = i32(0, 2, -1)
        both("plain", "traj_shift_knots", knots, slot)
        both("stride", "traj_shift_knots", knots, slot, stride=2)
        both("plain", "fleet_schedule", sm, 0.25)
        both("all", "fleet_schedule", sm, radius, t0=t0, flags=flags, group=group, T0=-0.1, dt_c=0.05, K=K, D=4, stride=2, order=i32(2, 0, 1),
             jmax=i32(3, -1, 2), want_table=True, want_knots=True)
        both("order list", "fleet_schedule", sm_nostatus, radius, D=4, stride=2, order=[2, 0, 1], jmax=1, want_table=True)
        both("short order", "fleet_schedule", sm, 0.25, order=[0])

        # -- re-planning
        B = 2
        Wq = (W + 31) // 32
        res = (np.arange((K + 1) * H * Wq, dtype=np.uint32) * np.uint32(2654435761)).reshape(K + 1, H, Wq)
        bstart, bgoal, t_start = i32(1, 20), i32(62, 44), i32(0, 2)
        both("plain", "traj_reserve", knots, None, 0.25, W, H, frame, 0.5)
        both("all", "traj_reserve", knots, tstatus, radius, W, H, frame, 1, select=i32(1, 0, 1), res=res)
        both("plain", "tplan", d2, bstart, bgoal, res)
        both("no res", "tplan", d2, bstart, bgoal, L=4, hold=False)
        both("all", "tplan", d2, bstart, bgoal, res, L=K, t_start=t_start, hold=1, r2=1, frame=frame, want_reach=True)
        both("plain", "fleet_replan", knots, None, 0.25, d2, bstart, bgoal, frame, 0.5)
        both("all", "fleet_replan", knots, tstatus, radius, d2, bstart, bgoal, frame, 1, r_new=np.array([0.2, 0.3]), select=i32(1, 0, 1),
             t_start=t_start, hold=False, r2=1, sequential=True, res=res, want_reach=True)
        both("number", "fleet_replan", knots, tstatus, radius, d2, bstart, bgoal, frame, 0.5, r_new=0.2, select=1)

        # -- assignment
        cells, col_cost = i32(3, 12, 60), i32(0, 5)
        cost = (np.arange(2 * 3 * 4, dtype=np.int32) * 5 % 17).reshape(2, 3, 4)
        both("plain", "field_cost_matrix", g, cells)
        both("col_cost", "field_cost_matrix", g, cells, col_cost=col_cost)
        call("out", "field_cost_matrix_host", g, cells, out=np.ones((3, 2), np.int32))
        call("out", "field_cost_matrix", _t(g), _t(cells), out=_t(np.ones((3, 2), np.int32)))
        both("2d", "assign", cost[0])
        both("3d", "assign", cost)
        both("plain", "fleet_assign", g, cells)
        both("all", "fleet_assign", g, cells, col_cost=col_cost, want_cost=True)

        # -- exploration
        discs = i32(2, 2, 9, 5, 6, 4).reshape(2, 3)
        both("plain", "known_from_discs", discs, W, H)
        both("base", "known_from_discs", discs, W, H, base=known)
        call("flat list", "known_from_discs_host", discs.ravel().tolist(), W, H)
        call("out", "known_from_discs", _t(discs), W, H, base=_t(known), out=_t(known))
        both("2d", "d2_known", d2, known)
        both("3d", "d2_known", d2s, np.stack([known, known]))
        call("out", "d2_known", _t(d2), _t(known), out=_t(d2))
        both("plain", "frontiers", d2, known)
        both("lean", "frontiers", d2s, np.stack([known, known]), r2=1, min_size=2, Cmax=4, want_label=False, want_slot=False, want_stats=False)
        call("out", "frontiers", _t(d2), _t(known), Cmax=4, out=ctx.frontiers(_t(d2), _t(known), Cmax=4))
        fr = dict(slot=d2 % 4 - 1, csize=i32(5, 3, 0, 0).reshape(1, 4))
        both("plain", "frontier_cost_matrix", g, fr)
        both("all", "frontier_cost_matrix", g, dict(slot=d2s % 4 - 1, csize=i32(5, 3, 0, 0, 1, 1, 1, 0).reshape(2, 4)), gain=3, size_cap=10, fgrid=fgrid)
        both("plain", "fleet_explore", d2, known, g)
        both("all", "fleet_explore", d2, known, g, r2=1, min_size=2, Cmax=4, gain=3, size_cap=10, want_all=True)
    finally:
        np.empty, torch.empty, torch.empty_like, sc._ptr = saved
    return cases


def dumps(cases):
    """One case per line, so that a diff of two recordings names the cases that differ."""
    return "[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]\n"


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/binding_calls.py --record FILE")
    with open(sys.argv[2], "w") as f:
        f.write(dumps(record()))
