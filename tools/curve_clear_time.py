"""Cost and effect of keeping smoothed curves clear of the grid, on the A* paths of a 1024^2 map (1024 queries, found, >= 64
cells) taken through their line-of-sight waypoints (sc_path_waypoints_batch, sc_cells_to_points_batch, 0.05 m cells), with
the map's own d2 and the r2_clear of the search; for the salt20 and the blocks20 map:
  call     Context.smooth_paths with r2_clear (sc_smooth_paths_clear_batch) against the limited call on the same inputs
           (every speed term off), alternating in one process: wall time around a device synchronise, median of the repeats
           after a warm-up;
  alone    sc_curve_clearance_batch and sc_curve_clear_batch on the legs of those paths;
  effect   paths and legs that hit at level 0, the histogram of the final levels, the most rounds, and how many paths end
           SMOOTH_COLLIDES.
Prints one JSON line.  Usage: python tools/curve_clear_time.py [--repeats 7] [--calls 10]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sea-current_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sea_current_amd as sc  # noqa: E402
from sea_current_amd import synth  # noqa: E402

INF = float("inf")
OFF = (INF, INF, INF, 0.0)
W, WMAX, CELL, MAX_LEVEL = 1024, 128, 0.05, 6


def wall(fn, ctx, calls):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def one_map(ctx, name, occ, a):
    d2 = ctx.edt(torch.from_numpy(occ).cuda())
    s, g = synth.queries(d2.cpu().numpy() >= 1, 1024)
    res = ctx.astar_batch(d2, torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda(), Lmax=4096)
    wr = ctx.path_waypoints(d2, res, r2=0, Wmax=WMAX)
    ctx.synchronize()
    sel = (res["status"] == 0) & (res["len"] >= 64) & (wr["status"] == 0)
    wr = {k: v[sel].contiguous() for k, v in wr.items()}
    frame = (0.0, 0.0, CELL, CELL)
    wp, npts = ctx.cells_to_points(wr, W, *frame)
    P = wp.shape[0]
    lim = torch.tensor([[-1.0, 1.0, -0.5, 0.5]], dtype=torch.float64, device="cuda").expand(P, 4).contiguous()
    fns, info = {}, {}
    for key, kw in (("limited", {}), ("clear", dict(r2_clear=0, max_level=MAX_LEVEL))):
        o = ctx.smooth_paths(wp, npts, lim, dyn=OFF, d2=d2, frame=frame, **kw)   # sizes the capacity
        need = int(o["needed"][0])
        o = ctx.smooth_paths(wp, npts, lim, capacity=need, dyn=OFF, d2=d2, frame=frame, **kw)
        fns[key] = (lambda need=need, o=o, kw=kw: ctx.smooth_paths(wp, npts, lim, capacity=need, out=o, dyn=OFF, d2=d2, frame=frame, **kw))
        st = o["status"].cpu().numpy()
        info[key] = {"samples": need, "status_counts": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}}
        if key == "limited":
            S = int(o["seg_off"][-1])
            ctrl, seg_off = o["ctrl"][:S].clone(), o["seg_off"].clone()
            legs_ok = torch.where(o["status"] <= 2, o["status"], torch.zeros_like(o["status"]))
        else:
            lv = o["level"][:S + P].cpu().numpy()
            info[key].update(level_histogram=np.bincount(lv, minlength=MAX_LEVEL + 1).tolist(), rounds_max=int(o["rounds"].max()),
                             collides=int((st == sc.SMOOTH_COLLIDES).sum()))
    for f in fns.values():
        f()
    walls = {k: [] for k in fns}
    for _ in range(a.repeats):
        for k, f in fns.items():
            walls[k].append(wall(f, ctx, a.calls))
    for k in fns:
        info[k]["ms_wall"] = float(np.median(walls[k]))
    chk = ctx.curve_clearance(ctrl, seg_off, d2, frame, 0, status=legs_ok)
    ctx.synchronize()
    lm, hl = chk["leg_min"].cpu().numpy(), chk["hit_legs"].cpu().numpy()
    alone = {}
    for key, f in (("check", lambda: ctx.curve_clearance(ctrl, seg_off, d2, frame, 0, status=legs_ok)),
                   ("repair", lambda: ctx.curve_clear(ctrl, seg_off, d2, frame, 0, MAX_LEVEL, status=legs_ok))):
        f()
        alone[key] = {"ms_wall": float(np.median([wall(f, ctx, a.calls) for _ in range(a.repeats)]))}
    deep = ctx.curve_clear(ctrl, seg_off, d2, frame, 0, sc.CURVE_MAX_LEVEL, status=legs_ok)
    ctx.synchronize()
    alone["repair"]["collides_at_max_level_30"] = int((deep["status"] == sc.SMOOTH_COLLIDES).sum())
    alone["repair"]["rounds_max_at_max_level_30"] = int(deep["rounds"].max())
    return {"map": name, "paths": P, "legs": S, "waypoints_max": int(npts.max()), "paths_hit_level0": int((hl > 0).sum()),
            "legs_hit_level0": int(hl.sum()), "leg_min_d2_lowest": int(lm[lm >= 0].min()) if (lm >= 0).any() else None, "call": info,
            "alone": alone, "clear_over_limited": info["clear"]["ms_wall"] / info["limited"]["ms_wall"],
            "added_ms_wall": info["clear"]["ms_wall"] - info["limited"]["ms_wall"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    ctx = sc.Context(0)
    out = {"grid": W, "cell_m": CELL, "max_level": MAX_LEVEL, "r2_clear": 0,
           "maps": [one_map(ctx, "salt20", synth.salt_grid(W, W, 0.20), a), one_map(ctx, "blocks20", synth.block_grid(W, W, 0.20), a)]}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
