"""Cost of the per-stage speed limits on the bench's smoothing leg: the A* paths of a 1024^2 salt20 map (1024 queries, len >= 64
cells), 16 waypoints each (pipeline.waypoints_from_cells, 0.05 m cells), with the map's own d2 as the clearance grid.
  kernel   sc_speed_limits_batch alone on the legs and tables of those paths: wall per call and event-bracketed kernel time,
           without a grid (curvature only) and with it;
  call     Context.smooth_paths with limits against the plain call on the same inputs, alternating in one process, median
           of the repeats after a warm-up.  "terms_off" passes the grid with every term off: the same samples as the plain
           call, so the difference is the limits kernel and the per-stage TOPP-RA inputs; "curvature" and "clearance" also
           lengthen the profiles, so their sampler and resample write more samples.
Prints one JSON line.  Usage: python tools/speed_limits_time.py [--repeats 7] [--calls 10]"""
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
from sea_current_amd import pipeline, synth  # noqa: E402

KIDS = (sc.K_SMOOTH, sc.K_BEZIER, sc.K_ARCLENGTH, sc.K_TOPPRA, sc.K_TOPPRA_SAMPLE, sc.K_RESAMPLE)
INF = float("inf")


def wall(fn, ctx, calls):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def kernel_ms(fn, ctx, calls):
    ctx.synchronize()
    ctx.reset_timing(); ctx.set_timing(True)
    for _ in range(calls):
        fn()
    per = {k: ctx.get_timing(k)[0] / calls for k in KIDS}
    ctx.set_timing(False)
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    ctx = sc.Context(0)
    W = 1024
    occ = synth.salt_grid(W, W, 0.20)
    d2 = ctx.edt(torch.from_numpy(occ).cuda())
    s, g = synth.queries(d2.cpu().numpy() >= 1, 1024)
    res = ctx.astar_batch(d2, torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda(), Lmax=4096)
    ctx.synchronize()
    ln, st = res["len"].cpu().numpy(), res["status"].cpu().numpy()
    sel = (st == 0) & (ln >= 64)
    wp = torch.from_numpy(pipeline.waypoints_from_cells(res["path"].cpu().numpy()[sel], ln[sel], W, n_wp=16, cell_m=0.05)).cuda()
    P = wp.shape[0]
    npts = torch.full((P,), 16, dtype=torch.int32, device="cuda")
    lim = torch.tensor([[-1.0, 1.0, -0.5, 0.5]], dtype=torch.float64, device="cuda").expand(P, 4).contiguous()
    frame = (0.0, 0.0, 0.05, 0.05)
    variants = {"plain": None, "terms_off": ((INF, INF, INF, 0.0), d2), "curvature": ((1.0, 0.5, INF, 0.0), None),
                "clearance": ((1.0, 0.5, 0.2, 2.0), d2)}
    fns, info = {}, {}
    for name, v in variants.items():
        kw = {} if v is None else dict(dyn=v[0], d2=v[1], frame=frame if v[1] is not None else None)
        o = ctx.smooth_paths(wp, npts, lim, **kw)                 # sizes the capacity
        need = int(o["needed"][0])
        o = ctx.smooth_paths(wp, npts, lim, capacity=need, **kw)
        fns[name] = (lambda need=need, o=o, kw=kw: ctx.smooth_paths(wp, npts, lim, capacity=need, out=o, **kw))
        info[name] = {"samples": need, "ok": int((o["status"] == 0).sum())}
        if v is not None:
            vs = o["vmax_stage"][o["status"] == 0]
            info[name]["vmax_stage_min"] = float(vs.min())
            info[name]["stages_below_vel_max"] = float((vs < 1.0).double().mean())
    for f in fns.values():
        f()
    walls = {k: [] for k in fns}
    for _ in range(a.repeats):
        for k, f in fns.items():
            walls[k].append(wall(f, ctx, a.calls))
    for k, f in fns.items():
        kern = kernel_ms(f, ctx, a.calls)
        info[k].update(ms_wall=float(np.median(walls[k])), ms_kernels=sum(kern.values()), ms_per_kernel_id={str(i): v for i, v in kern.items()})
    # the limits kernel alone, on the legs and tables of the plain call
    o = ctx.smooth_paths(wp, npts, lim, capacity=info["plain"]["samples"])
    S = int(o["seg_off"][-1])
    ctrl = o["ctrl"][:S].contiguous()
    cum, _ = ctx.bezier_arclength(ctrl, 100)
    alone = {}
    for name, (dyn, grid) in (("curvature", variants["curvature"]), ("clearance", variants["clearance"])):
        dyn_t = torch.tensor([list(dyn)], dtype=torch.float64, device="cuda").expand(P, 4).contiguous()
        f = lambda: ctx.speed_limits(ctrl, cum, o["seg_off"], o["arclength"], lim, dyn_t, status=o["status"], d2=grid,
                                     frame=frame if grid is not None else None)
        f()
        w = [wall(f, ctx, a.calls) for _ in range(a.repeats)]
        alone[name] = {"ms_wall": float(np.median(w)), "ms_kernel": kernel_ms(f, ctx, a.calls)[sc.K_SMOOTH]}
    out = {"paths": P, "legs": S, "stages": 101, "J": 4, "curve_samples_per_call": P * 101 * 9, "call": info, "kernel_alone": alone,
           "added_ms_wall_terms_off": info["terms_off"]["ms_wall"] - info["plain"]["ms_wall"]}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
