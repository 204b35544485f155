"""Wall time and kernel time of Context.smooth_paths (sc_smooth_paths_batch) on two workloads, in one process:
  bench   the bench's smoothing leg: the A* paths of a 1024^2 salt20 map (1024 queries, len >= 64 cells), 16 waypoints each
          (pipeline.waypoints_from_cells, 0.05 m cells), beside pipeline.smooth_batch on the same input;
  ragged  the same A* paths through path_waypoints + cells_to_points (line-of-sight waypoints, ragged counts).
Wall time per call around a device synchronise (calls of the two sequences alternate, median of the repeats); kernel
time = the summed event-bracketed times of the kernels the call launches (ctx.get_timing), in separate timed runs.
Prints one JSON line.  Usage: python tools/smooth_time.py [--repeats 15] [--calls 10]"""
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
    ap.add_argument("--repeats", type=int, default=15)
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
    wr = ctx.path_waypoints(d2, {k: v[torch.from_numpy(sel).cuda()].contiguous() for k, v in res.items()}, Wmax=256)
    rp, rn = ctx.cells_to_points(wr, W, 0.0, 0.0, 0.05, 0.05)
    out = {}
    for name, (x, n) in (("bench", (wp, npts)), ("ragged", (rp, rn))):
        o = ctx.smooth_paths(x, n, lim)                         # sizes the capacity
        need = int(o["needed"][0])
        o = ctx.smooth_paths(x, n, lim, capacity=need)
        f_new = lambda: ctx.smooth_paths(x, n, lim, capacity=need, out=o)
        fns = {"smooth_paths": f_new}
        if name == "bench":
            ref = pipeline.smooth_batch(ctx, wp)
            fns["pipeline.smooth_batch"] = lambda: pipeline.smooth_batch(ctx, wp, max_len=ref["max_len"])
        for f in fns.values():
            f()
        walls = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k, f in fns.items():
                walls[k].append(wall(f, ctx, a.calls))
        kern = kernel_ms(f_new, ctx, a.calls)
        ksum = sum(kern.values())
        r = {"paths": P, "samples": need, "ok": int((o["status"] == 0).sum()),
             "waypoints_mean": float(n.float().mean()), "ms_wall": {k: float(np.median(v)) for k, v in walls.items()},
             "ms_kernels": ksum, "ms_per_kernel_id": {str(k): v for k, v in kern.items()}}
        r["wall_over_kernels"] = r["ms_wall"]["smooth_paths"] / ksum
        out[name] = r
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
