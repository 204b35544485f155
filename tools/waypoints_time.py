"""Time of the waypoint kernel (SC_K_WAYPOINTS) beside the A* call of the same batch, on the issue's workloads:
(a) 1024^2 salt 0.20, r2 = 0 and (b) 1024^2 blocks 0.20, r2 = 4; 1024 queries, Lmax 4096.  Median of 5 launches of
each, and waypoints per path (mean, max) against cells per path.  Prints one JSON line per workload.
    python tools/waypoints_time.py [reps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sea-current_amd", "python"))
import numpy as np
import torch

import sea_current_amd as sc
from sea_current_amd import synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ctx = sc.Context(0)
for name, occ, r2 in (("a_salt20_r2_0", synth.salt_grid(1024, 1024, 0.20), 0), ("b_blocks20_r2_4", synth.block_grid(1024, 1024, 0.20), 4)):
    d2 = ctx.edt(torch.from_numpy(occ).cuda())
    s, g = synth.queries(d2.cpu().numpy() >= max(r2, 1), 1024)
    s, g = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    res = ctx.astar_batch(d2, s, g, r2=r2, Lmax=4096)          # warm-up of both calls
    out = ctx.path_waypoints(d2, res, r2=r2)
    ctx.synchronize()
    t_astar, t_wp = [], []
    ctx.set_timing(True)
    for _ in range(reps):
        ctx.reset_timing()
        ctx.astar_batch(d2, s, g, r2=r2, Lmax=4096, out=res)
        ctx.synchronize()
        t_astar.append(ctx.get_timing(sc.K_ASTAR)[0])
        ctx.reset_timing()
        ctx.path_waypoints(d2, res, r2=r2, out=out)
        ctx.synchronize()
        t_wp.append(ctx.get_timing(sc.K_WAYPOINTS)[0])
    ctx.set_timing(False)
    ok = out["status"].cpu().numpy() == sc.Q_OK
    n = out["n"].cpu().numpy()[ok]
    ln = res["len"].cpu().numpy()[ok]
    print(json.dumps(dict(workload=name, queries=1024, ok=int(ok.sum()), waypoints_ms_median=float(np.median(t_wp)),
                          waypoints_ms=[round(x, 4) for x in t_wp], astar_ms_median=float(np.median(t_astar)),
                          ratio=float(np.median(t_wp) / np.median(t_astar)), wp_per_path_mean=float(n.mean()), wp_per_path_max=int(n.max()),
                          cells_per_path_mean=float(ln.mean()), cells_per_path_max=int(ln.max()))), flush=True)
ctx.close()
