"""Time of sc_occ_from_polygons against the header's host rasteriser on the same worlds: the
14-polygon world at 1024^2 (G = 1 and G = 32) and 4096^2, the 2000-gon and the 200-tooth comb at 1024^2, and 10 000 random
triangles at 4096^2.  Per world: the median of `reps` warm calls of the device wall time around a synchronise, the SC_K_OCC
event time, the EDT of the same grid, the 2 B/cell floor at 5.3 TB/s, and the header's host make_grid() (one thread,
tests/cpp/rasterize_dump.cpp --time).  Prints one JSON line.
    python tools/occ_polygons_time.py [reps]"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sea-current_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import occ_twin as tw
import sea_current_amd as sc

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def triangles(n, W, seed=5):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-4.9, 4.9, (n, 2))
    r = rng.uniform(0.005, 0.03, n)
    obs = []
    for i in range(n):
        a = np.sort(rng.uniform(0, 2 * np.pi, 3))
        obs.append(tw.poly(np.stack([c[i, 0] + r[i] * np.cos(a), c[i, 1] + r[i] * np.sin(a)], 1)))
    return tw.world((5, -5, 5, -5), obs, W=W, H=W)


worlds = dict(poly14_1024=(tw.polygon_world(1024), 1), poly14_1024_G32=(tw.polygon_world(1024), 32),
              poly14_4096=(tw.polygon_world(4096), 1), ngon2000_1024=(tw.ngon_world(2000, 1024), 1),
              comb200_1024=(tw.comb_world(200, 1024), 1), triangles10k_4096=(triangles(10000, 4096), 1))

# host: the header's make_grid() / rasterize, one thread
tmp = tempfile.mkdtemp()
exe = os.path.join(tmp, "rasterize_dump")
subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "rasterize_dump.cpp"), "-L",
                       sc.NATIVE_DIR, "-lsea_current_hip", f"-Wl,-rpath,{sc.NATIVE_DIR}"])
spec = os.path.join(tmp, "worlds.txt")
names = [k for k in worlds if worlds[k][1] == 1]
tw.write_worlds(spec, [worlds[k][0] for k in names], names)
host = {}
for line in subprocess.run([exe, spec, "--time", str(max(3, reps // 4))], capture_output=True, text=True, check=True).stdout.splitlines():
    d = json.loads(line)
    host[d["world"]] = d["host_make_grid_ms_median"]

ctx = sc.Context(0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
res = {}
for name, (w, G) in worlds.items():
    W, H, x0, y0, rx, ry = w["frame"]
    L, off, cl, bx = tw.flatten(w["obstacles"])
    n_obs = len(off) - 1
    if G > 1:   # G copies of the world, one call
        L = np.tile(L, (G, 1))
        off = np.concatenate([[0]] + [off[1:] + g * off[-1] for g in range(G)]).astype(np.int32)
        cl, bx = np.tile(cl, G), np.tile(bx, (G, 1))
    args = dict(W=W, H=H, x_min=float(x0), y_min=float(y0), res_x=float(rx), res_y=float(ry), closed=t(cl), box=t(bx),
                grid_off=t(np.arange(G + 1, dtype=np.int32) * n_obs) if G > 1 else None)
    dl, doff = t(L), t(off)
    occ = ctx.occ_from_polygons(dl, doff, **args)
    d2 = ctx.edt(occ)
    ctx.synchronize()
    ok = bool(np.array_equal((occ[0] if G > 1 else occ).cpu().numpy(), tw.rasterize_world(w)))
    wall, ev, edt_ev = [], [], []
    ctx.set_timing(True)
    for _ in range(reps):
        ctx.reset_timing()
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.occ_from_polygons(dl, doff, out=occ, **args)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(ctx.get_timing(sc.K_OCC)[0])
        ctx.reset_timing()
        ctx.edt(occ, out=d2)
        ctx.synchronize()
        edt_ev.append(ctx.get_timing(sc.K_EDT_COLBITS)[0] + ctx.get_timing(sc.K_EDT_BAND)[0])
    ctx.set_timing(False)
    cells = G * W * H
    r = dict(W=W, H=H, G=G, obstacles=n_obs * G, edges=int(L.shape[0]), equal_twin=ok,
             device_wall_ms_median=round(float(np.median(wall)), 4), occ_event_ms_median=round(float(np.median(ev)), 4),
             edt_event_ms_median=round(float(np.median(edt_ev)), 4), floor_2B_per_cell_ms=round(2 * cells / 5.3e12 * 1e3, 4))
    if G == 1:
        r["host_make_grid_ms_median"] = host[name]
        r["host_over_device_wall"] = round(host[name] / r["device_wall_ms_median"], 1)
    res[name] = r
ctx.close()
print(json.dumps(dict(tool="occ_polygons_time", reps=reps, worlds=res)), flush=True)
