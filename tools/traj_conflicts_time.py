"""Wall time of the timed-path conflicts on the bench's smoothing workload: the A* paths of a 1024^2 salt20 map (1024 queries,
len >= 64 cells), 16 waypoints each (0.05 m cells), smoothed by Context.smooth_paths; radius 0.5 cell, dt_c 0.1 s, K to the end
of the longest path.
  knots        sc_traj_knots_batch alone
  pairs_dense  sc_traj_conflicts_batch on those knots, sep_cap = +inf
  pairs_sep_cap_4_radii_skip_not_built
               the same with sep_cap = 4 radii.  The skip of far-apart tiles is NOT built: this is the dense kernel again
               (the cap only filters min_sep), timed so that a later skip has its yardstick from the same run
  fleet        sc_fleet_conflicts_batch (knots in the context's scratch) beside smooth_paths, alternating in one process
  reference    tests/cpp/traj_ref.c (cc -O2 -ffp-contract=off, one thread) on the same data, once, and whether its outputs
               equal the GPU's bit for bit
Wall time per call around a device synchronise after warm-up, median of the repeats.  Prints one JSON line (also written
to --out).
Usage: python tools/traj_conflicts_time.py [--repeats 7] [--no-reference] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sea-current_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sea_current_amd as sc  # noqa: E402
from sea_current_amd import pipeline, synth  # noqa: E402

INF = float("inf")


def wall(fn, ctx, repeats):
    fn()
    ctx.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def reference(sm, radius, T0, dt_c, K):
    """The C reference on host copies: (seconds of tr_knots, seconds of tr_conflicts, outputs)."""
    so = os.path.join(tempfile.mkdtemp(prefix="traj_ref"), "libtraj_ref.so")
    subprocess.check_call(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "traj_ref.c"), "-lm"])
    lib = C.CDLL(so)
    lib.tr_knots.restype = lib.tr_conflicts.restype = None
    lib.tr_knots.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.tr_conflicts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_double] + \
        [C.c_void_p] * 6
    P = sm["length"].shape[0]
    p = lambda a: a.ctypes.data
    kn = np.zeros((P, K + 1, 2))
    o = dict(tstatus=np.zeros(P, np.int32), first_t=np.zeros(P), first_with=np.zeros(P, np.int32), min_sep=np.zeros(P),
             min_with=np.zeros(P, np.int32), n_conf=np.zeros(P, np.int32))
    t0 = time.perf_counter()
    lib.tr_knots(p(sm["time"]), p(sm["pts"]), p(sm["offsets"]), p(sm["length"]), p(sm["status"]), P, None, None, T0, dt_c, K, p(kn), p(o["tstatus"]))
    t1 = time.perf_counter()
    lib.tr_conflicts(p(kn), p(o["tstatus"]), P, K, T0, dt_c, p(radius), None, INF, p(o["first_t"]), p(o["first_with"]), p(o["min_sep"]),
                     p(o["min_with"]), p(o["n_conf"]), None)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=None)
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
    need = int(ctx.smooth_paths(wp, npts, lim)["needed"][0])
    sm = ctx.smooth_paths(wp, npts, lim, capacity=need)
    ctx.synchronize()
    T0, dt_c, rad = 0.0, 0.1, 0.5 * 0.05
    radius = torch.full((P,), rad, dtype=torch.float64, device="cuda")
    K = ctx._traj_ticks(sm, None, T0, dt_c)
    kn = ctx.traj_knots(sm, T0=T0, dt_c=dt_c, K=K)
    l, h, p = ctx._l, ctx._h, sc._ptr
    out = sc._on("cuda").traj_out(P, False)
    outs = [p(out[k]) for k in ("first_t", "first_with", "min_sep", "min_with", "n_conf")]

    def knots():
        ctx._ck(l.sc_traj_knots_batch(h, p(sm["time"]), p(sm["pts"]), p(sm["offsets"]), p(sm["length"]), p(sm["status"]), P, None, None, T0, dt_c, K,
                                      p(kn["knots"]), p(kn["tstatus"])), "sc_traj_knots_batch")

    def pairs(cap):
        ctx._ck(l.sc_traj_conflicts_batch(h, p(kn["knots"]), p(kn["tstatus"]), P, K, T0, dt_c, p(radius), None, cap, *outs, None),
                "sc_traj_conflicts_batch")

    def fleet():
        ctx._ck(l.sc_fleet_conflicts_batch(h, p(sm["time"]), p(sm["pts"]), p(sm["offsets"]), p(sm["length"]), p(sm["status"]), P, None, None, T0,
                                           dt_c, K, None, p(kn["tstatus"]), p(radius), None, INF, *outs, None), "sc_fleet_conflicts_batch")

    smooth = lambda: ctx.smooth_paths(wp, npts, lim, capacity=need, out=sm)
    r = {"paths": P, "samples": need, "K": K, "dt_c": dt_c, "radius": rad, "intervals": P * (P - 1) // 2 * K,
         "intervals_evaluated": P * (P - 1) * K}
    r["knots_ms"], _ = wall(knots, ctx, a.repeats)
    r["pairs_dense_ms"], r["pairs_dense_all"] = wall(lambda: pairs(INF), ctx, a.repeats)
    r["pairs_sep_cap_4_radii_skip_not_built_ms"], _ = wall(lambda: pairs(4 * rad), ctx, a.repeats)
    fl, smo = [], []
    fleet(); smooth(); ctx.synchronize()
    for _ in range(a.repeats):   # alternate
        smo.append(wall(smooth, ctx, 1)[0])
        fl.append(wall(fleet, ctx, 1)[0])
    r["fleet_ms"], r["smooth_paths_ms"], r["fleet_all"], r["smooth_paths_all"] = float(np.median(fl)), float(np.median(smo)), fl, smo
    ctx.reset_timing(); ctx.set_timing(True)
    pairs(INF)
    r["pairs_dense_event_ms"] = ctx.get_timing(sc.K_SMOOTH)[0]
    ctx.set_timing(False)
    r["ginterval_per_s_evaluated"] = r["intervals_evaluated"] / (r["pairs_dense_ms"] * 1e-3) / 1e9
    fleet(); ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    r["paths_in_conflict"] = int((got["n_conf"] > 0).sum())
    r["conflicting_pairs"] = int(got["n_conf"].sum()) // 2
    if not a.no_reference:
        host = {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in sm.items() if k in ("time", "pts", "offsets", "length", "status")}
        t_kn, t_cf, ref = reference(host, np.full(P, rad), T0, dt_c, K)
        r["reference_knots_s"], r["reference_pairs_s"] = t_kn, t_cf
        r["reference_equals_gpu"] = bool(all(ref[k].tobytes() == got[k].tobytes() for k in got))
        r["reference_over_gpu_pairs"] = t_cf * 1e3 / r["pairs_dense_ms"]
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
