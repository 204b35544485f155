"""Wall time of the delay schedules on the bench's smoothing workload: the A* paths of a 1024^2 salt20 map (1024 queries,
len >= 64 cells), 16 waypoints each (0.05 m cells), smoothed by Context.smooth_paths; radius 0.5 cell, dt_c 0.1 s, slots of
`--stride` ticks, K to the end of the longest path plus (D-1) * stride ticks.  For D = 8 and D = 32:
  table          sc_traj_shift_table_batch on the knots
  table_noskip   the same from a context created with SC_TRAJ_SCHED_NOSKIP=1 (every pair walks its ticks), and whether the two
                 tables are equal
  pairs_dense    sc_traj_conflicts_batch on the same knots in the same run: the same arithmetic at one shift, both (p, q) and
                 (q, p); ginterval_per_s of the two compares evaluated intervals (the table: P (P-1) / 2 * (2D-1) * K, an upper
                 bound, since a wavefront leaves a pair once every shift has conflicted)
  schedule       sc_traj_schedule_batch on that table
  shift_knots    sc_traj_shift_knots_batch
  fleet          sc_fleet_schedule_batch end to end (knots and table in the context's scratch)
  slots          histogram of the slots, counts, and the conflicts sc_traj_conflicts_batch still finds on knots_out (0: every
                 path rests where the shifts end)
  reference      tests/cpp/traj_sched_ref.c (cc -O2 -ffp-contract=off, one thread) on the same knots, D = 8 only, and whether
                 its table and slots equal the GPU's
Wall time per call around a device synchronise after warm-up, median of the repeats.  Prints one JSON line (also written
to --out).
Usage: python tools/traj_schedule_time.py [--repeats 7] [--stride 5] [--no-reference] [--out FILE]"""
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
    return float(np.median(ts))


def reference(kn, ts, radius, D, stride):
    """The C reference on host copies: (seconds of the table, seconds of the schedule, table, slot)."""
    so = os.path.join(tempfile.mkdtemp(prefix="traj_sched_ref"), "libtraj_sched_ref.so")
    subprocess.check_call(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "traj_sched_ref.c"), "-lm"])
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    lib.ts_shift_table.restype = lib.ts_schedule.restype = None
    lib.ts_shift_table.argtypes = [vp, vp, i, i, vp, vp, i, i, i, vp, vp]
    lib.ts_schedule.argtypes = [vp, vp, i, i, vp, vp, vp, vp]
    P, K = kn.shape[0], kn.shape[1] - 1
    p = lambda a: a.ctypes.data
    table, slot, counts, ts = np.zeros((P, P), np.uint64), np.zeros(P, np.int32), np.zeros(4, np.int32), ts.copy()
    t0 = time.perf_counter()
    lib.ts_shift_table(p(kn), p(ts), P, K, p(radius), None, D, stride, 1, p(table), None)
    t1 = time.perf_counter()
    lib.ts_schedule(p(table), p(ts), P, D, None, None, p(slot), p(counts))
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, table, slot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sc.Context(0)
    os.environ["SC_TRAJ_SCHED_NOSKIP"] = "1"
    dense_ctx = sc.Context(0)
    del os.environ["SC_TRAJ_SCHED_NOSKIP"]
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
    T0, dt_c, rad, stride = 0.0, 0.1, 0.5 * 0.05, a.stride
    radius = torch.full((P,), rad, dtype=torch.float64, device="cuda")
    ticks = ctx._traj_ticks(sm, None, T0, dt_c)
    l, p = ctx._l, sc._ptr
    r = {"paths": P, "samples": need, "ticks_of_the_longest_path": ticks, "dt_c": dt_c, "radius": rad, "stride": stride}
    for D in (8, 32):
        K = ticks + (D - 1) * stride
        kn = ctx.traj_knots(sm, T0=T0, dt_c=dt_c, K=K)
        table = torch.empty((P, P), dtype=torch.int64, device="cuda")
        dense = torch.empty((P, P), dtype=torch.int64, device="cuda")
        slot = torch.empty(P, dtype=torch.int32, device="cuda")
        counts = torch.empty(4, dtype=torch.int32, device="cuda")
        moved = torch.empty_like(kn["knots"])
        out = sc._on("cuda").traj_out(P, False)
        outs = [p(out[k]) for k in ("first_t", "first_with", "min_sep", "min_with", "n_conf")]

        def tab(c, t):
            c._ck(l.sc_traj_shift_table_batch(c._h, p(kn["knots"]), p(kn["tstatus"]), P, K, p(radius), None, D, stride, p(t)),
                  "sc_traj_shift_table_batch")

        def pairs(knots):
            ctx._ck(l.sc_traj_conflicts_batch(ctx._h, p(knots), p(kn["tstatus"]), P, K, T0, dt_c, p(radius), None, INF, *outs, None),
                    "sc_traj_conflicts_batch")

        def sched():
            ctx._ck(l.sc_traj_schedule_batch(ctx._h, p(table), p(kn["tstatus"]), P, D, None, None, p(slot), p(counts)), "sc_traj_schedule_batch")

        def shift():
            ctx._ck(l.sc_traj_shift_knots_batch(ctx._h, p(kn["knots"]), P, K, p(slot), stride, p(moved)), "sc_traj_shift_knots_batch")

        def fleet():
            ctx._ck(l.sc_fleet_schedule_batch(ctx._h, p(sm["time"]), p(sm["pts"]), p(sm["offsets"]), p(sm["length"]), p(sm["status"]), P, None,
                                              None, T0, dt_c, K, None, None, p(radius), None, D, stride, None, None, None, p(slot), p(counts),
                                              None), "sc_fleet_schedule_batch")

        e = {"K": K, "intervals": P * (P - 1) // 2 * (2 * D - 1) * K}
        e["table_ms"] = wall(lambda: tab(ctx, table), ctx, a.repeats)
        e["table_noskip_ms"] = wall(lambda: tab(dense_ctx, dense), dense_ctx, a.repeats)
        e["noskip_table_equal"] = bool(torch.equal(table, dense))
        e["pairs_dense_ms"] = wall(lambda: pairs(kn["knots"]), ctx, a.repeats)
        e["table_ginterval_per_s"] = e["intervals"] / (e["table_ms"] * 1e-3) / 1e9
        e["table_noskip_ginterval_per_s"] = e["intervals"] / (e["table_noskip_ms"] * 1e-3) / 1e9
        e["pairs_dense_ginterval_per_s"] = P * (P - 1) * K / (e["pairs_dense_ms"] * 1e-3) / 1e9
        e["schedule_ms"] = wall(sched, ctx, a.repeats)
        e["shift_knots_ms"] = wall(shift, ctx, a.repeats)
        e["fleet_ms"] = wall(fleet, ctx, a.repeats)
        shift()
        before = int(out["n_conf"].sum()) // 2
        pairs(moved)
        ctx.synchronize()
        sl = slot.cpu().numpy()
        tb = table.cpu().numpy().view(np.uint64)
        e["pairs_with_a_bit"] = int((tb != 0).sum()) // 2
        e["pairs_with_all_bits"] = int((tb == np.uint64(2 ** (2 * D - 1) - 1)).sum()) // 2
        e["counts"] = counts.cpu().numpy().tolist()
        e["slot_histogram"] = {str(v): int(n) for v, n in zip(*np.unique(sl, return_counts=True))}
        e["conflicting_pairs_before"] = before
        e["conflicting_pairs_among_scheduled"] = int(out["n_conf"].sum()) // 2
        if D == 8 and not a.no_reference:
            t_tab, t_sch, rt, rs = reference(np.ascontiguousarray(kn["knots"].cpu().numpy()), kn["tstatus"].cpu().numpy(), np.full(P, rad), D, stride)
            e["reference_table_s"], e["reference_schedule_s"] = t_tab, t_sch
            e["reference_equals_gpu"] = bool(np.array_equal(rt, tb) and np.array_equal(rs, sl))
            e["reference_over_gpu_table"] = t_tab * 1e3 / e["table_ms"]
        r["D%d" % D] = e
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    dense_ctx.close()
    ctx.close()


if __name__ == "__main__":
    main()
