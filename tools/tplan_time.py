"""Wall time of the space-time re-planning on the bench's smoothing workload: the A* paths of a 1024^2 salt20 map (1024
queries, len >= 64 cells), 16 waypoints each (0.05 m cells), smoothed by Context.smooth_paths and scheduled by
Context.fleet_schedule with D = 8 slots of `--stride` ticks (radius 0.5 cell, dt_c 0.1 s).  The paths with a slot are the fleet,
the unresolved ones the robots: each from the first to the last cell of its A* path, appearing at tick 0, one cell a tick,
parked at its goal; pad = radius + half the diagonal move.  The clock runs `--extra-ticks` past the schedule's.
  reserve        sc_traj_reserve_batch of the scheduled rows into a zeroed volume (the memset included)
  layers_H       for SC_TPLAN_LAYERS = H in 1, 4, 8, 16 (a context each): sc_tplan_batch of all robots against that volume
                 (batch_ms, per layer and per robot), and sc_fleet_replan_batch with sequential = 1 (the reservation and one
                 search and one reservation per robot; sequential_ms); whether every output equals the H = 1 context's
  outcome        how many robots get a path, and how much later they arrive than with nothing reserved; the conflicts
                 sc_traj_conflicts_batch finds between a re-planned row and a scheduled one (0 by the pad's proof), and for the
                 sequential plan among the re-planned rows as well
  reference      tests/cpp/tplan_ref.c (cc -O2 -ffp-contract=off, one thread): its search of the first `--ref-robots` robots
                 against the GPU's reservation volume (its own reservation pass tests every cell against every interval and is
                 not timed here), per robot, and whether status, arrive and path equal the GPU's
Wall time per call around a device synchronise after warm-up, median of the repeats.  Prints one JSON line (also written to
--out).
Usage: python tools/tplan_time.py [--repeats 7] [--seq-repeats 3] [--stride 5] [--extra-ticks 512] [--ref-robots 2] [--out FILE]"""
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


def reference(d2, res, L, start, goal):
    """The C reference's search on host copies: (seconds, status, arrive, path)."""
    so = os.path.join(tempfile.mkdtemp(prefix="tplan_ref"), "libtplan_ref.so")
    subprocess.check_call(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "cpp", "tplan_ref.c"),
                           "-lm"])
    lib = C.CDLL(so)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    lib.tp_plan.restype = None
    lib.tp_plan.argtypes = [vp, i, i, C.c_int32, vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp, f, f, f, f, vp]
    H, W = d2.shape
    B = len(start)
    p = lambda a: a.ctypes.data
    path, ln, arr, st = np.full((B, L), -1, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    reach = np.zeros((B, L, H, (W + 31) // 32), np.uint32)
    t0 = time.perf_counter()
    lib.tp_plan(p(d2), W, H, 0, p(res), L, p(start), p(goal), None, B, 1, p(path), p(ln), p(arr), p(st), None, 0.0, 0.0, 1.0, 1.0, p(reach))
    return time.perf_counter() - t0, st, arr, path


def context(**env):
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return sc.Context(0)
    finally:
        for k in env:
            del os.environ[k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seq-repeats", type=int, default=3)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--extra-ticks", type=int, default=512)
    ap.add_argument("--ref-robots", type=int, default=2)
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
    cell, dt_c, D, stride = 0.05, 0.1, 8, a.stride
    rad = 0.5 * cell
    frame = (-0.5 * cell, -0.5 * cell, cell, cell)          # the waypoints put cell (x, y) at (x, y) * cell
    c32 = float(np.float32(cell))
    pad = rad + np.sqrt(2 * c32 * c32) / 2 * (1 + 2.0 ** -20)
    K = ctx._traj_ticks(sm, None, 0.0, dt_c) + (D - 1) * stride + a.extra_ticks
    L = K + 1
    o = ctx.fleet_schedule(sm, rad, dt_c=dt_c, K=K, D=D, stride=stride, want_knots=True)
    ctx.synchronize()
    slot = o["slot"].cpu().numpy()
    robots = slot == sc.SLOT_UNRESOLVED
    B = int(robots.sum())
    start = torch.from_numpy(np.ascontiguousarray(s[sel][robots])).cuda()
    goal = torch.from_numpy(np.ascontiguousarray(g[sel][robots])).cuda()
    select = (o["slot"] >= 0).to(torch.int32)
    radius = torch.full((P,), rad, dtype=torch.float64, device="cuda")
    r = {"paths": P, "scheduled": int((slot >= 0).sum()), "robots": B, "K": K, "dt_c": dt_c, "radius": rad, "pad": pad, "stride": stride,
         "cell_path_len_of_the_robots_max": int(ln[sel][robots].max())}
    vol = torch.zeros((L, W, W // 32), dtype=torch.int32, device="cuda")

    def reserve():
        vol.zero_()
        ctx.traj_reserve(o["knots_out"], o["tstatus"], radius, W, W, frame, pad, select=select, res=vol)

    r["reserve_ms"] = wall(reserve, ctx, a.repeats)
    r["reserved_cell_layers"] = int(sum(int(np.unpackbits(v.cpu().numpy().view(np.uint8)).sum()) for v in vol.split(64)))
    free = ctx.tplan(d2, start, goal, L=L, hold=True)
    ctx.synchronize()
    free_arr = free["arrive"].cpu().numpy()
    base = None
    for h in (1, 4, 8, 16):
        cx = context(SC_TPLAN_LAYERS=h)
        e = {}
        out = {}

        def batch():
            out["b"] = cx.tplan(d2, start, goal, res=vol, hold=True, frame=frame)

        def seq():
            out["s"] = cx.fleet_replan(o["knots_out"], o["tstatus"], radius, d2, start, goal, frame, pad, r_new=rad, select=select, hold=True,
                                       sequential=True)

        e["batch_ms"] = wall(batch, cx, a.repeats)
        e["batch_us_per_layer"] = e["batch_ms"] * 1e3 / K
        e["batch_ms_per_robot"] = e["batch_ms"] / B
        e["sequential_ms"] = wall(seq, cx, a.seq_repeats)
        e["sequential_ms_per_robot"] = e["sequential_ms"] / B
        got = {m: {k: out[m][k].cpu().numpy() for k in ("status", "arrive", "len", "path", "knots_out")} for m in ("b", "s")}
        if base is None:
            base = got
        e["equals_layers_1"] = bool(all(np.array_equal(got[m][k], base[m][k], equal_nan=(k == "knots_out")) for m in got for k in got[m]))
        r["layers_%d" % h] = e
        last = out
        cx.close()
    oc = {}
    for m, name in (("b", "batch"), ("s", "sequential")):
        stt, arr = base[m]["status"], base[m]["arrive"]
        ok = stt == sc.TP_OK
        late = (arr - free_arr)[ok & (free_arr >= 0)]
        rows = torch.cat([o["knots_out"], last[m]["knots_out"]])
        group = None if m == "s" else torch.cat([torch.full((P,), -1, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)]).cuda()
        rep = ctx.traj_conflicts(rows, torch.zeros(P + B, dtype=torch.int32, device="cuda"), torch.full((P + B,), rad, dtype=torch.float64, device="cuda"),
                                 group=group, dt_c=dt_c)
        ctx.synchronize()
        oc[name] = {"ok": int(ok.sum()), "no_path": int((stt == sc.TP_NO_PATH).sum()), "start_blocked": int((stt == sc.TP_START_BLOCKED).sum()),
                    "free_space_no_path": int((free_arr < 0).sum()), "later_than_free": int((late > 0).sum()),
                    "ticks_later_median": float(np.median(late)) if len(late) else None, "ticks_later_mean": float(late.mean()) if len(late) else None,
                    "ticks_later_max": int(late.max()) if len(late) else None,
                    "conflicts_of_replanned_rows": int(rep["n_conf"][P:].sum())}
    r["outcome"] = oc
    n = min(a.ref_robots, B)
    if n > 0:
        t_ref, rs, ra, rp = reference(np.ascontiguousarray(d2.cpu().numpy()), np.ascontiguousarray(vol.cpu().numpy()).view(np.uint32), L,
                                      np.ascontiguousarray(start.cpu().numpy()[:n]), np.ascontiguousarray(goal.cpu().numpy()[:n]))
        b = base["b"]
        same = np.array_equal(rs, b["status"][:n]) and np.array_equal(ra, b["arrive"][:n]) and all(
            np.array_equal(rp[i, :b["len"][i]], b["path"][i, :b["len"][i]]) for i in range(n))
        r["reference"] = {"robots": n, "search_s_per_robot": t_ref / n, "equals_gpu": bool(same),
                          "over_gpu_batch_per_robot": t_ref / n * 1e3 / r["layers_8"]["batch_ms_per_robot"]}
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
