"""Wall time of wide-window scan matching (Context.scan_match_wide) beside the dense call (Context.scan_match), in one process.
  map          1024^2 blocks at 0.20; d2 is its EDT, every cell known
  points       the hits of square_fan of half-side 292 (2 336 beams, the beams without a return stay absent) from S poses on
               free cells, turned by R angles (rotate_points, 0 first)
  (a) dense    window +-64, prior off by (21, -21): scan_match beside scan_match_wide with top 0 .. 3, S = 1, 16, 256 and
               R = 16, 64; max_nodes = min(2^22, 2^26 / S); a case whose top level alone exceeds that is recorded as
               "not_possible"; best of the wide call must equal the dense call's on every scan
  (b) wide     windows +-256, +-1024, +-2048, priors off by a third of the window, S = 1 and 16, R = 16, top 2 .. 5: the time of
               every top and the best one; beside it the dense C statement's time per scan, extrapolated from its lookups per
               ns on a +-8 window of the same scan (marked "extrapolated")
  (c) per case the mean stats row, the share of the dense volume that was bounded or scored, and the number of launches
               (4 + 5 top kernels and 3 memsets)
  --trace-case W,TOP,S,R   run only that case five times and exit: for a kernel trace in a run of its own
Wall time per call around a device synchronise after warm-up, median of the repeats.  Prints one JSON line (also written to
--out).  Usage: python tools/match_wide_time.py [--repeats 7] [--out FILE] [--trace-case 1024,4,1,16]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sea-current_amd", "python"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import match_twin as mt  # noqa: E402
import scan_twin as st  # noqa: E402
import sea_current_amd as sc  # noqa: E402
from sea_current_amd import synth  # noqa: E402

CAP, UNK, RADIUS, N_GRID = 64, 1, 292, 1024


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-case", default=None)
    a = ap.parse_args()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n = N_GRID
    occ = synth.block_grid(n, n, 0.20)
    tocc = t(occ)
    free = np.flatnonzero(occ.ravel() == 0)
    ctx = sc.Context(0)
    d2 = ctx.edt(tocc)
    ctx.synchronize()
    cells = free[np.random.default_rng(1).choice(len(free), 256, replace=False)]
    rays = np.stack([st.square_fan(int(c) % n, int(c) // n, RADIUS) for c in cells])              # [S, N, 4]
    N = rays.shape[1]
    hit = ctx.scan_cast(t(rays.reshape(-1, 4)), tocc)
    ctx.synchronize()
    p0 = sc.points_from_hits(rays.reshape(-1, 4), hit.cpu().numpy(), n).reshape(len(cells), N, 2)
    pts_of = {R: sc.rotate_points(p0, np.arange(R) * (2 * np.pi / R)) for R in (16, 64)}           # [256, R, N, 2]

    def case(w, top, S, R, off, repeats):
        """One wide call: None where the top level alone exceeds max_nodes."""
        max_nodes = min(1 << 22, (1 << 26) // S)
        if R * (2 * w // 4 ** top + 1) ** 2 > max_nodes:
            return None, None
        pts = t(pts_of[R][:S])
        centre = t(np.stack([cells[:S] % n + off[0], cells[:S] // n + off[1]], 1).astype(np.int32))
        best, stats = ctx.scan_match_wide(pts, centre, d2, wx=w, wy=w, d2_cap=CAP, unk=UNK, top=top, max_nodes=max_nodes, stats=True)
        ctx.synchronize()
        ms = wall(lambda: ctx.scan_match_wide(pts, centre, d2, wx=w, wy=w, d2_cap=CAP, unk=UNK, top=top, max_nodes=max_nodes, out=best), ctx,
                  repeats)
        b, s = best.cpu().numpy(), stats.cpu().numpy().astype(np.int64)
        dense = R * (2 * w + 1) ** 2
        e = dict(ms=ms, max_nodes=max_nodes, launches=4 + 5 * top, overflowed=int((b[:, 0] == sc.SCAN_MATCH_OVERFLOW).sum()),
                 recovered=int((b[:, :3] == [0, -off[0], -off[1]]).all(1).sum()), unique=int((b[:, 5] == 1).sum()),
                 stats_mean=s.mean(0).tolist(), work_share_mean=float((s[:, :7].sum(1) / dense).mean()))
        return e, b

    if a.trace_case:
        w, top, S, R = (int(v) for v in a.trace_case.split(","))
        e, _ = case(w, top, S, R, (w // 3, -(w // 3)), 5)
        print(json.dumps(e))
        ctx.close()
        return

    res = dict(map="1024x1024 block_grid 0.20", radius=RADIUS, d2_cap=CAP, unk=UNK, points_per_scan=dict(slots=N, present_mean=float(mt.present(p0).sum(1).mean())))
    # the C statement's rate: the dense search of one scan, 16 rotations, +-8
    ref = mt.Ref(tempfile.mkdtemp())
    d2_h = d2.cpu().numpy()
    c0 = np.array([[int(cells[0]) % n + 3, int(cells[0]) // n - 2]], np.int32)
    t0 = time.perf_counter()
    ref.match(d2_h, None, pts_of[16][:1], c0, 8, 8, CAP, UNK, want_score=False)
    c_rate = 16 * 17 * 17 * N / ((time.perf_counter() - t0) * 1e9)                                   # lookups per ns
    res["c_reference_lookups_per_ns"] = c_rate

    equal_all = True
    off = (21, -21)
    for R in (16, 64):
        for S in (1, 16, 256):
            pts = t(pts_of[R][:S])
            centre = t(np.stack([cells[:S] % n + off[0], cells[:S] // n + off[1]], 1).astype(np.int32))
            dense = ctx.scan_match(pts, centre, d2, wx=64, wy=64, d2_cap=CAP, unk=UNK)
            ctx.synchronize()
            e = dict(dense_ms=wall(lambda: ctx.scan_match(pts, centre, d2, wx=64, wy=64, d2_cap=CAP, unk=UNK, out=dense), ctx, a.repeats))
            dense_h = dense.cpu().numpy()
            for top in range(4):
                c, b = case(64, top, S, R, off, a.repeats)
                if c is None:
                    e[f"top{top}"] = "not_possible"
                    continue
                ok = c["overflowed"] == 0
                c["equal_to_dense"] = bool(np.array_equal(b, dense_h)) if ok else None
                equal_all &= c["equal_to_dense"] is not False
                c["speedup_over_dense"] = e["dense_ms"] / c["ms"]
                e[f"top{top}"] = c
            res[f"a_S{S}_R{R}_w64"] = e
    for w in (256, 1024, 2048):
        for S in (1, 16):
            o = (w // 3, -(w // 3))
            e = {}
            for top in (2, 3, 4, 5):
                c, _ = case(w, top, S, 16, o, a.repeats)
                e[f"top{top}"] = "not_possible" if c is None else c
            good = {k: v["ms"] for k, v in e.items() if v != "not_possible" and v["overflowed"] == 0}
            e["best_top"] = min(good, key=good.get) if good else None
            e["c_dense_ms_per_scan_extrapolated"] = 16 * (2 * w + 1) ** 2 * N / c_rate / 1e6
            res[f"b_S{S}_R16_w{w}"] = e
    res["wide_equal_to_dense"] = equal_all
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
