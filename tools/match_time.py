"""Wall time of scan matching (Context.scan_match), in one process.
  map          1024^2 blocks at 0.20; d2 is its EDT, every cell known
  points       the hits of square_fan of half-side 292 (2 336 beams, the beams without a return stay absent) from S poses on
               free cells, turned by R angles (rotate_points, 0 first); the prior is the pose moved by (3, -2)
  timed        S = 1, 16, 256 scans x R = 1, 16, 64 rotations x windows +-8 and +-32, with the volume and without it
  alongside    the single-threaded C statement (tests/cpp/match_ref.c, cc -O2) on one scan of each (R, window); the EDT of the
               same grid (the neighbour in the chain); the cost pass: a call with one point and a window of one candidate on
               the 1024^2 grid (cost pass + two launches of one workgroup) beside the same call on an 8 x 8 grid (the launches
               alone)
  equal        best and the volume of the first and the last scan of every case equal the C statement's (of every scan while
               that takes the C statement less than about 2e9 lookups); the case says how many scans were compared
  derived      lookups = S R (2w+1)^2 N with N all 2 336 slots (an absent point still costs its loop round), and lookups per
               ns of the call
Wall time per call around a device synchronise after warm-up, median of the repeats.  Prints one JSON line (also written to
--out).  Usage: python tools/match_time.py [--repeats 7] [--scans 1,16,256] [--rotations 1,16,64] [--windows 8,32] [--out FILE]"""
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

CAP, UNK, RADIUS = 64, 1, 292


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
    ap.add_argument("--scans", default="1,16,256")
    ap.add_argument("--rotations", default="1,16,64")
    ap.add_argument("--windows", default="8,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n = 1024
    occ = synth.block_grid(n, n, 0.20)
    tocc = t(occ)
    free = np.flatnonzero(occ.ravel() == 0)
    ref = mt.Ref(tempfile.mkdtemp())
    ctx = sc.Context(0)
    d2 = ctx.edt(tocc)
    ctx.synchronize()
    d2_h = d2.cpu().numpy()
    res = dict(map="1024x1024 block_grid 0.20", radius=RADIUS, d2_cap=CAP, unk=UNK)
    res["edt_ms"] = wall(lambda: ctx.edt(tocc, out=d2), ctx, a.repeats)
    one_pt, one_c, one_out = t(np.zeros((1, 1, 1, 2), np.int32)), t(np.array([[4, 4]], np.int32)), torch.zeros((1, 6), dtype=torch.int32, device="cuda")
    small = t(np.ones((8, 8), np.int32))
    res["one_point_1024_ms"] = wall(lambda: ctx.scan_match(one_pt, one_c, d2, wx=0, wy=0, out=one_out), ctx, a.repeats)
    res["one_point_8x8_ms"] = wall(lambda: ctx.scan_match(one_pt, one_c, small, wx=0, wy=0, out=one_out), ctx, a.repeats)
    res["cost_pass_ms"] = res["one_point_1024_ms"] - res["one_point_8x8_ms"]

    S_all = [int(v) for v in a.scans.split(",")]
    cells = free[np.random.default_rng(1).choice(len(free), max(S_all), replace=False)]
    rays = np.stack([st.square_fan(int(c) % n, int(c) // n, RADIUS) for c in cells])              # [S, N, 4]
    N = rays.shape[1]
    hit = ctx.scan_cast(t(rays.reshape(-1, 4)), tocc)
    ctx.synchronize()
    p0 = sc.points_from_hits(rays.reshape(-1, 4), hit.cpu().numpy(), n).reshape(len(cells), N, 2)
    res["points_per_scan"] = dict(slots=N, present_mean=float(mt.present(p0).sum(1).mean()))
    centre_all = np.stack([cells % n + 3, cells // n - 2], 1).astype(np.int32)
    equal_all = True
    c_ms = {}
    for R in (int(v) for v in a.rotations.split(",")):
        pts_all = sc.rotate_points(p0, np.arange(R) * (2 * np.pi / R))                            # [S, R, N, 2]
        for w in (int(v) for v in a.windows.split(",")):
            for S in S_all:
                pts_h, centre_h = np.ascontiguousarray(pts_all[:S]), centre_all[:S]
                pts, centre = t(pts_h), t(centre_h)
                lookups = S * R * (2 * w + 1) ** 2 * N
                per_scan = lookups // S
                checked = list(range(S)) if lookups <= 2e9 else sorted({0, S - 1})
                best, vol = ctx.scan_match(pts, centre, d2, wx=w, wy=w, d2_cap=CAP, unk=UNK, score=True)
                alone = ctx.scan_match(pts, centre, d2, wx=w, wy=w, d2_cap=CAP, unk=UNK)
                ctx.synchronize()
                best_h, vol_h, alone_h = best.cpu().numpy(), vol.cpu().numpy(), alone.cpu().numpy()
                equal = True
                for s in checked:
                    t0 = time.perf_counter()
                    wb, wv = ref.match(d2_h, None, pts_h[s:s + 1], centre_h[s:s + 1], w, w, CAP, UNK)
                    c_ms.setdefault((R, w), (time.perf_counter() - t0) * 1e3)
                    equal &= bool(np.array_equal(best_h[s], wb[0]) and np.array_equal(alone_h[s], wb[0]) and np.array_equal(vol_h[s], wv[0]))
                equal_all &= equal
                e = dict(lookups=lookups, scans_compared=len(checked), equal_to_c_reference=equal, c_reference_ms_per_scan=c_ms[(R, w)],
                         recovered=int((best_h[:, :3] == [0, -3, 2]).all(1).sum()), unique=int((best_h[:, 5] == 1).sum()))
                e["match_ms"] = wall(lambda: ctx.scan_match(pts, centre, d2, wx=w, wy=w, d2_cap=CAP, unk=UNK, out=best), ctx, a.repeats)
                e["match_volume_ms"] = wall(lambda: ctx.scan_match(pts, centre, d2, wx=w, wy=w, d2_cap=CAP, unk=UNK, out=best, score=vol), ctx,
                                            a.repeats)
                e["lookups_per_ns"] = lookups / (e["match_ms"] * 1e6)
                e["c_reference_lookups_per_ns"] = per_scan / (c_ms[(R, w)] * 1e6)
                res[f"S{S}_R{R}_w{w}"] = e
                del pts, vol
    res["equal_to_c_reference"] = equal_all
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
