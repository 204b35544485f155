"""Wall time of line-of-sight sensing (Context.known_from_views, view_gain), in one process.
  maps         1024^2 blocks20 and 1024^2 salt at p = 0.02, each with the three views of frontier_twin.three_discs (radius 292:
               a box of 585^2 cells) and 4096^2 blocks20 with its three views (radius 1170)
  known        known_from_views (with occ_seen) beside known_from_discs of the same rows, and beside the single-threaded C
               statement (tests/cpp/views_ref.c, cc -O2); seen cells, known cells, cells in the discs
  gain         view_gain for 16, 256 and 1024 candidates on free cells, at a radius of 30 and of 290 cells (1024^2 maps)
  equal        every timed output equals the C reference's (the gains at radius 290: the first 16 candidates of each batch)
Wall time per call around a device synchronise after warm-up, median of the repeats.  Prints one JSON line (also written to
--out).  --calls N: only N calls of known_from_views on the first map and no timing -- the run a kernel trace is taken of.
Usage: python tools/views_time.py [--repeats 7] [--maps blocks1024,salt1024,blocks4096] [--out FILE] [--calls N]"""
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

import frontier_twin as ft  # noqa: E402
import sea_current_amd as sc  # noqa: E402
import views_twin as vt  # noqa: E402
from sea_current_amd import synth  # noqa: E402


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


def host_wall(fn, repeats):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--maps", default="blocks1024,salt1024,blocks4096")
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=0)
    a = ap.parse_args()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    cases = {"blocks1024": (1024, lambda: synth.block_grid(1024, 1024, 0.20)), "salt1024": (1024, lambda: synth.salt_grid(1024, 1024, 0.02)),
             "blocks4096": (4096, lambda: synth.block_grid(4096, 4096, 0.20, seed=4))}
    ctx = sc.Context(0)
    if a.calls:
        n, mk = cases[a.maps.split(",")[0]]
        occ = mk()
        views = t(vt.free_centres(occ, ft.three_discs(n, n)))
        tocc = t(occ)
        for _ in range(a.calls):
            ctx.known_from_views(views, tocc, occ_seen=True)
        ctx.synchronize()
        ctx.close()
        return
    ref = vt.Ref(tempfile.mkdtemp())
    res = {}
    for key in a.maps.split(","):
        n, mk = cases[key]
        occ = mk()
        views_h = vt.free_centres(occ, ft.three_discs(n, n))
        tocc, views = t(occ), t(views_h)
        out = {}
        c_ms = host_wall(lambda: out.update(zip(("known", "occ_seen"), ref.known_from_views(None, occ, views_h))), 1 if n > 1024 else 3)
        r = dict(radius=int(np.sqrt(views_h[0, 2])), c_reference_known_ms=c_ms, known_cells=int(out["known"].sum()),
                 seen_cells=int(ref.view_gain(occ, np.zeros_like(occ), views_h).sum()),       # an upper bound: the views overlap
                 disc_cells=int(ft.known_from_discs(None, views_h, n, n).sum()))
        free = np.flatnonzero(occ.ravel() == 0)
        cands = {}
        if n <= 1024:
            for radius in (30, 290):
                for N in (16, 256, 1024):
                    cells = free[np.random.default_rng(N + radius).choice(len(free), N, replace=False)]
                    cand_h = np.stack([cells % n, cells // n, np.full(N, radius * radius)], 1).astype(np.int32)
                    checked = N if radius == 30 else 16                # the C statement of a view of radius 290 takes 0.1 s
                    cands[radius, N] = (cand_h, checked, ref.view_gain(occ, out["known"], cand_h[:checked]))
        known, seen = ctx.known_from_views(views, tocc, occ_seen=True)
        kd = ctx.known_from_discs(views, n, n)
        ctx.synchronize()
        equal = bool(np.array_equal(known.cpu().numpy(), out["known"]) and np.array_equal(seen.cpu().numpy(), out["occ_seen"]))
        r["known_from_views_ms"] = wall(lambda: ctx.known_from_views(views, tocc, out=known, occ_seen=seen), ctx, a.repeats)
        r["known_from_discs_ms"] = wall(lambda: ctx.known_from_discs(views, n, n, out=kd), ctx, a.repeats)
        for (radius, N), (cand_h, checked, want) in cands.items():
            cand = t(cand_h)
            gain = ctx.view_gain(cand, tocc, known)
            r[f"view_gain_r{radius}_N{N}_ms"] = wall(lambda: ctx.view_gain(cand, tocc, known, out=gain), ctx, a.repeats)
            equal &= bool(np.array_equal(gain.cpu().numpy()[:checked], want))
        r["equal_to_c_reference"] = equal
        res[key] = r
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
