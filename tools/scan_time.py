"""Wall time of the range-scan calls (Context.scan_cast, logodds_update), in one process.
  map          1024^2 blocks at 0.20
  beams        square_fan of half-side 64 and 292 from 1, 16 and 256 poses on free cells (8 r beams per pose)
  timed        the cast, the update (with occ_est and known, in place on L), and the two chained
  baselines    the single-threaded C statement (tests/cpp/scan_ref.c, cc -O2) of cast and update; known_from_views of the same
               poses and radius (a neighbour for orientation, not a target: it casts one ray per cell, this casts 8 r); the
               combine pass alone (N = 0), the floor of the update
  mark kernel  update minus combine, with every beam a no-return as well (the longest walks); the cells the beams miss counted
               beam by beam (= the byte stores the kernel issues), from which ns per column of a wave's serial chain
               (mark time / half-side, meaningful while the beams fit the machine in one round) and stores per ns follow
  equal        every timed output equals the C statement's
Wall time per call around a device synchronise after warm-up, median of the repeats.  Prints one JSON line (also written to
--out).  Usage: python tools/scan_time.py [--repeats 7] [--poses 1,16,256] [--radii 64,292] [--out FILE]"""
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

import scan_twin as st  # noqa: E402
import sea_current_amd as sc  # noqa: E402
from sea_current_amd import synth  # noqa: E402

P = dict(l_hit=2, l_miss=1, l_clamp=8, t_occ=2, t_free=1)


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


def host_wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--poses", default="1,16,256")
    ap.add_argument("--radii", default="64,292")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n = 1024
    occ = synth.block_grid(n, n, 0.20)
    tocc = t(occ)
    free = np.flatnonzero(occ.ravel() == 0)
    ref = st.Ref(tempfile.mkdtemp())
    ctx = sc.Context(0)
    res = {}
    L, est, known = (torch.zeros((n, n), dtype=d, device="cuda") for d in (torch.int32, torch.uint8, torch.uint8))
    res["combine_only_ms"] = wall(lambda: ctx.logodds_update(None, None, n, n, L=L, out=L, occ_est=est, known=known, **P), ctx, a.repeats)
    equal_all = True
    for r in (int(v) for v in a.radii.split(",")):
        for poses in (int(v) for v in a.poses.split(",")):
            cells = free[np.random.default_rng(poses + r).choice(len(free), poses, replace=False)]
            rays_h = np.concatenate([st.square_fan(int(c) % n, int(c) // n, r) for c in cells])
            views = t(np.stack([cells % n, cells // n, np.full(poses, r * r)], 1).astype(np.int32))
            N = len(rays_h)
            rays = t(rays_h)
            c_cast_ms, want_hit = host_wall(lambda: ref.cast(occ, rays_h))
            c_update_ms, want = host_wall(lambda: ref.update(None, rays_h, want_hit, n, n, **P))
            none_h = np.where(want_hit == st.IGNORED, want_hit, st.NO_RETURN).astype(np.int32)
            want_none = ref.update(None, rays_h, none_h, n, n, **P)[0]
            hit = ctx.scan_cast(rays, tocc)
            out = ctx.logodds_update(rays, hit, n, n, occ_est=True, known=True, **P)
            none = t(none_h)
            out_none = ctx.logodds_update(rays, none, n, n, **P)
            ctx.synchronize()
            equal = bool(np.array_equal(hit.cpu().numpy(), want_hit) and np.array_equal(out_none.cpu().numpy(), want_none))
            equal &= all(bool(np.array_equal(g.cpu().numpy(), w)) for g, w in zip(out, want))
            equal_all &= equal
            e = dict(beams=N, c_reference_cast_ms=c_cast_ms, c_reference_update_ms=c_update_ms, equal_to_c_reference=equal,
                     hits=int((want_hit >= 0).sum()), miss_stores=ref.miss_steps(rays_h, want_hit, n, n),
                     miss_stores_no_return=ref.miss_steps(rays_h, none_h, n, n))
            L.zero_()
            e["cast_ms"] = wall(lambda: ctx.scan_cast(rays, tocc, out=hit), ctx, a.repeats)
            e["update_ms"] = wall(lambda: ctx.logodds_update(rays, hit, n, n, L=L, out=L, occ_est=est, known=known, **P), ctx, a.repeats)
            e["update_no_return_ms"] = wall(lambda: ctx.logodds_update(rays, none, n, n, L=L, out=L, occ_est=est, known=known, **P), ctx,
                                            a.repeats)

            def chained():
                ctx.scan_cast(rays, tocc, out=hit)
                ctx.logodds_update(rays, hit, n, n, L=L, out=L, occ_est=est, known=known, **P)
            e["cast_update_ms"] = wall(chained, ctx, a.repeats)
            kv, seen = ctx.known_from_views(views, tocc, occ_seen=True)
            e["known_from_views_ms"] = wall(lambda: ctx.known_from_views(views, tocc, out=kv, occ_seen=seen), ctx, a.repeats)
            for key, stores in (("update_ms", "miss_stores"), ("update_no_return_ms", "miss_stores_no_return")):
                mark = e[key] - res["combine_only_ms"]
                tag = key.replace("update", "mark").replace("_ms", "")
                e[tag + "_ms"] = mark
                e[tag + "_ns_per_column"] = mark * 1e6 / r
                e[tag + "_stores_per_ns"] = e[stores] / (mark * 1e6) if mark > 0 else None
            res[f"r{r}_poses{poses}"] = e
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
