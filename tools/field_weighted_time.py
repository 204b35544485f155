"""Wall time of the clearance-weighted cost fields (Context.cost_fields / field_paths with pen=) against the unweighted
ones on the same maps and roots, in one process.
  fields   per map and F: the weighted field with the helper's penalty (r2_soft 25, pen_max 60) and sc_cost_field_batch
           alternate, median of the repeats; 1024^2 salt20, blocks20 (r2 4) and open (2e-5) for F = 1, 16, 256, and
           4096^2 salt20 for F = 1 (pen_max 60 is within what the overflow contract allows there)
  random   the same for a random full-range costmap on salt20, F = 1 (the general costmap)
  penalty  the penalty kernel alone, 1024^2 and 4096^2
  readout  the weighted and the unweighted read-out of 1024 paths on salt20
Wall time per call around a device synchronise after warm-up.  Prints one JSON line (also written to --out, default
profiles/field_weighted_time.json).
Usage: python tools/field_weighted_time.py [--repeats 7] [--quick] [--out FILE]"""
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
from sea_current_amd import synth  # noqa: E402

R2_SOFT, PEN_MAX = 25, 60


def once(fn, ctx):
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fw, f0, ctx, repeats):
    """Median wall time of two calls that take turns, after one warm-up of each."""
    fw(); f0()
    ctx.synchronize()
    w, u = [], []
    for _ in range(repeats):
        w.append(once(fw, ctx))
        u.append(once(f0, ctx))
    mw, mu = float(np.median(w)), float(np.median(u))
    return dict(weighted_ms=mw, unweighted_ms=mu, ratio=mw / mu, weighted_all=w, unweighted_all=u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="F = 1 at 1024^2 only (profiling runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_weighted_time.json"))
    a = ap.parse_args()
    ctx = sc.Context(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    res = dict(r2_soft=R2_SOFT, pen_max=PEN_MAX, repeats=a.repeats)
    rng = np.random.default_rng(1)
    cases = [("salt20_1024", synth.salt_grid(1024, 1024, 0.20), 0), ("blocks20_1024", synth.block_grid(1024, 1024, 0.20), 4),
             ("open_1024", synth.salt_grid(1024, 1024, 2e-5, seed=3), 0)]
    if not a.quick:
        cases.append(("salt20_4096", synth.salt_grid(4096, 4096, 0.20, seed=4), 0))
    fields, penalty = {}, {}
    for name, occ, r2 in cases:
        d2 = ctx.edt(t(occ))
        pen = ctx.clearance_penalty(d2, r2=r2, r2_soft=R2_SOFT, pen_max=PEN_MAX)
        ctx.synchronize()
        penalty[name] = float(np.median([once(lambda: ctx.clearance_penalty(d2, r2=r2, r2_soft=R2_SOFT, pen_max=PEN_MAX, out=pen), ctx)
                                         for _ in range(a.repeats)]))
        T = np.flatnonzero((d2.cpu().numpy() >= max(r2, 1)).ravel())
        for F in ((1,) if a.quick or name.endswith("4096") else (1, 16, 256)):
            roots = t(rng.choice(T, size=F, replace=False).astype(np.int32))
            ow = ctx.cost_fields(d2, roots, r2=r2, pen=pen, pen_cap=PEN_MAX)
            o0 = ctx.cost_fields(d2, roots, r2=r2)
            ctx.synchronize()
            r = alternate(lambda: ctx.cost_fields(d2, roots, r2=r2, pen=pen, pen_cap=PEN_MAX, out=ow),
                          lambda: ctx.cost_fields(d2, roots, r2=r2, out=o0), ctx, a.repeats)
            r["reachable_equal"] = bool(torch.equal(ow["g"] == sc.FIELD_INF, o0["g"] == sc.FIELD_INF))
            fields[f"{name}_F{F}"] = r
            if name == "salt20_1024" and F == 1:
                rp = t(rng.integers(0, 256, size=occ.shape, dtype=np.uint8))
                res["random_costmap_salt20_1024_F1"] = alternate(lambda: ctx.cost_fields(d2, roots, pen=rp, out=ow),
                                                                 lambda: ctx.cost_fields(d2, roots, out=o0), ctx, a.repeats)
                _, g = synth.queries(occ == 0, 1024)
                goals, qf = t(g), t(np.zeros(1024, np.int32))
                ctx.cost_fields(d2, roots, pen=pen, pen_cap=PEN_MAX, out=ow)
                pw = ctx.field_paths(d2, ow["g"], roots, qf, goals, Lmax=4096, pen=pen, pen_cap=PEN_MAX)
                p0 = ctx.field_paths(d2, o0["g"], roots, qf, goals, Lmax=4096)
                ctx.synchronize()
                r = alternate(lambda: ctx.field_paths(d2, ow["g"], roots, qf, goals, Lmax=4096, pen=pen, pen_cap=PEN_MAX, out=pw),
                              lambda: ctx.field_paths(d2, o0["g"], roots, qf, goals, Lmax=4096, out=p0), ctx, a.repeats)
                r["mean_len_weighted"] = float(pw["len"].float().mean())
                r["mean_len_unweighted"] = float(p0["len"].float().mean())
                res["readout_1024_paths"] = r
            del ow, o0
            torch.cuda.empty_cache()
    res["field"] = fields
    res["penalty_ms"] = penalty
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
