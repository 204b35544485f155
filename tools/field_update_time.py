"""Times the field repair (Context.cost_fields_update) against a fresh cost_fields of the same frame, alternating in one
run: wall time around a synchronise, the median of 7 after warm-up.  Writes profiles/field_update_time.json.

Maps: 1024^2 blocks (256 rectangles, r2 4) and salt20, each changed by synth.move_rects at K = 0 (no change), 1, 4 and 32
(the bench's stream; on salt20 the rectangles are laid over the salt).  Roots F = 1, 16, 256 (the same map for every
field); 4096^2 at K = 4, F = 1.  Per case the stats of field 0.  A sweep of `rounds` (0 .. 64 and the defaults) on ten cases.  The C statement once (1024^2 blocks, K = 4).
Per phase: --phases CSV --label NAME takes the kernel statistics of a profiler run of `--one blocks:32:1` (kernel name,
calls, total time; the run holds 20 repairs and no other field kernel: its old field comes from the CPU twin) and adds
the masks + diff, raise and relax times per repair to the JSON.

    python tools/field_update_time.py [--out profiles/field_update_time.json] [--quick]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sea-current_amd", "python"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

REPS, WARM = 7, 2
ONE_REPS = 20


def frames(kind, N, K):
    """(occ_old, occ_new, r2) of one frame."""
    from sea_current_amd import synth
    if kind == "blocks":
        rects = synth.block_rects(N, N, 0.2, seed=1)[:256] if N == 1024 else synth.block_rects(N, N, 0.2, seed=1)
        base, r2 = None, 4
    else:
        rects = synth.block_rects(N, N, 0.02, seed=2, smin=4, smax=24)
        base, r2 = synth.salt_grid(N, N, 0.2, seed=1), 0
    occ0 = synth.raster_rects(rects, N, N, base=base)
    occ1 = synth.raster_rects(synth.move_rects(rects, 0, N, N, K=K, step=2, seed=1), N, N, base=base) if K else occ0.copy()
    return occ0, occ1, r2


def case(ctx, kind, N, K, F, reps=REPS, rounds=-1):
    import torch
    occ0, occ1, r2 = frames(kind, N, K)
    d0, d1 = ctx.edt(torch.from_numpy(occ0).cuda()), ctx.edt(torch.from_numpy(occ1).cuda())
    ctx.synchronize()
    free = np.flatnonzero((d0.cpu().numpy().ravel() >= max(r2, 1)) & (d1.cpu().numpy().ravel() >= max(r2, 1)))
    roots = torch.from_numpy(free[np.linspace(0, free.size - 1, F).astype(np.int64)].astype(np.int32)).cuda()
    old = ctx.cost_fields(d0, roots, r2=r2)["g"]
    fresh = dict(g=torch.empty_like(old), status=torch.empty(F, dtype=torch.int32, device="cuda"))
    g = torch.empty_like(old)
    ctx.synchronize()
    t_up, t_fr, stats = [], [], None
    for i in range(WARM + reps):
        g.copy_(old)
        torch.cuda.synchronize()
        t = time.perf_counter()
        o = ctx.cost_fields_update(d0, d1, g, roots, r2=r2, rounds=rounds)
        ctx.synchronize()
        a = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        ctx.cost_fields(d1, roots, r2=r2, out=fresh)
        ctx.synchronize()
        b = (time.perf_counter() - t) * 1e3
        if i >= WARM:
            t_up.append(a)
            t_fr.append(b)
        stats = o["stats"][0].cpu().tolist()
    assert bool((g == fresh["g"]).all()), (kind, N, K, F)
    return dict(update_ms=statistics.median(t_up), fresh_ms=statistics.median(t_fr), update_all=t_up, fresh_all=t_fr,
                changed=stats[0], unsupported=stats[1], reachable=int((old[0] < 2**31 - 1).sum()))


def c_statement(tmp):
    from field_twin import Twin
    from field_update_twin import TwinU
    from oracle import oracle
    oracle.build()
    occ0, occ1, r2 = frames("blocks", 1024, 4)
    d0, d1 = oracle.edt(occ0), oracle.edt(occ1)
    root = int(np.flatnonzero((d0.ravel() >= r2) & (d1.ravel() >= r2))[0])
    g0, _ = Twin(tmp).field(d0, root, r2)
    tu = TwinU(tmp)
    t = time.perf_counter()
    _, _, stats = tu.update(d0, d1, g0, root, r2)
    return dict(ms=(time.perf_counter() - t) * 1e3, changed=stats[0], unsupported=stats[1])


def phases(path):
    """Kernel time per repair and phase, in ms, from a profiler's kernel statistics (Name, Calls, TotalDurationNs columns) of
    a --one run (ONE_REPS repairs)."""
    out = {"masks_diff": 0.0, "raise": 0.0, "relax": 0.0, "other": 0.0}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, total = row["Name"], float(row["TotalDurationNs"]) * 1e-6 / ONE_REPS
            if "raise_" in name:
                out["raise"] += total
            elif "field_round" in name or "field_finish" in name:
                out["relax"] += total
            elif "field_mask" in name or "update_" in name:
                out["masks_diff"] += total
            elif "field_" in name:
                out["other"] += total
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_update_time.json"))
    ap.add_argument("--quick", action="store_true", help="F = 1 only, no 4096^2, no C statement")
    ap.add_argument("--one", help="kind:K:F -- 20 repairs of that case and nothing else (for a profiler)")
    ap.add_argument("--phases", help="kernel statistics CSV of a profiled --one run: adds the per-phase times to --out")
    ap.add_argument("--label", default="blocks_1024_K32_F1", help="the case the CSV of --phases belongs to")
    args = ap.parse_args()
    if args.phases:
        res = json.load(open(args.out))
        res.setdefault("phases_kernel_ms_per_repair", {})[args.label] = phases(args.phases)
        json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
        return
    import sea_current_amd as sc
    ctx = sc.Context(0)
    if args.one:
        import torch
        import tempfile
        from field_twin import Twin
        kind, K, F = args.one.split(":")
        occ0, occ1, r2 = frames(kind, 1024, int(K))
        d0, d1 = ctx.edt(torch.from_numpy(occ0).cuda()), ctx.edt(torch.from_numpy(occ1).cuda())
        d0h = d0.cpu().numpy()
        free = np.flatnonzero((d0h.ravel() >= max(r2, 1)) & (d1.cpu().numpy().ravel() >= max(r2, 1)))
        roots_h = free[np.linspace(0, free.size - 1, int(F)).astype(np.int64)].astype(np.int32)
        roots = torch.from_numpy(roots_h).cuda()
        with tempfile.TemporaryDirectory() as tmp:               # the old field from the CPU twin: no field kernel but the repair's runs
            tw = Twin(tmp)
            old = torch.from_numpy(np.stack([tw.field(d0h, int(r), r2)[0] for r in roots_h])).cuda()
        g = torch.empty_like(old)
        for _ in range(ONE_REPS):
            g.copy_(old)
            ctx.cost_fields_update(d0, d1, g, roots, r2=r2)
        ctx.synchronize()
        return
    res = {}
    for kind in ("blocks", "salt20"):
        for K in (0, 1, 4, 32):
            for F in ((1,) if args.quick else (1, 16, 256)):
                res[f"{kind}_1024_K{K}_F{F}"] = case(ctx, kind, 1024, K, F)
                print(f"{kind}_1024_K{K}_F{F}", {k: v for k, v in res[f"{kind}_1024_K{K}_F{F}"].items() if not k.endswith("_all")}, flush=True)
    if not args.quick:
        # one `rounds` for both phases (the call has one argument): the repair's median per value, -1 = the defaults
        sweep = {}
        for kind in ("blocks", "salt20"):
            for K, F in ((0, 1), (1, 1), (1, 16), (32, 1), (32, 16)):
                sweep[f"{kind}_1024_K{K}_F{F}"] = {str(r): case(ctx, kind, 1024, K, F, reps=5, rounds=r)["update_ms"] for r in (0, 4, 8, 16, 32, 64, -1)}
                print("rounds sweep", f"{kind}_1024_K{K}_F{F}", {k: round(v, 2) for k, v in sweep[f"{kind}_1024_K{K}_F{F}"].items()}, flush=True)
        res["rounds_sweep_update_ms"] = sweep
        res["blocks_4096_K4_F1"] = case(ctx, "blocks", 4096, 4, 1)
        print("blocks_4096_K4_F1", res["blocks_4096_K4_F1"], flush=True)
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            res["c_statement_blocks_1024_K4"] = c_statement(tmp)
    ctx.close()
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
