"""Wall time of the cost fields (Context.cost_fields / field_paths) against A* on the same queries, in one process.
  gate     1024^2 salt20, r2 = 0: one field rooted at the first start of synth.queries plus the read-out of its 1024 goals,
           against sc_astar_batch on the same 1024 (root, goal) queries; the two alternate, median of the repeats
  fields   the field alone for F = 1, 16, 256 per call on salt20, blocks20 (r2 4) and open (2e-5) at 1024^2, and F = 1 on
           salt20 at 4096^2
  rounds   1024^2 salt20, F = 1, for several `rounds` (0 = the finisher alone)
  readout  the read-out of the 1024 paths alone
Wall time per call around a device synchronise after warm-up.  Prints one JSON line (also written to --out).
Usage: python tools/field_time.py [--repeats 7] [--quick] [--out FILE]"""
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


def wall(fn, ctx, repeats, calls=1):
    fn()
    ctx.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) / calls * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the gate and F = 1 only (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sc.Context(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    res = {}
    maps = {}
    for name, occ, r2 in (("salt20", synth.salt_grid(1024, 1024, 0.20), 0), ("blocks20", synth.block_grid(1024, 1024, 0.20), 4),
                          ("open", synth.salt_grid(1024, 1024, 2e-5, seed=3), 0)):
        d2 = ctx.edt(t(occ))
        ctx.synchronize()
        maps[name] = (d2, r2, occ)

    # ---- the gate
    d2, r2, occ = maps["salt20"]
    s, g = synth.queries(occ == 0, 1024)
    root = t(s[:1])
    starts = t(np.full(1024, s[0], np.int32))
    goals = t(g)
    qf = t(np.zeros(1024, np.int32))
    fl = ctx.cost_fields(d2, root, r2=r2)
    out = ctx.field_paths(d2, fl["g"], root, qf, goals, r2=r2, Lmax=4096)
    ref = ctx.astar_batch(d2, starts, goals, r2=r2, Lmax=4096)
    ctx.synchronize()
    same = all(torch.equal(out[k], ref[k]) for k in ("status", "len", "cost"))
    f_ms, a_ms = [], []
    for _ in range(a.repeats):   # alternate the two
        f_ms.append(wall(lambda: (ctx.cost_fields(d2, root, r2=r2, out=fl), ctx.field_paths(d2, fl["g"], root, qf, goals, r2=r2, Lmax=4096, out=out)), ctx, 1))
        a_ms.append(wall(lambda: ctx.astar_batch(d2, starts, goals, r2=r2, Lmax=4096, out=ref), ctx, 1))
    res["gate_1024_salt20"] = dict(field_plus_readout_ms=float(np.median(f_ms)), astar_ms=float(np.median(a_ms)),
                                   field_plus_readout_all=f_ms, astar_all=a_ms, same_status_len_cost=bool(same),
                                   mean_len=float(out["len"].float().mean()))
    res["readout_1024_paths_ms"] = wall(lambda: ctx.field_paths(d2, fl["g"], root, qf, goals, r2=r2, Lmax=4096, out=out), ctx, a.repeats)
    res["rounds_1024_salt20_F1_ms"] = {str(r): wall(lambda: ctx.cost_fields(d2, root, r2=r2, rounds=r, out=fl), ctx, a.repeats)
                                       for r in ((0, 16, 32, 48, 64, -1) if not a.quick else (-1,))}

    # ---- the field alone
    rng = np.random.default_rng(1)
    fields = {}
    for name, (d2, r2, occ) in maps.items():
        T = np.flatnonzero((torch.as_tensor(d2).cpu().numpy() >= max(r2, 1)).ravel())
        for F in ((1,) if a.quick else (1, 16, 256)):
            roots = t(rng.choice(T, size=F, replace=False).astype(np.int32))
            o = ctx.cost_fields(d2, roots, r2=r2)
            fields[f"{name}_1024_F{F}"] = wall(lambda: ctx.cost_fields(d2, roots, r2=r2, out=o), ctx, a.repeats)
            del o
            torch.cuda.empty_cache()
    if not a.quick:
        occ = synth.salt_grid(4096, 4096, 0.20, seed=4)
        d2 = ctx.edt(t(occ))
        ctx.synchronize()
        T = np.flatnonzero(occ.ravel() == 0)
        roots = t(rng.choice(T, size=1).astype(np.int32))
        o = ctx.cost_fields(d2, roots)
        fields["salt20_4096_F1"] = wall(lambda: ctx.cost_fields(d2, roots, out=o), ctx, max(5, a.repeats // 2))
        fields["salt20_4096_F1_rounds0"] = wall(lambda: ctx.cost_fields(d2, roots, rounds=0, out=o), ctx, 5)
    res["field_ms"] = fields
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
