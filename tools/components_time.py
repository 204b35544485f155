"""Wall time of the component labelling (Context.components) and of the screened A* (astar_batch(label=)), in one process.
  labelling    1024^2 salt20, salt41, blocks20 (r2 4) and open (2e-5), and 4096^2 salt20: ms per grid for the labels alone
               and for labels + ncomp + largest, the rate against the algorithmic 8 B per cell (read d2, write label), the
               EDT of the same grid from the same run as the yardstick, kernels per call
  unreachable  what an unreachable query costs the unscreened search: 1024 queries between random free cells of 1024^2
               salt35, against the same batch with the queries that have no path removed
  screened     labelling + the screened call against the unscreened call, alternating, on that salt35 batch and on salt41
  reachable    the same on synth.queries of salt20 (both ends in the largest component): screening removes nothing
Wall time per call around a device synchronise after warm-up, median of the repeats.  Prints one JSON line (also written
to --out).
Usage: python tools/components_time.py [--repeats 7] [--out FILE]"""
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
    a = ap.parse_args()
    ctx = sc.Context(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    res = {}

    # ---- labelling
    lab = {}
    for name, n, mk, r2 in (("salt20_1024", 1024, lambda: synth.salt_grid(1024, 1024, 0.20), 0),
                            ("salt41_1024", 1024, lambda: synth.salt_grid(1024, 1024, 0.41), 0),
                            ("blocks20_1024", 1024, lambda: synth.block_grid(1024, 1024, 0.20), 4),
                            ("open_1024", 1024, lambda: synth.salt_grid(1024, 1024, 2e-5, seed=3), 0),
                            ("salt20_4096", 4096, lambda: synth.salt_grid(4096, 4096, 0.20, seed=4), 0)):
        occ = t(mk())
        d2 = ctx.edt(occ)
        o = ctx.components(d2, r2=r2)
        ctx.synchronize()
        labels_only = lambda: ctx._ck(ctx._l.sc_components_batch(ctx._h, d2.data_ptr(), 1, n, n, r2, o["label"].data_ptr(), None, None, None),
                                      "sc_components_batch")
        ms_l = wall(labels_only, ctx, a.repeats)
        ms_all = wall(lambda: ctx.components(d2, r2=r2, out=o), ctx, a.repeats)
        ms_edt = wall(lambda: ctx.edt(occ, out=d2.view(1, n, n)), ctx, a.repeats)
        tiles = ((n + 63) // 64) ** 2
        lab[name] = dict(labels_ms=ms_l, labels_ncomp_largest_ms=ms_all, edt_ms=ms_edt, gb_per_s_of_8B_per_cell=8.0 * n * n / (ms_l * 1e-3) / 1e9,
                         ncomp=int(o["ncomp"][0]), largest_share_of_free=float((o["label"] == o["largest"][0]).sum() / (o["label"] >= 0).sum()),
                         kernels_labels=2 + (tiles > 1), kernels_all=4 + (tiles > 1))
        del occ, d2, o
        torch.cuda.empty_cache()
    res["labelling"] = lab

    # ---- the searches
    def pairs(occ, Q, seed):
        free = np.flatnonzero(occ.ravel() == 0)
        rng = np.random.default_rng(seed)
        return rng.choice(free, Q).astype(np.int32), rng.choice(free, Q).astype(np.int32)

    def compare(occ, s, g):
        d2 = ctx.edt(t(occ))
        ds, dg = t(s), t(g)
        comp = ctx.components(d2)
        reach = ctx.reachable(comp["label"], ds, dg)
        plain = ctx.astar_batch(d2, ds, dg, Lmax=4096)
        ctx.synchronize()
        n_plain = ctx.astar_last_expansions()
        scr = ctx.astar_batch(d2, ds, dg, Lmax=4096, label=comp["label"])
        ctx.synchronize()
        n_scr = ctx.astar_last_expansions()
        same = all(torch.equal(plain[k], scr[k]) for k in ("status", "len", "cost"))
        p_ms, s_ms, so_ms = [], [], []
        for _ in range(a.repeats):   # alternate
            p_ms.append(wall(lambda: ctx.astar_batch(d2, ds, dg, Lmax=4096, out=plain), ctx, 1))
            s_ms.append(wall(lambda: ctx.astar_batch(d2, ds, dg, Lmax=4096, out=scr, label=ctx.components(d2, out=comp)["label"]), ctx, 1))
            so_ms.append(wall(lambda: ctx.astar_batch(d2, ds, dg, Lmax=4096, out=scr, label=comp["label"]), ctx, 1))
        keep = (reach != sc.Q_NO_PATH).cpu().numpy()
        out = dict(no_path_share=float(1 - keep.mean()), unscreened_ms=float(np.median(p_ms)), labelling_plus_screened_ms=float(np.median(s_ms)),
                   screened_alone_ms=float(np.median(so_ms)), unscreened_all=p_ms, labelling_plus_screened_all=s_ms,
                   expansions_unscreened=n_plain, expansions_screened=n_scr, same_status_len_cost=bool(same))
        return out, d2, keep

    occ = synth.salt_grid(1024, 1024, 0.35)
    s, g = pairs(occ, 1024, 1)
    r35, d2, keep = compare(occ, s, g)
    ds, dg = t(s[keep]), t(g[keep])
    o = ctx.astar_batch(d2, ds, dg, Lmax=4096)
    res["unreachable_salt35_1024"] = dict(queries=1024, no_path=int((~keep).sum()), all_queries_ms=r35["unscreened_ms"],
                                          without_the_no_path_queries_ms=wall(lambda: ctx.astar_batch(d2, ds, dg, Lmax=4096, out=o), ctx, a.repeats))
    res["screened_salt35_1024"] = r35
    occ = synth.salt_grid(1024, 1024, 0.41)
    res["screened_salt41_1024"] = compare(occ, *pairs(occ, 1024, 2))[0]
    occ = synth.salt_grid(1024, 1024, 0.20)
    res["reachable_salt20_1024"] = compare(occ, *synth.queries(occ == 0, 1024))[0]

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
