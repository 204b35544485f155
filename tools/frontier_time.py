"""Wall time of the exploration frontiers (Context.frontiers, frontier_cost_matrix, fleet_explore), in one process.
  maps         1024^2 salt20 with three sensing discs, the same map with everything known (no frontier: what the passes over
               the cells cost by themselves), and 4096^2 salt20 with three discs
  frontiers    ms per call with every output and with the mandatory ones only (no label, slot, box, sums), frontier cells,
               clusters, kernels per call
  matrix       frontier_cost_matrix for 1, 16 and 256 fields rooted at random known free cells (1024^2 only: 256 fields of
               4096^2 are 16 GiB)
  explore      fleet_explore for 16 robots, Cmax 1024 (frontiers + matrix + matching + goals)
  c_reference  the single-threaded C statement of the same work (tests/cpp/frontier_ref.c, cc -O2): clusters, and the matrix
               for 16 fields
  components   sc_components_batch on the same d2 (labels only), the 4-connected labelling of section 15
Wall time per call around a device synchronise after warm-up, median of the repeats.  Prints one JSON line (also written
to --out).
Usage: python tools/frontier_time.py [--repeats 7] [--maps 1024,known,4096] [--out FILE]"""
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
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--maps", default="1024,known,4096")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sc.Context(0)
    ref = ft.Ref(tempfile.mkdtemp())
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    CMAX = 1024
    res = {}
    cases = {"1024": ("salt20_1024_three_discs", 1024, lambda: synth.salt_grid(1024, 1024, 0.20), True),
             "known": ("salt20_1024_all_known", 1024, lambda: synth.salt_grid(1024, 1024, 0.20), False),
             "4096": ("salt20_4096_three_discs", 4096, lambda: synth.salt_grid(4096, 4096, 0.20, seed=4), True)}
    for key in a.maps.split(","):
        name, n, mk, discs = cases[key]
        occ = mk()
        known_h = ft.known_from_discs(None, ft.three_discs(n, n), n, n) if discs else np.ones((n, n), np.uint8)
        known = t(known_h)
        discs_d = t(ft.three_discs(n, n))
        d2 = ctx.edt(t(np.where(known_h != 0, occ, 0).astype(np.uint8)))      # the obstacles seen so far
        d2k = ctx.d2_known(d2, known)
        full = ctx.frontiers(d2k, known, Cmax=CMAX)
        lean = ctx.frontiers(d2k, known, Cmax=CMAX, want_label=False, want_slot=False, want_stats=False)
        comp_label = torch.empty_like(d2k)
        ctx.synchronize()
        tiles = ((n + 63) // 64) ** 2
        r = dict(frontier_cells=int((full["label"] >= 0).sum()), clusters=int(full["ncl"][0, 1]), listed=int(full["ncl"][0, 0]), Cmax=CMAX,
                 frontiers_ms=wall(lambda: ctx.frontiers(d2k, known, Cmax=CMAX, out=full), ctx, a.repeats),
                 frontiers_mandatory_only_ms=wall(lambda: ctx.frontiers(d2k, known, Cmax=CMAX, out=lean), ctx, a.repeats),
                 kernels_full=7 + (tiles > 1), kernels_mandatory_only=6 + (tiles > 1),
                 known_from_discs_ms=wall(lambda: ctx.known_from_discs(discs_d, n, n, out=known), ctx, a.repeats) if discs else None,
                 d2_known_ms=wall(lambda: ctx.d2_known(d2, known, out=d2k), ctx, a.repeats),
                 components_labels_ms=wall(lambda: ctx._ck(ctx._l.sc_components_batch(ctx._h, d2k.data_ptr(), 1, n, n, 0, comp_label.data_ptr(), None,
                                                                                       None, None), "sc_components_batch"), ctx, a.repeats))
        d2k_h = d2k.cpu().numpy()
        free = np.flatnonzero(d2k_h.ravel() >= 1)
        roots = free[np.random.default_rng(1).choice(len(free), 256 if n == 1024 else 16, replace=False)].astype(np.int32)
        fields = ctx.cost_fields(d2k, t(roots))["g"]
        ctx.synchronize()
        for F in ((1, 16, 256) if n == 1024 else (1, 16)):
            g = fields[:F].contiguous()
            r[f"matrix_{F}_fields_ms"] = wall(lambda: ctx.frontier_cost_matrix(g, full, gain=1, size_cap=64), ctx, a.repeats)
        g16 = fields[:16].contiguous()
        r["fleet_explore_16_robots_ms"] = wall(lambda: ctx.fleet_explore(d2k, known, g16, Cmax=CMAX), ctx, a.repeats)
        ex = ctx.fleet_explore(d2k, known, g16, Cmax=CMAX)
        ctx.synchronize()
        r["robots_with_a_goal"] = int((ex["goal"] >= 0).sum())
        # the C statement of the same work, one thread
        out = {}
        r["c_reference_frontiers_ms"] = host_wall(lambda: out.update(ref.frontiers(d2k_h, known_h, Cmax=CMAX)), max(1, a.repeats // 2))
        g16_h = g16.cpu().numpy()
        r["c_reference_matrix_16_fields_ms"] = host_wall(lambda: ref.cost_matrix(g16_h, out["slot"], out["csize"], CMAX, 1, 64), max(1, a.repeats // 2))
        r["equal_to_c_reference"] = bool(all(np.array_equal(full[k].cpu().numpy(), out[k]) for k in ft.KEYS))
        res[name] = r
        del d2, d2k, known, full, lean, fields, g16, comp_label
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
