"""Wall time of the multi-source cost fields (Context.cost_fields_multi / field_paths_multi), in one process.
  generalisation  1024^2 salt20: the multi entry with one seed and no owner against sc_cost_field_batch on the same root;
                  the two alternate, median and spread (max - min) of the repeats
  gate            tools/field_time.py's gate (one single-root field plus the read-out of 1024 goals), for comparing this
                  commit with its parent
  buys            1024^2 salt20, K = 16 and 256 seeds, 1024 targets: multi field + owner + read-out against K single-root
                  fields in one sc_cost_field_batch call + a torch gather and argmin of the K x Q costs + the read-out;
                  the two alternate; the bytes of g (and owner) each route holds
  owner           the field with and without the owner pass, alternating, at 1024^2 salt20 (K = 16), on the 256^2
                  serpentine (one seed at the corridor's end) and at 4096^2 salt20 (K = 16): the difference is the pass
Wall time per call around a device synchronise after warm-up.  Prints one JSON line (also written to --out).
Usage: python tools/field_multi_time.py [--repeats 7] [--out FILE]"""
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


def once(fn, ctx):
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, ctx, repeats):
    """fns: dict name -> callable.  Warm every one up, then time them in turn `repeats` times."""
    for fn in fns.values():
        fn()
    ctx.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ts[k].append(once(fn, ctx))
    out = {}
    for k, v in ts.items():
        out[k + "_ms"] = float(np.median(v))
        out[k + "_spread_ms"] = float(max(v) - min(v))
        out[k + "_all"] = v
    return out


def serpentine(n, wall=2, gap=2):
    occ = np.zeros((n, n), np.uint8)
    k = 0
    for y in range(gap, n - 1, wall + gap):
        occ[y:y + wall, :] = 1
        if k % 2 == 0:
            occ[y:y + wall, n - gap:] = 0
        else:
            occ[y:y + wall, :gap] = 0
        k += 1
    return occ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sc.Context(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    res = {}
    occ = synth.salt_grid(1024, 1024, 0.20)
    d2 = ctx.edt(t(occ))
    ctx.synchronize()
    s, g = synth.queries(occ == 0, 1024)
    root, goals, qf = t(s[:1]), t(g), t(np.zeros(1024, np.int32))
    off1 = t(np.array([0, 1], np.int32))

    # ---- cost of the generalisation
    single = ctx.cost_fields(d2, root)
    multi = ctx.cost_fields_multi(d2, root, off1, want_owner=False)
    ctx.synchronize()
    r = alternate({"single_root": lambda: ctx.cost_fields(d2, root, out=single),
                   "multi_one_seed_no_owner": lambda: ctx.cost_fields_multi(d2, root, off1, want_owner=False, out=multi)}, ctx, a.repeats)
    r["same_g"] = bool(torch.equal(single["g"], multi["g"]))
    res["generalisation_1024_salt20"] = r

    # ---- the gate of tools/field_time.py
    out = ctx.field_paths(d2, single["g"], root, qf, goals, Lmax=4096)
    res["gate_1024_salt20"] = alternate({"field_plus_readout": lambda: (ctx.cost_fields(d2, root, out=single),
                                                                         ctx.field_paths(d2, single["g"], root, qf, goals, Lmax=4096, out=out))},
                                        ctx, a.repeats)

    # ---- what the feature buys
    rng = np.random.default_rng(1)
    T = np.flatnonzero(occ.ravel() == 0)
    buys = {}
    for K in (16, 256):
        seeds = t(rng.choice(T, size=K, replace=False).astype(np.int32))
        offK = t(np.array([0, K], np.int32))
        fm = ctx.cost_fields_multi(d2, seeds, offK)
        pm = ctx.field_paths_multi(d2, fm, seeds, qf, goals, Lmax=4096)
        fs = ctx.cost_fields(d2, seeds)
        ps = ctx.field_paths(d2, fs["g"], seeds, qf, goals, Lmax=4096)
        gl = goals.long()

        def route_multi():
            ctx.cost_fields_multi(d2, seeds, offK, out=fm)
            ctx.field_paths_multi(d2, fm, seeds, qf, goals, Lmax=4096, out=pm)

        def route_single():
            ctx.cost_fields(d2, seeds, out=fs)
            best = fs["g"].view(K, -1)[:, gl].argmin(dim=0).to(torch.int32)       # gather K x Q costs, argmin
            ctx.field_paths(d2, fs["g"], seeds, best, goals, Lmax=4096, out=ps)
            return best

        r = alternate({"multi_field_owner_readout": route_multi, "k_single_fields_argmin_readout": route_single}, ctx, a.repeats)
        best = route_single()
        ctx.synchronize()
        ok = pm["status"] == 0
        r["same_cost"] = bool(torch.equal(pm["cost"][ok], ps["cost"][ok]))
        r["paths_found"] = int(ok.sum())
        r["multi_g_plus_owner_bytes"] = int(fm["g"].numel() * 4 + fm["owner"].numel() * 4)
        r["k_single_g_bytes"] = int(fs["g"].numel() * 4)
        buys[f"K{K}"] = r
        del fm, pm, fs, ps, best
        torch.cuda.empty_cache()
    res["buys_1024_salt20_Q1024"] = buys

    # ---- the owner pass alone
    owner = {}

    def owner_case(name, d2x, seeds, repeats):
        off = t(np.array([0, seeds.shape[0]], np.int32))
        with_o = ctx.cost_fields_multi(d2x, seeds, off)
        without = ctx.cost_fields_multi(d2x, seeds, off, want_owner=False)
        r = alternate({"field_with_owner": lambda: ctx.cost_fields_multi(d2x, seeds, off, out=with_o),
                       "field_without_owner": lambda: ctx.cost_fields_multi(d2x, seeds, off, want_owner=False, out=without)}, ctx, repeats)
        r["owner_pass_ms"] = r["field_with_owner_ms"] - r["field_without_owner_ms"]
        H, W = d2x.shape
        r["jump_launches"] = int(np.ceil(np.log2(W * H)))
        owner[name] = r

    owner_case("salt20_1024_K16", d2, t(rng.choice(T, size=16, replace=False).astype(np.int32)), a.repeats)
    sp = t(np.where(serpentine(256) != 0, 0, 1).astype(np.int32))
    owner_case("serpentine_256_K1", sp, t(np.array([0], np.int32)), a.repeats)
    occ4 = synth.salt_grid(4096, 4096, 0.20, seed=4)
    d24 = ctx.edt(t(occ4))
    ctx.synchronize()
    T4 = np.flatnonzero(occ4.ravel() == 0)
    owner_case("salt20_4096_K16", d24, t(rng.choice(T4, size=16, replace=False).astype(np.int32)), max(3, a.repeats // 2))
    res["owner_pass"] = owner

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
