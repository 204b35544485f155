"""Wall time of the goals by gain (Context.explore_gain, fleet_explore_gain), in one process.
  map          1024^2 blocks20; known from the map's three views by line of sight (the maps of tools/views_time.py)
  candidates   frontier_centres of that map (min_size 3, Cmax 512: the rows beyond the listed clusters are dead)
  robots       R = 1, 16, 256 on known free cells, their cost fields on the known map; sensing radius 30 and 290 cells
  forms        (i)   explore_gain: selection and delta update on the stream
               (ii)  the same procedure through the existing entry points only: view_gain over all candidates per round, the
                     argmax on the host, known_from_views of the pick; its picks and its known map must equal (i)'s
               (a third form, a full re-cast of the candidates whose boxes meet the chosen one, was built behind a switch,
               measured by this tool and not kept: DESIGN.md section 29.4, profiles/explore_gain_forms_time.json)
  floor        a call whose first round finds no eligible pair (min_gain above every gain): R rounds of kernels that leave at
               once, against the same call with rounds = 0; the launches of a round
  fleet        fleet_explore beside fleet_explore_gain on the same inputs: the time, and the free cells of the true map the
               goals' views reveal
Wall time per call around a device synchronise after warm-up, median of the repeats, the forms alternating.  Prints one JSON line
(also written to --out).
Usage: python tools/explore_gain_time.py [--repeats 7] [--robots 1,16,256] [--radii 30,290] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sea-current_amd", "python"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import frontier_twin as ft  # noqa: E402
import sea_current_amd as sc  # noqa: E402
import views_twin as vt  # noqa: E402
from sea_current_amd import synth  # noqa: E402

INF = sc.FIELD_INF
LAUNCHES_PER_ROUND = dict(full_circle=5, table=6)   # sel1, sel2, view, delta, (best), combine


def timed(fn, ctx):
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternating(forms, ctx, repeats):
    """{name: median ms} of the forms, run in turn `repeats` times after one warm-up each; the last outputs."""
    ts, outs = {k: [] for k in forms}, {}
    for rep in range(repeats + 1):
        for k, fn in forms.items():
            ms, outs[k] = timed(fn, ctx)
            if rep:
                ts[k].append(ms)
    return {k: float(np.median(v)) for k, v in ts.items()}, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--robots", default="1,16,256")
    ap.add_argument("--radii", default="30,290")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n, Cmax, wg = 1024, 512, 2
    ctx = sc.Context(0)
    occ = synth.block_grid(n, n, 0.20)
    tocc = t(occ)
    known, seen = ctx.known_from_views(t(vt.free_centres(occ, ft.three_discs(n, n))), tocc, occ_seen=True)
    d2k = ctx.d2_known(ctx.edt(seen), known)
    fr = ctx.frontiers(d2k, known, min_size=3, Cmax=Cmax)
    cand = ctx.frontier_centres(fr, n, n)[0].contiguous()
    ctx.synchronize()
    known_h, cand_h = known.cpu().numpy(), cand.cpu().numpy()
    res = dict(map="blocks1024", Cmax=Cmax, listed=int(fr["ncl"].cpu().numpy()[0, 0]), wg=wg, wc=1, min_gain=1, launches_per_round=LAUNCHES_PER_ROUND)
    rng = np.random.default_rng(1)
    free_known = np.flatnonzero((known_h.ravel() != 0) & (d2k.cpu().numpy().ravel() >= 1))
    equal = True
    for R in (int(v) for v in a.robots.split(",")):
        robots = t(rng.choice(free_known, R, replace=False).astype(np.int32))
        g = ctx.cost_fields(d2k, robots)["g"]
        ctx.synchronize()
        live = (cand_h >= 0)
        cost_h = np.where(live[None, :], g.reshape(R, -1)[:, t(np.where(live, cand_h, 0).astype(np.int64))].cpu().numpy().astype(np.int64), INF)
        for radius in (int(v) for v in a.radii.split(",")):
            r2 = radius * radius
            views = ctx.views_from_cells(cand, n, n, r2)
            kw, gain = torch.empty_like(known), torch.empty(Cmax, dtype=torch.int32, device="cuda")

            def new_form():
                return ctx.explore_gain(seen, known, g, cand, r2, wg=wg, wc=1, min_gain=1)

            def baseline():
                """view_gain over all candidates per round, a host argmax, known_from_views of the pick"""
                kw.copy_(known)
                goal, ggain = np.full(R, -1, np.int32), np.zeros(R, np.int32)
                free_r, free_n = np.ones(R, bool), live.copy()
                for _ in range(min(R, Cmax)):
                    ctx.view_gain(views, seen, kw, out=gain)
                    ctx.synchronize()
                    gh = gain.cpu().numpy().astype(np.int64)
                    ok = free_r[:, None] & (free_n & (gh >= 1))[None, :] & (cost_h != INF)
                    if not ok.any():
                        break
                    score = np.where(ok, wg * gh[None, :] - cost_h, np.iinfo(np.int64).min)
                    r, c = np.unravel_index(np.argmax(score), score.shape)           # the first maximum: smallest r, then n
                    goal[r], ggain[r] = cand_h[c], gh[c]
                    free_r[r], free_n[c] = False, False
                    ctx.known_from_views(views[c:c + 1], seen, base=kw, out=kw)
                return dict(goal=goal, ggain=ggain, known_out=kw)

            forms = {"new": new_form, "baseline": baseline}
            ms, outs = alternating(forms, ctx, a.repeats)
            key = f"R{R}_r{radius}"
            host = lambda x: x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
            for k in ("goal", "ggain", "known_out"):
                equal &= all(bool(np.array_equal(host(outs["new"][k]), host(outs[f][k]))) for f in forms if f != "new")
            res[key] = dict(new_ms=ms["new"], baseline_ms=ms["baseline"], picks=int(outs["new"]["npick"].cpu().numpy()[0]),
                            new_over_baseline=ms["new"] / ms["baseline"])
            # the launch floor: every round's kernels leave at once
            fl, _ = alternating({"done": lambda: ctx.explore_gain(seen, known, g, cand, r2, wg=wg, min_gain=1 << 30, want_all=False),
                                 "none": lambda: ctx.explore_gain(seen, known, g, cand, r2, wg=wg, min_gain=1 << 30, rounds=0, want_all=False)},
                                ctx, a.repeats)
            res[key].update(done_rounds_ms=fl["done"], no_rounds_ms=fl["none"], done_round_us=(fl["done"] - fl["none"]) * 1e3 / min(R, Cmax))
            # the chain it stands beside, and what the goals' views reveal of the true map
            fe, fo = alternating({"fleet_explore": lambda: ctx.fleet_explore(d2k, known, g, min_size=3, Cmax=Cmax),
                                  "fleet_explore_gain": lambda: ctx.fleet_explore_gain(d2k, known, seen, g, r2, min_size=3, Cmax=Cmax, wg=wg)},
                                 ctx, a.repeats)
            rev = {}
            for k, o in fo.items():
                after = ctx.known_from_views(ctx.views_from_cells(o["goal"], n, n, r2), tocc, base=known)
                ctx.synchronize()
                rev[k] = int(((after != 0) & (known == 0) & (tocc == 0)).sum().item())
            equal &= bool(np.array_equal(fo["fleet_explore_gain"]["goal"].cpu().numpy(), outs["new"]["goal"].cpu().numpy()))
            res[key].update(fleet_explore_ms=fe["fleet_explore"], fleet_explore_gain_ms=fe["fleet_explore_gain"],
                            revealed_fleet_explore=rev["fleet_explore"], revealed_fleet_explore_gain=rev["fleet_explore_gain"])
            print(key, json.dumps(res[key]), file=sys.stderr, flush=True)
        del g
        torch.cuda.empty_cache()
    res["forms_equal"] = equal
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
