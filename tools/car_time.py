"""Wall time of car-like pose planning (Context.arc_mask / car_fields / car_paths), all cases in one process, on 1024^2 salt20
and blocks20 with r2 = 4 and the (1,1,0,0) body:
  mask    arc_mask for arc_n 1, 2 and 4
  field   car_fields (arc_n 2) with F = 1 and F = 16, alternating with pose_fields of the same roots with turn_cost =
          arc_cost: `ratio` = car field / pose field.  Reported, not gated: the car field does different work (a halo of
          2 arc_n cells, an arc gather, no turn closure)
  rounds  the F = 1 field with rounds = 0, 16, 32, .. up to the default: the time stops falling where the chip-wide rounds
          have no queued tile left (the working rounds); past it a round is an empty launch
  paths   car_paths of 1024 targets (thead -1, to_root) from the F = 1 toward field
  c       the C statement (tests/cpp/car_ref.c), single-threaded, once: the arc mask and the F = 1 field; the GPU results are
          compared with it
Wall time per call around a device synchronise, the median of --repeats after warm-up.  Prints one JSON line (also written to
--out, default profiles/car_time.json).
Usage: python tools/car_time.py [--repeats 7] [--out FILE]"""
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

import car_twin as ct  # noqa: E402
import sea_current_amd as sc  # noqa: E402
from sea_current_amd import synth  # noqa: E402

R2, ARC_N, ARC_COST, REV = 4, 2, 5, 7
BODY = (1, 1, 0, 0)   # 3 x 1 cells: on salt20 a longer body fits almost nowhere


def once(fn, ctx):
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, ctx, repeats):
    """fns: dict name -> callable.  Warm every one up, then time them in turn `repeats` times: name -> median ms."""
    for fn in fns.values():
        fn()
    ctx.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ts[k].append(once(fn, ctx))
    return {k: float(np.median(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "car_time.json"))
    a = ap.parse_args()
    ctx = sc.Context(0)
    ref = ct.Ref(tempfile.mkdtemp())
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    res = {"repeats": a.repeats, "r2": R2, "arc_n": ARC_N, "arc_cost": ARC_COST, "rev_cost": REV, "body": list(BODY),
           "device": torch.cuda.get_device_name(0)}
    for name, occ in (("salt20", synth.salt_grid(1024, 1024, 0.20)), ("blocks20", synth.block_grid(1024, 1024, 0.20))):
        r = res[name] = {}
        d2 = ctx.edt(t(occ))
        hm = ctx.footprint_mask(d2, *BODY, r2=R2)
        ctx.synchronize()
        d2h, hmh = d2.cpu().numpy(), hm.cpu().numpy()
        s, g = synth.queries(d2h >= R2, 1024)
        fit = [c for c in s if hmh.ravel()[c] == 0xFF][:16]                         # roots the body fits at every heading
        fit = np.array(fit + [c for c in np.flatnonzero(hmh.ravel() == 0xFF) if c not in fit][:16 - len(fit)], np.int32)
        assert len(fit) == 16
        # mask
        r["mask_ms"] = {str(n): alternate({"m": lambda n=n: ctx.arc_mask(d2, n, r2=R2, hmask=hm)}, ctx, a.repeats)["m"] for n in (1, 2, 4)}
        am = ctx.arc_mask(d2, ARC_N, r2=R2, hmask=hm)
        # field
        for F in (1, 16):
            roots, rh = t(fit[:F]), t(np.zeros(F, np.int32))
            out_c = ctx.car_fields(d2, am, roots, rh, ARC_N, ARC_COST, REV, r2=R2, hmask=hm)
            out_p = ctx.pose_fields(d2, roots, rh, ARC_COST, REV, r2=R2, hmask=hm)
            m = alternate({"car": lambda: ctx.car_fields(d2, am, roots, rh, ARC_N, ARC_COST, REV, r2=R2, hmask=hm, out=out_c),
                           "pose": lambda: ctx.pose_fields(d2, roots, rh, ARC_COST, REV, r2=R2, hmask=hm, out=out_p)}, ctx, a.repeats)
            ctx.synchronize()
            r[f"field_F{F}"] = dict(car_ms=m["car"], pose_ms=m["pose"], ratio=m["car"] / m["pose"],
                                    car_ge_pose=bool((out_c["gp"] >= out_p["gp"]).all()))
        # rounds
        roots, rh = t(fit[:1]), t(np.zeros(1, np.int32))
        default = 4 * (32 + 32) + 16
        out_1 = ctx.car_fields(d2, am, roots, rh, ARC_N, ARC_COST, REV, r2=R2, hmask=hm)
        sweep = {}
        for rounds in (0, 16, 32, 48, 64, 96, 128, 192, default):
            sweep[str(rounds)] = alternate({"f": lambda rounds=rounds: ctx.car_fields(d2, am, roots, rh, ARC_N, ARC_COST, REV, r2=R2, hmask=hm,
                                                                                      rounds=rounds, out=out_1)}, ctx, 3)["f"]
        r["rounds_sweep_ms"] = sweep
        best = min(sweep.values())
        r["working_rounds_upper"] = int(next(k for k, v in sweep.items() if v <= 1.05 * best))
        # paths
        tw = ctx.car_fields(d2, am, roots, rh, ARC_N, ARC_COST, REV, toward=True, r2=R2, hmask=hm)
        qf, th, tg = t(np.zeros(1024, np.int32)), t(np.full(1024, -1, np.int32)), t(g)
        kw = dict(toward=True, r2=R2, hmask=hm, Lmax=8192, to_root=True)
        out_q = ctx.car_paths(d2, am, tw["gp"], roots, rh, qf, tg, th, ARC_N, ARC_COST, REV, **kw)
        r["paths_1024_ms"] = alternate({"p": lambda: ctx.car_paths(d2, am, tw["gp"], roots, rh, qf, tg, th, ARC_N, ARC_COST, REV, out=out_q, **kw)},
                                       ctx, a.repeats)["p"]
        ctx.synchronize()
        r["paths_ok"] = int((out_q["status"] == 0).sum())
        # the C statement, once, and equality
        t0 = time.perf_counter()
        amc = ref.arc_mask(d2h, ARC_N, R2, hmh)
        t1 = time.perf_counter()
        gpc, _ = ref.car_field(d2h, int(fit[0]), 0, ARC_N, ARC_COST, REV, False, R2, hmh)
        t2 = time.perf_counter()
        gp = ctx.car_fields(d2, am, roots, rh, ARC_N, ARC_COST, REV, r2=R2, hmask=hm)["gp"]
        ctx.synchronize()
        r["c_mask_ms"], r["c_field_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
        r["equal_c"] = bool(np.array_equal(am.cpu().numpy().view(np.uint16), amc) and np.array_equal(gp.cpu().numpy()[0], gpc))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
