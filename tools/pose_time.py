"""Wall time of planning in poses (Context.footprint_mask / pose_fields / pose_paths), all cases in one process, on 1024^2
salt20 and blocks20 with r2 = 4:
  mask    footprint_mask for the bodies (0,0,0,0), (3,3,1,1) and (16,16,8,8)
  field   pose_fields with F = 1 and F = 16, hmask None and the (3,3,1,1) mask, alternating with cost_fields of the same
          roots: `ratio` = pose field / plain field.  A pose field has 8x the states of a plain field; that is the yardstick
          to read the ratio against
  rounds  the F = 1 masked field with rounds = 0, 16, 32, .. up to the default: the time stops falling where the chip-wide
          rounds have no queued tile left (the working rounds); past it a round is an empty launch
  paths   pose_paths of 1024 targets (thead -1, to_root, cells_only) from the F = 1 masked toward field
  c       the C statement (tests/cpp/pose_ref.c), single-threaded, once: mask (3,3,1,1) and the F = 1 masked field; the GPU
          results are compared with it
Wall time per call around a device synchronise, the median of --repeats after warm-up.  Prints one JSON line (also written to
--out, default profiles/pose_time.json).
Usage: python tools/pose_time.py [--repeats 7] [--out FILE]"""
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

import pose_twin as pt  # noqa: E402
import sea_current_amd as sc  # noqa: E402
from sea_current_amd import synth  # noqa: E402

R2, TURN, REV = 4, 5, 7
BODIES = [(0, 0, 0, 0), (3, 3, 1, 1), (16, 16, 8, 8)]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_time.json"))
    a = ap.parse_args()
    ctx = sc.Context(0)
    ref = pt.Ref(tempfile.mkdtemp())
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    res = {"repeats": a.repeats, "r2": R2, "turn_cost": TURN, "rev_cost": REV, "device": torch.cuda.get_device_name(0)}
    for name, occ in (("salt20", synth.salt_grid(1024, 1024, 0.20)), ("blocks20", synth.block_grid(1024, 1024, 0.20))):
        r = res[name] = {}
        d2 = ctx.edt(t(occ))
        ctx.synchronize()
        d2h = d2.cpu().numpy()
        s, g = synth.queries(d2h >= R2, 1024)
        # mask
        r["mask_ms"] = {str(b): alternate({"m": lambda b=b: ctx.footprint_mask(d2, *b, r2=R2)}, ctx, a.repeats)["m"] for b in BODIES}
        hm = ctx.footprint_mask(d2, *BODIES[1], r2=R2)
        ctx.synchronize()
        hmh = hm.cpu().numpy()
        fit = [c for c in s if hmh.ravel()[c] == 0xFF][:16]                         # roots the body fits at every heading
        # on salt20 the (3,3,1,1) body fits at every heading in 18 cells, none of them a query start: take those
        fit = np.array(fit + [c for c in np.flatnonzero(hmh.ravel() == 0xFF) if c not in fit][:16 - len(fit)], np.int32)
        assert len(fit) == 16
        # field
        for F in (1, 16):
            roots, rh = t(fit[:F]), t(np.zeros(F, np.int32))
            out_p = ctx.pose_fields(d2, roots, rh, TURN, REV, r2=R2, hmask=hm)
            out_g = ctx.cost_fields(d2, roots, r2=R2)
            m = alternate({"pose_masked": lambda: ctx.pose_fields(d2, roots, rh, TURN, REV, r2=R2, hmask=hm, out=out_p),
                           "plain_a": lambda: ctx.cost_fields(d2, roots, r2=R2, out=out_g),
                           "pose_disc": lambda: ctx.pose_fields(d2, roots, rh, TURN, REV, r2=R2, out=out_p),
                           "plain_b": lambda: ctx.cost_fields(d2, roots, r2=R2, out=out_g)}, ctx, a.repeats)
            plain = 0.5 * (m["plain_a"] + m["plain_b"])
            r[f"field_F{F}"] = dict(pose_masked_ms=m["pose_masked"], pose_disc_ms=m["pose_disc"], plain_ms=plain,
                                    ratio_masked=m["pose_masked"] / plain, ratio_disc=m["pose_disc"] / plain)
        # rounds
        roots, rh = t(fit[:1]), t(np.zeros(1, np.int32))
        default = 4 * (32 + 32) + 16
        out_1 = ctx.pose_fields(d2, roots, rh, TURN, REV, r2=R2, hmask=hm)
        sweep = {}
        for rounds in (0, 16, 32, 48, 64, 96, 128, 192, default):
            sweep[str(rounds)] = alternate({"f": lambda rounds=rounds: ctx.pose_fields(d2, roots, rh, TURN, REV, r2=R2, hmask=hm, rounds=rounds,
                                                                                       out=out_1)}, ctx, 3)["f"]
        r["rounds_sweep_ms"] = sweep
        best = min(sweep.values())
        r["working_rounds_upper"] = int(next(k for k, v in sweep.items() if v <= 1.05 * best))
        # paths
        tw = ctx.pose_fields(d2, roots, rh, TURN, REV, toward=True, r2=R2, hmask=hm)
        qf, th, tg = t(np.zeros(1024, np.int32)), t(np.full(1024, -1, np.int32)), t(g)
        kw = dict(toward=True, r2=R2, hmask=hm, Lmax=8192, to_root=True, cells_only=True)
        out_q = ctx.pose_paths(d2, tw["gp"], roots, rh, qf, tg, th, TURN, REV, **kw)
        r["paths_1024_ms"] = alternate({"p": lambda: ctx.pose_paths(d2, tw["gp"], roots, rh, qf, tg, th, TURN, REV, out=out_q, **kw)}, ctx,
                                       a.repeats)["p"]
        ctx.synchronize()
        r["paths_ok"] = int((out_q["status"] == 0).sum())
        # the C statement, once, and equality
        t0 = time.perf_counter()
        hmc = ref.footprint_mask(d2h, *BODIES[1], r2=R2)
        t1 = time.perf_counter()
        gpc, _ = ref.pose_field(d2h, int(fit[0]), 0, TURN, REV, False, R2, hmc)
        t2 = time.perf_counter()
        gp = ctx.pose_fields(d2, roots, rh, TURN, REV, r2=R2, hmask=hm)["gp"]
        ctx.synchronize()
        r["c_mask_ms"], r["c_field_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
        r["equal_c"] = bool(np.array_equal(hmh, hmc) and np.array_equal(gp.cpu().numpy()[0], gpc))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
