"""Wall time of the assignment calls (sc_field_cost_matrix, sc_assign_batch) next to the single-threaded C reference
(tests/cpp/assign_ref.c, cc -O2) on the same inputs in the same run:
  fields_1024    one 1024 x 1024 matrix taken from real fields of the bench's 1024^2 salt20 map: 1024 random free goals (one
                 field each, sc_cost_field_batch) x 1024 random free robots
  random_1024    the same size with full-range random costs
  batch_64       256 problems of 64 x 64 (octile-like costs 10a + 14b)
  batch_16       1024 problems of 16 x 16
  cost_matrix    sc_field_cost_matrix at R = F = 1024 on those fields
Per case: the steps the procedure took, GPU milliseconds, microseconds per step, the reference's milliseconds, the ratio
reference / GPU (above 1: the GPU is faster), and whether all five outputs are equal.  Wall time per call around a device
synchronise after warm-up, median of the repeats.  Prints one JSON line (also written to --out).
Usage: python tools/assign_time.py [--repeats 7] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sea-current_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sea_current_amd as sc  # noqa: E402
from sea_current_amd import synth  # noqa: E402

KEYS = ("col_of", "row_of", "u", "v", "info")


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


def reference_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="assign_ref"), "libassign_ref.so")
    subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "cpp", "assign_ref.c")])
    lib = C.CDLL(so)
    lib.assign_ref.restype = None
    lib.assign_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    return lib


def reference(lib, cost, repeats):
    B, R, Cc = cost.shape
    o = dict(col_of=np.zeros((B, R), np.int32), row_of=np.zeros((B, Cc), np.int32), u=np.zeros((B, R), np.int64), v=np.zeros((B, Cc), np.int64),
             info=np.zeros((B, 4), np.int64))
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        lib.assign_ref(cost.ctypes.data, B, R, Cc, *(o[k].ctypes.data for k in KEYS), None)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), o


def case(ctx, lib, cost, repeats):
    d = torch.from_numpy(cost).cuda()
    out = {}
    gpu_ms = wall(lambda: out.update(ctx.assign(d)), ctx, repeats)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    ref_ms, ref = reference(lib, cost, min(repeats, 3))
    steps = int(got["info"][:, 2].sum())
    return dict(shape=list(cost.shape), steps=steps, matched=int(got["info"][:, 0].sum()), gpu_ms=gpu_ms, us_per_step=1e3 * gpu_ms / max(steps, 1),
                reference_ms=ref_ms, reference_over_gpu=ref_ms / gpu_ms, equal=bool(all(np.array_equal(got[k], ref[k]) for k in KEYS)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = sc.Context(0)
    lib = reference_lib()
    rng = np.random.default_rng(7)
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    occ = synth.salt_grid(1024, 1024, 0.20)
    d2 = ctx.edt(torch.from_numpy(occ).cuda())
    free = np.flatnonzero(occ.ravel() == 0)
    pick = rng.choice(free, 2048, replace=False).astype(np.int32)
    goals, robots = torch.from_numpy(pick[:1024]).cuda(), torch.from_numpy(pick[1024:]).cuda()
    g = torch.empty((1024, 1024, 1024), dtype=torch.int32, device="cuda")
    status = torch.empty(1024, dtype=torch.int32, device="cuda")
    for k in range(0, 1024, 256):
        ctx.cost_fields(d2, goals[k:k + 256], out=dict(g=g[k:k + 256], status=status[k:k + 256]))
    m = {}
    res["cost_matrix"] = dict(R=1024, F=1024, gpu_ms=wall(lambda: m.update(cost=ctx.field_cost_matrix(g, robots)), ctx, args.repeats))
    cost = m["cost"].cpu().numpy()
    res["cost_matrix"]["equal_numpy"] = bool(np.array_equal(cost, g.reshape(1024, -1)[:, robots.long()].T.cpu().numpy()))
    res["cost_matrix"]["forbidden_share"] = float((cost == sc.FIELD_INF).mean())
    del g
    res["fields_1024"] = case(ctx, lib, cost[None], args.repeats)
    res["random_1024"] = case(ctx, lib, rng.integers(0, 2**31 - 1, (1, 1024, 1024)).astype(np.int32), args.repeats)
    octile = lambda B, n: (10 * rng.integers(0, 200, (B, n, n)) + 14 * rng.integers(0, 200, (B, n, n))).astype(np.int32)
    res["batch_64"] = case(ctx, lib, octile(256, 64), args.repeats)
    res["batch_16"] = case(ctx, lib, octile(1024, 16), args.repeats)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
