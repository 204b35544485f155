"""The kernels the cost-field entries enqueue, in order: one call of each of the three build entries (single-root,
weighted, multi-source with owner) and of the three read-outs on a 130 x 70 map with rounds = 2.  The map and every
argument are made on the host and copied, so the trace holds the library's kernels, the runtime's fill kernels of the
library's memsets (__amd_rocclr_fillBufferAligned) and its copy kernels of the uploads before and the read-backs after
the calls (__amd_rocclr_copyBuffer), nothing else.
  python tools/field_launch_sequence.py                   the calls (run it under rocprofv3 --kernel-trace, alone)
  python tools/field_launch_sequence.py --list TRACE.csv  the kernel names of that trace in start order, one per line,
                                                          template arguments kept, argument lists dropped
profiles/field_launch_sequence_*.txt hold such lists; two builds of the library enqueue the same work iff they are equal."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sea-current_amd", "python")]


def calls():
    import numpy as np
    import torch

    import sea_current_amd as sc
    W, H = 130, 70
    ctx = sc.Context(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d2 = np.ones((H, W), np.int32)
    d2[10:60, 64] = 0                                     # a wall across the tile border, open at both ends
    pen = np.full((H, W), 2, np.uint8)
    d2, pen = t(d2), t(pen)
    roots, seeds, off = t(np.array([0], np.int32)), t(np.array([0, W * H - 1], np.int32)), t(np.array([0, 2], np.int32))
    qf, tg = t(np.zeros(3, np.int32)), t(np.array([W - 1, 35 * W + 70, (H - 1) * W], np.int32))
    f = ctx.cost_fields(d2, roots, rounds=2)
    fw = ctx.cost_fields(d2, roots, rounds=2, pen=pen, pen_cap=255)
    fm = ctx.cost_fields_multi(d2, seeds, off, rounds=2)
    p = ctx.field_paths(d2, f["g"], roots, qf, tg, Lmax=256)
    pw = ctx.field_paths(d2, fw["g"], roots, qf, tg, Lmax=256, pen=pen, pen_cap=255)
    pm = ctx.field_paths_multi(d2, fm, seeds, qf, tg, Lmax=256)
    ctx.synchronize()
    assert all(int(r["status"].cpu().max()) == 0 for r in (f, fw, fm, p, pw, pm))
    ctx.close()


def names(trace):
    with open(trace, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    out = []
    for r in rows:
        n = r["Kernel_Name"]
        if n.endswith(" [clone .kd]"):
            n = n[:-len(" [clone .kd]")]
        if n.endswith(")"):                               # drop the argument list, keep the template arguments
            depth = 0
            for i in range(len(n) - 1, -1, -1):
                depth += (n[i] == ")") - (n[i] == "(")
                if depth == 0:
                    n = n[:i]
                    break
        out.append(n)
    return out


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        print("\n".join(names(sys.argv[2])))
    else:
        calls()
