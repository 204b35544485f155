"""Wall time of the field-of-view calls (Context.view_gain_headings, sector_gain, known_from_sectors), in one process.
  maps         1024^2 blocks20 and 1024^2 salt at p = 0.02 (the maps of tools/views_time.py)
  headings     view_gain_headings (best alone: hist in scratch) for 16, 256 and 1024 candidates on free cells at a radius of 30
               and of 290 cells, tables of 16 and 64 directions, span B / 4; beside view_gain of the same poses (the floor: the
               same rays, no bins) and beside the same headings asked as N * B rows of sector_gain
  known        known_from_sectors of the map's three views (radius 292) looking along heading 0 with span B / 4, B = 16,
               beside known_from_views of the same views; the share of the boxes' tiles the sector kernel skips (the kernel's
               rule restated on the host)
  equal        every timed output equals the C statement's (tests/cpp/sectors_ref.c; at radius 290 the first 8 candidates)
Wall time per call around a device synchronise after warm-up, median of the repeats.  Prints one JSON line (also written to
--out).
Usage: python tools/sectors_time.py [--repeats 7] [--maps blocks1024,salt1024] [--out FILE]"""
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
import sectors_twin as st  # noqa: E402
import views_twin as vt  # noqa: E402
from sea_current_amd import synth  # noqa: E402

TILE = 16


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


def tiles_skipped(row, W, H):
    """(tiles of the row's clipped box, tiles the sector kernel skips): the four-corner rule of sectors.hip."""
    cx, cy, r2, ax, ay, bx, by = (int(v) for v in row)
    r = int(np.sqrt(r2))
    x0, y0, x1, y1 = max(cx - r, 0), max(cy - r, 0), min(cx + r, W - 1), min(cy + r, H - 1)
    tx, ty = (x1 - x0) // TILE + 1, (y1 - y0) // TILE + 1
    s = ax * by - ay * bx
    skipped = 0
    for j in range(ty):
        for i in range(tx):
            lx, ly = x0 + i * TILE - cx, y0 + j * TILE - cy
            if lx <= 0 <= lx + TILE - 1 and ly <= 0 <= ly + TILE - 1:
                continue
            corners = [(dx, dy) for dx in (lx, lx + TILE - 1) for dy in (ly, ly + TILE - 1)]
            ad = [ax * dy - ay * dx for dx, dy in corners]
            db = [dx * by - dy * bx for dx, dy in corners]
            if s > 0:
                skipped += all(v < 0 for v in ad) or all(v <= 0 for v in db)
            elif s < 0:
                skipped += all(p < 0 and q <= 0 for p, q in zip(ad, db))
            else:
                skipped += all(v < 0 for v in ad)
    return tx * ty, skipped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--maps", default="blocks1024,salt1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    cases = {"blocks1024": (1024, lambda: synth.block_grid(1024, 1024, 0.20)), "salt1024": (1024, lambda: synth.salt_grid(1024, 1024, 0.02))}
    ctx = sc.Context(0)
    res = {}
    ref = st.Ref(tempfile.mkdtemp())
    for key in a.maps.split(","):
        n, mk = cases[key]
        occ = mk()
        views_h = vt.free_centres(occ, ft.three_discs(n, n))
        tocc, views = t(occ), t(views_h)
        known, seen = ctx.known_from_views(views, tocc, occ_seen=True)
        ctx.synchronize()
        known_h = known.cpu().numpy()
        free = np.flatnonzero(occ.ravel() == 0)
        r = dict(known_from_views_ms=wall(lambda: ctx.known_from_views(views, tocc, out=known, occ_seen=seen), ctx, a.repeats))

        def poses(radius, N):
            cells = free[np.random.default_rng(N + radius).choice(len(free), N, replace=False)]
            return np.stack([cells % n, cells // n, np.full(N, radius * radius)], 1).astype(np.int32)

        equal = True
        # known_from_sectors beside known_from_views
        dirs16 = sc.heading_dirs(16)
        rows_h = sc.sector_views(views_h, dirs16, 0, 4)
        rows = t(rows_h)
        ks, ss = ctx.known_from_sectors(rows, tocc, occ_seen=True)
        r["known_from_sectors_ms"] = wall(lambda: ctx.known_from_sectors(rows, tocc, out=ks, occ_seen=ss), ctx, a.repeats)
        wk, ws = ref.known_from_sectors(None, occ, rows_h)
        equal &= bool(np.array_equal(ks.cpu().numpy(), wk) and np.array_equal(ss.cpu().numpy(), ws))
        tiles = [tiles_skipped(row, n, n) for row in rows_h]
        r["sector_tiles"], r["sector_tiles_skipped"] = int(sum(a_ for a_, _ in tiles)), int(sum(b_ for _, b_ in tiles))
        r["sector_known_cells"], r["view_known_cells"] = int(wk.sum()), int(known_h.sum())
        for radius in (30, 290):
            for N in (16, 256, 1024):
                cand_h = poses(radius, N)
                cand = t(cand_h)
                checked = N if radius == 30 else 8
                gain = ctx.view_gain(cand, tocc, known)
                floor = wall(lambda: ctx.view_gain(cand, tocc, known, out=gain), ctx, a.repeats)
                r[f"view_gain_r{radius}_N{N}_ms"] = floor
                for B in (16, 64):
                    dirs, span = sc.heading_dirs(B), B // 4
                    best = ctx.view_gain_headings(cand, tocc, known, dirs, span)
                    ms = wall(lambda: ctx.view_gain_headings(cand, tocc, known, dirs, span, out=best), ctx, a.repeats)
                    full = ctx.view_gain_headings(cand, tocc, known, dirs, span, hist=True, gainh=True)
                    want = ref.view_gain_headings(occ, known_h, cand_h[:checked], dirs, span)
                    ctx.synchronize()
                    equal &= bool(np.array_equal(best.cpu().numpy()[:checked], want["best"]))
                    equal &= all(bool(np.array_equal(full[k].cpu().numpy()[:checked], want[k])) for k in ("hist", "gainh", "best"))
                    srows_h = np.concatenate([sc.sector_views(cand_h, dirs, h, span) for h in range(B)])   # heading-major: row h * N + i
                    srows = t(srows_h)
                    sg = ctx.sector_gain(srows, tocc, known)
                    rows_ms = wall(lambda: ctx.sector_gain(srows, tocc, known, out=sg), ctx, a.repeats)
                    equal &= bool(np.array_equal(sg.cpu().numpy().reshape(B, N).T, full["gainh"].cpu().numpy()))
                    r[f"headings_r{radius}_N{N}_B{B}_ms"] = ms
                    r[f"headings_r{radius}_N{N}_B{B}_over_view_gain"] = ms / floor
                    r[f"sector_rows_r{radius}_N{N}_B{B}_ms"] = rows_ms
                    r[f"sector_rows_r{radius}_N{N}_B{B}_over_headings"] = rows_ms / ms
                    del srows, sg
        r["equal_to_c_statement"] = equal
        res[key] = r
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
