"""CPU model of the two-wavefront A* step loop (throughput build of csrc/astar.hip): which 64-byte lines a step touches.

A restatement of the kernel's step structure, not of its timing: the f-level rings in HBM, refill chunks of 512 entries,
steps of at most 64 pops, narrow steps (<= 16 nodes) with runs of KL = 8 / 4 / 2 cells along the two same-f moves, the same-f
appends of wavefront 0 (diagonal entries first, then straight ones), the table that settles duplicates inside a step, the
hand-over of the won nodes, wavefront 1's lazy batches of 48 .. 64 nodes (flushed at the end of a level), and the pruning
tables.  What it cannot know is when wavefront 1 runs relative to wavefront 0; it lets wavefront 1 take a batch after every
step that leaves it 48 records or more.

Per map family it prints, and writes to --out:
  popped entries per expansion (the kernel's counters say 1.36 on the headline map: check that first);
  distinct 64-byte lines per expansion of the closed-word loads, the closed-bit ORs, the g bytes (per wavefront-1 batch),
  the legal-move loads and the ring traffic, with pops in push order and with every refill chunk of more than 64 entries
  grouped by tile bin (--order push / bin / sort: the kernel's 64-bin counting sort, or a full sort by tile);
  the legal-move lines under an 8 x 8-tile layout of the bytes (a figure for a later decision, nothing uses it);
  per query the sizes of its levels (entries taken from the level's HBM ring).

  python tools/astar_lines_model.py --out profiles/astar_tile_order_model.json
  python tools/astar_lines_model.py --size 320x192 --salt 0.2 --corner --queries 4     # shapes for the tests

simulate() is also what tests/test_gpu_astar_tile_order.py uses to show that its maps reach the binned refill."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "sea-current_amd", "python")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

CQ, REFILL, HQ_LAZY = 1024, 512, 48
E_RUN = 1 << 18
E_START = 4 << 13 | 3 << 16
DX = (1, -1, 0, 0, 1, -1, 1, -1)
DY = (0, 0, 1, -1, 1, 1, -1, -1)
WC = (10, 10, 10, 10, 14, 14, 14, 14)
_ALWAYS = 0x75B6D9EA34C851A2


def _e01(d):
    return (0x6476 >> (4 * (d & 3))) & 7, (0x7554 >> (4 * (d & 3))) & 7


def entry_pack(x, y, d, pmv):
    e0, e1 = _e01(d)
    side = (((pmv >> e0) & 1) | (((pmv >> e1) & 1) << 1)) if d < 4 else 0
    return y << 19 | side << 16 | d << 13 | x


def entry_prune(e):
    d = (e >> 13) & 7
    prune = (_ALWAYS >> (8 * d)) & 0xFF
    k0, k1 = (3, 2) if d < 2 else (0, 1)
    e0, e1 = _e01(d)
    if (e >> 16) & 1:
        prune |= (1 << k0) | (1 << e0)
    if (e >> 17) & 1:
        prune |= (1 << k1) | (1 << e1)
    if e & E_RUN:
        prune |= 1 << d
    return 0 if (e & 0x3E000) == E_START else prune


PRUNE_TBL = [entry_prune(i << 13) for i in range(64)]


def tile_bin(e):
    return ((e >> 20) & 0x38) | ((e >> 5) & 7)


def tile_key(e):
    return ((e >> 23) << 8) | ((e & 0x1FFF) >> 5)      # closed-bitmap tile (row, column): the full sort


def simulate(mv, W, H, s, g, order="push"):
    """One search on the legal-move bytes mv [H * W] (a flat list or array of ints).  Returns counters and level sizes."""
    mv = mv if isinstance(mv, (list, bytes, bytearray)) else np.asarray(mv).ravel().tolist()
    sx, sy, gx, gy = s % W, s // W, g % W, g // W

    def h(x, y):
        dx, dy = abs(x - gx), abs(y - gy)
        return 10 * max(dx, dy) + 4 * min(dx, dy)

    closed = bytearray(W * H)
    rings = {}                     # f -> entries waiting in the level's HBM ring
    ring_pos = [0] * 32            # running tail position of the 32 rings (for the lines of the stores)
    st = dict(expanded=0, popped=0, steps=0, closed_lines=0, or_lines=0, g_lines=0, mv_lines=0, mv_lines_tiled=0,
              ring_lines=0, batches=0, requeued=0)
    levels, level_f = [], []       # entries every level took from its HBM ring, and the level's f
    dup_tbl = {}
    pending = []                   # hand-over records (x, y, moves to push, legal moves, g)
    found = False

    def wave1(flush):
        while pending and (flush or len(pending) >= HQ_LAZY):
            batch = pending[:64]
            del pending[:64]
            st["batches"] += 1
            st["g_lines"] += len({(y >> 3, x >> 3) for x, y, _, _, _ in batch})
            stores = set()
            for x, y, m, pm, gq in batch:
                d = 0
                while m:
                    if m & 1:
                        nx, ny = x + DX[d], y + DY[d]
                        fs = gq + WC[d] + h(nx, ny)
                        rings.setdefault(fs, []).append(entry_pack(nx, ny, d, pm))
                        stores.add((fs & 31, ring_pos[fs & 31] >> 4))
                        ring_pos[fs & 31] += 1
                    m >>= 1
                    d += 1
            st["ring_lines"] += len(stores)

    fcur = h(sx, sy)
    cur = [sy << 19 | E_START | sx]
    head = 0
    while True:
        taken = 0
        while True:
            if head == len(cur):
                lvl = rings.get(fcur)
                if not lvl:
                    break
                chunk = lvl[:REFILL]
                del lvl[:REFILL]
                n = len(chunk)
                taken += n
                st["ring_lines"] += (n + 15) // 16
                if n > 64 and order != "push":
                    chunk.sort(key=tile_bin if order == "bin" else tile_key)       # stable, like a counting sort
                cur = chunk
                head = 0
            n = min(64, len(cur) - head)
            ents = cur[head:head + n]
            head += n
            st["popped"] += n
            st["steps"] += 1
            narrow = n <= 16
            kl = (8 if n <= 4 else 4 if n <= 8 else 2) if narrow else 1
            cl_lines, or_lines, mv_lines, mv_tiled = set(), set(), set(), set()
            slot_of = {}
            app_d, app_s = [], []      # same-f appends: a wide step queues the diagonal entries first, a narrow one goes lane by lane
            for e in ents:
                x, y = e & 0x1FFF, e >> 19
                c = y * W + x
                cl_lines.add((y >> 4, x >> 5))
                mv_lines.add(c >> 6)
                mv_tiled.add((y >> 3, x >> 3))
                byte = mv[c]
                dxg, dyg = gx - x, gy - y
                adx, ady = abs(dxg), abs(dyg)
                dD = 4 + ((1 if dxg < 0 else 0) | (2 if dyg < 0 else 0))
                dS = (1 if dxg < 0 else 0) if adx > ady else (3 if dyg < 0 else 2)
                bD = 1 << dD if adx >= 1 and ady >= 1 else 0
                bS = 1 << dS if adx != ady else 0
                if narrow:   # the lanes of both directions load their cells whoever wins the node
                    for dd, bb, lg in ((dD, bD, min(adx, ady)), (dS, bS, abs(adx - ady))):
                        if bb:
                            for k in range(1, min(kl, lg)):
                                cc = c + k * (DY[dd] * W + DX[dd])
                                mv_lines.add(cc >> 6)
                                mv_tiled.add(((y + k * DY[dd]) >> 3, (x + k * DX[dd]) >> 3))
                # duplicates: the table keeps the node last popped under a hash; a step admits one node per slot
                hsh = (x + 32 * y) & 1023
                key = y << 16 | x
                closed_before = dup_tbl.get(hsh) == key           # popped under this hash most recently: closed
                if hsh in slot_of:
                    if slot_of[hsh] != key and not closed_before:  # lost its slot to a different node: back into the ring
                        cur.append(e)
                        st["popped"] -= 1
                        st["requeued"] += 1
                    continue
                slot_of[hsh] = key
                if closed_before or closed[c]:
                    continue
                closed[c] = 1
                or_lines.add((y >> 4, x >> 5))
                st["expanded"] += 1
                if x == gx and y == gy:
                    found = True
                prune = PRUNE_TBL[(e >> 13) & 63]
                if narrow:
                    for dd, bb, lg, out in ((dD, bD, min(adx, ady), app_d), (dS, bS, abs(adx - ady), app_d)):
                        if not bb or (prune >> dd) & 1:
                            continue
                        run = 0
                        while run < kl and run < lg and (mv[c + run * (DY[dd] * W + DX[dd])] >> dd) & 1:
                            run += 1
                        for k in range(run):
                            out.append(entry_pack(x + (k + 1) * DX[dd], y + (k + 1) * DY[dd], dd, mv[c + k * (DY[dd] * W + DX[dd])])
                                       | (E_RUN if k + 1 < run else 0))
                else:
                    cand = byte & ~prune
                    if cand & bD:
                        app_d.append((y + (-1 if dyg < 0 else 1)) << 19 | dD << 13 | (x + (-1 if dxg < 0 else 1)))
                    if cand & bS:
                        app_s.append(entry_pack(x + DX[dS], y + DY[dS], dS, byte))
                pending.append((x, y, (byte & ~prune) & ~(bD | bS), byte, fcur - h(x, y)))
            dup_tbl.update(slot_of)
            cur.extend(app_d)
            cur.extend(app_s)
            st["closed_lines"] += len(cl_lines)
            st["or_lines"] += len(or_lines)
            st["mv_lines"] += len(mv_lines)
            st["mv_lines_tiled"] += len(mv_tiled)
            wave1(False)
        wave1(True)
        levels.append(taken)
        level_f.append(fcur)
        rings.pop(fcur, None)
        left = [f for f, v in rings.items() if v]
        if found or not left:
            break
        fcur = min(left)
    st["levels"] = levels
    st["level_f"] = level_f
    st["found"] = found
    return st


def family_grid(name, W, H, seed=None):
    from sea_current_amd import synth
    kw = {} if seed is None else {"seed": seed}
    if name.startswith("salt"):
        return synth.salt_grid(W, H, int(name[4:]) / 100.0, **kw)
    return synth.block_grid(W, H, 0.20, **kw)


def run_family(name, W, H, nq, corner=False, orders=("push", "bin", "sort"), seed=None):
    from oracle import oracle
    from sea_current_amd import synth
    oracle.build()
    d2 = oracle.edt(family_grid(name, W, H, seed))
    mv = oracle.moves(d2).ravel().tolist()
    if corner:
        comp = synth.largest_component(d2 >= 1)
        ys, xs = np.nonzero(comp)
        a, b = np.flatnonzero((xs < 40) & (ys < 40)), np.flatnonzero((xs >= W - 40) & (ys >= H - 40))
        rng = np.random.default_rng(8)
        ia, ib = rng.choice(a, nq), rng.choice(b, nq)
        s, g = ys[ia] * W + xs[ia], ys[ib] * W + xs[ib]
    else:
        s, g = synth.queries(d2 >= 1, nq)
    ref = oracle.astar_batch(d2, s.astype(np.int32), g.astype(np.int32), Lmax=4, nthreads=4)
    out = {"map": name, "size": [W, H], "queries": int(nq), "orders": {}}
    for order in orders:
        tot = {}
        per_query = []
        for q in range(nq):
            if s[q] == g[q]:
                continue
            r = simulate(mv, W, H, int(s[q]), int(g[q]), order)
            assert r["expanded"] == int(ref["expanded"][q]), (q, r["expanded"], int(ref["expanded"][q]))   # E is the oracle's
            lv = np.array(r.pop("levels"))
            r.pop("level_f")
            per_query.append({"expanded": r["expanded"], "levels": int(lv.size), "levels_above_64": int((lv > 64).sum()),
                              "levels_above_512": int((lv > REFILL).sum()), "largest_level": int(lv.max()),
                              "median_level_above_64": float(np.median(lv[lv > 64])) if (lv > 64).any() else 0.0})
            for k, v in r.items():
                if k != "found":
                    tot[k] = tot.get(k, 0) + v
        ex = tot["expanded"]
        lines = {k: tot[k] / ex for k in ("closed_lines", "or_lines", "g_lines", "mv_lines", "ring_lines")}
        out["orders"][order] = {"expansions": ex, "popped_per_expansion": tot["popped"] / ex, "steps": tot["steps"],
                                "lines_per_expansion": dict(lines, sum=sum(lines.values())),
                                "mv_lines_per_expansion_8x8_tiles": tot["mv_lines_tiled"] / ex,
                                "g_lines_per_batch": tot["g_lines"] / tot["batches"], "requeued_per_expansion": tot["requeued"] / ex,
                                "per_query": per_query}
        l = out["orders"][order]["lines_per_expansion"]
        print("%-7s %-4s exp %7d pop/exp %.3f  closed %.3f or %.3f g %.3f mv %.3f ring %.3f sum %.3f | mv 8x8 %.3f | largest level %d" %
              (name, order, ex, tot["popped"] / ex, l["closed_lines"], l["or_lines"], l["g_lines"], l["mv_lines"], l["ring_lines"], l["sum"],
               tot["mv_lines_tiled"] / ex, max(p["largest_level"] for p in per_query)), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="salt20,salt05,blocks")
    ap.add_argument("--size", default="1024x1024")
    ap.add_argument("--salt", type=float, default=None, help="one salt map of this density instead of --maps")
    ap.add_argument("--queries", type=int, default=6)
    ap.add_argument("--corner", action="store_true", help="queries from the top-left to the bottom-right corner region")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    maps = ["salt%02d" % round(100 * a.salt)] if a.salt is not None else a.maps.split(",")
    res = {"tool": "tools/astar_lines_model.py", "is": "a CPU model of the step structure, not a measurement",
           "families": [run_family(m, W, H, a.queries, a.corner, seed=a.seed) for m in maps]}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
