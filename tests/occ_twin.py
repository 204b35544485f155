"""A numpy float32 restatement of the polygon rasterisation rule (include/sea_current_hip.h, sc_occ_from_polygons; the
successor header's occupancy_grid::rasterize), the worlds the tests and tools/occ_polygons_time.py run, and the text form
tests/cpp/rasterize_dump.cpp reads.  Every scalar is np.float32, so nothing widens to float64.

A world is dict(frame=(W, H, x_min, y_min, res_x, res_y), br=(x_max, x_min, y_max, y_min), grid_cells=int or 0,
obstacles=[dict(verts=float32 [n, 2], edges=None (polygon constructor) or [(i, j)], closed=bool)])."""
import numpy as np

F = np.float32


# ---- frames, the header's way ----------------------------------------------------------------------------------------
def frame_wh(br, W, H):
    """occupancy_grid(br, W, H): resolution = (x_max - x_min) / (float)W, ry = (y_max - y_min) / (float)H."""
    x_max, x_min, y_max, y_min = (F(v) for v in br)
    return (int(W), int(H), x_min, y_min, (x_max - x_min) / F(W), (y_max - y_min) / F(H))


def frame_cells(br, grid_cells):
    """planning_space::make_grid(): cells along the longer side = grid_cells."""
    x_max, x_min, y_max, y_min = (F(v) for v in br)
    wx, wy = x_max - x_min, y_max - y_min
    res = (wy if wx < wy else wx) / F(grid_cells)
    W, H = max(1, int(np.ceil(wx / res))), max(1, int(np.ceil(wy / res)))
    return frame_wh(br, W, H)


def world(br, obstacles, W=None, H=None, grid_cells=0):
    fr = frame_cells(br, grid_cells) if grid_cells else frame_wh(br, W, H)
    return dict(frame=fr, br=tuple(F(v) for v in br), grid_cells=int(grid_cells), obstacles=obstacles)


def poly(verts, closed=True):
    return dict(verts=np.asarray(verts, F).reshape(-1, 2), edges=None, closed=bool(closed))


def edge_list(verts, edges, closed=True):
    return dict(verts=np.asarray(verts, F).reshape(-1, 2), edges=[(int(i), int(j)) for i, j in edges], closed=bool(closed))


def flatten(obstacles):
    """-> lines float32 [E, 4], obs_off int32 [n+1], closed uint8 [n], box float32 [n, 4] (bound_rect order: the
    constructors' boxes, which start at vertices[0])."""
    lines, off, closed, box = [], [0], [], []
    for ob in obstacles:
        v = ob["verts"]
        if len(v) == 0:
            pairs = []
        elif ob["edges"] is None:
            pairs = [(i, (i + 1) % len(v)) for i in range(len(v))]
        else:
            pairs = ob["edges"]
        for i, j in pairs:
            lines.append(np.concatenate([v[i], v[j]]))
        used = [0] + [k for p in pairs for k in p] if len(v) else []
        if len(v):
            u = v[used] if ob["edges"] is not None else v
            box.append([u[:, 0].max(), u[:, 0].min(), u[:, 1].max(), u[:, 1].min()])
        else:
            box.append([0, 0, 0, 0])
        off.append(len(lines))
        closed.append(1 if ob["closed"] else 0)
    L = np.array(lines, F).reshape(-1, 4)
    return L, np.array(off, np.int32), np.array(closed, np.uint8), np.array(box, F).reshape(-1, 4)


# ---- the rule ----------------------------------------------------------------------------------------------------------
def _cell(v, lo, res, n):
    f = np.floor((np.asarray(v, F) - lo) / res)
    return np.clip(f, F(0), F(n - 1)).astype(np.int64)


def rasterize(frame, lines, obs_off, closed=None, box=None, base=None):
    """occ uint8 [H, W] of one grid (see the header comment of sc_occ_from_polygons)."""
    W, H, x_min, y_min, res_x, res_y = frame
    x_min, y_min, res_x, res_y = F(x_min), F(y_min), F(res_x), F(res_y)
    occ = np.zeros((H, W), np.uint8) if base is None else np.array(base, np.uint8).reshape(H, W).copy()
    lines = np.asarray(lines, F).reshape(-1, 4)
    hstep = F(0.5) * (res_y if res_y < res_x else res_x)
    for o in range(len(obs_off) - 1):
        L = lines[obs_off[o]:obs_off[o + 1]]
        if len(L) == 0:
            continue
        ax, ay, bx, by = L[:, 0], L[:, 1], L[:, 2], L[:, 3]
        if box is None:
            B = np.array([max(ax.max(), bx.max()), min(ax.min(), bx.min()), max(ay.max(), by.max()), min(ay.min(), by.min())], F)
        else:
            B = np.asarray(box[o], F)
        if closed is None or closed[o]:
            iy0, iy1 = int(_cell(B[3], y_min, res_y, H)), int(_cell(B[2], y_min, res_y, H))
            ix0, ix1 = int(_cell(B[1], x_min, res_x, W)), int(_cell(B[0], x_min, res_x, W))
            if iy0 <= iy1 and ix0 <= ix1:
                ix = np.arange(ix0, ix1 + 1)
                px = x_min + (ix.astype(F) + F(0.5)) * res_x
                cin = (px <= B[0]) & (px >= B[1])
                for r0 in range(iy0, iy1 + 1, 256):
                    iy = np.arange(r0, min(r0 + 256, iy1 + 1))
                    py = (y_min + (iy.astype(F) + F(0.5)) * res_y)[:, None]
                    cond = (ay > py) != (by > py)
                    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                        xi = ax + (py - ay) * (bx - ax) / (by - ay)
                    for r in range(len(iy)):
                        if not (py[r, 0] <= B[2] and py[r, 0] >= B[3]):
                            continue
                        xs = np.sort(xi[r][cond[r]])
                        cnt = len(xs) - np.searchsorted(xs, px, side="right")   # crossings with px < xi
                        occ[iy[r], ix[((cnt & 1) == 1) & cin]] = 1
        dx, dy = bx - ax, by - ay
        ln = np.sqrt(dx * dx + dy * dy)
        n = np.maximum(1, np.ceil(ln / hstep).astype(np.int64))
        e = np.repeat(np.arange(len(L)), n + 1)
        k = np.arange(len(e)) - np.repeat(np.cumsum(n + 1) - (n + 1), n + 1)
        t = k.astype(F) / n[e].astype(F)
        occ[_cell(ay[e] + dy[e] * t, y_min, res_y, H), _cell(ax[e] + dx[e] * t, x_min, res_x, W)] = 1
    return occ


def rasterize_world(w, base=None):
    L, off, cl, bx = flatten(w["obstacles"])
    return rasterize(w["frame"], L, off, cl, bx, base)


# ---- the text form of tests/cpp/rasterize_dump.cpp ---------------------------------------------------------------------
def write_worlds(path, worlds, outs):
    h = lambda v: float(F(v)).hex()
    with open(path, "w") as f:
        f.write(f"{len(worlds)}\n")
        for w, out in zip(worlds, outs):
            W, H = w["frame"][:2]
            f.write(f"{out}\n{w['grid_cells']} {W} {H} {' '.join(h(v) for v in w['br'])}\n{len(w['obstacles'])}\n")
            for ob in w["obstacles"]:
                ne = -1 if ob["edges"] is None else len(ob["edges"])
                f.write(f"{int(ob['closed'])} {len(ob['verts'])} {ne}\n")
                for x, y in ob["verts"]:
                    f.write(f"{h(x)} {h(y)}\n")
                for i, j in ob["edges"] or []:
                    f.write(f"{i} {j}\n")


def read_dump(path):
    raw = open(path, "rb").read()
    W, H = np.frombuffer(raw[:8], np.int32)
    return np.frombuffer(raw[8:], np.uint8).reshape(H, W)


# ---- worlds ------------------------------------------------------------------------------------------------------------
def examples_obstacles(s=1.0):
    """The reference examples' three obstacles (examples/test.cpp), scaled by s."""
    s = F(s)
    return [poly([(F(-0.5) * s, 0), (s, 0), (s, s), (0, s)]), poly([(0, F(-0.5) * s), (s, 0), (s, s), (0, s)]),
            poly([(F(-0.6) * s, F(0.148) * s), (-s, F(0.148) * s), (-s, 0), (F(-0.6) * s, 0)])]


def examples_world(cells=256):
    return world((1, -1, 1, -1), examples_obstacles(), grid_cells=cells)


def nondyadic_world(cells):
    """tests/cpp/test_waypoints.cpp's world: the examples' polygons scaled by 3 and an open two-vertex wall."""
    obs = examples_obstacles(3.0) + [edge_list([(-2.5, -2.0), (-0.5, -2.8)], [(0, 1)], closed=False)]
    return world((4.4, -3.3, 4.4, -3.3), obs, grid_cells=cells)


def polygon_world(W, n_poly=14, half=5.0, H=None):
    """sea_current_amd.synth.polygon_world on [-half, half]^2 at W x H cells."""
    from sea_current_amd import synth
    L, off = synth.polygon_world(n_poly, half)
    obs = [poly(L[off[o]:off[o + 1], :2]) for o in range(len(off) - 1)]
    return world((half, -half, half, -half), obs, W=W, H=H or W)


def ngon_world(n=2000, W=1024):
    a = np.arange(n) * (2 * np.pi / n)
    r = 3.0 + 0.8 * np.sin(7 * a)
    return world((5, -5, 5, -5), [poly(np.stack([r * np.cos(a), r * np.sin(a)], 1))], W=W, H=W)


def comb_world(teeth=200, W=1024):
    """One closed polygon with `teeth` vertical teeth: >= 2 * teeth crossings on every row through them."""
    xs = np.linspace(-4.5, 4.5, 2 * teeth + 1)
    v = [(xs[0], -4.5)]
    for i in range(teeth):
        v += [(xs[2 * i], 4.0), (xs[2 * i + 1], 4.0), (xs[2 * i + 1], -4.0), (xs[2 * i + 2], -4.0)]
    v[-1] = (xs[-1], -4.5)
    return world((5, -5, 5, -5), [poly(v)], W=W, H=W)


def left60_world(W, H=None):
    """One filled rectangle over the left 60 % of [-5, 5]^2 (polygon_world's frame), the right side empty: the EDT's
    open-space build with more than 508 obstacle columns a row at widths of 850 .. 1024."""
    return world((5, -5, 5, -5), [poly([(-5.1, -5.1), (1.0, -5.1), (1.0, 5.1), (-5.1, 5.1)])], W=W, H=H or W)


def special_worlds():
    """name -> world: the examples, the non-dyadic world, the polygon world, a non-square frame, the 2000-gon, the comb,
    a bow-tie, an edge-list obstacle with an unreferenced vertex 0, horizontal and zero-length edges, vertices on cell-centre
    lines, obstacles partly or fully outside the frame."""
    out = dict(examples=examples_world(), nondyadic_300=nondyadic_world(300), nondyadic_1024=nondyadic_world(1024),
               poly14_1024=polygon_world(1024), ngon2000=ngon_world(), comb200=comb_world())
    out["nonsquare"] = world((3.7, -1.1, 2.3, -0.9), examples_obstacles(1.3) + polygon_world(64, 6, 1.2)["obstacles"], W=517, H=211)
    out["bowtie"] = world((1, -1, 1, -1), [poly([(-0.8, -0.7), (0.8, 0.7), (0.8, -0.7), (-0.8, 0.7)])], W=301, H=257)
    out["edgelist_unref_v0"] = world((2, -2, 2, -2), [
        edge_list([(-1.9, 1.9), (-1.0, -1.0), (1.0, -0.5), (0.2, 1.2)], [(1, 2), (2, 3), (3, 1)]),
        edge_list([(1.5, -1.8), (-1.5, -1.2), (-0.3, 0.1)], [(1, 2)], closed=False)], W=333, H=333)
    fr = frame_wh((1, -1, 1, -1), 200, 160)
    cy = lambda i: fr[3] + (F(i) + F(0.5)) * fr[5]      # cell-centre lines
    cx = lambda i: fr[2] + (F(i) + F(0.5)) * fr[4]
    out["degenerate_edges"] = world((1, -1, 1, -1), [
        poly([(-0.9, 0.2), (-0.1, 0.2), (-0.1, 0.6), (-0.9, 0.6)]),                  # horizontal edges
        poly([(0.3, 0.3), (0.3, 0.3), (0.7, 0.35), (0.5, 0.8), (0.5, 0.8)]),          # zero-length edges
        edge_list([(0.1, -0.5), (0.1, -0.5)], [(0, 1)], closed=False),                # a point
        poly([(0.3, -0.9), (0.6, -0.9)])], W=200, H=160)                             # a two-vertex closed "polygon"
    out["centre_lines"] = world((1, -1, 1, -1), [
        poly([(cx(20), cy(30)), (cx(80), cy(30)), (cx(80), cy(90)), (cx(50), cy(120)), (cx(20), cy(90))]),
        poly([(cx(100), cy(10)), (cx(150), cy(60)), (cx(120), cy(60)), (cx(170), cy(140))]),
        edge_list([(cx(5), cy(5)), (cx(190), cy(150))], [(0, 1)], closed=False)], W=200, H=160)
    out["outside"] = world((1, -1, 1, -1), [
        poly([(-1.5, -0.2), (-0.5, -0.3), (-0.6, 0.4)]), poly([(0.8, 0.8), (1.6, 0.9), (1.2, 1.7)]),
        poly([(2.0, 2.0), (3.0, 2.0), (3.0, 3.0)]), poly([(-3.0, -0.1), (-2.0, -0.1), (-2.5, 0.1)]),
        edge_list([(-2.0, 0.5), (2.0, 0.7)], [(0, 1)], closed=False), poly([(-1.2, -1.2), (1.2, -1.2), (1.2, 1.2), (-1.2, 1.2)])],
        W=128, H=96)
    return out


def random_world(seed):
    """W, H in 1 .. 1100 (a few 4096 and 8192 wide), 0 .. 40 obstacles of 0 .. 12 edges, open and closed, polygon and
    edge-list constructors, some vertices on cell-centre lines, some obstacles past the frame."""
    rng = np.random.default_rng(seed)
    if seed % 60 == 7:
        W, H = int(rng.choice([4096, 8192])), int(rng.integers(1, 48))
    else:
        W, H = int(rng.integers(1, 1101)), int(rng.integers(1, 1101))
    x0, y0 = F(rng.uniform(-20, 20)), F(rng.uniform(-20, 20))
    sx = F(rng.uniform(0.5, 30))
    sy = sx if rng.random() < 0.5 else F(rng.uniform(0.5, 30))
    br = (x0 + sx, x0, y0 + sy, y0)
    fr = frame_wh(br, W, H)
    obs = []
    for _ in range(int(rng.integers(0, 41))):
        ne = int(rng.integers(0, 13))
        c = np.array([rng.uniform(x0 - 0.2 * sx, x0 + 1.2 * sx), rng.uniform(y0 - 0.2 * sy, y0 + 1.2 * sy)])
        rad = rng.uniform(0.0, 0.4) * np.array([sx, sy], np.float64)
        v = (c + rad * rng.uniform(-1, 1, (max(ne, 1), 2))).astype(F)
        if rng.random() < 0.3:                           # snap some vertices onto cell-centre lines
            m = rng.random(len(v)) < 0.5
            v[m, 1] = fr[3] + (F(int(rng.integers(0, H))) + F(0.5)) * fr[5]
        closed = rng.random() < 0.7
        if ne == 0:
            obs.append(poly(np.zeros((0, 2), F), closed))
        elif rng.random() < 0.6:
            obs.append(poly(v, closed))
        else:
            v = np.concatenate([(c + rad * rng.uniform(-1.5, 1.5, 2)).astype(F)[None], v])   # vertex 0 maybe unused
            obs.append(edge_list(v, [(int(rng.integers(0, len(v))), int(rng.integers(1, len(v)))) for _ in range(ne)], closed))
    return world(br, obs, W=W, H=H)
