"""Every grid entry at the dimension limit of include/sea_current_hip.h (W, H <= SC_MAX_DIM = 8192): the cases of
tests/test_limit_cases.py (the conditions on the reference, no GPU) and tests/test_gpu_limit.py (the comparison).

The grids are strips, SHAPES as W x H: the limit on either axis (72 = two 32-cell tiles + 8) and one that crosses 4096 with a
partial tile of four cells.  A strip has few cells and every coordinate bit in play.  The chains are those of
tests/stream_cases.py with other inputs: what the kernels read out (starts, goals, roots, seeds, targets, robots, views, discs,
scan origins, match centres) is drawn from the far window, the last FAR cells of the long axis, so that the queries end Q_OK
inside Lmax = 512, and per chain and shape some of it is pinned: on the last line L - 1 of the long axis (or within the
family's margin of it), on the far corner cell W * H - 1, and, on the 8192 strips, on either side of 4095 | 4096 from a second
window around 4096.  Fields, owner maps, labels, known, d2 and log-odds maps are compared over the whole strip.  These chains
are not in stream_cases.CHAINS: the gated stream tests do not grow.
"""
import numpy as np

import stream_cases as sc_cases
from stream_cases import Q_BAD_ENDPOINT, Q_NO_PATH, Q_OK, Q_TRUNCATED, _rng, _salt_occ

SHAPES = [(8192, 72), (72, 8192), (4100, 70)]
FAR, MID = 384, 4096
SMOOTH_OK = sc_cases.SMOOTH_OK


class Strip:
    """A W x H grid by its long axis (coordinate l in 0 .. L - 1) and its short one (s in 0 .. S - 1)."""

    def __init__(self, W, H):
        self.W, self.H, self.xlong = W, H, W >= H
        self.L, self.S = max(W, H), min(W, H)
        self.mid = MID if self.L > MID + FAR else None           # the 8192 strips: a second window around 4095 | 4096
        self.corner = W * H - 1

    def cell(self, l, s):
        return int(s * self.W + l if self.xlong else l * self.W + s)

    def long(self, c):
        c = np.asarray(c)
        return c % self.W if self.xlong else c // self.W

    def band(self, lo, hi, margin=0):
        """bool [H,W]: long coordinate in lo .. hi - 1, short coordinate `margin` cells inside the grid."""
        m = np.zeros((self.S, self.L), bool)
        m[margin:self.S - margin, max(lo, 0):min(hi, self.L)] = True
        return m if self.xlong else m.T.copy()

    def far(self, margin=0):
        return self.band(self.L - FAR, self.L - margin, margin)

    def middle(self, margin=0):
        return self.band(MID - FAR // 2, MID + FAR // 2, margin)

    def window(self, k, margin=0):
        """Window k of a chain that takes two: 0 the far one, 1 the one around 4096 where the strip has it."""
        return self.middle(margin) if k == 1 and self.mid else self.far(margin)

    def clear(self, occ, l0, l1, s, m=0):
        """Frees the corridor l0 .. l1 at short coordinate s, m cells wide on every side."""
        a = occ if self.xlong else occ.T
        a[max(s - m, 0):s + m + 1, max(l0 - m, 0):l1 + m + 1] = 0

    def pick(self, rng, mask, n, replace=True):
        return rng.choice(np.flatnonzero(np.asarray(mask).ravel()), n, replace=replace).astype(np.int32)

    def pairs(self, occ=None, m=0):
        """The pinned (start, goal) pairs: to the far corner along the last short line (the border of _salt_occ is free), and on
        the 8192 strips across 4095 | 4096 through a corridor cleared in occ."""
        L, S = self.L, self.S
        out = [(self.cell(L - 40, S - 1), self.corner)]
        if occ is not None and m:
            self.clear(occ, L - 40, L - 1, S - 1, m)
        if self.mid:
            out.append((self.cell(MID - 16, S // 2), self.cell(MID + 14, S // 2)))
            if occ is not None:
                self.clear(occ, MID - 16, MID + 14, S // 2, m)
        return out


def _spoil(rng, c, lo, W, H):
    """Two cells outside the grid at positions from lo on that depend on the draw."""
    c[lo + rng.choice(len(c) - lo, 2, replace=False)] = [-1, W * H]
    return c


class Limit:
    """A chain of stream_cases on a strip: same calls, same twins, inputs of its own."""
    readouts = ()
    edge_margin = 0          # how close to L - 1 a path of this family can come (a footprint keeps its extent away from the border)

    def __init__(self, W, H):
        self.W, self.H, self.strip = W, H, Strip(W, H)
        self.name = f"{type(self).name} {W}x{H}"

    def queries(self, o):
        """{read-out: (status, len, path)} of an expected view: what the share and edge conditions are checked on."""
        return {p: (o[p + "status"], o[p + "len"], o[p + "path"]) for p in self.readouts}


# ---- chain 1 -------------------------------------------------------------------------------------------------------------------
class Grids(Limit, sc_cases.Grids):
    Q, Lmax = 24, 512
    readouts = ("a_",)

    def __init__(self, W, H):
        Limit.__init__(self, W, H)
        self.frame = (-0.05 * W, -0.05 * H, 0.1, 0.1)

    def inputs(self, which):
        """`wide`, the chain's second EDT input (there a grid of 1100 cells a row), is a sparse strip of the same shape here."""
        st, rng = self.strip, _rng(which, 21)
        L, S, k, lines = st.L, st.S, 5, []
        lat = np.arange(20, L - 20, 40)                               # small obstacles all along the strip: the oracle's nearest-obstacle search
        per = 8 + 2 * len(lat)                                       #   takes time with the distance; then eight larger ones per grid
        for _ in range(self.G):
            c_long = np.concatenate([[L - 3.0], rng.uniform(L - FAR + 10, L - 12, 4), [MID, MID - 20.5, MID + 17.0] if st.mid else
                                     rng.uniform(L - FAR + 10, L - 12, 3), np.repeat(lat, 2) + rng.uniform(-8, 8, 2 * len(lat))])
            c_short = np.concatenate([rng.uniform(14, S - 14, 8), np.tile([S / 4, 3 * S / 4], len(lat)) + rng.uniform(-5, 5, 2 * len(lat))])
            for i in range(per):                                     # star-shaped pentagons, kept off the two border lines of the short axis
                c = (np.array([c_long[i], c_short[i]]) if st.xlong else np.array([c_short[i], c_long[i]])) * 0.1 + np.array(self.frame[:2])
                a = np.sort(rng.uniform(0, 2 * np.pi, k))
                v = c + rng.uniform(*((0.3, 0.9) if i < 8 else (0.15, 0.4)), k)[:, None] * np.stack([np.cos(a), np.sin(a)], 1)
                lines += [np.concatenate([v[j], v[(j + 1) % k]]) for j in range(k)]
        n_obs = per * self.G
        r_long = np.concatenate([rng.integers(L - FAR, L + 2, 4), rng.integers(MID - 12, MID + 1, 2) if st.mid else rng.integers(L - 12, L + 2, 2)])
        r_short = rng.integers(-4, S, 6)
        rects = np.stack([r_long, r_short] if st.xlong else [r_short, r_long], 1)
        rects = np.concatenate([rects, rects + rng.integers(1, 12, (6, 2))], 1).astype(np.int32)
        inner = st.far(2)                                            # the two outer lines stay for the pins
        start, goal = st.pick(rng, inner, self.Q), st.pick(rng, inner, self.Q)
        qgrid = rng.integers(0, self.G, self.Q).astype(np.int32)
        pins = [(st.cell(L - 40, S - 1), st.corner)] + ([(st.cell(MID - 16, 1), st.cell(MID + 14, S - 2))] if st.mid else [])
        for i, (s, g) in enumerate(pins + pins):                     # every pin on either grid
            start[i], goal[i], qgrid[i] = s, g, (i // len(pins)) % self.G
        n = 2 * len(pins)
        return dict(lines=np.array(lines, np.float32), obs_off=(k * np.arange(n_obs + 1)).astype(np.int32),
                    grid_off=np.array([0, per, n_obs], np.int32), wide=_salt_occ(self.W, self.H, 0.02, which, 33), rects=rects, qgrid=qgrid,
                    start=_spoil(rng, start, n, self.W, self.H), goal=_spoil(rng, goal, n, self.W, self.H))


# ---- chain 4 -------------------------------------------------------------------------------------------------------------------
class Components(Limit, sc_cases.Components):
    readouts = ("a_",)
    salt = 4          # a set outside the bounds of test_limit_cases.py gets another seed here, the bounds stay

    def inputs(self, which):
        st, rng = self.strip, _rng(which, 24)
        occ = _salt_occ(self.W, self.H, 0.41, which, self.salt)
        occ[0, :"ABC".index(which)] = 1
        pins = st.pairs(occ)
        pins.append((st.cell(st.L - 60, st.S // 3), st.cell(st.L - 1, st.S // 3)))      # through the salt to the last line
        st.clear(occ, st.L - 60, st.L - 1, st.S // 3)
        free = st.far() & (occ == 0)
        start, goal = st.pick(rng, free, self.Q), st.pick(rng, free, self.Q)
        for i, (s, g) in enumerate(pins):
            start[i], goal[i] = s, g
        return dict(occ=occ, start=_spoil(rng, start, len(pins), self.W, self.H), goal=_spoil(rng, goal, len(pins), self.W, self.H))


def _rooted(chain, which, occ, rng, fits=None):
    """Roots and targets of a family of F = 3 fields, one of them blocked (another one in every set): the first open field in the
    far window with its root on (or within the family's margin of) the last line, the second around 4096 where the strip has it, with a
    target across 4095 | 4096; the far corner is a target of the first."""
    st, F, Q = chain.strip, chain.F, chain.Q
    ok = (occ == 0) if fits is None else fits
    bad = "ABC".index(which)
    good = [k for k in range(F) if k != bad]
    win = {good[0]: 0, good[1]: 1, bad: 0}
    roots = np.array([st.pick(rng, st.window(win[k]) & ok, 1)[0] for k in range(F)], np.int32)
    roots[bad] = np.flatnonzero((st.far() & (occ != 0)).ravel())[0]
    last = np.flatnonzero((st.far() & ok).ravel())
    roots[good[0]] = last[np.argmax(st.long(last))]
    assert st.long(roots[good[0]]) >= st.L - 1 - chain.edge_margin
    qfield = np.array(good, np.int32)[rng.integers(0, 2, Q)]
    qfield[rng.choice(np.arange(4, Q), 2, replace=False)] = bad
    targets = np.array([st.pick(rng, st.window(win[k]) & ok, 1)[0] for k in qfield], np.int32)
    targets[0], qfield[0] = st.corner, good[0]
    targets[1], qfield[1] = last[np.argsort(st.long(last))[-2]], good[0]
    if st.mid:
        def near(l):
            c = np.flatnonzero((st.band(l - 6, l + 7, 8) & ok).ravel())
            return c[np.argmin(np.abs(st.long(c) - l))]
        roots[good[1]] = near(MID - 16)
        targets[2], qfield[2] = near(MID + 14), good[1]
        assert st.long(roots[good[1]]) < MID <= st.long(targets[2])
    return roots, _spoil(rng, targets, 4, chain.W, chain.H), qfield, good, bad, win


# ---- chain 5 -------------------------------------------------------------------------------------------------------------------
class Fields(Limit, sc_cases.Fields):
    readouts = ("p_", "pw_", "pm_")
    seed = 28
    R = 2          # fewer robots than open fields: every row is matched, so the row potentials differ between the sets

    def inputs(self, which):
        st, rng = self.strip, _rng(which, self.seed)
        occ = _salt_occ(self.W, self.H, 0.15, which, 25)
        if st.mid:
            st.clear(occ, MID - 22, MID + 20, st.S // 2, 3)
        roots, targets, qfield, good, bad, win = _rooted(self, which, occ, rng)
        free, blocked = occ == 0, np.flatnonzero((st.far() & (occ != 0)).ravel())
        seeds = np.concatenate([st.pick(rng, st.window(win[k]) & free, 2, replace=False) for k in range(self.F)])
        seeds[2 * bad:2 * bad + 2] = blocked[1:3]
        seeds[2 * good[0]] = st.cell(st.L - 1, 2 * st.S // 3)        # a seed on the last line
        return dict(occ=occ, roots=roots, seeds=seeds, seed_off=self.seed_off, seed_cost=rng.integers(0, 300, 6).astype(np.int32),
                    targets=targets, qfield=qfield, robots=st.pick(rng, st.far() & free, self.R), col_cost=rng.integers(0, 50, self.F).astype(np.int32))


# ---- chain 6 -------------------------------------------------------------------------------------------------------------------
class Explore(Limit, sc_cases.Explore):
    seed = 28
    def inputs(self, which):
        import frontier_twin as ft
        st, rng = self.strip, _rng(which, self.seed)
        L, S = st.L, st.S
        occ = _salt_occ(self.W, self.H, 0.05, which, 26)
        d_long = [L - 16, int(rng.integers(L - FAR + 15, L - 40)), MID - 3 if st.mid else int(rng.integers(L - FAR + 15, L - 40))]
        d_short = rng.integers(15, S - 15, 3)
        discs = np.stack([d_long, d_short] if st.xlong else [d_short, d_long], 1)
        discs = np.concatenate([discs, rng.integers(100, 500, (3, 1))], 1).astype(np.int32)
        discs[0, 2] = rng.integers(260, 500)                         # 16 cells and more: over the last line
        ok = (ft.known_from_discs(None, discs, self.W, self.H) != 0) & (occ == 0)
        ok[[0, -1], :] = ok[:, [0, -1]] = False
        roots = st.pick(rng, ok & st.far(), self.F, replace=False)
        for r in roots[:"ABC".index(which)]:
            occ.ravel()[[r - 1, r + 1, r - self.W, r + self.W]] = 1
        return dict(occ=occ, discs=discs, roots=roots)


# ---- chain 7 -------------------------------------------------------------------------------------------------------------------
class Views(Limit, sc_cases.Views):
    def inputs(self, which):
        import sectors_twin
        st, rng = self.strip, _rng(which, 27)
        occ = _salt_occ(self.W, self.H, 0.04, which, 27)
        pins = [st.cell(st.L - 1, st.S // 2), st.corner] + ([st.cell(MID, st.S // 3), st.cell(MID - 1, st.S // 3 + 9)] if st.mid else [])
        occ.ravel()[pins] = 0
        cells = st.pick(rng, st.far() & (occ == 0), self.N, replace=False)
        cells[:len(pins)] = pins                                     # among the four views that are applied
        cells[int(rng.integers(4, self.N))] = self.W * self.H
        views = sectors_twin.views_from_cells(cells, self.W, self.H, self.r2)
        return dict(occ=occ, cells=cells, sviews=sectors_twin.sector_views(views, self.dirs(), rng.integers(0, 8, self.N), self.span))


# ---- chain 8 -------------------------------------------------------------------------------------------------------------------
class Scan(Limit, sc_cases.Scan):
    seed = 29
    S = 3          # a scan inside the far window, one whose fan ends on the last line, one whose rays leave the grid

    def inputs(self, which):
        import scan_twin
        st, rng = self.strip, _rng(which, self.seed)
        occ = _salt_occ(self.W, self.H, 0.05, which, 28)
        at = [int(st.pick(rng, st.band(st.L - FAR + 25, st.L - 60, 25) & (occ == 0), 1)[0]),
              st.cell(st.L - 1 - self.r, int(rng.integers(25, st.S - 25))), st.cell(st.L - 1 - self.r // 2, int(rng.integers(25, st.S - 25)))]
        at = np.array(at)
        occ.ravel()[at] = 0
        rays = np.concatenate([scan_twin.square_fan(int(c % self.W), int(c // self.W), self.r) for c in at])
        centre = np.stack([at % self.W, at // self.W], 1) + rng.integers(-3, 4, (self.S, 2))
        return dict(occ=occ, rays=rays.astype(np.int32), centre=centre.astype(np.int32))


# ---- chain 9 -------------------------------------------------------------------------------------------------------------------
class Pose(Limit, sc_cases.Pose):
    readouts = ("pp_",)
    edge_margin = 3          # a footprint that fits in all eight headings keeps front = 2 cells (three on a diagonal) off the border

    def inputs(self, which):
        import pose_twin
        st, rng = self.strip, _rng(which, 29)
        occ = _salt_occ(self.W, self.H, 0.05, which, 29)
        fits = pose_twin.footprint_mask(pose_twin.d2_of(occ), *self.foot) == 0xFF
        roots, targets, qfield, good, bad, win = _rooted(self, which, occ, rng, fits)
        return dict(occ=occ, roots=roots, rhead=rng.integers(-1, 8, self.F).astype(np.int32), targets=targets,
                    thead=rng.integers(-1, 8, self.Q).astype(np.int32), qfield=qfield)


# ---- chain 2, the grid half ------------------------------------------------------------------------------------------------------
class Smooth(Limit, sc_cases.Smooth):
    """EDT -> A* -> waypoints -> points, then what the smoothing calls ask of the grid: the speed limits with d2, the clearance of
    the curves and their repair.  The time parametrisation and the samples (no grid in them) stay with chain 2 of stream_cases; the
    legs are taken as the checked run wrote them (staged), so no float32 tolerance is stretched to coordinates of 400 m."""
    readouts = ("a_",)
    Wmax = 48
    tol = {k: v for k, v in sc_cases.Smooth.tol.items() if k.split("_")[-1] not in ("ctrl", "pos", "vel", "pts", "curvature")}
    KEYS = ("d2", "npts", "wp", "cum", "sl_vmax_stage", "sl_min_clear", "sp_vhi", "sp_min_clear", "sp_status", "cc_leg_min", "cc_path_min", "cc_hit_legs",
            "cc_hit_leg", "cc_hit_t", "cl_rounds", "cl_status", "cl_leg_min", "cl_ctrl", "cl_level", "sc_rounds", "sc_level", "sc_leg_min", "sc_ctrl",
            "w_n", "w_status", "w_wp", "a_status", "a_len", "a_cost", "a_path")

    def inputs(self, which):
        st, rng = self.strip, _rng(which, 22)
        occ = _salt_occ(self.W, self.H, 0.04, which, 22)
        pins = st.pairs(occ)
        free = st.far() & (occ == 0)
        start, goal = st.pick(rng, free, self.P), st.pick(rng, free, self.P)
        for i, (s, g) in enumerate(pins):
            start[i], goal[i] = s, g
        start[int(rng.integers(len(pins), self.P))] = -1
        pairs = np.array([(1.0, 0.5), (0.6, 0.3), (1.5, 1.0), (0.4, 0.8)])[rng.integers(0, 4, self.P)]
        lim = np.stack([-pairs[:, 0], pairs[:, 0], -pairs[:, 1], pairs[:, 1]], 1)
        inf = float("inf")
        return dict(occ=occ, start=start, goal=goal, lim=lim, dyn=np.tile(np.array(self.dyn), (self.P, 1)), dyn_off=np.tile(np.array([inf, inf, inf, 0.0]), (self.P, 1)))

    def _form(self, out, pre, tw, inp, pts, npts, d2, up, legs0, cum_key, dyn=None, status=None):
        """Smooth._form without the time parametrisation: legs, offsets, lengths, status, and with dyn the limits of every stage."""
        import speed_twin
        o, P, S = tw.oracle, self.P, self.P * (self.Wmax - 1)
        ok = npts >= 2
        st = np.where(ok, SMOOTH_OK, sc_cases.SMOOTH_BAD_INPUT).astype(np.int32) if status is None else status
        seg_off = np.concatenate([[0], np.cumsum(np.where(ok, npts - 1, 0))]).astype(np.int32)
        ctrl, arcl = np.zeros((S, 4, 2), np.float32), np.zeros(P, np.float32)
        vmax, minc = np.ones((P, self.N + 1)), np.zeros(P, np.float32)
        for p in np.flatnonzero(ok):
            a, b = seg_off[p], seg_off[p + 1]
            ctrl[a:b] = o.bezier_from_path(pts[p, :npts[p]]) if legs0 is None else legs0[a:b]
            if st[p] != SMOOTH_OK:
                continue
            legs = ctrl[a:b] if up is None else np.asarray(up[pre + "ctrl"])[a:b]
            tot, c64 = o.bezier_arclength(legs, self.nsub)
            cum = c64.astype(np.float32) if up is None else np.asarray(up[cum_key])[a:b]
            arcl[p] = tot
            AL = np.float32(cum[:, -1].astype(np.float32).cumsum(dtype=np.float32)[-1]) if up is None else np.asarray(up[pre + "arclength"])[p]
            if dyn is not None:
                t = speed_twin.speed_limits(legs, cum, AL, inp["lim"][p], dyn, N=self.N, J=self.J, d2=d2, frame=self.frame)
                assert not t["flagged"].any()
                vmax[p], minc[p] = t["vhi"], np.float32(t["min_clear"])
        out.update({pre + "ctrl": ctrl, pre + "seg_off": seg_off, pre + "arclength": arcl, pre + "status": st})
        return seg_off, st, vmax, minc

    def view(self, o):
        S_used = int(np.asarray(o["sm_seg_off"])[-1])
        out = {k: np.asarray(o[k]) for k in self.KEYS if k[:2] not in ("a_", "w_")}
        out.update(sc_cases.paths_view(sc_cases._sub(o, "a_"), "a_"))
        n, st = np.asarray(o["w_n"]), np.asarray(o["w_status"])
        out.update(w_n=n, w_status=st, w_wp=np.where((np.arange(self.Wmax)[None, :] < n[:, None]) & (st == Q_OK)[:, None], np.asarray(o["w_wp"]), -1))
        out["wp"] = np.where((np.arange(self.Wmax)[None, :] < out["npts"][:, None])[:, :, None], np.asarray(o["wp"]), 0)
        legs = lambda a, n: np.where((np.arange(len(a)) < n).reshape((-1,) + (1,) * (a.ndim - 1)), a, 0)
        out["cum"] = legs(out["cum"], S_used)
        for k in ("cl_ctrl", "sc_ctrl", "sc_leg_min"):
            out[k] = legs(out[k], S_used)
        for k in ("cl_level", "sc_level"):
            out[k] = legs(out[k], S_used + self.P)
        for f in self.forms:
            for k in ("seg_off", "status"):
                out[f + k] = np.asarray(o[f + k])
            out[f + "arclength"] = np.where(out[f + "status"] == SMOOTH_OK, np.asarray(o[f + "arclength"]), 0)
        return out


FAMILIES = [Grids, Smooth, Components, Fields, Explore, Views, Scan, Pose]
_MADE = {}


def chain(family, shape):
    """The one instance of a family on a shape: its expected values are computed once and shared."""
    if (family, shape) not in _MADE:
        _MADE[family, shape] = family(*shape)
    return _MADE[family, shape]


CASES = [(f, s) for f in FAMILIES for s in SHAPES]
case_id = lambda c: f"{c[0].name.split()[1]}-{c[1][0]}x{c[1][1]}" if isinstance(c, tuple) else None

# the device entries of the header that take no W, H: out of reach of a grid's size
NO_GRID = {"sc_toppra_hermite_batch", "sc_toppra_sample_batch", "sc_bezier_from_path_batch", "sc_bezier_resample_batch", "sc_bezier_eval_batch",
           "sc_bezier_curve_batch", "sc_bezier_shrink_tangent_batch", "sc_chebfit_batch", "sc_chebeval_batch", "sc_fmt_star_batch", "sc_gather_pack",
           "sc_gather_unpack", "sc_traj_knots_batch", "sc_traj_conflicts_batch", "sc_fleet_conflicts_batch", "sc_traj_shift_table_batch",
           "sc_traj_schedule_batch", "sc_traj_shift_knots_batch", "sc_fleet_schedule_batch"}
# what tplan_case runs beside the chains (sc_fleet_replan_batch is how its builder calls the two)
TPLAN_SYMBOLS = {"sc_traj_reserve_batch", "sc_tplan_batch", "sc_fleet_replan_batch"}


def covered_symbols():
    return set().union(*(f.symbols for f in FAMILIES)) | TPLAN_SYMBOLS


# ---- what the conditions of test_limit_cases.py are read from --------------------------------------------------------------------
def counts(status):
    """(valid, Q_OK, Q_NO_PATH, Q_TRUNCATED) of a status array: valid = the endpoints were accepted."""
    status = np.asarray(status)
    return tuple(int(v) for v in ((status != Q_BAD_ENDPOINT).sum(), (status == Q_OK).sum(), (status == Q_NO_PATH).sum(), (status == Q_TRUNCATED).sum()))


def path_reach(strip, status, ln, path, margin=0):
    """(a Q_OK path has a cell on the last line L - 1 less margin, a Q_OK path has cells on both sides of 4095 | 4096)."""
    edge = cross = False
    for q in np.flatnonzero(np.asarray(status) == Q_OK):
        l = strip.long(np.asarray(path)[q, :ln[q]])
        edge |= bool((l >= strip.L - 1 - margin).any())
        cross |= bool((l < MID).any() and (l >= MID).any())
    return edge, cross


# ---- A* rounds on a fixed strip ------------------------------------------------------------------------------------------------------
ASTAR_Q, ASTAR_LMAX = 96, 512


def astar_limit_case(oracle, rng, W, H, fam=None, nthreads=8):
    """One map on the strip (salt 0.15 .. 0.35, or sparse salt and walls with gaps across the short axis), a clearance r2 of 0, 1 or 4, and
    ASTAR_Q queries between traversable cells of the far window with the pins of Strip.pairs; the oracle's results."""
    from sea_current_amd import synth
    st = Strip(W, H)
    fam = int(rng.integers(0, 2)) if fam is None else fam
    if fam == 0:
        occ = synth.salt_grid(W, H, float(rng.uniform(0.15, 0.35)), seed=int(rng.integers(1 << 30)))
        r2 = int(rng.choice([0, 1]))
    else:
        occ = synth.salt_grid(W, H, 0.03, seed=int(rng.integers(1 << 30)))
        a = occ if st.xlong else occ.T
        r2 = int(rng.choice([0, 1, 4]))
        w = 4 if r2 > 1 else 2                                       # a gap stays open under the clearance
        for l in range(4, st.L - 4, int(rng.integers(5, 17))):
            a[1:st.S - 1, l] = 1
            for _ in range(2):
                s = int(rng.integers(w + 1, st.S - w - 1))
                a[s - w:s + w + 1, l] = 0
    m = 2 if r2 > 1 else 0                                           # d2 >= 4: two cells of clearance around a pin
    pins = st.pairs(occ, m)
    d2 = oracle.edt(occ)
    trav = (d2 >= max(r2, 1)) & st.far()
    s, g = st.pick(rng, trav, ASTAR_Q), st.pick(rng, trav, ASTAR_Q)
    for i, (a_, b_) in enumerate(pins + [(b, a) for a, b in pins]):  # either direction: the start and the goal of a query are not popped alike
        s[i], g[i] = a_, b_
    ref = oracle.astar_batch(d2, s, g, r2=r2, Lmax=ASTAR_LMAX, nthreads=nthreads)
    return dict(W=W, H=H, fam=fam, r2=r2, d2=d2, start=s, goal=g, ref=ref)


def astar_limit_round(ctx, oracle, rng, W, H, fam=None):
    """stress_cases.astar_round's comparison on a fixed strip: status, cost, len, path and the number of nodes every search expanded;
    then sc_astar_gfield of one far-window query against the oracle's field, as test_gpu_astar.py::test_astar_gfield_bit_exact does."""
    import torch
    from stress_cases import _t
    c = astar_limit_case(oracle, rng, W, H, fam, nthreads=16)
    ref, d2, s, g, r2 = c["ref"], c["d2"], c["start"], c["goal"], c["r2"]
    d2g = _t(d2)
    out = ctx.astar_batch(d2g, _t(s), _t(g), r2=r2, Lmax=ASTAR_LMAX)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    tag = (W, H, c["fam"], r2)
    for k in ("status", "cost", "len"):
        bad = np.flatnonzero(got[k] != ref[k])
        assert bad.size == 0, (tag, k, bad[:8].tolist(), got[k][bad[:8]].tolist(), ref[k][bad[:8]].tolist())
    for q in np.flatnonzero(ref["status"] == Q_OK):
        assert np.array_equal(got["path"][q, :ref["len"][q]], ref["path"][q, :ref["len"][q]]), (tag, "path", q)
    ex = ctx.astar_debug_stats(ASTAR_Q)[0]
    bad = np.flatnonzero(ex != ref["expanded"])
    assert bad.size == 0, ("expansion counts differ", tag, bad[:8].tolist(), ex[bad[:8]].tolist(), ref["expanded"][bad[:8]].tolist())
    q = int(np.flatnonzero(ref["status"] == Q_OK)[-1])                # past the pins: a random query of the far window
    one = oracle.astar(d2, s[q], g[q], r2=r2, want_g=True)
    gf, cost, status = ctx.astar_gfield(d2g, s[q], g[q], r2=r2)
    assert status == one["status"] and cost == one["cost"], (tag, q)
    yy, xx = np.divmod(np.arange(W * H), W)
    dx, dy = np.abs(xx - g[q] % W), np.abs(yy - g[q] // W)
    h = (10 * np.maximum(dx, dy) + 4 * np.minimum(dx, dy)).reshape(H, W)
    inE = (one["g"] != 0xFFFFFFFF) & (one["g"].astype(np.int64) + h <= one["cost"])
    assert inE.sum() == one["expanded"], (tag, q)
    assert np.array_equal(gf[inE], one["g"][inE]) and np.all(gf[~inE] >= one["g"][~inE]), (tag, q, "gfield")
    return c


def astar_rng(W, H):
    """The generator of a shape's rounds: the same maps for the CPU conditions and for every A* build."""
    return np.random.default_rng(8192 * W + H)


# ---- space-time planning on strips three cells wide ------------------------------------------------------------------------------------
TPLAN_SHAPES = [(8192, 3), (3, 8192)]


def tplan_case(W, H, L=24, P=3, B=10):
    """The case of test_gpu_tplan.py::test_word_and_tile_edges (its builder: salt, knot rows, radii, t_start) with the robots and
    the reserved motions in the far window: one motion stands on the last cell, one robot ends three cells from it, one crosses 4095 | 4096."""
    import tplan_twin as tw
    from test_gpu_tplan import make_case
    st = Strip(W, H)
    c = make_case(W, H, L, P=P, B=B)
    rng = np.random.default_rng(1000 * W + H + 1)
    frame = c["frame"]
    cx, cy = tw.centres(W, H, frame)
    cl, res_l = (cx, frame[2]) if st.xlong else (cy, frame[3])
    ax = 0 if st.xlong else 1
    first = np.array([k[np.isfinite(k[:, ax])][0, ax] for k in c["knots"]])
    c["knots"][:, :, ax] += (rng.uniform(cl[st.L - FAR], cl[st.L - 1], P) - first)[:, None]      # the same motions, moved along the strip
    c["knots"][0] = (cx[-1], cy[-1])                                  # stands on W * H - 1 throughout
    free = c["d2"].ravel() != 0
    for l in (st.L - 4, st.L - 12, MID - 5, MID + 4):
        free[st.cell(l, 1)] = True
    c["d2"] = free.reshape(H, W).astype(np.int32)
    start = rng.choice(np.flatnonzero(free & st.far().ravel()), B)
    to = np.array([st.cell(int(np.clip(st.long(s) + rng.integers(-8, 9), 0, st.L - 1)), int(rng.integers(0, st.S))) for s in start])
    goal = np.where(free[to], to, start)                             # within the L - 1 moves the layers allow
    start[:3] = [st.cell(st.L - 12, 1), st.corner, st.cell(MID - 5, 1)]
    goal[:3] = [st.cell(st.L - 4, 1), st.cell(st.L - 12, 1), st.cell(MID + 4, 1)]
    c["start"], c["goal"] = start.astype(np.int32), goal.astype(np.int32)
    return c
