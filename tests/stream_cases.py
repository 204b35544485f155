"""The chains of tests/test_gpu_stream_order.py: every device entry of include/sea_current_hip.h in one sequence of calls
that is run behind a gate on a caller's stream ("The stream contract").

A chain is a Chain: the C symbols it runs, its inputs (two sets, A and B, of equal shapes and different values), `run`
(the library calls, on device tensors, with no synchronisation and nothing that makes the host wait: no .item(), no
tensor built from a Python list), `expected` (the same values from the CPU oracle and the twins of tests/, never from
a second run of the library) and `view`, which brings a result into the form that is compared (cells the library leaves
unspecified, such as a path past its length, are masked).  A `staged` chain, whose family states its tolerance for equal
inputs, feeds every later stage of the reference from the arrays the checked run itself wrote upstream (Chain.staged).
expected() and differs() need no GPU: tests/test_stream_cases.py runs them for every chain.
"""
import os

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sea_current_hip.h")
Q_OK, Q_NO_PATH, Q_BAD_ENDPOINT, Q_TRUNCATED = 0, 1, 2, 3

# ---- coverage ----------------------------------------------------------------------------------------------------------
EXCLUDED = {
    # context management: no work on the stream (sc_ctx_synchronize and sc_ctx_get_timing wait by definition)
    "sc_abi_version", "sc_status_string", "sc_last_error", "sc_ctx_create", "sc_ctx_destroy", "sc_ctx_set_stream",
    "sc_ctx_use_own_stream", "sc_ctx_synchronize", "sc_ctx_set_timing", "sc_ctx_reset_timing", "sc_ctx_get_timing",
    "sc_ctx_scratch_bytes",
    # host arithmetic, no context
    "sc_rank_range", "sc_gather_msg_words",
    # need RCCL peers
    "sc_comm_unique_id", "sc_comm_init", "sc_comm_adopt", "sc_comm_destroy", "sc_allgather_paths", "sc_allgather_last_bytes",
    # the documented synchronising reads (test_documented_exceptions_wait_on_the_callers_stream)
    "sc_astar_gfield", "sc_astar_last_expansions", "sc_astar_debug_stats", "sc_astar_debug_peek",
}


def device_entries():
    """The device forms the header declares, read the way the binding reads it: every prototype, less the _host forms
    and EXCLUDED."""
    import sea_current_amd as sc
    with open(HEADER) as f:
        names = set(sc._signatures(f.read()))
    assert EXCLUDED <= names, sorted(EXCLUDED - names)
    return {n for n in names if not n.endswith("_host")} - EXCLUDED


# ---- twins -------------------------------------------------------------------------------------------------------------
class Twins:
    """The CPU references, built on demand in one directory."""

    def __init__(self, tmpdir):
        self.dir = str(tmpdir)
        self._made = {}

    def _get(self, key, make):
        if key not in self._made:
            d = os.path.join(self.dir, key)
            os.makedirs(d, exist_ok=True)
            self._made[key] = make(d)
        return self._made[key]

    @property
    def oracle(self):
        def make(_):
            from oracle import oracle as o
            o.build()
            return o
        return self._get("oracle", make)

    def __getattr__(self, key):
        if key.startswith("_") or key not in self.TWINS:
            raise AttributeError(key)
        mod, cls = self.TWINS[key]
        return self._get(key, lambda d: getattr(__import__(mod), cls)(d))

    TWINS = {"components": ("components_twin", "Twin"), "field": ("field_twin", "Twin"), "field_w": ("field_w_twin", "TwinW"),
             "field_m": ("field_multi_twin", "TwinM"), "waypoints": ("waypoints_twin", "Twin"), "frontier": ("frontier_twin", "Ref"),
             "views": ("views_twin", "Ref"), "sectors": ("sectors_twin", "Ref"), "match": ("match_twin", "Ref"),
             "match_wide": ("match_wide_twin", "Ref"), "explore": ("explore_gain_twin", "Ref"), "pose": ("pose_twin", "Ref"),
             "scan": ("scan_twin", "Ref")}


# ---- views of results -----------------------------------------------------------------------------------------------------
def paths_view(o, prefix, extra=()):
    """astar_batch's dict in the form that is compared: status, len, cost, and the path of every Q_OK query up to its
    length (-1 elsewhere: a path past its length, or of a query without one, is unspecified)."""
    st, ln = np.asarray(o["status"]), np.asarray(o["len"])
    path = np.array(o["path"])
    keep = (np.arange(path.shape[1])[None, :] < ln[:, None]) & (st == Q_OK)[:, None]
    out = {prefix + "status": st, prefix + "len": ln, prefix + "cost": np.asarray(o["cost"]), prefix + "path": np.where(keep, path, -1)}
    for k in extra:
        out[prefix + k] = np.asarray(o[k])
    return out


def oracle_astar_multi(oracle, d2, qgrid, start, goal, r2, Lmax):
    """sc_astar_batch_multi from the oracle's single-grid search: a query with a grid out of range is Q_BAD_ENDPOINT."""
    Q = len(start)
    out = dict(path=np.full((Q, Lmax), -1, np.int32), len=np.zeros(Q, np.int32), cost=np.full(Q, -1, np.int32), status=np.full(Q, Q_BAD_ENDPOINT, np.int32))
    for g in range(d2.shape[0]):
        q = np.flatnonzero(qgrid == g)
        if q.size:
            r = oracle.astar_batch(d2[g], start[q], goal[q], r2=r2, Lmax=Lmax)
            for k in out:
                out[k][q] = r[k][:, :Lmax] if k == "path" else r[k]
    return out


class Chain:
    """name, symbols (the C entries run), tol ({key: (rtol, atol) or a function (gpu, expected) -> bool array}; keys not named
    compare equal), constant (the keys whose expected value is the same in every input set by construction: compared on
    the GPU like the others, left out of differs())."""
    name, symbols, tol, constant = "", (), {}, ()

    def inputs(self, which):
        raise NotImplementedError

    def run(self, ctx, d, prev=None):
        raise NotImplementedError

    def expected(self, inp, tw):
        raise NotImplementedError

    def view(self, o):
        return o

    # -- shared
    staged = False      # True: expected(inp, tw, up) takes the inputs of every later stage from `up`, the results of the run that is
    #                     checked (its own upstream outputs, copied on the stream at the end), where the family's tolerance is stated
    #                     for equal inputs; up None is the oracle fed by itself, which is what differs() compares

    def expected_view(self, which, tw, up=None):
        if up is not None:
            return self.view(self.expected(self.inputs(which), tw, up))
        key = (self.name, which)
        if key not in _EXPECTED:
            _EXPECTED[key] = self.view(self.expected(self.inputs(which), tw))
        return _EXPECTED[key]

    def differs(self, tw):
        """expected(A) != expected(B) for every compared array: a stale result cannot pass for a fresh one."""
        a, b = self.expected_view("A", tw), self.expected_view("B", tw)
        assert set(a) == set(b)
        for k in a:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (self.name, k, a[k].shape, b[k].shape)
            if k in self.constant:
                assert np.array_equal(a[k], b[k]), (self.name, k)
                continue
            assert not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), f"{self.name}: {k} is the same for A and B"

    def compare(self, got, want):
        assert set(got) == set(want), (self.name, sorted(set(got) ^ set(want)))
        for k in want:
            g, w = np.asarray(got[k]), np.asarray(want[k])
            assert g.shape == w.shape, (self.name, k, g.shape, w.shape)
            if callable(self.tol.get(k)):
                ok = np.asarray(self.tol[k](g, w))
            elif k in self.tol:
                rtol, atol = self.tol[k]
                ok = np.isclose(g, w, rtol=rtol, atol=atol, equal_nan=True)
            else:
                ok = (g == w) | ((g != g) & (w != w)) if w.dtype.kind == "f" else g == w
            if not ok.all():
                bad = np.argwhere(~ok)
                i = tuple(bad[0])
                what = f"gpu {g[i]} expected {w[i]}" if ok.shape == g.shape else f"gpu {g[i[0]].ravel()[:4]} expected {w[i[0]].ravel()[:4]}"
                raise AssertionError(f"{self.name}: {k}: {len(bad)} of {ok.size} differ, first at {i}: {what}")


_EXPECTED = {}


def _rng(which, salt=0):
    return np.random.default_rng({"A": 101, "B": 202, "C": 303}[which] + 1000 * salt)


def _salt_occ(W, H, p, which, salt=0):
    """A random occupancy grid with a free border, different for A and B."""
    occ = (_rng(which, salt).random((H, W)) < p).astype(np.uint8)
    occ[0, :] = occ[-1, :] = 0
    occ[:, 0] = occ[:, -1] = 0
    return occ


def _cells(rng, W, H, n, bad=2):
    """n random cell indices, the first `bad` of them outside the grid at positions that depend on the draw."""
    c = rng.integers(0, W * H, n).astype(np.int32)
    c[rng.choice(n, bad, replace=False)] = [-1, W * H][:bad]
    return c


# ---- chain 1: polygons / rectangles -> EDT of a stack -> A* over several grids; nearest obstacle; legal moves --------------
class Grids(Chain):
    name = "1 grids"
    symbols = ("sc_occ_from_polygons", "sc_occ_from_rects", "sc_edt_u8_i32", "sc_astar_batch_multi", "sc_edt_nearest_i32", "sc_moves_i32_u8")
    W, H, G, Q, Lmax, r2 = 96, 64, 2, 24, 256, 1
    frame = (-4.8, -3.2, 0.1, 0.1)

    def inputs(self, which):
        rng = _rng(which, 1)
        n_obs, k, lines = 8, 5, []
        for _ in range(n_obs):                                            # star-shaped pentagons: A and B share every shape
            c = rng.uniform([-4.0, -2.6], [4.0, 2.6])
            a = np.sort(rng.uniform(0, 2 * np.pi, k))
            v = c + rng.uniform(0.3, 0.9, k)[:, None] * np.stack([np.cos(a), np.sin(a)], 1)
            lines += [np.concatenate([v[i], v[(i + 1) % k]]) for i in range(k)]
        rects = np.stack([rng.integers(-4, self.W, 6), rng.integers(-4, self.H, 6)], 1)
        rects = np.concatenate([rects, rects + rng.integers(1, 12, (6, 2))], 1).astype(np.int32)
        return dict(lines=np.array(lines, np.float32), obs_off=(k * np.arange(n_obs + 1)).astype(np.int32),
                    grid_off=np.array([0, n_obs // 2, n_obs], np.int32),
                    wide=_salt_occ(1100, 40, 0.02, which, 13),             # rows past 1024 cells: the wide-row EDT kernels and their scratch
                    rects=rects, qgrid=rng.integers(0, self.G, self.Q).astype(np.int32), start=_cells(rng, self.W, self.H, self.Q),
                    goal=_cells(rng, self.W, self.H, self.Q))

    def run(self, ctx, d, prev=None):
        p = prev or {}
        occ = ctx.occ_from_polygons(d["lines"], d["obs_off"], self.W, self.H, *self.frame, grid_off=d["grid_off"], out=p.get("occ"))
        occ_r = ctx.occ_from_rects(d["rects"], self.W, self.H, base=occ[1], out=p.get("occ_rects"))
        d2 = ctx.edt(occ, out=p.get("d2"))
        d2_wide = ctx.edt(d["wide"], out=p.get("d2_wide"))
        nearest = ctx.edt_nearest(occ, d2)
        moves = ctx.moves(d2[0], r2=self.r2)
        res = ctx.astar_batch_multi(d2, d["qgrid"], d["start"], d["goal"], r2=self.r2, Lmax=self.Lmax,
                                    out={k[2:]: v for k, v in p.items() if k.startswith("a_")} or None)
        return dict(occ=occ, occ_rects=occ_r, d2=d2, d2_wide=d2_wide, nearest=nearest, moves=moves, **{"a_" + k: v for k, v in res.items()})

    def expected(self, inp, tw):
        import occ_twin
        from sea_current_amd import synth
        o = tw.oracle
        fr = (self.W, self.H) + tuple(np.float32(v) for v in self.frame)
        go, oo = inp["grid_off"], inp["obs_off"]
        occ = np.stack([occ_twin.rasterize(fr, inp["lines"], oo[go[g]:go[g + 1] + 1]) for g in range(self.G)])
        occ_r = synth.raster_rects(inp["rects"], self.W, self.H, base=occ[1], free_border=True)
        d2 = np.stack([o.edt(occ[g]) for g in range(self.G)])
        nearest = np.stack([o.edt_nearest(occ[g], d2[g]) for g in range(self.G)])
        res = oracle_astar_multi(o, d2, inp["qgrid"], inp["start"], inp["goal"], self.r2, self.Lmax)
        return dict(occ=occ, occ_rects=occ_r, d2=d2, d2_wide=o.edt(inp["wide"]), nearest=nearest, moves=o.moves(d2[0], self.r2),
                    **{"a_" + k: v for k, v in res.items()})

    def view(self, o):
        out = {k: np.asarray(o[k]) for k in ("occ", "occ_rects", "d2", "d2_wide", "nearest", "moves")}
        out.update(paths_view({k[2:]: v for k, v in o.items() if k.startswith("a_")}, "a_"))
        return out


# ---- chain 4: EDT -> components -> reachable -> screened A* ---------------------------------------------------------------
class Components(Chain):
    name = "4 components"
    symbols = ("sc_edt_u8_i32", "sc_components_batch", "sc_reachable_batch", "sc_astar_batch_screened")
    W, H, Q, Lmax = 130, 70, 32, 512

    def inputs(self, which):
        rng = _rng(which, 4)
        occ = _salt_occ(self.W, self.H, 0.41, which, 4)
        occ[0, :"ABC".index(which)] = 1                     # the largest component's smallest cell differs between the sets
        return dict(occ=occ, start=_cells(rng, self.W, self.H, self.Q), goal=_cells(rng, self.W, self.H, self.Q))

    def run(self, ctx, d, prev=None):
        p = prev or {}
        d2 = ctx.edt(d["occ"], out=p.get("d2"))
        comp = ctx.components(d2, want_size=True, out={k[2:]: v for k, v in p.items() if k.startswith("c_")} or None)
        reach = ctx.reachable(comp["label"], d["start"], d["goal"])
        res = ctx.astar_batch(d2, d["start"], d["goal"], Lmax=self.Lmax, label=comp["label"],
                              out={k[2:]: v for k, v in p.items() if k.startswith("a_")} or None)
        return dict(d2=d2, reach=reach, **{"c_" + k: v for k, v in comp.items()}, **{"a_" + k: v for k, v in res.items()})

    def expected(self, inp, tw):
        d2 = tw.oracle.edt(inp["occ"])
        comp = tw.components.components(d2)
        reach = tw.components.reachable(comp["label"], inp["start"], inp["goal"])
        res = tw.oracle.astar_batch(d2, inp["start"], inp["goal"], Lmax=self.Lmax)
        return dict(d2=d2, reach=reach, **{"c_" + k: v for k, v in comp.items()}, **{"a_" + k: res[k] for k in ("path", "len", "cost", "status")})

    def view(self, o):
        out = {k: np.asarray(o[k]) for k in ("d2", "reach", "c_label", "c_size", "c_ncomp", "c_largest")}
        out.update(paths_view({k[2:]: v for k, v in o.items() if k.startswith("a_")}, "a_"))
        return out


def _sub(o, prefix):
    """The entries of a flat dict under a prefix, without it (None when there are none)."""
    return {k[len(prefix):]: v for k, v in (o or {}).items() if k.startswith(prefix)} or None


def _pre(prefix, o):
    return {prefix + k: v for k, v in o.items()}


# ---- chain 5: EDT -> costmap -> cost fields (plain, weighted, multi-source) -> their read-outs -> cost matrix -> assignment ----
class Fields(Chain):
    name = "5 fields"
    symbols = ("sc_edt_u8_i32", "sc_clearance_penalty_u8", "sc_cost_field_batch", "sc_cost_field_weighted_batch", "sc_cost_field_multi_batch",
               "sc_field_paths_batch", "sc_field_paths_weighted_batch", "sc_field_paths_multi_batch", "sc_field_cost_matrix",
               "sc_assign_batch", "sc_fleet_assign_batch")
    W, H, F, Q, R, Lmax, cap = 130, 70, 3, 16, 5, 512, 99
    seed_off = np.array([0, 2, 4, 6], np.int32)

    def inputs(self, which):
        rng = _rng(which, 5)
        occ = _salt_occ(self.W, self.H, 0.15, which, 5)
        free, blocked = np.flatnonzero(occ.ravel() == 0), np.flatnonzero(occ.ravel() != 0)
        bad = "ABC".index(which)                                 # the field with a blocked root / blocked seeds: another one in every set
        roots = rng.choice(free, self.F, replace=False).astype(np.int32)
        seeds = rng.choice(free, 6, replace=False).astype(np.int32)
        roots[bad] = blocked[0]
        seeds[2 * bad:2 * bad + 2] = blocked[1:3]
        targets = rng.choice(free, self.Q).astype(np.int32)
        targets[rng.choice(self.Q, 2, replace=False)] = [-1, self.W * self.H]
        return dict(occ=occ, roots=roots, seeds=seeds, seed_off=self.seed_off, seed_cost=rng.integers(0, 300, 6).astype(np.int32),
                    targets=targets, qfield=rng.integers(0, self.F, self.Q).astype(np.int32), robots=rng.choice(free, self.R).astype(np.int32),
                    col_cost=rng.integers(0, 50, self.F).astype(np.int32))

    def run(self, ctx, d, prev=None):
        p = prev or {}
        d2 = ctx.edt(d["occ"], out=p.get("d2"))
        pen = ctx.clearance_penalty(d2, r2_soft=25, pen_max=60, out=p.get("pen"))
        f = ctx.cost_fields(d2, d["roots"], out=_sub(p, "f_"))
        fw = ctx.cost_fields(d2, d["roots"], pen=pen, pen_cap=self.cap, out=_sub(p, "fw_"))
        fm = ctx.cost_fields_multi(d2, d["seeds"], d["seed_off"], d["seed_cost"], out=_sub(p, "fm_"))
        pa = ctx.field_paths(d2, f["g"], d["roots"], d["qfield"], d["targets"], Lmax=self.Lmax, out=_sub(p, "p_"))
        pw = ctx.field_paths(d2, fw["g"], d["roots"], d["qfield"], d["targets"], Lmax=self.Lmax, to_root=True, pen=pen, pen_cap=self.cap,
                             out=_sub(p, "pw_"))
        pm = ctx.field_paths_multi(d2, fm, d["seeds"], d["qfield"], d["targets"], Lmax=self.Lmax, out=_sub(p, "pm_"))
        m = ctx.field_cost_matrix(f["g"], d["robots"], d["col_cost"], out=p.get("matrix"))
        return dict(d2=d2, pen=pen, matrix=m, **_pre("f_", f), **_pre("fw_", fw), **_pre("fm_", fm), **_pre("p_", pa), **_pre("pw_", pw),
                    **_pre("pm_", pm), **_pre("as_", ctx.assign(m)), **_pre("fa_", ctx.fleet_assign(f["g"], d["robots"], d["col_cost"], want_cost=True)))

    def expected(self, inp, tw):
        import assign_twin
        from field_w_twin import penalty_numpy
        d2 = tw.oracle.edt(inp["occ"])
        pen = penalty_numpy(d2, 0, 25, 60)
        roots, seeds, cost, off, tg, qf = (inp[k] for k in ("roots", "seeds", "seed_cost", "seed_off", "targets", "qfield"))
        f = [tw.field.field(d2, int(r)) for r in roots]
        fw = [tw.field_w.field(d2, pen, int(r), 0, self.cap) for r in roots]
        fm = [tw.field_m.field(d2, seeds[off[k]:off[k + 1]], cost[off[k]:off[k + 1]], s0=off[k]) for k in range(self.F)]
        o = dict(d2=d2, pen=pen, f_g=np.stack([g for g, _ in f]), f_status=np.array([s for _, s in f], np.int32),
                 fw_g=np.stack([g for g, _ in fw]), fw_status=np.array([s for _, s in fw], np.int32), fm_g=np.stack([g for g, _, _ in fm]),
                 fm_owner=np.stack([w for _, w, _ in fm]), fm_status=np.array([s for _, _, s in fm], np.int32))
        keys = ("path", "len", "cost", "status")
        pa, pw, pm = ({k: np.zeros((self.Q, self.Lmax) if k == "path" else self.Q, np.int32) for k in kk} for kk in (keys, keys, keys + ("which",)))
        for k in range(self.F):
            q = np.flatnonzero(qf == k)
            for dst, src in ((pa, tw.field.paths(d2, o["f_g"][k], int(roots[k]), tg[q], Lmax=self.Lmax)),
                             (pw, tw.field_w.paths(d2, pen, o["fw_g"][k], int(roots[k]), tg[q], cap=self.cap, Lmax=self.Lmax, to_root=True)),
                             (pm, tw.field_m.paths(d2, o["fm_g"][k], seeds[off[k]:off[k + 1]], tg[q], cost[off[k]:off[k + 1]], s0=off[k],
                                                   Lmax=self.Lmax))):
                for kk in dst:
                    dst[kk][q] = src[kk]
        m = assign_twin.field_cost_matrix(o["f_g"], inp["robots"], inp["col_cost"]).astype(np.int32)
        o.update(matrix=m, **_pre("p_", pa), **_pre("pw_", pw), **_pre("pm_", pm), **_pre("as_", {k: v[0] for k, v in assign_twin.assign(m[None]).items()}),
                 **_pre("fa_", {k: v[0] for k, v in assign_twin.assign(m[None]).items()}), fa_cost=m)
        return o

    def view(self, o):
        out = {k: np.asarray(v) for k, v in o.items() if k[:2] not in ("p_", "pw", "pm")}
        for pre, extra in (("p_", ()), ("pw_", ()), ("pm_", ("which",))):
            out.update(paths_view(_sub(o, pre), pre, extra))
        return out

# ---- chain 6: sensing discs -> known space -> frontiers -> matrix -> a goal per robot; cluster centres -> picks by gain -----
class Explore(Chain):
    name = "6 explore"
    symbols = ("sc_edt_u8_i32", "sc_known_from_discs", "sc_d2_known_i32", "sc_frontier_batch", "sc_cost_field_batch", "sc_frontier_cost_matrix",
               "sc_fleet_explore_batch", "sc_frontier_centres", "sc_explore_gain_batch", "sc_fleet_explore_gain_batch")
    W, H, F, Cmax, r2s, wg, span = 130, 70, 3, 64, 15 * 15, 3, 4
    constant = ("f_status",)           # every robot stands on a free cell: Q_OK in every set

    @staticmethod
    def dirs():
        import sectors_twin
        return sectors_twin.heading_dirs(8)          # a sensor with a field of view: the heading of a pick differs between the sets

    def inputs(self, which):
        import frontier_twin as ft
        rng = _rng(which, 6)
        occ = _salt_occ(self.W, self.H, 0.05, which, 6)
        discs = np.stack([rng.integers(15, self.W - 15, 3), rng.integers(15, self.H - 15, 3), rng.integers(100, 500, 3)], 1).astype(np.int32)
        ok = (ft.known_from_discs(None, discs, self.W, self.H) != 0) & (occ == 0)
        ok[[0, -1], :] = ok[:, [0, -1]] = False
        roots = rng.choice(np.flatnonzero(ok.ravel()), self.F, replace=False).astype(np.int32)
        for r in roots[:"ABC".index(which)]:                    # walled in: a robot without a pick, so npick differs between the sets
            occ.ravel()[[r - 1, r + 1, r - self.W, r + self.W]] = 1
        return dict(occ=occ, discs=discs, roots=roots)

    def run(self, ctx, d, prev=None):
        p = prev or {}
        known = ctx.known_from_discs(d["discs"], self.W, self.H, out=p.get("known"))
        d2k = ctx.d2_known(ctx.edt(d["occ"], out=p.get("d2")), known, out=p.get("d2k"))
        fr = ctx.frontiers(d2k, known, Cmax=self.Cmax, out=_sub(p, "fr_"))
        g = ctx.cost_fields(d2k, d["roots"], out=_sub(p, "f_"))
        cm = ctx.frontier_cost_matrix(g["g"], fr)
        fe = ctx.fleet_explore(d2k, known, g["g"], Cmax=self.Cmax)
        centre = ctx.frontier_centres(fr, self.W, self.H, out=p.get("centre"))
        eg = ctx.explore_gain(d["occ"], known, g["g"], centre[0], self.r2s, self.dirs(), self.span, wg=self.wg)
        feg = ctx.fleet_explore_gain(d2k, known, d["occ"], g["g"], self.r2s, Cmax=self.Cmax, dirs=self.dirs(), span=self.span, wg=self.wg)
        return dict(known=known, d2k=d2k, centre=centre, **_pre("fr_", fr), **_pre("f_", g), **_pre("cm_", cm), **_pre("fe_", fe), **_pre("eg_", eg),
                    **_pre("feg_", feg))

    def expected(self, inp, tw):
        import explore_gain_twin as et
        import frontier_twin as ft
        occ = inp["occ"]
        known = ft.known_from_discs(None, inp["discs"], self.W, self.H)
        d2k = ft.d2_known(tw.oracle.edt(occ), known)
        fr = ft.frontiers(d2k, known, Cmax=self.Cmax)
        f = [tw.field.field(d2k, int(r)) for r in inp["roots"]]
        g = np.stack([a for a, _ in f])
        cost, cell = ft.cost_matrix(g, fr["slot"], fr["csize"], self.Cmax)
        fe = ft.fleet_explore(d2k, known, g, Cmax=self.Cmax)
        centre = et.frontier_centres(fr["slot"], fr["csize"], fr["csum"], self.Cmax)
        eg = tw.explore.explore_gain(occ, known, g, centre[0], self.r2s, self.dirs(), self.span, wg=self.wg)
        return dict(known=known, d2k=d2k, centre=centre, **_pre("fr_", fr), f_g=g, f_status=np.array([s for _, s in f], np.int32), cm_cost=cost,
                    cm_cell=cell, fe_goal=fe["goal"], fe_gcost=fe["gcost"], **_pre("eg_", eg), **_pre("feg_", eg))

    def view(self, o):
        return {k: np.asarray(v) for k, v in o.items()}


# ---- chain 7: line-of-sight views, sector views, the gain of every heading ----------------------------------------------------
class Views(Chain):
    name = "7 views"
    symbols = ("sc_views_from_cells", "sc_known_from_views", "sc_view_gain_batch", "sc_known_from_sectors", "sc_sector_gain_batch",
               "sc_view_gain_headings_batch")
    W, H, N, r2, span = 130, 70, 16, 144, 3

    @staticmethod
    def dirs():
        import sectors_twin
        return sectors_twin.heading_dirs(8)

    def inputs(self, which):
        import sectors_twin
        rng = _rng(which, 7)
        occ = _salt_occ(self.W, self.H, 0.04, which, 7)
        cells = rng.choice(np.flatnonzero(occ.ravel() == 0), self.N, replace=False).astype(np.int32)
        cells[int(rng.integers(4, self.N))] = self.W * self.H                  # an ignored view, not among the four that are applied
        views = sectors_twin.views_from_cells(cells, self.W, self.H, self.r2)
        return dict(occ=occ, cells=cells, sviews=sectors_twin.sector_views(views, self.dirs(), rng.integers(0, 8, self.N), self.span))

    def run(self, ctx, d, prev=None):
        p = prev or {}
        views = ctx.views_from_cells(d["cells"], self.W, self.H, self.r2, out=p.get("views"))
        known, seen = ctx.known_from_views(views[:4], d["occ"], out=p.get("known"), occ_seen=p.get("seen", True))
        gain = ctx.view_gain(views, d["occ"], known, out=p.get("gain"))
        known_s, seen_s = ctx.known_from_sectors(d["sviews"][:4], d["occ"], base=known, out=p.get("known_s"), occ_seen=p.get("seen_s", True))
        sgain = ctx.sector_gain(d["sviews"], d["occ"], known, out=p.get("sgain"))
        vh = ctx.view_gain_headings(views, d["occ"], known, self.dirs(), self.span, hist=p.get("vh_hist", True), gainh=p.get("vh_gainh", True),
                                    out=p.get("vh_best"))
        return dict(views=views, known=known, seen=seen, gain=gain, known_s=known_s, seen_s=seen_s, sgain=sgain, **_pre("vh_", vh))

    def expected(self, inp, tw):
        import sectors_twin
        occ = inp["occ"]
        views = sectors_twin.views_from_cells(inp["cells"], self.W, self.H, self.r2)
        known, seen = tw.views.known_from_views(None, occ, views[:4])
        known_s, seen_s = tw.sectors.known_from_sectors(known, occ, inp["sviews"][:4])
        return dict(views=views, known=known, seen=seen, gain=tw.views.view_gain(occ, known, views), known_s=known_s, seen_s=seen_s,
                    sgain=tw.sectors.sector_gain(occ, known, inp["sviews"]),
                    **_pre("vh_", tw.sectors.view_gain_headings(occ, known, views, self.dirs(), self.span)))


# ---- chain 8: a range scan -> the log-odds map, twice -> its EDT -> the scan's pose, narrow and wide window --------------------
class Scan(Chain):
    name = "8 scan"
    symbols = ("sc_scan_cast_batch", "sc_logodds_update", "sc_edt_u8_i32", "sc_scan_match_batch", "sc_scan_match_wide_batch")
    W, H, S, r, cap = 130, 70, 2, 20, 16
    params = dict(l_hit=2, l_miss=1, l_clamp=8, t_occ=2, t_free=1)

    def inputs(self, which):
        import scan_twin
        rng = _rng(which, 8)
        occ = _salt_occ(self.W, self.H, 0.05, which, 8)
        ok = occ == 0
        ok[:, :25] = ok[:, -25:] = ok[:25, :] = ok[-25:, :] = False
        at = rng.choice(np.flatnonzero(ok.ravel()), self.S, replace=False)
        rays = np.concatenate([scan_twin.square_fan(int(c % self.W), int(c // self.W), self.r) for c in at])
        centre = np.stack([at % self.W, at // self.W], 1) + rng.integers(-3, 4, (self.S, 2))     # the prior: a few cells off
        return dict(occ=occ, rays=rays.astype(np.int32), centre=centre.astype(np.int32))

    def run(self, ctx, d, prev=None):
        import torch
        import sea_current_amd as sc
        p = prev or {}
        n = 8 * self.r
        rays = d["rays"]
        hit = ctx.scan_cast(rays, d["occ"], out=p.get("hit"))
        L1 = ctx.logodds_update(rays[:n], hit[:n], self.W, self.H, out=p.get("L1"), **self.params)
        # the second update relies on the flag maps the first one left zeroed on the stream
        L2, est, known = ctx.logodds_update(rays[n:], hit[n:], self.W, self.H, L=L1, out=p.get("L2"), occ_est=p.get("est", True),
                                            known=p.get("known", True), **self.params)
        d2 = ctx.edt(est, out=p.get("d2"))
        off = torch.stack([hit % self.W - rays[:, 0], torch.div(hit, self.W, rounding_mode="floor") - rays[:, 1]], 1)
        pts = torch.where((hit >= 0)[:, None], off, sc.SCAN_MATCH_ABSENT).to(torch.int32).reshape(self.S, 1, n, 2).contiguous()
        best, score = ctx.scan_match(pts, d["centre"], d2, known, wx=8, wy=8, d2_cap=self.cap, out=p.get("best"), score=p.get("score", True))
        wide, stats = ctx.scan_match_wide(pts, d["centre"], d2, known, wx=40, wy=30, d2_cap=self.cap, top=2, out=p.get("wide"),
                                          stats=p.get("stats", True))
        return dict(hit=hit, L1=L1, L2=L2, est=est, known=known, d2=d2, pts=pts, best=best, score=score, wide=wide, stats=stats)

    def expected(self, inp, tw):
        import match_twin
        n = 8 * self.r
        rays, occ = inp["rays"], inp["occ"]
        hit = tw.scan.cast(occ, rays)
        par = tuple(self.params[k] for k in ("l_hit", "l_miss", "l_clamp", "t_occ", "t_free"))
        L1, _, _ = tw.scan.update(None, rays[:n], hit[:n], self.W, self.H, *par)
        L2, est, known = tw.scan.update(L1, rays[n:], hit[n:], self.W, self.H, *par)
        d2 = tw.oracle.edt(est)
        pts = match_twin.points_from_hits(rays, hit, self.W).reshape(self.S, 1, n, 2)
        best, score = tw.match.match(d2, known, pts, inp["centre"], 8, 8, self.cap, 1)
        wide, stats = tw.match_wide.match(d2, known, pts, inp["centre"], 40, 30, self.cap, 1, 2, 1 << 16)
        return dict(hit=hit, L1=L1, L2=L2, est=est, known=known, d2=d2, pts=pts, best=best, score=score, wide=wide, stats=stats)


# ---- chain 9: EDT -> footprint mask -> pose fields -> pose paths ---------------------------------------------------------------
class Pose(Chain):
    name = "9 pose"
    symbols = ("sc_edt_u8_i32", "sc_footprint_mask_u8", "sc_pose_field_batch", "sc_pose_paths_batch")
    W, H, F, Q, Lmax, foot, turn, rev = 130, 70, 3, 12, 512, (2, 1, 1, 0), 5, 7

    def inputs(self, which):
        import pose_twin
        rng = _rng(which, 9)
        occ = _salt_occ(self.W, self.H, 0.05, which, 9)
        fits = np.flatnonzero(pose_twin.footprint_mask(pose_twin.d2_of(occ), *self.foot).ravel() == 0xFF)
        roots = rng.choice(fits, self.F, replace=False).astype(np.int32)
        roots["ABC".index(which)] = np.flatnonzero(occ.ravel() != 0)[0]        # a blocked root: another field in every set
        targets = rng.choice(fits, self.Q).astype(np.int32)
        targets[rng.choice(self.Q, 2, replace=False)] = [-1, self.W * self.H]
        return dict(occ=occ, roots=roots, rhead=rng.integers(-1, 8, self.F).astype(np.int32), targets=targets,
                    thead=rng.integers(-1, 8, self.Q).astype(np.int32), qfield=rng.integers(0, self.F, self.Q).astype(np.int32))

    def run(self, ctx, d, prev=None):
        p = prev or {}
        d2 = ctx.edt(d["occ"], out=p.get("d2"))
        hm = ctx.footprint_mask(d2, *self.foot, out=p.get("hmask"))
        pf = ctx.pose_fields(d2, d["roots"], d["rhead"], self.turn, self.rev, hmask=hm, out=_sub(p, "pf_"))
        pp = ctx.pose_paths(d2, pf["gp"], d["roots"], d["rhead"], d["qfield"], d["targets"], d["thead"], self.turn, self.rev, hmask=hm,
                            Lmax=self.Lmax, out=_sub(p, "pp_"))
        return dict(d2=d2, hmask=hm, **_pre("pf_", pf), **_pre("pp_", pp))

    def expected(self, inp, tw):
        d2 = tw.oracle.edt(inp["occ"])
        hm = tw.pose.footprint_mask(d2, *self.foot)
        f = [tw.pose.pose_field(d2, int(r), int(h), self.turn, self.rev, False, 0, hm) for r, h in zip(inp["roots"], inp["rhead"])]
        gp = np.stack([g for g, _ in f])
        pp = dict(path=np.full((self.Q, self.Lmax), -1, np.int32), head=np.zeros((self.Q, self.Lmax), np.uint8),
                  **{k: np.zeros(self.Q, np.int32) for k in ("len", "cost", "status")})
        for k in range(self.F):
            q = np.flatnonzero(inp["qfield"] == k)
            one = tw.pose.pose_paths(d2, gp[k], int(inp["roots"][k]), int(inp["rhead"][k]), inp["targets"][q], inp["thead"][q], self.turn,
                                     self.rev, False, 0, hm, self.Lmax)
            for kk in pp:
                pp[kk][q] = one[kk]
        return dict(d2=d2, hmask=hm, pf_gp=gp, pf_status=np.array([s for _, s in f], np.int32), **_pre("pp_", pp))

    def view(self, o):
        out = {k: np.asarray(o[k]) for k in ("d2", "hmask", "pf_gp", "pf_status")}
        pp = _sub(o, "pp_")
        out.update(paths_view(pp, "pp_"))
        out["pp_head"] = np.where(out["pp_path"] >= 0, np.asarray(pp["head"]), 0)     # headings past a path's length are unspecified
        return out


# ---- chain 10: the planners and curve tools that stand alone ----------------------------------------------------------------
def _relmax(eps):
    """The bar of the TOPP-RA tests: per plan, max |gpu - ref| over the plan's entries relative to max |ref|."""
    def ok(g, w):
        g2, w2 = g.reshape(g.shape[0], -1).astype(np.float64), w.reshape(w.shape[0], -1).astype(np.float64)
        return np.abs(g2 - w2).max(1) / (np.abs(w2).max(1) + 1e-300) < eps
    return ok


class Toppra(Chain):
    name = "10a toppra"
    symbols = ("sc_toppra_hermite_batch", "sc_toppra_sample_batch")
    staged = True
    P, dof, N, dt, max_len = 8, 6, 50, 0.05, 1024
    tol = dict(K=_relmax(1e-9), x=_relmax(1e-9), u=_relmax(1e-9), t=_relmax(1e-9), s_pos=_relmax(1e-5), s_vel=_relmax(1e-5), s_acc=_relmax(1e-5))

    def inputs(self, which):
        from sea_current_amd import synth
        pl = synth.toppra_plans(self.P, self.dof, first=100 * "ABC".index(which))
        alo, ahi = -pl["alim"], pl["alim"].copy()
        alo["ABC".index(which), 0], ahi["ABC".index(which), 0] = 1.0, 0.5           # an empty acceleration interval: this plan fails
        return dict(p0=pl["p0"], p1=pl["p1"], v0=pl["v0"], v1=pl["v1"], vlo=-pl["vlim"], vhi=pl["vlim"], alo=alo, ahi=ahi)

    def run(self, ctx, d, prev=None):
        tp = ctx.toppra(d["p0"], d["p1"], d["v0"], d["v1"], d["vlo"], d["vhi"], d["alo"], d["ahi"], N=self.N)
        sm = ctx.toppra_sample(d["p0"], d["p1"], d["v0"], d["v1"], tp["x"], tp["t"], self.dt, self.max_len)
        return dict(**tp, s_pos=sm["pos"], s_vel=sm["vel"], s_acc=sm["acc"], s_length=sm["length"])

    def expected(self, inp, tw, up=None):
        o, P = tw.oracle, self.P
        out = dict(K=np.zeros((P, self.N + 1, 2)), x=np.zeros((P, self.N + 1)), u=np.zeros((P, self.N)), t=np.zeros((P, self.N + 1)),
                   status=np.zeros(P, np.int32), s_length=np.zeros(P, np.int32),
                   **{k: np.zeros((P, self.dof, self.max_len), np.float32) for k in ("s_pos", "s_vel", "s_acc")})
        ends = [inp[k] for k in ("p0", "p1", "v0", "v1")]
        for p in range(P):
            r = o.toppra(*(e[p] for e in ends), inp["vlo"][p], inp["vhi"][p], inp["alo"][p], inp["ahi"][p], N=self.N)
            out["status"][p] = r["status"]
            if r["status"] != 0:
                continue
            for k in ("K", "x", "u", "t"):
                out[k][p] = r[k]
            src = r if up is None else {k: np.asarray(up[k])[p] for k in ("x", "t")}
            s = o.toppra_sample(*(e[p] for e in ends), src["x"], src["t"], self.dt, self.max_len)
            out["s_length"][p] = s["length"]
            for k in ("pos", "vel", "acc"):
                out["s_" + k][p, :, :s[k].shape[1]] = s[k]
        return out

    def view(self, o):
        st = np.asarray(o["status"])
        ok = st == 0                                             # the outputs of a plan that failed are unspecified
        out = dict(status=st, s_length=np.where(ok, np.asarray(o["s_length"]), 0))
        for k in ("K", "x", "u", "t"):
            out[k] = np.where(ok.reshape((-1,) + (1,) * (np.asarray(o[k]).ndim - 1)), np.asarray(o[k]), 0)
        keep = ok[:, None, None] & (np.arange(self.max_len)[None, None, :] < out["s_length"][:, None, None])
        for k in ("s_pos", "s_vel", "s_acc"):
            out[k] = np.where(keep, np.asarray(o[k]), 0)
        return out


class Bezier(Chain):
    name = "10b bezier"
    symbols = ("sc_bezier_from_path_batch", "sc_bezier_arclength_batch", "sc_bezier_resample_batch", "sc_bezier_eval_batch",
               "sc_bezier_curve_batch", "sc_bezier_shrink_tangent_batch", "sc_chebfit_batch", "sc_chebeval_batch")
    staged = True
    P, n_max, nsub, M, Mp, degree, k_shrink = 6, 5, 50, 64, 40, 6, 0.4
    sizes = (40, 300)
    constant = ("r_status",)          # every profile is clean: all splines resample
    tol = dict(ctrl=(1e-6, 1e-6), cum=(2e-6, 1e-6), seg_len=(2e-6, 1e-6), al=lambda g, w: np.abs(g - w) / w < 2e-6, r_t=(0, 5e-7), r_pts=(0, 1e-5),
               r_curv=lambda g, w: (np.abs(w) >= 1e3) | np.isclose(g, w, rtol=2e-4, atol=1e-5), ev0=(2e-6, 2e-6), ev1=(2e-6, 2e-6),
               ev2=(2e-6, 2e-6), cv=lambda g, w: np.abs(g - w) < 2e-6 * max(1.0, np.abs(w).max()), sh=(1e-6, 1e-6),
               yh_small=lambda g, w: np.abs(g - w) < 5e-5 * max(1.0, np.abs(w).max()), yh_big=lambda g, w: np.abs(g - w) < 5e-5 * max(1.0, np.abs(w).max()),
               coef_big=lambda g, w: np.abs(g - w) < 1e-4 * max(1.0, np.abs(w).max()))

    def inputs(self, which):
        rng = _rng(which, 10)
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        P, n = self.P, self.n_max
        x = np.concatenate([np.sort(rng.uniform(-1, 5, s)) for s in self.sizes])
        return dict(path=f32(np.cumsum(rng.uniform(0.3, 2.0, (P, n, 2)) * rng.choice([-1, 1], (P, n, 2)), axis=1)), npts=np.full(P, n, np.int32),
                    lines=f32(rng.uniform(-5, 5, (4, 4))), frac=f32(np.sort(rng.uniform(0, 1, (P, self.Mp)), axis=1)),
                    seg_off=(np.arange(P + 1) * (n - 1)).astype(np.int32), prof_off=(np.arange(P + 1) * self.Mp).astype(np.int32),
                    e_ctrl=f32(rng.uniform(-3, 3, (11, 4, 2))), e_seg=rng.integers(0, 11, self.M).astype(np.int32), e_t=f32(rng.uniform(0, 1, self.M)),
                    g_ctrl=f32(rng.uniform(-4, 4, (3, 6, 2))), g_seg=rng.integers(0, 3, self.M).astype(np.int32), T=f32(rng.uniform(-3, 3, (32, 2))),
                    Wp=f32(rng.uniform(-5, 5, (32, 2))), cx=f32(x), cy=f32(np.cos(1.3 * x) + 0.05 * x ** 3 + rng.normal(0, 0.01, x.size)),
                    c_off=np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32))

    def run(self, ctx, d, prev=None):
        import torch
        P, n = self.P, self.n_max
        ctrl = ctx.bezier_from_path(d["path"], d["npts"], lines=d["lines"])
        cum, seg_len = ctx.bezier_arclength(ctrl, self.nsub)
        al = seg_len.reshape(P, n - 1).sum(1)
        pos = (d["frac"] * al[:, None]).reshape(-1).contiguous()
        pos_in = pos.clone()
        rs = ctx.bezier_resample(ctrl.reshape(-1, 4, 2), cum, al, d["seg_off"], pos, d["prof_off"], nudge=True)     # nudges pos in place
        ev = [ctx.bezier_eval(d["e_ctrl"], d["e_seg"], d["e_t"], order) for order in (0, 1, 2)]
        cv = ctx.bezier_curve(d["g_ctrl"], d["g_seg"], d["e_t"])
        sh = torch.empty_like(d["T"])
        ctx._call("sc_bezier_shrink_tangent_batch", d["T"].data_ptr(), d["Wp"].data_ptr(), d["T"].shape[0], self.k_shrink, d["lines"].data_ptr(),
                  d["lines"].shape[0], sh.data_ptr())
        coef, xr = ctx.chebfit(d["cx"], d["cy"], d["c_off"], self.degree)
        yh = ctx.chebeval(d["cx"], d["c_off"], coef, xr)
        return dict(ctrl=ctrl, cum=cum, seg_len=seg_len, al=al, pos_in=pos_in, r_pos=pos, r_status=rs["status"], r_seg=rs["seg"], r_t=rs["t"],
                    r_pts=rs["pts"], r_curv=rs["curvature"], ev0=ev[0], ev1=ev[1], ev2=ev[2], cv=cv, sh=sh, coef=coef, xr=xr, yh=yh)

    def expected(self, inp, tw, up=None):
        o, P, n, Mp = tw.oracle, self.P, self.n_max, self.Mp
        ctrl = np.stack([o.bezier_from_path(inp["path"][p], lines=inp["lines"]) for p in range(P)])
        src_ctrl = ctrl if up is None else np.asarray(up["ctrl"])
        arc = [o.bezier_arclength(src_ctrl[p], self.nsub) for p in range(P)]
        cum = np.concatenate([c for _, c in arc])
        al = np.array([t for t, _ in arc])
        if up is None:
            src_cum = cum.astype(np.float32)
            src_al = src_cum[:, -1].reshape(P, n - 1).sum(1, dtype=np.float32)
        else:
            src_cum, src_al = np.asarray(up["cum"]), np.asarray(up["al"])
        pos_in = (inp["frac"] * src_al[:, None]).astype(np.float32).reshape(-1)
        src_pos = pos_in if up is None else np.asarray(up["pos_in"])
        rs = [o.bezier_resample(src_ctrl[p], src_cum[p * (n - 1):(p + 1) * (n - 1)], src_al[p], src_pos[p * Mp:(p + 1) * Mp], True) for p in range(P)]
        t64 = inp["e_t"].astype(np.float64)
        fits = [o.chebfit(inp["cx"][a:b], inp["cy"][a:b], self.degree) for a, b in zip(inp["c_off"][:-1], inp["c_off"][1:])]
        coef = np.stack([c for c, _, _ in fits])
        xr = np.array([[lo, hi] for _, lo, hi in fits], np.float32)
        src_coef, src_xr = (coef, xr) if up is None else (np.asarray(up["coef"]), np.asarray(up["xr"]))
        yh = np.concatenate([o.chebeval(inp["cx"][a:b], src_coef[k], float(src_xr[k, 0]), float(src_xr[k, 1]))
                             for k, (a, b) in enumerate(zip(inp["c_off"][:-1], inp["c_off"][1:]))])
        return dict(ctrl=ctrl, cum=cum, seg_len=cum[:, -1], al=al, pos_in=pos_in, r_pos=np.concatenate([r["pos"] for r in rs]),
                    r_status=np.array([r["status"] for r in rs], np.int32), r_seg=np.concatenate([r["seg"] for r in rs]),
                    r_t=np.concatenate([r["t"] for r in rs]), r_pts=np.concatenate([r["pts"] for r in rs]),
                    r_curv=np.concatenate([r["curvature"] for r in rs]), **{"ev%d" % k: o.bezier_eval(inp["e_ctrl"], inp["e_seg"], t64, k) for k in (0, 1, 2)},
                    cv=o.bezier_curve(inp["g_ctrl"], inp["g_seg"], t64), sh=o.bezier_shrink_tangent(inp["T"], inp["Wp"], self.k_shrink, inp["lines"]),
                    coef=coef, xr=xr, yh=yh)

    def view(self, o):
        out = {k: np.asarray(v) for k, v in o.items() if k not in ("coef", "yh")}
        a = self.sizes[0]
        # the free fit's coefficients are held to the oracle's for the large problem only, its values for both (test_gpu_bezier.py)
        out.update(coef_big=np.asarray(o["coef"])[1], yh_small=np.asarray(o["yh"])[:a], yh_big=np.asarray(o["yh"])[a:])
        return out


class Fmt(Chain):
    name = "10c fmt"
    symbols = ("sc_fmt_star_batch",)
    n, Q, rn, Lmax = 200, 10, 0.6, 64
    polys = [[(-0.5, 0), (1, 0), (1, 1), (0, 1)], [(0, -0.5), (1, 0), (1, 1), (0, 1)], [(-0.6, 0.148), (-1, 0.148), (-1, 0), (-0.6, 0)]]

    def world(self):
        lines, off = [], [0]
        for q in self.polys:
            lines += [tuple(q[i]) + tuple(q[(i + 1) % len(q)]) for i in range(len(q))]
            off.append(len(lines))
        return np.array(lines, np.float32).reshape(-1, 4), np.array(off, np.int32)

    def inputs(self, which):
        from oracle import oracle
        rng = _rng(which, 11)
        lines, off = self.world()
        k = "ABC".index(which)
        samples, _ = oracle.sample_free(self.n, (-1, 1, -1, 1), lines, off, hstate=(3 * k, 8 * k, 7 * k, 27 * k))
        starts, goals = samples[rng.integers(1, self.n, self.Q)].copy(), samples[rng.integers(1, self.n, self.Q)].copy()
        starts[rng.integers(0, self.Q)] = (0.5, 0.5)              # inside an obstacle
        return dict(samples=samples, starts=starts, goals=goals, lines=lines)

    def run(self, ctx, d, prev=None):
        return ctx.fmt_star(d["samples"], d["starts"], d["goals"], self.rn, d["lines"], Lmax=self.Lmax)

    def expected(self, inp, tw):
        out = dict(path=np.zeros((self.Q, self.Lmax, 2), np.float32), len=np.zeros(self.Q, np.int32), cost=np.zeros(self.Q, np.float32),
                   status=np.zeros(self.Q, np.int32))
        for q in range(self.Q):
            r = tw.oracle.fmt_star(inp["samples"], inp["starts"][q], inp["goals"][q], self.rn, inp["lines"], Lmax=self.Lmax)
            out["status"][q], out["len"][q], out["cost"][q] = r["status"], r["len"], np.float32(r["cost"])
            out["path"][q, :len(r["path"])] = r["path"]
        return out

    def view(self, o):
        st = np.asarray(o["status"])
        ok = st == 0                                              # len, cost and path are stated for the queries that found a path
        ln = np.where(ok, np.asarray(o["len"]), 0)
        keep = np.arange(self.Lmax)[None, :] < ln[:, None]
        return dict(status=st, len=ln, cost=np.where(ok, np.asarray(o["cost"]), 0), path=np.where(keep[:, :, None], np.asarray(o["path"]), 0))


class Gather(Chain):
    name = "10d gather"
    symbols = ("sc_edt_u8_i32", "sc_astar_batch", "sc_gather_pack", "sc_gather_unpack")
    W, H, Q, Lmax, world, cap = 130, 70, 10, 256, 2, 1280
    constant = ("g_truncated",)        # the messages are roomy: 0 in every set

    def inputs(self, which):
        rng = _rng(which, 12)
        return dict(occ=_salt_occ(self.W, self.H, 0.2, which, 12), start=_cells(rng, self.W, self.H, self.Q, 1), goal=_cells(rng, self.W, self.H, self.Q, 1))

    def run(self, ctx, d, prev=None):
        """One process plays both ranks, as tests/test_gpu_gather.py does: pack per rank block, the messages back to back, unpack."""
        import torch
        import sea_current_amd as sc
        p = prev or {}
        d2 = ctx.edt(d["occ"], out=p.get("d2"))
        res = ctx.astar_batch(d2, d["start"], d["goal"], Lmax=self.Lmax, out=_sub(p, "a_"))
        words = int(sc.lib().sc_gather_msg_words(self.Q, self.world, self.cap))
        msgs = torch.full((self.world * words,), -99, dtype=torch.int32, device=d2.device)
        per = self.Q // self.world
        for r in range(self.world):
            blk = {k: v[r * per:(r + 1) * per] for k, v in res.items()}
            ctx.gather_pack(blk, self.Q, self.world, r, self.cap, msg=msgs[r * words:(r + 1) * words], Lmax=self.Lmax)
        got = ctx.gather_unpack(msgs, self.world, self.Q, self.Lmax, self.cap, want_path=True)
        return dict(d2=d2, **_pre("a_", res), **_pre("g_", got))

    def expected(self, inp, tw):
        d2 = tw.oracle.edt(inp["occ"])
        ref = tw.oracle.astar_batch(d2, inp["start"], inp["goal"], Lmax=self.Lmax)
        eff = np.where(ref["status"] == 0, ref["len"], 0).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(eff)])
        cells, path = np.full(self.world * self.cap, -7, np.int32), np.full((self.Q, self.Lmax), -7, np.int32)
        for q in range(self.Q):
            cells[off[q]:off[q + 1]] = path[q, :eff[q]] = ref["path"][q, :eff[q]]
        return dict(d2=d2, **_pre("a_", {k: ref[k] for k in ("path", "len", "cost", "status")}), g_len=ref["len"], g_cost=ref["cost"],
                    g_status=ref["status"], g_offsets=off, g_cells=cells, g_path=path, g_truncated=np.zeros(1, np.int32))

    def view(self, o):
        out = {k: np.asarray(o[k]) for k in ("d2", "g_len", "g_cost", "g_status", "g_offsets", "g_cells", "g_path", "g_truncated")}
        out.update(paths_view(_sub(o, "a_"), "a_"))
        return out


# ---- chain 2: EDT -> A* -> waypoints -> points -> the three smoothing calls; speed limits, curve check and repair ------------
SMOOTH_OK, SMOOTH_BAD_INPUT, SMOOTH_COLLIDES = 0, 1, 6
_relerr = lambda eps: (lambda g, w: (g == w) | (np.abs(g - w) <= eps * np.abs(w)))


class Smooth(Chain):
    """The smoothing calls are held to the CPU chain the way tests/test_gpu_speed_limits.py::test_composition_matches_the_cpu_chain
    holds them: twin limits -> oracle TOPP-RA -> sampler -> resample on the legs and tables of the run that is checked, with
    that test's bars (a path whose sample count is one off the CPU's is not compared sample by sample; three in four must be)."""
    name = "2 smooth"
    symbols = ("sc_edt_u8_i32", "sc_astar_batch", "sc_path_waypoints_batch", "sc_cells_to_points_batch", "sc_smooth_paths_batch",
               "sc_smooth_paths_limited_batch", "sc_smooth_paths_clear_batch", "sc_bezier_arclength_batch", "sc_speed_limits_batch",
               "sc_curve_clearance_batch", "sc_curve_clear_batch")
    staged = True
    W, H, P, Lmax, Wmax, r2, r2c, max_level, N, J, nsub = 130, 70, 12, 512, 24, 1, 2, 6, 100, 4, 100
    frame, dt, dyn, cap = (0.0, 0.0, 0.05, 0.05), 0.02, (0.8, 0.3, 0.05, 1.0), 12 * 8000
    forms = ("sm_", "sl_", "sc_")
    _curv = lambda g, w: (np.abs(w) >= 1e2) | np.isclose(g, w, rtol=2e-3, atol=2e-3)
    tol = dict(sp_vhi=_relerr(1e-9), sp_min_clear=_relerr(1e-9), sl_vmax_stage=_relerr(1e-9), sl_min_clear=_relerr(1e-9))
    for _f in forms:
        tol.update({_f + "ctrl": (0, 1e-5), _f + "arclength": _relerr(2e-6), _f + "pos": (0, 2e-4), _f + "vel": (0, 2e-5), _f + "pts": (0, 2e-4),
                    _f + "curvature": _curv})
    del tol["sc_ctrl"]                                             # the repaired legs are the twin's, bit for bit

    def inputs(self, which):
        rng = _rng(which, 2)
        occ = _salt_occ(self.W, self.H, 0.04, which, 2)
        free = np.flatnonzero(occ.ravel() == 0)
        start, goal = rng.choice(free, self.P).astype(np.int32), rng.choice(free, self.P).astype(np.int32)
        start[int(rng.integers(0, self.P))] = -1                   # a query without a path: a BAD_INPUT path for the smoother
        pairs = np.array([(1.0, 0.5), (0.6, 0.3), (1.5, 1.0), (0.4, 0.8)])[rng.integers(0, 4, self.P)]
        lim = np.stack([-pairs[:, 0], pairs[:, 0], -pairs[:, 1], pairs[:, 1]], 1)
        inf = float("inf")
        return dict(occ=occ, start=start, goal=goal, lim=lim, dyn=np.tile(np.array(self.dyn), (self.P, 1)), dyn_off=np.tile(np.array([inf, inf, inf, 0.0]), (self.P, 1)))

    def run(self, ctx, d, prev=None):
        p = prev or {}
        d2 = ctx.edt(d["occ"], out=p.get("d2"))
        res = ctx.astar_batch(d2, d["start"], d["goal"], r2=self.r2, Lmax=self.Lmax, out=_sub(p, "a_"))
        wr = ctx.path_waypoints(d2, res, r2=self.r2, Wmax=self.Wmax, out=_sub(p, "w_"))
        wp, npts = ctx.cells_to_points(wr, self.W, *self.frame)
        kw = dict(dt=self.dt, N=self.N, nsub=self.nsub, capacity=self.cap)
        sm = ctx.smooth_paths(wp, npts, d["lim"], out=_sub(p, "sm_"), **kw)
        sl = ctx.smooth_paths(wp, npts, d["lim"], dyn=d["dyn"], J=self.J, d2=d2, frame=self.frame, out=_sub(p, "sl_"), **kw)
        sc = ctx.smooth_paths(wp, npts, d["lim"], dyn=d["dyn_off"], J=self.J, d2=d2, frame=self.frame, r2_clear=self.r2c, max_level=self.max_level,
                              out=_sub(p, "sc_"), **kw)
        cum, _ = ctx.bezier_arclength(sm["ctrl"], self.nsub)
        cum_c, _ = ctx.bezier_arclength(sc["ctrl"], self.nsub)
        sp = ctx.speed_limits(sm["ctrl"], cum, sm["seg_off"], sm["arclength"], d["lim"], d["dyn"], N=self.N, J=self.J, status=sm["status"], d2=d2,
                              frame=self.frame)
        cc = ctx.curve_clearance(sm["ctrl"], sm["seg_off"], d2, self.frame, self.r2c, status=sm["status"])
        cl = ctx.curve_clear(sm["ctrl"], sm["seg_off"], d2, self.frame, self.r2c, self.max_level, status=sm["status"])
        return dict(d2=d2, wp=wp, npts=npts, cum=cum, cum_c=cum_c, **_pre("a_", res), **_pre("w_", wr), **_pre("sm_", sm), **_pre("sl_", sl),
                    **_pre("sc_", sc), **_pre("sp_", sp), **_pre("cc_", cc), **_pre("cl_", cl))

    # -- the CPU side
    def _form(self, out, pre, tw, inp, pts, npts, d2, up, legs0, cum_key, dyn=None, status=None):
        """One smoothing call's expected arrays into `out` under the prefix `pre`.  legs0: the legs before any repair, float32
        [S,4,2] in the call's layout (None: from_path of the oracle), status: the per-path status the repair left."""
        import speed_twin
        o, P, S = tw.oracle, self.P, self.P * (self.Wmax - 1)
        lim = inp["lim"]
        ok = npts >= 2
        st = np.where(ok, SMOOTH_OK, SMOOTH_BAD_INPUT).astype(np.int32) if status is None else status
        seg_off = np.concatenate([[0], np.cumsum(np.where(ok, npts - 1, 0))]).astype(np.int32)
        g = (lambda k: np.asarray(up[pre + k])) if up is not None else None
        ctrl = np.zeros((S, 4, 2), np.float32)
        arcl, length = np.zeros(P, np.float32), np.zeros(P, np.int32)
        vmax, minc = np.ones((P, self.N + 1)), np.zeros(P, np.float32)           # the header: a skipped path gets vhi = 1 and min_clear = 0
        rows = {}
        for p in np.flatnonzero(ok):
            a, b = seg_off[p], seg_off[p + 1]
            ctrl[a:b] = o.bezier_from_path(pts[p, :npts[p]]) if legs0 is None else legs0[a:b]
            if st[p] != SMOOTH_OK:
                continue
            legs = ctrl[a:b] if up is None else g("ctrl")[a:b]
            tot, c64 = o.bezier_arclength(legs, self.nsub)
            cum = c64.astype(np.float32) if up is None else np.asarray(up[cum_key])[a:b]
            arcl[p] = tot
            AL = np.float32(cum[:, -1].astype(np.float32).cumsum(dtype=np.float32)[-1]) if up is None else g("arclength")[p]
            vlo, vhi = np.full(self.N + 1, lim[p, 0]), np.full(self.N + 1, lim[p, 1])
            if dyn is not None:
                t = speed_twin.speed_limits(legs, cum, AL, lim[p], dyn, N=self.N, J=self.J, d2=d2, frame=self.frame)
                assert not t["flagged"].any()
                vhi, vmax[p], minc[p] = t["vhi"], t["vhi"], np.float32(t["min_clear"])
            r = o.toppra([0.0], [float(AL)], [0.0], [0.0], vlo[:, None], vhi[:, None], [lim[p, 2]], [lim[p, 3]], N=self.N)
            assert r["status"] == 0
            s = o.toppra_sample([0.0], [float(AL)], [0.0], [0.0], r["x"], r["t"], float(np.float32(self.dt)))
            L = int(s["length"])
            length[p] = L if up is None or abs(L - int(g("length")[p])) > 1 else g("length")[p]
            if length[p] == L:
                rs = o.bezier_resample(legs, cum, AL, s["pos"][0, :L].astype(np.float32).copy(), True)
                assert rs["status"] == 0
                rows[p] = dict(pos=rs["pos"], vel=s["vel"][0, :L], pts=rs["pts"], curvature=rs["curvature"])
        assert len(rows) >= 0.75 * int((st == SMOOTH_OK).sum()), (pre, len(rows))
        offsets = np.concatenate([[0], np.cumsum(length)]).astype(np.int32)
        out.update({pre + "ctrl": ctrl, pre + "seg_off": seg_off, pre + "arclength": arcl, pre + "length": length, pre + "offsets": offsets,
                    pre + "status": st, pre + "needed": np.array([offsets[-1]], np.int64)})
        for k in ("pos", "vel", "pts", "curvature"):
            full = np.zeros((self.cap, 2) if k == "pts" else self.cap, np.float32) if up is None else g(k).copy()
            for p, row in rows.items():
                full[offsets[p]:offsets[p] + length[p]] = row[k]
            out[pre + k] = full
        return seg_off, st, vmax, minc

    def expected(self, inp, tw, up=None):
        import curve_twin
        import speed_twin
        o, P, S = tw.oracle, self.P, self.P * (self.Wmax - 1)
        d2 = o.edt(inp["occ"])
        res = o.astar_batch(d2, inp["start"], inp["goal"], r2=self.r2, Lmax=self.Lmax)
        wr = tw.waypoints.waypoints(d2, res["path"], res["len"], res["status"], r2=self.r2, Wmax=self.Wmax)
        assert (wr["status"] != Q_TRUNCATED).all()
        npts = np.where((wr["status"] == 0) & (wr["n"] >= 1), wr["n"], 0).astype(np.int32)
        x_min, y_min, rx, ry = (np.float32(v) for v in self.frame)
        c = np.where(np.arange(self.Wmax)[None, :] < npts[:, None], wr["wp"], 0)
        pts = np.stack([x_min + ((c % self.W).astype(np.float32) + np.float32(0.5)) * rx, y_min + ((c // self.W).astype(np.float32) + np.float32(0.5)) * ry], 2)
        pts = np.where((np.arange(self.Wmax)[None, :] < npts[:, None])[:, :, None], pts, 0).astype(np.float32)
        out = dict(d2=d2, wp=pts, npts=npts, **_pre("a_", {k: res[k] for k in ("path", "len", "cost", "status")}), **_pre("w_", wr))
        seg_off, st, _, _ = self._form(out, "sm_", tw, inp, pts, npts, d2, up, None, "cum")
        _, _, vmax, minc = self._form(out, "sl_", tw, inp, pts, npts, d2, up, None, "cum", dyn=self.dyn)
        out.update(sl_vmax_stage=vmax, sl_min_clear=minc)
        legs = out["sm_ctrl"] if up is None else np.asarray(up["sm_ctrl"])
        S_used = int(seg_off[-1])
        # the tables: of the legs of the run that is checked
        out["cum"] = np.zeros((S, self.nsub + 1)) if up is None else np.asarray(up["cum"]).astype(np.float64)
        out["cum"][:S_used] = o.bezier_arclength(legs[:S_used], self.nsub)[1]
        # the limits, the check and the repair on the plain call's legs
        sp_vhi, sp_minc = np.ones((P, self.N + 1)), np.zeros(P, np.float32)
        cum32 = out["cum"].astype(np.float32) if up is None else np.asarray(up["cum"])
        AL = out["sm_arclength"] if up is None else np.asarray(up["sm_arclength"])
        if up is None:
            AL = np.array([cum32[seg_off[p]:seg_off[p + 1], -1].cumsum(dtype=np.float32)[-1] if st[p] == 0 else 0 for p in range(P)], np.float32)
        for p in np.flatnonzero(st == 0):
            t = speed_twin.speed_limits(legs[seg_off[p]:seg_off[p + 1]], cum32[seg_off[p]:seg_off[p + 1]], AL[p], inp["lim"][p], self.dyn, N=self.N,
                                        J=self.J, d2=d2, frame=self.frame)
            sp_vhi[p], sp_minc[p] = t["vhi"], np.float32(t["min_clear"])
        out.update(sp_vhi=sp_vhi, sp_min_clear=sp_minc, sp_status=st)
        cc = curve_twin.clearance(legs, seg_off, d2, self.frame, self.r2c, status=st)
        cc["leg_min"] = np.concatenate([cc["leg_min"], np.full(S - S_used, -1, np.int32)])
        cl = curve_twin.clear(legs, seg_off, d2, self.frame, self.r2c, self.max_level, status=st)
        cl_full = dict(ctrl=np.zeros((S, 4, 2), np.float32), level=np.zeros(S + P, np.uint8), rounds=cl["rounds"], status=cl["status"],
                       leg_min=np.concatenate([cl["leg_min"], np.full(S - S_used, -1, np.int32)]))
        cl_full["ctrl"][:S_used], cl_full["level"][:S_used + P] = cl["ctrl"], cl["level"]
        out.update(**_pre("cc_", cc), **_pre("cl_", cl_full))
        # the call that repairs: its legs are the repair of the plain call's, its samples the CPU chain on them
        self._form(out, "sc_", tw, inp, pts, npts, d2, up, cl_full["ctrl"], "cum_c", status=cl["status"])
        out.update(sc_level=cl_full["level"], sc_leg_min=cl_full["leg_min"], sc_rounds=cl["rounds"])
        legs_c = out["sc_ctrl"] if up is None else np.asarray(up["sc_ctrl"])
        out["cum_c"] = np.zeros((S, self.nsub + 1)) if up is None else np.asarray(up["cum_c"]).astype(np.float64)
        out["cum_c"][:S_used] = o.bezier_arclength(legs_c[:S_used], self.nsub)[1]
        return out

    tol.update(cum=(2e-6, 1e-6), cum_c=(2e-6, 1e-6))

    def view(self, o):
        S_used = int(np.asarray(o["sm_seg_off"])[-1])
        out = {k: np.asarray(o[k]) for k in ("d2", "npts", "sl_vmax_stage", "sl_min_clear", "sp_vhi", "sp_min_clear", "sp_status", "cc_leg_min",
                                             "cc_path_min", "cc_hit_legs", "cc_hit_leg", "cc_hit_t", "cl_rounds", "cl_status", "cl_leg_min",
                                             "sc_rounds")}
        out.update(paths_view(_sub(o, "a_"), "a_"))
        n, st = np.asarray(o["w_n"]), np.asarray(o["w_status"])
        out.update(w_n=n, w_status=st, w_wp=np.where((np.arange(self.Wmax)[None, :] < n[:, None]) & (st == Q_OK)[:, None], np.asarray(o["w_wp"]), -1))
        out["wp"] = np.where((np.arange(self.Wmax)[None, :] < out["npts"][:, None])[:, :, None], np.asarray(o["wp"]), 0)
        legs = lambda a, n: np.where((np.arange(len(a)) < n).reshape((-1,) + (1,) * (a.ndim - 1)), a, 0)      # what a call wrote
        for k in ("cum", "cum_c"):
            out[k] = legs(np.asarray(o[k]), S_used)
        out.update(cl_ctrl=legs(np.asarray(o["cl_ctrl"]), S_used), cl_level=legs(np.asarray(o["cl_level"]), S_used + self.P),
                   sc_level=legs(np.asarray(o["sc_level"]), S_used + self.P), sc_leg_min=legs(np.asarray(o["sc_leg_min"]), S_used))
        for f in self.forms:
            M = int(np.asarray(o[f + "needed"])[0])
            for k in ("seg_off", "length", "offsets", "status", "needed"):
                out[f + k] = np.asarray(o[f + k])
            out[f + "arclength"] = np.where(out[f + "status"] == SMOOTH_OK, np.asarray(o[f + "arclength"]), 0)     # of the paths that were smoothed
            out[f + "ctrl"] = legs(np.asarray(o[f + "ctrl"]), S_used)
            for k in ("pos", "vel", "pts", "curvature"):
                out[f + k] = legs(np.asarray(o[f + k]), min(M, self.cap))
        return out


# ---- chain 3: smoothed paths -> knots -> conflicts -> shift table -> schedule -> shifted knots -> reservations -> re-plans -------
class Traj(Chain):
    """Behind one smooth_paths call (chain 2 holds that call to the CPU chain; here its samples, as this run wrote them, are
    what the twins start from, and every later array is theirs bit for bit)."""
    name = "3 traj"
    symbols = ("sc_traj_knots_batch", "sc_traj_conflicts_batch", "sc_fleet_conflicts_batch", "sc_traj_shift_table_batch", "sc_traj_schedule_batch",
               "sc_traj_shift_knots_batch", "sc_fleet_schedule_batch", "sc_traj_reserve_batch", "sc_tplan_batch", "sc_fleet_replan_batch")
    staged = True
    W, H, P, n, B, K, D, stride, dt_c, pad, cap = 48, 32, 8, 4, 4, 80, 4, 2, 0.5, 0.2, 8 * 4000
    frame = (0.0, 0.0, 0.25, 0.25)

    def inputs(self, which):
        rng = _rng(which, 3)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        wp = np.stack([rng.uniform(1.0, 11.0, (self.P, self.n)), rng.uniform(1.0, 7.0, (self.P, self.n))], 2).astype(np.float32)
        occ = _salt_occ(self.W, self.H, 0.03, which, 3)
        free = np.flatnonzero(occ.ravel() == 0)
        npts, radius = np.full(self.P, self.n, np.int32), rng.uniform(0.2, 0.5, self.P)
        bstart = rng.choice(free, self.B)
        bstart["ABC".index(which)] = -1                            # TP_BAD_ENDPOINT: another robot in every set
        npts["ABC".index(which)] = 1                               # not smoothed: a skipped path, another one in every set
        radius[3 + "ABC".index(which)] = -1.0                      # outside the contract: TRAJ_BAD
        return dict(wp=wp, npts=npts, lim=f64(np.tile([-1.0, 1.0, -0.5, 0.5], (self.P, 1))), occ=occ,
                    radius=f64(radius), group=i32(rng.integers(-1, 3, self.P)), t0=f64(rng.uniform(0, 3, self.P)),
                    flags=i32(rng.integers(0, 4, self.P)), order=i32(rng.permutation(self.P)), jmax=i32(rng.integers(-1, self.D, self.P)),
                    select=i32(rng.integers(0, 2, self.P)), bstart=i32(bstart), bgoal=i32(rng.choice(free, self.B)),
                    t_start=i32(rng.integers(0, 5, self.B)), r_new=f64(rng.uniform(0.2, 0.4, self.B)))

    def run(self, ctx, d, prev=None):
        import torch
        kw = dict(T0=0.0, dt_c=self.dt_c, K=self.K)
        sm = ctx.smooth_paths(d["wp"], d["npts"], d["lim"], capacity=self.cap)
        kn = ctx.traj_knots(sm, t0=d["t0"], flags=d["flags"], **kw)
        knots, ts = kn["knots"], kn["tstatus"].clone()
        cf = ctx.traj_conflicts(knots, kn["tstatus"], d["radius"], group=d["group"], dt_c=self.dt_c, want_matrix=True)
        fc = ctx.fleet_conflicts(sm, d["radius"], t0=d["t0"], flags=d["flags"], group=d["group"], want_matrix=True, want_knots=True, **kw)
        tb = ctx.traj_shift_table(knots, ts.clone(), d["radius"], group=d["group"], D=self.D, stride=self.stride)
        sch = ctx.traj_schedule(tb["table"], tb["tstatus"], D=self.D, order=d["order"], jmax=d["jmax"])
        sk = ctx.traj_shift_knots(knots, sch["slot"], stride=self.stride)
        fs = ctx.fleet_schedule(sm, d["radius"], t0=d["t0"], flags=d["flags"], group=d["group"], D=self.D, stride=self.stride, order=d["order"],
                                jmax=d["jmax"], want_table=True, want_knots=True, **kw)
        d2 = ctx.edt(d["occ"])
        rs_ts = tb["tstatus"].clone()
        res = ctx.traj_reserve(sk, rs_ts, d["radius"], self.W, self.H, self.frame, self.pad, select=d["select"])
        tp = ctx.tplan(d2, d["bstart"], d["bgoal"], res, t_start=d["t_start"], frame=self.frame)
        fr = ctx.fleet_replan(sk, tb["tstatus"].clone(), d["radius"], d2, d["bstart"], d["bgoal"], self.frame, self.pad, r_new=d["r_new"],
                              select=d["select"], t_start=d["t_start"], sequential=True)
        out = dict(ts=ts, sk=sk, res=res, rs_ts=rs_ts, **_pre("sm_", {k: sm[k] for k in ("time", "pts", "offsets", "length", "status")}),
                   **_pre("kn_", kn), **_pre("cf_", cf), **_pre("fc_", fc), **_pre("tb_", tb), **_pre("sch_", sch), **_pre("fs_", fs), **_pre("tp_", tp),
                   **_pre("fr_", fr))
        return {k: v for k, v in out.items() if torch.is_tensor(v)}

    def expected(self, inp, tw, up=None):
        import tplan_twin
        import traj_sched_twin as sched
        import traj_twin
        P, L = self.P, self.K + 1
        if up is None:                                             # the oracle's smoothing, on the sampler's clock
            one = [tw.oracle.smooth_one(inp["wp"][p], vmax=1.0, amax=0.5, dt=0.02) for p in np.flatnonzero(inp["npts"] >= 2)]
            length = np.zeros(P, np.int32)
            length[inp["npts"] >= 2] = [o["length"] for o in one]
            sm = dict(time=np.concatenate([np.arange(n) * float(np.float32(0.02)) for n in length]), pts=np.concatenate([o["pts"] for o in one]),
                      offsets=np.concatenate([[0], np.cumsum(length)]).astype(np.int32), length=length, status=(inp["npts"] < 2).astype(np.int32))
        else:
            sm = {k: np.asarray(up["sm_" + k]) for k in ("time", "pts", "offsets", "length", "status")}
            ok = inp["npts"] >= 2
            assert np.array_equal(sm["status"] == 0, ok) and (sm["length"][ok] > 100).all() and int(sm["offsets"][-1]) <= self.cap
        path = (sm["time"], sm["pts"], sm["offsets"], sm["length"], sm["status"], inp["t0"], inp["flags"], 0.0, self.dt_c, self.K)
        radius, group = inp["radius"], inp["group"]
        kn, ts = traj_twin.knots(*path)
        cf = traj_twin.conflicts(kn, ts, 0.0, self.dt_c, radius, group)
        fc = traj_twin.fleet(*path, radius, group)
        table, ts2 = sched.shift_table(kn, ts, radius, group, self.D, self.stride)
        slot, counts = sched.schedule(table, ts2, self.D, inp["order"], inp["jmax"])
        sk = sched.shift_knots(kn, slot, self.stride)
        fs = sched.fleet_schedule(*path, radius, group, self.D, self.stride, inp["order"], inp["jmax"])
        d2 = tw.oracle.edt(inp["occ"])
        res, ts3 = tplan_twin.reserve(sk, ts2, radius, inp["select"], self.pad, self.W, self.H, self.frame)
        tp = tplan_twin.plan(d2, 0, res, L, inp["bstart"], inp["bgoal"], inp["t_start"], True, self.frame)
        fr = tplan_twin.fleet_replan(sk, ts2, radius, inp["select"], self.pad, self.W, self.H, self.frame, None, d2, 0, inp["bstart"], inp["bgoal"],
                                     inp["t_start"], True, inp["r_new"], sequential=True)
        fr["res"] = tplan_twin.pack(fr["res"])
        return dict(ts=ts, sk=sk, res=tplan_twin.pack(res), rs_ts=ts3, **_pre("sm_", sm), kn_knots=kn, kn_tstatus=cf["tstatus"], **_pre("cf_", cf),
                    **_pre("fc_", fc), tb_table=table, tb_tstatus=ts2, sch_slot=slot, sch_counts=counts, **_pre("fs_", fs), **_pre("tp_", tp),
                    **_pre("fr_", fr))

    def view(self, o):
        out = {}
        for k, v in o.items():
            v = np.asarray(v)
            if k.startswith("sm_"):
                continue                                           # this run's own samples: where the twins start, not a result
            if v.dtype.kind in "iu" and v.dtype.itemsize == 8 and "table" in k:
                v = v.view(np.uint64)                              # torch holds the bit words as signed integers
            if k.endswith("conflict") or k.endswith("res"):
                v = v.view(np.uint32)
            if k.endswith("_path"):
                v = np.where(np.arange(v.shape[1])[None, :] < np.asarray(o[k[:-4] + "len"])[:, None], v, -1)
            out[k] = v
        return out


CHAINS = [Grids(), Smooth(), Traj(), Components(), Fields(), Explore(), Views(), Scan(), Pose(), Toppra(), Bezier(), Fmt(), Gather()]


def declared_symbols():
    return set().union(*(c.symbols for c in CHAINS))
