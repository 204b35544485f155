"""sea_current_amd -- Python plumbing over libsea_current_hip.so (MI355X / gfx950).

The product is the C-ABI library (include/sea_current_hip.h) and the C++ header
sea-current_amd/sea_current.hpp; this module only binds the C ABI with ctypes so that
tests/ and bench.py can drive it with torch device tensors.  There is NO CPU fallback:
if the HIP library is missing or no GPU is present, calls raise.

The ctypes signatures are read from the header at import (_signatures): the header is the only
place where the ABI is written down, and a declaration that cannot be mapped raises.  A device
method and its _host twin are two short delegations to one private body; the body takes the
home of its arrays (_Home: _HOST for numpy, _on(device) for torch), which holds everything the
twins differ in.  _ptr is the one function through which a pointer is taken.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
NATIVE_DIR = os.path.normpath(os.path.join(_PKG, "..", ".."))          # sea-current_amd/
REPO_ROOT = os.path.normpath(os.path.join(NATIVE_DIR, ".."))
LIB_PATH = os.environ.get("SC_LIB_PATH") or os.path.join(NATIVE_DIR, "libsea_current_hip.so")   # SC_LIB_PATH: experiment builds
HEADER_PATH = os.path.join(REPO_ROOT, "include", "sea_current_hip.h")
HEADER_UPDATE_PATH = os.path.join(REPO_ROOT, "include", "sea_current_hip_update.h")
HEADER_CAR_PATH = os.path.join(REPO_ROOT, "include", "sea_current_hip_car.h")

EDT_INF = 2**31 - 1
FIELD_INF = 2**31 - 1
FIELD_SEED_COST_MAX = 1 << 24
Q_OK, Q_NO_PATH, Q_BAD_ENDPOINT, Q_TRUNCATED, Q_RING_OVERFLOW, Q_BAD_PATH = 0, 1, 2, 3, 4, 5
K_EDT_COLBITS, K_EDT_BAND, K_MOVES, K_ASTAR, K_TOPPRA, K_TOPPRA_SAMPLE, K_BEZIER, K_ARCLENGTH, K_RESAMPLE, K_OCC, K_NEAREST, K_FMT, K_GATHER = range(13)
K_WAYPOINTS = 13
K_SMOOTH = 14
SMOOTH_OK, SMOOTH_BAD_INPUT, SMOOTH_NONFINITE, SMOOTH_TOPPRA_FAILED, SMOOTH_TRUNCATED, SMOOTH_EMPTY_SEGMENT = range(6)
SMOOTH_COLLIDES = 6
CURVE_MAX_LEGS, CURVE_MAX_LEVEL = 1024, 30
TRAJ_OK, TRAJ_SKIPPED, TRAJ_BAD = range(3)
TRAJ_MAX_TICKS = 65535
SLOT_UNRESOLVED, SLOT_NOT_OK, SLOT_UNNAMED = -1, -2, -3
TP_OK, TP_NO_PATH, TP_BAD_ENDPOINT, TP_START_BLOCKED = range(4)
ASSIGN_MAX_DIM = 1024
ASSIGN_BIG = 1 << 42
ASSIGN_OK, ASSIGN_BAD = 0, 1
SCAN_NO_RETURN, SCAN_IGNORED, SCAN_MAX_REACH = -1, -2, 16384
LOGODDS_HIT, LOGODDS_MISS, LOGODDS_CLAMP, LOGODDS_T_OCC, LOGODDS_T_FREE = 2, 1, 8, 2, 1   # logodds_update's defaults
SCAN_MATCH_ABSENT, SCAN_MATCH_IGNORED, SCAN_MATCH_MAX_HALF, SCAN_MATCH_MAX_POINTS, SCAN_MATCH_MAX_ROT = -2**31, -1, 64, 65536, 256
SCAN_MATCH_OVERFLOW, SCAN_MATCH_WIDE_MAX_HALF, SCAN_MATCH_WIDE_MAX_TOP = -2, 2048, 5
VIEW_MAX_BINS = 64
POSE_HEADINGS, FOOTPRINT_MAX = 8, 32
POSE_HX, POSE_HY = (1, 1, 0, -1, -1, -1, 0, 1), (0, 1, 1, 1, 0, -1, -1, -1)   # heading k, counter-clockwise in (x, y)
ARC_MAX = 4

_lib = None


class SeaCurrentError(RuntimeError):
    pass


def build(force=False):
    """Compile libsea_current_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", NATIVE_DIR, "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", NATIVE_DIR])
    return LIB_PATH


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_RESULTS = {"void": None, "int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}


def _signatures(header, path=HEADER_PATH):
    """{name: (restype, argtypes)} of every function the header declares: a pointer is c_void_p (which also takes byref() of
    the scalar outputs), a scalar its exact ctype.  A declaration this cannot map raises; none is skipped."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", "", header, flags=re.S)
    sigs = {}
    for res, name, params in re.findall(r"([\w \t]+?[\w*])\s*\b(sc_\w+)\s*\(([^()]*)\)\s*;", src):
        res = " ".join(res.replace("*", "* ").split()).replace(" *", "*")
        params = [" ".join(p.split()) for p in params.split(",")]
        if res not in _RESULTS:
            raise SeaCurrentError(f"{path}: {name}: no ctypes result type for '{res}'")
        args = []
        for p in ([] if params == ["void"] else params):
            words = [w for w in p.replace("*", " ").split() if w != "const"]
            if "*" not in p and (len(words) != 2 or words[0] not in _SCALARS):
                raise SeaCurrentError(f"{path}: {name}: no ctypes type for parameter '{p}'")
            args.append(C.c_void_p if "*" in p else _SCALARS[words[0]])
        sigs[name] = (_RESULTS[res], args)
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", src))
    if declared != set(sigs):
        raise SeaCurrentError(f"{path}: cannot read the declaration of {sorted(declared - set(sigs))}")
    return sigs


with open(HEADER_PATH) as _f:
    _SIGNATURES = _signatures(_f.read())
EXPORTS = tuple(_SIGNATURES)
# the field repair's header of its own: read the same way, kept in a table of its own
with open(HEADER_UPDATE_PATH) as _f:
    _SIGNATURES_UPDATE = _signatures(_f.read(), HEADER_UPDATE_PATH)
EXPORTS_UPDATE = tuple(_SIGNATURES_UPDATE)
# car-like pose planning's header of its own, likewise
with open(HEADER_CAR_PATH) as _f:
    _SIGNATURES_CAR = _signatures(_f.read(), HEADER_CAR_PATH)
EXPORTS_CAR = tuple(_SIGNATURES_CAR)


def lib():
    """Load the in-tree HIP library; fail loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SeaCurrentError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                  "or `make -C sea-current_amd` (there is no CPU fallback)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in list(_SIGNATURES.items()) + list(_SIGNATURES_UPDATE.items()) + list(_SIGNATURES_CAR.items()):
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def _ptr(t):
    """Device/host pointer of a torch tensor or numpy array (must be contiguous)."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return t.ctypes.data
    assert t.is_contiguous()
    return t.data_ptr()


def _count(x):
    """Elements of a torch tensor or numpy array."""
    return int(x.size) if isinstance(x, np.ndarray) else int(x.numel())


def _sized(what, x, n):
    """x (may be None) has n elements: the calls whose grid size is an argument, not a tensor's shape, check it here, since
    the library would write W * H elements whatever the tensor holds."""
    if x is not None and _count(x) != n:
        raise SeaCurrentError(f"{what} has {_count(x)} elements, the call needs {n}")


def _car_ranges(arc_n, arc_cost, rev_cost):
    """The parameter ranges of the car calls (include/sea_current_hip_car.h), refused before the library is reached."""
    if not (1 <= int(arc_n) <= ARC_MAX and 0 <= int(arc_cost) <= 255 and -1 <= int(rev_cost) <= 255):
        raise SeaCurrentError(f"arc_n {arc_n} (1 .. {ARC_MAX}), arc_cost {arc_cost} (0 .. 255) or rev_cost {rev_cost} (-1 .. 255) out of range")


def _ghw(d2):
    """(G, H, W) of a map-shaped tensor or array: [H,W] is one grid, [G,H,W] a stack."""
    return (1,) + tuple(d2.shape) if len(d2.shape) == 2 else tuple(d2.shape)


class _Home:
    """Where the arrays of a call live.  A device method and its _host twin are one body that takes a home: _HOST (numpy) or
    _on(device) (torch).  What differs between the twins is here and nowhere else: the suffix of the C name, how an output is
    allocated (new), how an input is taken (arr, own, words, seq), how a per-path argument is broadcast (per_path, rows4), and
    the dtypes, of which only the bit words w16 / w32 / w64 differ."""

    def paths_out(self, Q, Lmax, which=False):
        """The result dict of a path read-out (astar_batch's layout; which: the multi-source read-out's).  On the host path
        is -1 and the rest 0; on the device nothing is initialised."""
        out = dict(path=self.new((Q, Lmax), self.i32, host_fill=-1))
        for k in ("len", "cost", "status") + (("which",) if which else ()):
            out[k] = self.new(Q, self.i32)
        return out

    def traj_out(self, P, want_matrix):
        """traj_conflicts' result dict; the bits of a conflict row are w32 words: bit q % 32 of word q // 32."""
        f, i = (lambda: self.new(P, self.f64)), (lambda: self.new(P, self.i32))
        return dict(first_t=f(), first_with=i(), min_sep=f(), min_with=i(), n_conf=i(),
                    conflict=self.new((P, (P + 31) // 32), self.w32) if want_matrix else None)

    def timed_paths(self, sm):
        """time, pts, offsets, length and status (or None) of smooth_paths' dict, as the C calls take them."""
        return dict(time=self.arr(sm["time"], self.f64), pts=self.arr(sm["pts"], self.f32), offsets=self.arr(sm["offsets"], self.i32),
                    length=self.arr(sm["length"], self.i32), status=self.arr(sm.get("status"), self.i32))

    def field_entry(self, stem, pen, pen_cap):
        """The single-root field entry `stem` (sc_cost_field / sc_field_paths) for a costmap or none: its name and the
        arguments the weighted form takes after d2."""
        name = stem + ("_batch" if pen is None else "_weighted_batch") + self.suffix
        return name, (() if pen is None else (_ptr(pen), pen_cap))


class _Host(_Home):
    """numpy: inputs are coerced to contiguous arrays of the C type (lists are accepted), outputs are zero-filled unless a
    fill is given, bit words are unsigned."""
    suffix = "_host"
    u8, i32, i64, f32, f64, w32, w64 = np.uint8, np.int32, np.int64, np.float32, np.float64, np.uint32, np.uint64
    w16 = np.uint16

    @staticmethod
    def new(shape, dtype, fill=None, host_fill=0):
        fill = host_fill if fill is None else fill
        return np.zeros(shape, dtype) if fill == 0 else np.full(shape, fill, dtype)

    @staticmethod
    def arr(x, dtype):
        """An input: contiguous, of dtype; None stays None."""
        return None if x is None else np.ascontiguousarray(x, dtype=dtype)

    seq = arr

    @staticmethod
    def rows(x, dtype, n):
        """An input of n numbers per row, which may come flat: [-1, n]."""
        return None if x is None else np.ascontiguousarray(x, dtype=dtype).reshape(-1, n)

    @staticmethod
    def own(x, dtype):
        """An argument the call writes to: a copy, the caller's array is not updated."""
        return None if x is None else np.array(x, dtype=dtype)

    @staticmethod
    def words(x, dtype):
        """Bit words of either signedness, viewed as dtype."""
        return None if x is None else np.ascontiguousarray(x).view(dtype)

    @staticmethod
    def per_path(v, P, dtype):
        """A per-path argument as a contiguous [P] array of dtype (a number stands for every path; None stays None)."""
        return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (P,)))

    @staticmethod
    def rows4(v, P):
        """Four numbers per path, or the same four for every path, as float64 [P,4]."""
        return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (P, 4)))

    @staticmethod
    def delay(slot, stride, dt_c):
        """Start delays in seconds of fleet_schedule's slots, NaN for slot < 0."""
        with np.errstate(invalid="ignore"):
            return np.where(slot >= 0, (slot * stride).astype(np.float64) * dt_c, np.nan)


class _Device(_Home):
    """torch tensors on one device: inputs are taken as they are (never converted, copied or moved; _ptr asserts that they
    are contiguous), outputs are uninitialised unless a fill is given, arguments the call writes to are updated in place, and
    bit words are signed (torch has no uint32 / uint64 arithmetic)."""
    suffix = ""

    def __init__(self, dev):
        import torch
        self.torch, self.dev = torch, dev
        self.u8, self.i32, self.i64, self.f32, self.f64 = torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64
        self.w16, self.w32, self.w64 = torch.int16, torch.int32, torch.int64

    def new(self, shape, dtype, fill=None, host_fill=0):
        if fill is None:
            return self.torch.empty(shape, dtype=dtype, device=self.dev)
        return self.torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dtype, device=self.dev)

    @staticmethod
    def arr(x, dtype):
        return x

    own = words = arr

    @staticmethod
    def rows(x, dtype, n):
        return x

    def seq(self, x, dtype):
        """A tensor or a list of numbers as a contiguous tensor of dtype."""
        return None if x is None else (x if self.torch.is_tensor(x) else self.torch.tensor(x, device=self.dev)).to(dtype).contiguous()

    def per_path(self, v, P, dtype):
        if v is None:
            return None
        v = v if self.torch.is_tensor(v) else self.torch.tensor(v, dtype=dtype, device=self.dev)
        return v.to(dtype).expand(P).contiguous()

    def rows4(self, v, P):
        v = v if self.torch.is_tensor(v) else self.torch.tensor([list(map(float, v))] * P, dtype=self.f64, device=self.dev)
        return v.to(self.f64).expand(P, 4).contiguous()

    def delay(self, slot, stride, dt_c):
        return self.torch.where(slot >= 0, (slot * stride).to(self.f64) * dt_c, float("nan"))


_HOST = _Host()
_homes = {}


def _on(dev):
    """The home of the tensors on torch device `dev`."""
    home = _homes.get(dev)
    if home is None:
        home = _homes[dev] = _Device(dev)
    return home


class Context:
    """One sc_ctx: one GPU, one stream.  `device` is the HIP device ordinal."""

    def __init__(self, device=0, use_torch_stream=True):
        # torch brings its own HIP runtime: let it initialise first, so that the library binds to the runtime that is already
        # in the process (loaded the other way round, the second runtime finds no GPU)
        import torch
        torch.cuda.is_available()
        self._l = lib()
        h = C.c_void_p()
        st = self._l.sc_ctx_create(device, C.byref(h))
        if st != 0:
            raise SeaCurrentError(f"sc_ctx_create(device={device}): {self._l.sc_status_string(st).decode()} "
                                  "(a gfx950 GPU is required; there is no CPU fallback)")
        self._h = h
        self.device = device
        if use_torch_stream:
            import torch
            self.set_stream(torch.cuda.current_stream(device).cuda_stream)

    def _ck(self, st, what):
        if st != 0:
            raise SeaCurrentError(f"{what}: {self._l.sc_status_string(st).decode()}: "
                                  f"{self._l.sc_last_error(self._h).decode()}")

    def close(self):
        if self._h:
            self._l.sc_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        self._ck(self._l.sc_ctx_set_stream(self._h, C.c_void_p(hip_stream or None)), "sc_ctx_set_stream")

    def use_own_stream(self):
        self._ck(self._l.sc_ctx_use_own_stream(self._h), "sc_ctx_use_own_stream")

    def synchronize(self):
        self._ck(self._l.sc_ctx_synchronize(self._h), "sc_ctx_synchronize")

    # -- timing
    def set_timing(self, on):
        self._ck(self._l.sc_ctx_set_timing(self._h, int(bool(on))), "sc_ctx_set_timing")

    def reset_timing(self):
        self._ck(self._l.sc_ctx_reset_timing(self._h), "sc_ctx_reset_timing")

    def get_timing(self, kid):
        ms, n = C.c_double(0), C.c_int64(0)
        self._ck(self._l.sc_ctx_get_timing(self._h, kid, C.byref(ms), C.byref(n)), "sc_ctx_get_timing")
        return ms.value, n.value

    def scratch_bytes(self):
        b = C.c_int64(0)
        self._ck(self._l.sc_ctx_scratch_bytes(self._h, C.byref(b)), "sc_ctx_scratch_bytes")
        return b.value

    def _call(self, name, *args):
        self._ck(getattr(self._l, name)(self._h, *args), name)

    # -- entry points.  A method takes torch tensors on the GPU and only enqueues unless it says otherwise; its _host twin takes
    # numpy arrays (or lists) and returns numpy arrays.  Both delegate to one private body, which takes the home of the arrays.
    def edt(self, occ, out=None):
        """occ: uint8 [B,H,W] or [H,W] on the GPU -> int32 d2 of the same shape."""
        import torch
        assert occ.is_cuda and occ.dtype == torch.uint8
        return self._edt(_on(occ.device), occ.contiguous(), out)

    def edt_host(self, occ):
        return self._edt(_HOST, occ)

    def _edt(self, A, occ, out=None):
        occ = A.arr(occ, A.u8)
        o3 = occ if len(occ.shape) == 3 else occ[None]
        B, H, W = o3.shape
        if out is None:
            out = A.new(tuple(o3.shape), A.i32)
        self._call("sc_edt_u8_i32" + A.suffix, _ptr(o3), W, H, B, _ptr(out))
        return out if len(occ.shape) == 3 else out.reshape(H, W)

    def moves(self, d2, r2=0):
        import torch
        H, W = d2.shape
        out = torch.empty((H, W), dtype=torch.uint8, device=d2.device)
        self._ck(self._l.sc_moves_i32_u8(self._h, _ptr(d2), W, H, r2, _ptr(out)), "sc_moves_i32_u8")
        return out

    def astar_batch(self, d2, start, goal, r2=0, Lmax=4096, out=None, label=None):
        """d2 int32 [H,W]; start/goal int32 [Q] (GPU).  Returns dict of GPU tensors.  label (int32 [H,W], what components
        returned for the same d2 and r2): the screened search (sc_astar_batch_screened), the same results without searching
        the queries whose endpoints lie in different components."""
        return self._astar_batch(_on(d2.device), d2, start, goal, r2, Lmax, out, label)

    def astar_batch_host(self, d2, start, goal, r2=0, Lmax=4096):
        return self._astar_batch(_HOST, d2, start, goal, r2, Lmax)

    def _astar_batch(self, A, d2, start, goal, r2, Lmax, out=None, label=None):
        d2, start, goal = A.arr(d2, A.i32), A.arr(start, A.i32), A.arr(goal, A.i32)
        H, W = d2.shape
        Q = start.shape[0]
        if out is None:
            out = A.paths_out(Q, Lmax)
        res = [_ptr(out[k]) for k in ("path", "len", "cost", "status")]
        if label is not None:
            self._call("sc_astar_batch_screened", _ptr(d2), _ptr(label), 1, None, W, H, r2, _ptr(start), _ptr(goal), Q, Lmax, *res)
        else:
            self._call("sc_astar_batch" + A.suffix, _ptr(d2), W, H, r2, _ptr(start), _ptr(goal), Q, Lmax, *res)
        return out

    def astar_batch_multi(self, d2, qgrid, start, goal, r2=0, Lmax=4096, out=None, label=None):
        """Several grids in one launch: d2 int32 [G,H,W], qgrid int32 [Q] (grid of every query), start/goal int32 [Q].
        label (int32 [G,H,W] from components): the screened search, as in astar_batch."""
        G, H, W = d2.shape
        Q = start.shape[0]
        if out is None:
            out = _on(d2.device).paths_out(Q, Lmax)
        if label is not None:
            self._ck(self._l.sc_astar_batch_screened(self._h, _ptr(d2), _ptr(label), G, _ptr(qgrid), W, H, r2, _ptr(start), _ptr(goal), Q,
                                                     Lmax, _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]), _ptr(out["status"])),
                     "sc_astar_batch_screened")
            return out
        self._ck(self._l.sc_astar_batch_multi(self._h, _ptr(d2), G, _ptr(qgrid), W, H, r2, _ptr(start), _ptr(goal), Q, Lmax,
                                              _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]), _ptr(out["status"])), "sc_astar_batch_multi")
        return out

    def components(self, d2, r2=0, want_size=False, out=None):
        """Connected components of the traversable cells (sc_components_batch).  d2 int32 [H,W] or [G,H,W] on the GPU.
        Returns dict(label int32 shaped like d2: the smallest cell index of the cell's component, -1 where it is not
        traversable; size int32 shaped like d2 (the cell count at every representative, 0 elsewhere) or None without
        want_size; ncomp int32 [G]; largest int32 [G], -1 on a grid without a traversable cell).  `out`: the dict of an
        earlier call with the same shapes, reused.  Only enqueues."""
        return self._components(_on(d2.device), d2, r2, want_size, out)

    def components_host(self, d2, r2=0, want_size=False):
        """Host form of components (numpy in, numpy out)."""
        return self._components(_HOST, d2, r2, want_size)

    def _components(self, A, d2, r2, want_size, out=None):
        d2 = A.arr(d2, A.i32)
        G, H, W = _ghw(d2)
        if out is None:
            shape = tuple(d2.shape)
            out = dict(label=A.new(shape, A.i32), size=A.new(shape, A.i32) if want_size else None, ncomp=A.new(G, A.i32),
                       largest=A.new(G, A.i32))
        self._call("sc_components_batch" + A.suffix, _ptr(d2), G, W, H, r2, _ptr(out["label"]), _ptr(out.get("size")), _ptr(out["ncomp"]),
                   _ptr(out["largest"]))
        return out

    def reachable(self, label, start, goal, qgrid=None):
        """The status astar_batch would give every query, from the labels alone (sc_reachable_batch): label int32 [H,W] or
        [G,H,W] from components, start / goal int32 [Q], qgrid int32 [Q] (None only with one grid), on the GPU.  Returns
        int32 [Q]: Q_BAD_ENDPOINT, Q_NO_PATH, or Q_OK where A* returns Q_OK or Q_TRUNCATED."""
        return self._reachable(_on(label.device), label, start, goal, qgrid)

    def reachable_host(self, label, start, goal, qgrid=None):
        """Host form of reachable (numpy in, numpy out)."""
        return self._reachable(_HOST, label, start, goal, qgrid)

    def _reachable(self, A, label, start, goal, qgrid):
        label, start, goal, qgrid = (A.arr(a, A.i32) for a in (label, start, goal, qgrid))
        G, H, W = _ghw(label)
        Q = start.shape[0]
        status = A.new(Q, A.i32)
        self._call("sc_reachable_batch" + A.suffix, _ptr(label), G, _ptr(qgrid), W, H, _ptr(start), _ptr(goal), Q, _ptr(status))
        return status

    def clearance_penalty(self, d2, r2=0, r2_soft=36, pen_max=40, out=None):
        """The costmap of the weighted cost fields from d2 (sc_clearance_penalty_u8): d2 int32 [H,W] or [G,H,W] on the GPU ->
        uint8 of the same shape, pen_max next to the hard clearance falling linearly to 0 at distance sqrt(r2_soft)."""
        return self._clearance_penalty(_on(d2.device), d2, r2, r2_soft, pen_max, out)

    def clearance_penalty_host(self, d2, r2=0, r2_soft=36, pen_max=40):
        """Host form of clearance_penalty (numpy in, numpy out)."""
        return self._clearance_penalty(_HOST, d2, r2, r2_soft, pen_max)

    def _clearance_penalty(self, A, d2, r2, r2_soft, pen_max, out=None):
        d2 = A.arr(d2, A.i32)
        G, H, W = _ghw(d2)
        if out is None:
            out = A.new(tuple(d2.shape), A.u8)
        self._call("sc_clearance_penalty_u8" + A.suffix, _ptr(d2), W, H, G, r2, r2_soft, pen_max, _ptr(out))
        return out

    def cost_fields(self, d2, roots, r2=0, fgrid=None, rounds=-1, out=None, pen=None, pen_cap=255):
        """Cost-to-come fields (sc_cost_field_batch).  d2 int32 [H,W] or [G,H,W], roots int32 [F], fgrid int32 [F] (the grid
        of every field; None only with one grid), all on the GPU.  Returns dict(g int32 [F,H,W], status int32 [F]).
        pen (uint8, shaped like d2): the weighted fields (sc_cost_field_weighted_batch), entering cell c costs
        min(pen[c], pen_cap) more."""
        return self._cost_fields(_on(d2.device), d2, roots, r2, fgrid, rounds, pen, pen_cap, out)

    def cost_fields_host(self, d2, roots, r2=0, fgrid=None, rounds=-1, pen=None, pen_cap=255):
        """Host form of cost_fields (numpy in, numpy out)."""
        return self._cost_fields(_HOST, d2, roots, r2, fgrid, rounds, pen, pen_cap)

    def _cost_fields(self, A, d2, roots, r2, fgrid, rounds, pen, pen_cap, out=None):
        d2, roots, fgrid, pen = A.arr(d2, A.i32), A.arr(roots, A.i32), A.arr(fgrid, A.i32), A.arr(pen, A.u8)
        G, H, W = _ghw(d2)
        F = roots.shape[0]
        if out is None:
            out = dict(g=A.new((F, H, W), A.i32), status=A.new(F, A.i32))
        name, costmap = A.field_entry("sc_cost_field", pen, pen_cap)
        self._call(name, _ptr(d2), *costmap, G, _ptr(fgrid), W, H, r2, _ptr(roots), F, rounds, _ptr(out["g"]), _ptr(out["status"]))
        return out

    def cost_fields_update(self, d2_old, d2_new, g, roots, r2=0, fgrid=None, rounds=-1, pen_old=None, pen_new=None, pen_cap=255, stats=True):
        """Repair cost fields after a map change (sc_cost_field_update_batch): g int32 [F,H,W] holds the fields cost_fields
        built on d2_old (with pen_old) for these roots, r2, fgrid and pen_cap, and is updated in place to what cost_fields
        returns on d2_new (with pen_new), bit for bit.  Returns dict(g, status int32 [F], stats int32 [F,2] or None): per
        field the changed cells of its grid and the cells that lost their support."""
        return self._cost_fields_update(_on(d2_new.device), d2_old, d2_new, g, roots, r2, fgrid, rounds, pen_old, pen_new, pen_cap, stats)

    def cost_fields_update_host(self, d2_old, d2_new, g, roots, r2=0, fgrid=None, rounds=-1, pen_old=None, pen_new=None, pen_cap=255,
                                stats=True):
        """Host form of cost_fields_update (numpy in, numpy out; the g returned is a copy, the caller's array stays)."""
        return self._cost_fields_update(_HOST, d2_old, d2_new, g, roots, r2, fgrid, rounds, pen_old, pen_new, pen_cap, stats)

    def _cost_fields_update(self, A, d2_old, d2_new, g, roots, r2, fgrid, rounds, pen_old, pen_new, pen_cap, stats):
        d2_old, d2_new, roots, fgrid = (A.arr(a, A.i32) for a in (d2_old, d2_new, roots, fgrid))
        pen_old, pen_new, g = A.arr(pen_old, A.u8), A.arr(pen_new, A.u8), A.own(g, A.i32)
        G, H, W = _ghw(d2_new)
        F = roots.shape[0]
        if (pen_old is None) != (pen_new is None):
            raise SeaCurrentError("pen_old and pen_new go together")
        _sized("d2_old", d2_old, G * H * W)
        _sized("pen_old", pen_old, G * H * W)
        _sized("pen_new", pen_new, G * H * W)
        _sized("g", g, F * H * W)
        _sized("fgrid", fgrid, F)
        out = dict(g=g, status=A.new(F, A.i32), stats=A.new((F, 2), A.i32) if stats else None)
        name = "sc_cost_field" + ("" if pen_new is None else "_weighted") + "_update_batch" + A.suffix
        maps = (_ptr(d2_old), _ptr(d2_new)) if pen_new is None else (_ptr(d2_old), _ptr(pen_old), _ptr(d2_new), _ptr(pen_new), pen_cap)
        self._call(name, *maps, G, _ptr(fgrid), W, H, r2, _ptr(roots), F, rounds, _ptr(g), _ptr(out["status"]), _ptr(out["stats"]))
        return out

    def field_paths(self, d2, g, roots, qfield, targets, r2=0, Lmax=4096, to_root=False, fgrid=None, out=None, pen=None, pen_cap=255):
        """Paths read from cost fields (sc_field_paths_batch): query q follows field qfield[q] (g int32 [F,H,W] and roots [F]
        as cost_fields took and returned them) to targets[q].  Returns astar_batch's dict of GPU tensors; to_root=True
        writes every path target..root.  pen, pen_cap: those cost_fields computed g with (sc_field_paths_weighted_batch)."""
        return self._field_paths(_on(d2.device), d2, g, roots, qfield, targets, r2, Lmax, to_root, fgrid, pen, pen_cap, out)

    def field_paths_host(self, d2, g, roots, qfield, targets, r2=0, Lmax=4096, to_root=False, fgrid=None, pen=None, pen_cap=255):
        """Host form of field_paths (numpy in, numpy out)."""
        return self._field_paths(_HOST, d2, g, roots, qfield, targets, r2, Lmax, to_root, fgrid, pen, pen_cap)

    def _field_paths(self, A, d2, g, roots, qfield, targets, r2, Lmax, to_root, fgrid, pen, pen_cap, out=None):
        d2, g, roots, qfield, targets, fgrid = (A.arr(a, A.i32) for a in (d2, g, roots, qfield, targets, fgrid))
        pen = A.arr(pen, A.u8)
        G, H, W = _ghw(d2)
        F, Q = roots.shape[0], targets.shape[0]
        if out is None:
            out = A.paths_out(Q, Lmax)
        name, costmap = A.field_entry("sc_field_paths", pen, pen_cap)
        self._call(name, _ptr(d2), *costmap, G, _ptr(fgrid), W, H, r2, _ptr(g), _ptr(roots), F, _ptr(qfield), _ptr(targets), Q, Lmax,
                   int(bool(to_root)), _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]), _ptr(out["status"]))
        return out

    def cost_fields_multi(self, d2, seeds, seed_off, seed_cost=None, r2=0, fgrid=None, rounds=-1, want_owner=True, pen=None, pen_cap=255,
                          out=None):
        """Multi-source cost fields (sc_cost_field_multi_batch): field f starts from seeds[seed_off[f]:seed_off[f+1]] (cell
        indices on grid fgrid[f]), each with the start cost seed_cost[s] (None: 0).  d2 int32 [H,W] or [G,H,W], seeds /
        seed_cost int32 [n_seed], seed_off int32 [F+1], fgrid int32 [F] (None only with one grid), pen uint8 shaped like d2
        (None: unweighted), all on the GPU.  Returns dict(g int32 [F,H,W], owner int32 [F,H,W]: the index into seeds of the
        seed every cell's path ends at, -1 where g is FIELD_INF, None without want_owner; status int32 [F])."""
        return self._cost_fields_multi(_on(d2.device), d2, seeds, seed_off, seed_cost, r2, fgrid, rounds, want_owner, pen, pen_cap, out)

    def cost_fields_multi_host(self, d2, seeds, seed_off, seed_cost=None, r2=0, fgrid=None, rounds=-1, want_owner=True, pen=None,
                               pen_cap=255):
        """Host form of cost_fields_multi (numpy in, numpy out)."""
        return self._cost_fields_multi(_HOST, d2, seeds, seed_off, seed_cost, r2, fgrid, rounds, want_owner, pen, pen_cap)

    def _cost_fields_multi(self, A, d2, seeds, seed_off, seed_cost, r2, fgrid, rounds, want_owner, pen, pen_cap, out=None):
        d2, seeds, seed_off, seed_cost, fgrid = (A.arr(a, A.i32) for a in (d2, seeds, seed_off, seed_cost, fgrid))
        pen = A.arr(pen, A.u8)
        G, H, W = _ghw(d2)
        F = seed_off.shape[0] - 1
        if out is None:
            out = dict(g=A.new((F, H, W), A.i32), owner=A.new((F, H, W), A.i32) if want_owner else None, status=A.new(F, A.i32))
        self._call("sc_cost_field_multi_batch" + A.suffix, _ptr(d2), _ptr(pen), pen_cap, G, _ptr(fgrid), W, H, r2, _ptr(seeds),
                   _ptr(seed_cost), _ptr(seed_off), seeds.shape[0], F, rounds, _ptr(out["g"]), _ptr(out.get("owner")), _ptr(out["status"]))
        return out

    def field_paths_multi(self, d2, fields, seeds, qfield, targets, r2=0, Lmax=4096, to_seed=False, fgrid=None, pen=None, pen_cap=255,
                          out=None):
        """Paths read from multi-source fields (sc_field_paths_multi_batch): query q follows field qfield[q] of `fields` (the
        dict cost_fields_multi returned, with its owner) from targets[q] to the seed that owns it.  Returns astar_batch's dict
        of GPU tensors plus which int32 [Q] (the index into seeds of that seed, -1 without a path); to_seed=True writes every
        path target..seed.  pen, pen_cap: those cost_fields_multi computed the fields with."""
        return self._field_paths_multi(_on(d2.device), d2, fields, seeds, qfield, targets, r2, Lmax, to_seed, fgrid, pen, pen_cap, out)

    def field_paths_multi_host(self, d2, fields, seeds, qfield, targets, r2=0, Lmax=4096, to_seed=False, fgrid=None, pen=None, pen_cap=255):
        """Host form of field_paths_multi (numpy in, numpy out)."""
        return self._field_paths_multi(_HOST, d2, fields, seeds, qfield, targets, r2, Lmax, to_seed, fgrid, pen, pen_cap)

    def _field_paths_multi(self, A, d2, fields, seeds, qfield, targets, r2, Lmax, to_seed, fgrid, pen, pen_cap, out=None):
        d2, g, owner, seeds, qfield, targets, fgrid = (A.arr(a, A.i32) for a in (d2, fields["g"], fields["owner"], seeds, qfield, targets,
                                                                                 fgrid))
        pen = A.arr(pen, A.u8)
        G, H, W = _ghw(d2)
        F, Q = g.shape[0], targets.shape[0]
        if out is None:
            out = A.paths_out(Q, Lmax, which=True)
        self._call("sc_field_paths_multi_batch" + A.suffix, _ptr(d2), _ptr(pen), pen_cap, G, _ptr(fgrid), W, H, r2, _ptr(g), _ptr(owner),
                   _ptr(seeds), seeds.shape[0], F, _ptr(qfield), _ptr(targets), Q, Lmax, int(bool(to_seed)), _ptr(out["path"]),
                   _ptr(out["len"]), _ptr(out["cost"]), _ptr(out["status"]), _ptr(out["which"]))
        return out

    def path_waypoints(self, d2, res, r2=0, Wmax=None, out=None):
        """Line-of-sight waypoints of astar_batch's paths (sc_path_waypoints_batch).  d2 int32 [H,W] and `res` (the dict
        astar_batch returned, same r2) on the GPU; Wmax defaults to its Lmax.  Returns dict(wp int32 [Q,Wmax] cell indices,
        n int32 [Q], status int32 [Q]) as GPU tensors."""
        return self._path_waypoints(_on(d2.device), d2, res["path"], res["len"], res.get("status"), r2, Wmax, out)

    def path_waypoints_host(self, d2, path, lens, status=None, r2=0, Wmax=None):
        """Host form of path_waypoints (numpy in, numpy out): path int32 [Q,Lmax], lens / status int32 [Q] (status may be None)."""
        return self._path_waypoints(_HOST, d2, path, lens, status, r2, Wmax)

    def _path_waypoints(self, A, d2, path, lens, status, r2, Wmax, out=None):
        d2, path, lens, status = (A.arr(a, A.i32) for a in (d2, path, lens, status))
        H, W = d2.shape
        Q, Lmax = path.shape
        if Wmax is None:
            Wmax = Lmax
        if out is None:
            out = dict(wp=A.new((Q, Wmax), A.i32, host_fill=-1), n=A.new(Q, A.i32), status=A.new(Q, A.i32))
        self._call("sc_path_waypoints_batch" + A.suffix, _ptr(d2), W, H, r2, _ptr(path), _ptr(lens), _ptr(status), Q, Lmax, Wmax,
                   _ptr(out["wp"]), _ptr(out["n"]), _ptr(out["status"]))
        return out

    def cells_to_points(self, wr, W, x_min, y_min, res_x, res_y, starts=None, goals=None):
        """path_waypoints' result (dict wp int32 [Q,Wmax], n, status) -> (path float32 [Q,Wmax,2], npts int32 [Q]), the cell
        centres of a W-wide grid (sc_cells_to_points_batch); starts / goals float32 [Q,2] replace the two ends."""
        import torch
        Q, Wmax = wr["wp"].shape
        dev = wr["wp"].device
        path = torch.zeros((Q, Wmax, 2), dtype=torch.float32, device=dev)
        npts = torch.empty(Q, dtype=torch.int32, device=dev)
        self._ck(self._l.sc_cells_to_points_batch(self._h, _ptr(wr["wp"]), _ptr(wr["n"]), _ptr(wr.get("status")), Q, Wmax, W, x_min, y_min,
                                                  res_x, res_y, _ptr(starts), _ptr(goals), _ptr(path), _ptr(npts)), "sc_cells_to_points_batch")
        return path, npts

    @staticmethod
    def _smooth_estimate(wp, npts, limits, dt):
        """Samples to reserve for smooth_paths(capacity=None), the rule of the C++ header's smooth_paths_batch: per path
        (1.5 * polyline length / vel_max + 2 vel_max / acc_max) / dt * 1.25 + 64 (64 where that is not finite).  Only a
        first guess: a call that needs more is repeated with the exact count."""
        import torch
        n_max = wp.shape[1]
        leg = (wp[:, 1:] - wp[:, :-1]).double().norm(dim=-1)
        use = torch.arange(n_max - 1, device=wp.device)[None, :] < (npts.long()[:, None] - 1)
        poly = torch.where(use, leg, torch.zeros_like(leg)).sum(1)
        v = torch.where(limits[:, 1] > 0, limits[:, 1], torch.ones_like(limits[:, 1]))
        a = torch.where(limits[:, 3] > 0, limits[:, 3], torch.ones_like(limits[:, 3]))
        T = 1.5 * poly / v + 2.0 * v / a
        est = torch.where(torch.isfinite(T), (T / dt * 1.25).clamp(max=1e6).floor() + 64, torch.full_like(T, 64.0))
        return int(est.sum().item())

    @staticmethod
    def _frame(d2, frame):
        """(W, H, x_min, y_min, res_x, res_y) of a grid argument; frame = (x_min, y_min, res_x, res_y)."""
        if d2 is None:
            return (0, 0, 0.0, 0.0, 0.0, 0.0)
        if frame is None:
            raise ValueError("d2 needs frame=(x_min, y_min, res_x, res_y)")
        H, W = d2.shape
        return (W, H) + tuple(float(v) for v in frame)

    def speed_limits(self, ctrl, cum, seg_off, arclength, limits, dyn, N=100, J=4, status=None, d2=None, frame=None):
        """Per-stage speed limits of P curves from curvature and clearance (sc_speed_limits_batch; the definition is in
        include/sea_current_hip.h).  GPU tensors: ctrl float32 [S,4,2], cum float32 [S,nsub+1], seg_off int32 [P+1], arclength
        float32 [P], limits / dyn float64 [P,4] or 4 numbers for every curve, dyn = (omega_max, alat_max, clear_floor,
        clear_gain), status int32 [P] or None, d2 int32 [H,W] with frame = (x_min, y_min, res_x, res_y) or None.  Returns
        dict(vhi float64 [P,N+1], min_clear float32 [P], status int32 [P])."""
        return self._speed_limits(_on(arclength.device), ctrl, cum, seg_off, arclength, limits, dyn, N, J, status, d2, frame)

    def speed_limits_host(self, ctrl, cum, seg_off, arclength, limits, dyn, N=100, J=4, status=None, d2=None, frame=None):
        """Host form of speed_limits (numpy in, numpy out; sc_speed_limits_batch_host checks the contract of dyn first)."""
        return self._speed_limits(_HOST, ctrl, cum, seg_off, arclength, limits, dyn, N, J, status, d2, frame)

    def _speed_limits(self, A, ctrl, cum, seg_off, arclength, limits, dyn, N, J, status, d2, frame):
        ctrl, cum, arclength = A.arr(ctrl, A.f32), A.arr(cum, A.f32), A.arr(arclength, A.f32)
        seg_off, status, d2 = A.arr(seg_off, A.i32), A.arr(status, A.i32), A.arr(d2, A.i32)
        P = arclength.shape[0]
        limits, dyn = A.rows4(limits, P), A.rows4(dyn, P)
        out = dict(vhi=A.new((P, N + 1), A.f64), min_clear=A.new(P, A.f32), status=A.new(P, A.i32))
        self._call("sc_speed_limits_batch" + A.suffix, _ptr(ctrl), _ptr(cum), _ptr(seg_off), _ptr(arclength), _ptr(status), P,
                   cum.shape[-1] - 1, N, J, _ptr(limits), _ptr(dyn), _ptr(d2), *self._frame(d2, frame), _ptr(out["vhi"]),
                   _ptr(out["min_clear"]), _ptr(out["status"]))
        return out

    def curve_clearance(self, ctrl, seg_off, d2, frame, r2_clear=0, status=None):
        """Which cells P curves visit (sc_curve_clearance_batch; the definition is in include/sea_current_hip.h).  GPU tensors:
        ctrl float32 [S,4,2], seg_off int32 [P+1], d2 int32 [H,W] with frame = (x_min, y_min, res_x, res_y), status int32 [P] or
        None.  Returns dict(leg_min int32 [S], path_min, hit_legs, hit_leg int32 [P], hit_t float32 [P]); the legs of skipped
        paths read -1 in leg_min."""
        return self._curve_clearance(_on(ctrl.device), ctrl, seg_off, d2, frame, r2_clear, status)

    def curve_clearance_host(self, ctrl, seg_off, d2, frame, r2_clear=0, status=None):
        """Host form of curve_clearance (numpy in, numpy out)."""
        return self._curve_clearance(_HOST, ctrl, seg_off, d2, frame, r2_clear, status)

    def _curve_clearance(self, A, ctrl, seg_off, d2, frame, r2_clear, status):
        ctrl, seg_off, d2, status = A.arr(ctrl, A.f32), A.arr(seg_off, A.i32), A.arr(d2, A.i32), A.arr(status, A.i32)
        P, S = seg_off.shape[0] - 1, ctrl.shape[0]
        o = dict(leg_min=A.new(S, A.i32, fill=-1), path_min=A.new(P, A.i32), hit_legs=A.new(P, A.i32), hit_leg=A.new(P, A.i32),
                 hit_t=A.new(P, A.f32))
        self._call("sc_curve_clearance_batch" + A.suffix, _ptr(ctrl), _ptr(seg_off), _ptr(status), P, _ptr(d2), *self._frame(d2, frame),
                   int(r2_clear), *[_ptr(o[k]) for k in ("leg_min", "path_min", "hit_legs", "hit_leg", "hit_t")])
        return o

    def curve_clear(self, ctrl, seg_off, d2, frame, r2_clear=0, max_level=6, status=None, inplace=False):
        """Shrink the tangents of curves that hit the grid until none does (sc_curve_clear_batch).  Arguments as
        curve_clearance; inplace=True repairs ctrl itself.  Returns dict(ctrl float32 [S,4,2], level uint8 [S+P] (waypoint j of
        path p at seg_off[p] + p + j), rounds int32 [P], leg_min int32 [S] (-1 on the legs of skipped paths), status int32 [P],
        SMOOTH_COLLIDES where shrinking did not help)."""
        return self._curve_clear(_on(ctrl.device), ctrl, seg_off, d2, frame, r2_clear, max_level, status, inplace)

    def curve_clear_host(self, ctrl, seg_off, d2, frame, r2_clear=0, max_level=6, status=None):
        """Host form of curve_clear (numpy in, numpy out)."""
        return self._curve_clear(_HOST, ctrl, seg_off, d2, frame, r2_clear, max_level, status)

    def _curve_clear(self, A, ctrl, seg_off, d2, frame, r2_clear, max_level, status, inplace=False):
        ctrl, seg_off, d2, status = A.arr(ctrl, A.f32), A.arr(seg_off, A.i32), A.arr(d2, A.i32), A.arr(status, A.i32)
        P, S = seg_off.shape[0] - 1, ctrl.shape[0]
        o = dict(ctrl=ctrl if inplace else A.new(tuple(ctrl.shape), ctrl.dtype), level=A.new(S + P, A.u8), rounds=A.new(P, A.i32),
                 leg_min=A.new(S, A.i32, fill=-1), status=A.new(P, A.i32))
        self._call("sc_curve_clear_batch" + A.suffix, _ptr(ctrl), _ptr(seg_off), _ptr(status), P, _ptr(d2), *self._frame(d2, frame),
                   int(r2_clear), int(max_level), *[_ptr(o[k]) for k in ("ctrl", "level", "rounds", "leg_min", "status")])
        return o

    def smooth_paths(self, wp, npts, limits, dt=0.02, N=100, nsub=100, start_angle=float("nan"), lines=None, capacity=None, out=None,
                     dyn=None, J=4, d2=None, frame=None, r2_clear=None, max_level=6):
        """The post-planner sequence for a batch of paths in one call (sc_smooth_paths_batch).  wp float32 [P,n_max,2],
        npts int32 [P], limits float64 [P,4] (vel_min, vel_max, acc_min, acc_max) or 4 numbers for every path, lines float32
        [E,4] or None; all on the GPU.  capacity=None: room for an estimate of the samples, the call repeated once with the
        exact count if that was short (reads `needed`: synchronises), and the per-sample outputs cut to `needed`.  With a
        capacity the call only enqueues.  `out`: the dict of an earlier call with the same P, n_max and capacity, reused.
        Returns dict(ctrl [P*(n_max-1),4,2], seg_off, arclength, length, offsets, status, needed [1], and per sample time,
        pos, vel, acc, pts [M,2], curvature, ang_vel, tpar, seg).
        dyn (float64 [P,4] or 4 numbers: omega_max, alat_max, clear_floor, clear_gain) asks for per-stage speed limits from
        curvature and, with d2 int32 [H,W] and frame = (x_min, y_min, res_x, res_y), clearance (sc_smooth_paths_limited_batch,
        J samples to each side of a stage); the dict then also holds vmax_stage float64 [P,N+1] and min_clear float32 [P].
        With dyn None the call is sc_smooth_paths_batch as before.
        r2_clear (needs d2; dyn None then means every speed term off) also keeps the curves clear of the grid
        (sc_smooth_paths_clear_batch): legs that visit a cell with d2 < max(r2_clear, 1) get the tangents at their ends halved,
        up to max_level times; the dict then also holds level uint8 [P*(n_max-1) + P], leg_min int32 [P*(n_max-1)] and rounds
        int32 [P], and a path that shrinking cannot fix reads SMOOTH_COLLIDES.  With r2_clear None the calls are those above."""
        return self._smooth_paths(_on(wp.device), wp, npts, limits, capacity, dt, N, nsub, start_angle, lines, dyn, J, d2, frame, r2_clear,
                                  max_level, out)

    def smooth_paths_host(self, wp, npts, limits, capacity, dt=0.02, N=100, nsub=100, start_angle=float("nan"), lines=None, dyn=None, J=4,
                          d2=None, frame=None, r2_clear=None, max_level=6):
        """Host form (numpy in, numpy out) of smooth_paths with room for `capacity` samples (sc_smooth_paths_batch_host; with
        dyn sc_smooth_paths_limited_batch_host, which adds vmax_stage and min_clear; with r2_clear
        sc_smooth_paths_clear_batch_host, which adds level, leg_min and rounds)."""
        return self._smooth_paths(_HOST, wp, npts, limits, capacity, dt, N, nsub, start_angle, lines, dyn, J, d2, frame, r2_clear, max_level)

    def _smooth_paths(self, A, wp, npts, limits, capacity, dt, N, nsub, start_angle, lines, dyn, J, d2, frame, r2_clear, max_level, out=None):
        if r2_clear is not None:
            if d2 is None:
                raise ValueError("r2_clear needs d2 and frame")
            if dyn is None:
                dyn = (float("inf"), float("inf"), float("inf"), 0.0)
        if dyn is None and d2 is not None:
            raise ValueError("d2 without dyn: the grid only enters through the speed limits")
        wp, npts, lines, d2 = A.arr(wp, A.f32), A.arr(npts, A.i32), A.arr(lines, A.f32), A.arr(d2, A.i32)
        P, n_max, _ = wp.shape
        S = P * (n_max - 1)
        limits = A.rows4(limits, P)
        if dyn is not None:
            dyn = A.rows4(dyn, P)
            fr = self._frame(d2, frame)
        nl = 0 if lines is None else lines.shape[0]
        auto = capacity is None
        cap = min(self._smooth_estimate(wp, npts, limits, dt), 2**31 - 1) if auto else int(capacity)
        f, i = (lambda *s: A.new(s, A.f32)), (lambda *s: A.new(s, A.i32))

        def run(cap, o):
            if o is None or o["pos"].shape[0] != cap or o["status"].shape[0] != P or o["ctrl"].shape[0] != S:
                o = dict(ctrl=f(S, 4, 2), seg_off=i(P + 1), arclength=f(P), length=i(P), offsets=i(P + 1), status=i(P), needed=A.new(1, A.i64),
                         time=A.new(cap, A.f64), pos=f(cap), vel=f(cap), acc=f(cap), pts=f(cap, 2), curvature=f(cap), ang_vel=f(cap),
                         tpar=f(cap), seg=i(cap))
            args = [_ptr(wp), _ptr(npts), P, n_max, _ptr(limits), start_angle, _ptr(lines) if nl else None, nl, dt, N, nsub, cap,
                    *[_ptr(o[k]) for k in ("ctrl", "seg_off", "arclength", "length", "offsets", "status", "needed", "time", "pos", "vel", "acc",
                                           "pts", "curvature", "ang_vel", "tpar", "seg")]]
            if dyn is None:
                self._call("sc_smooth_paths_batch" + A.suffix, *args)
                return o
            if "vmax_stage" not in o or o["vmax_stage"].shape != (P, N + 1):
                o["vmax_stage"], o["min_clear"] = A.new((P, N + 1), A.f64), A.new(P, A.f32)
            args += [_ptr(dyn), J, _ptr(d2), *fr, _ptr(o["vmax_stage"]), _ptr(o["min_clear"])]
            if r2_clear is None:
                self._call("sc_smooth_paths_limited_batch" + A.suffix, *args)
                return o
            if "level" not in o:
                o["level"], o["leg_min"], o["rounds"] = A.new(S + P, A.u8, fill=0), A.new(S, A.i32, fill=-1), A.new(P, A.i32)
            self._call("sc_smooth_paths_clear_batch" + A.suffix, *args, int(r2_clear), int(max_level), _ptr(o["level"]), _ptr(o["leg_min"]),
                       _ptr(o["rounds"]))
            return o

        o = run(cap, out)
        if not auto:
            return o
        need = int(o["needed"][0])      # synchronises
        if need > cap:
            o = run(need, None)
        return {k: (v[:need] if k in ("time", "pos", "vel", "acc", "pts", "curvature", "ang_vel", "tpar", "seg") else v) for k, v in o.items()}

    # ---- conflicts between timed paths (sc_traj_knots_batch, sc_traj_conflicts_batch, sc_fleet_conflicts_batch) ----
    @staticmethod
    def _traj_ticks(sm, t0, T0, dt_c):
        """K that covers the longest path plus its delay: the last tick at or after max(time[last] + t0) over the paths that
        have samples.  Reads the paths' end times (torch: synchronises)."""
        off, ln = sm["offsets"], sm["length"]
        st = sm.get("status")
        if isinstance(ln, np.ndarray):
            use = (ln >= 1) & ((st == SMOOTH_OK) if st is not None else True)
            if not use.any():
                return 1
            end = sm["time"][(off[:-1] + ln - 1)[use]] + (0.0 if t0 is None else np.asarray(t0, np.float64)[use])
            end = float(end[np.isfinite(end)].max()) if np.isfinite(end).any() else T0
        else:
            import torch
            use = ln >= 1
            if st is not None:
                use = use & (st == SMOOTH_OK)
            idx = (off[:-1].long() + ln.long() - 1)[use]
            if idx.numel() == 0:
                return 1
            end = sm["time"][idx] + (0.0 if t0 is None else t0[use])
            end = end[torch.isfinite(end)]
            end = float(end.max()) if end.numel() else T0
        return int(min(max(np.ceil((end - T0) / dt_c), 1), TRAJ_MAX_TICKS))

    def traj_knots(self, sm, t0=None, flags=None, T0=0.0, dt_c=0.1, K=None):
        """The positions of P timed paths on the common clock T0 + k * dt_c, k = 0 .. K (sc_traj_knots_batch; the definition
        is in include/sea_current_hip.h).  sm: the dict smooth_paths returned, or any dict of GPU tensors time float64 [M],
        pts float32 [M,2], offsets int32 [P+1], length int32 [P] and optionally status int32 [P].  t0 float64 [P] start
        delays, flags int32 [P] (bit 0 / 1: stands at its first / last point before / after its run; None = 3).  K=None
        covers the longest path plus its delay (reads the end times: synchronises); with a K the call only enqueues.
        Returns dict(knots float64 [P,K+1,2], NaN where a path is absent; tstatus int32 [P]; K)."""
        return self._traj_knots(_on(sm["length"].device), sm, t0, flags, T0, dt_c, K)

    def traj_knots_host(self, sm, t0=None, flags=None, T0=0.0, dt_c=0.1, K=None):
        """Host form of traj_knots (numpy in, numpy out; sc_traj_knots_batch_host)."""
        return self._traj_knots(_HOST, sm, t0, flags, T0, dt_c, K)

    def _traj_knots(self, A, sm, t0, flags, T0, dt_c, K):
        sm = A.timed_paths(sm)
        P = sm["length"].shape[0]
        t0, flags = A.per_path(t0, P, A.f64), A.per_path(flags, P, A.i32)
        if K is None:
            K = self._traj_ticks(sm, t0, T0, dt_c)
        out = dict(knots=A.new((P, K + 1, 2), A.f64), tstatus=A.new(P, A.i32), K=K)
        self._call("sc_traj_knots_batch" + A.suffix, *[_ptr(sm[k]) for k in ("time", "pts", "offsets", "length", "status")], P, _ptr(t0),
                   _ptr(flags), T0, dt_c, K, _ptr(out["knots"]), _ptr(out["tstatus"]))
        return out

    def traj_conflicts(self, knots, tstatus, radius, group=None, T0=0.0, dt_c=0.1, sep_cap=float("inf"), want_matrix=False):
        """Who meets whom, when and how close, from knots (sc_traj_conflicts_batch): knots float64 [P,K+1,2] and tstatus int32
        [P] as traj_knots returned them (tstatus is updated: TRAJ_BAD for a radius outside the contract), radius float64 [P]
        or a number, group int32 [P] or None, T0 and dt_c those of the knots.  Returns dict(first_t, first_with, min_sep,
        min_with, n_conf, conflict int32 [P, ceil(P/32)] bit words or None without want_matrix, tstatus).  Only enqueues."""
        return self._traj_conflicts(_on(knots.device), knots, tstatus, radius, group, T0, dt_c, sep_cap, want_matrix)

    def traj_conflicts_host(self, knots, tstatus, radius, group=None, T0=0.0, dt_c=0.1, sep_cap=float("inf"), want_matrix=False):
        """Host form of traj_conflicts (numpy in, numpy out; sc_traj_conflicts_batch_host).  tstatus is copied, not updated in
        place; conflict is uint32 [P, ceil(P/32)]."""
        return self._traj_conflicts(_HOST, knots, tstatus, radius, group, T0, dt_c, sep_cap, want_matrix)

    def _traj_conflicts(self, A, knots, tstatus, radius, group, T0, dt_c, sep_cap, want_matrix):
        knots = A.arr(knots, A.f64)
        P, K = knots.shape[0], knots.shape[1] - 1
        radius, group = A.per_path(radius, P, A.f64), A.per_path(group, P, A.i32)
        out = A.traj_out(P, want_matrix)
        out["tstatus"] = A.own(tstatus, A.i32)
        self._call("sc_traj_conflicts_batch" + A.suffix, _ptr(knots), _ptr(out["tstatus"]), P, K, T0, dt_c, _ptr(radius), _ptr(group), sep_cap,
                   *[_ptr(out[k]) for k in ("first_t", "first_with", "min_sep", "min_with", "n_conf", "conflict")])
        return out

    def fleet_conflicts(self, sm, radius, t0=None, flags=None, group=None, T0=0.0, dt_c=0.1, K=None, sep_cap=float("inf"),
                        want_matrix=False, want_knots=False):
        """traj_knots and traj_conflicts in one call behind smooth_paths (sc_fleet_conflicts_batch): sm is the dict
        smooth_paths returned (see traj_knots), the other arguments are those of the two calls.  K=None covers the longest
        path plus its delay (synchronises once to read it); with a K the call only enqueues.  Returns traj_conflicts' dict
        plus K, and knots with want_knots (otherwise they stay in the context's scratch)."""
        return self._fleet_conflicts(_on(sm["length"].device), sm, radius, t0, flags, group, T0, dt_c, K, sep_cap, want_matrix, want_knots)

    def fleet_conflicts_host(self, sm, radius, t0=None, flags=None, group=None, T0=0.0, dt_c=0.1, K=None, sep_cap=float("inf"),
                             want_matrix=False, want_knots=False):
        """Host form of fleet_conflicts (numpy in, numpy out; sc_fleet_conflicts_batch_host)."""
        return self._fleet_conflicts(_HOST, sm, radius, t0, flags, group, T0, dt_c, K, sep_cap, want_matrix, want_knots)

    def _fleet_args(self, A, sm, radius, t0, flags, group):
        """What the fleet calls share: the timed paths, P, and the four per-path arguments as arrays."""
        sm = A.timed_paths(sm)
        P = sm["length"].shape[0]
        return (sm, P, A.per_path(t0, P, A.f64), A.per_path(flags, P, A.i32), A.per_path(radius, P, A.f64), A.per_path(group, P, A.i32),
                [_ptr(sm[k]) for k in ("time", "pts", "offsets", "length", "status")])

    def _fleet_conflicts(self, A, sm, radius, t0, flags, group, T0, dt_c, K, sep_cap, want_matrix, want_knots):
        sm, P, t0, flags, radius, group, paths = self._fleet_args(A, sm, radius, t0, flags, group)
        if K is None:
            K = self._traj_ticks(sm, t0, T0, dt_c)
        out = A.traj_out(P, want_matrix)
        out["tstatus"] = A.new(P, A.i32)
        out["K"] = K
        if want_knots:
            out["knots"] = A.new((P, K + 1, 2), A.f64)
        self._call("sc_fleet_conflicts_batch" + A.suffix, *paths, P, _ptr(t0), _ptr(flags), T0, dt_c, K, _ptr(out.get("knots")),
                   _ptr(out["tstatus"]), _ptr(radius), _ptr(group), sep_cap,
                   *[_ptr(out[k]) for k in ("first_t", "first_with", "min_sep", "min_with", "n_conf", "conflict")])
        return out

    # ---- delay schedules for timed paths (sc_traj_shift_table_batch, sc_traj_schedule_batch, sc_traj_shift_knots_batch,
    # sc_fleet_schedule_batch) ----
    def traj_shift_table(self, knots, tstatus, radius, group=None, D=8, stride=1):
        """For every pair of paths and every relative delay of -(D-1) .. D-1 slots of `stride` ticks: do they still meet
        (sc_traj_shift_table_batch; the definition is in include/sea_current_hip.h)?  knots, tstatus, radius and group as in
        traj_conflicts (tstatus is updated).  Returns dict(table int64 [P,P]: bit r + D - 1 of table[p][q] is set iff p,
        started r slots later than q, meets q; tstatus).  Only enqueues."""
        return self._traj_shift_table(_on(knots.device), knots, tstatus, radius, group, D, stride)

    def traj_shift_table_host(self, knots, tstatus, radius, group=None, D=8, stride=1):
        """Host form of traj_shift_table (numpy in, numpy out; sc_traj_shift_table_batch_host).  tstatus is copied, not
        updated in place; table is uint64 [P,P]."""
        return self._traj_shift_table(_HOST, knots, tstatus, radius, group, D, stride)

    def _traj_shift_table(self, A, knots, tstatus, radius, group, D, stride):
        knots = A.arr(knots, A.f64)
        P, K = knots.shape[0], knots.shape[1] - 1
        radius, group = A.per_path(radius, P, A.f64), A.per_path(group, P, A.i32)
        out = dict(table=A.new((P, P), A.w64), tstatus=A.own(tstatus, A.i32))
        self._call("sc_traj_shift_table_batch" + A.suffix, _ptr(knots), _ptr(out["tstatus"]), P, K, _ptr(radius), _ptr(group), D, stride,
                   _ptr(out["table"]))
        return out

    def traj_schedule(self, table, tstatus, D=8, order=None, jmax=None):
        """Start slots by priority from a shift table (sc_traj_schedule_batch): walks order (int32 [P], None = 0, 1, ..) and
        gives every path the first slot <= jmax[p] (int32 [P] or a number, None = D-1, negative = pinned to slot 0) in which
        it meets none of the paths placed before it.  Returns dict(slot int32 [P]: >= 0, SLOT_UNRESOLVED, SLOT_NOT_OK or
        SLOT_UNNAMED; counts int32 [4]: slot 0, slot > 0, unresolved, not scheduled).  Only enqueues."""
        return self._traj_schedule(_on(table.device), table, tstatus, D, order, jmax)

    def traj_schedule_host(self, table, tstatus, D=8, order=None, jmax=None):
        """Host form of traj_schedule (numpy in, numpy out; sc_traj_schedule_batch_host)."""
        return self._traj_schedule(_HOST, table, tstatus, D, order, jmax)

    @staticmethod
    def _priority(A, order, jmax, P):
        """order and jmax of the two scheduling calls as arrays."""
        order = A.seq(order, A.i32)
        if order is not None and order.shape[0] != P:
            raise ValueError("order has P entries")
        return order, A.per_path(jmax, P, A.i32)

    def _traj_schedule(self, A, table, tstatus, D, order, jmax):
        table, tstatus = A.words(table, A.w64), A.arr(tstatus, A.i32)
        P = table.shape[0]
        order, jmax = self._priority(A, order, jmax, P)
        out = dict(slot=A.new(P, A.i32), counts=A.new(4, A.i32))
        self._call("sc_traj_schedule_batch" + A.suffix, _ptr(table), _ptr(tstatus), P, D, _ptr(order), _ptr(jmax), _ptr(out["slot"]),
                   _ptr(out["counts"]))
        return out

    def traj_shift_knots(self, knots, slot, stride=1):
        """knots with every path held at its first knot for slot[p] * stride ticks; a path with slot < 0 becomes absent
        (sc_traj_shift_knots_batch).  Returns float64 [P,K+1,2].  Only enqueues."""
        return self._traj_shift_knots(_on(knots.device), knots, slot, stride)

    def traj_shift_knots_host(self, knots, slot, stride=1):
        """Host form of traj_shift_knots (numpy in, numpy out; sc_traj_shift_knots_batch_host)."""
        return self._traj_shift_knots(_HOST, knots, slot, stride)

    def _traj_shift_knots(self, A, knots, slot, stride):
        knots, slot = A.arr(knots, A.f64), A.arr(slot, A.i32)
        out = A.new(tuple(knots.shape), knots.dtype)
        self._call("sc_traj_shift_knots_batch" + A.suffix, _ptr(knots), knots.shape[0], knots.shape[1] - 1, _ptr(slot), stride, _ptr(out))
        return out

    def fleet_schedule(self, sm, radius, t0=None, flags=None, group=None, T0=0.0, dt_c=0.1, K=None, D=8, stride=1, order=None, jmax=None,
                       want_table=False, want_knots=False):
        """traj_knots, traj_shift_table, traj_schedule and traj_shift_knots in one call behind smooth_paths
        (sc_fleet_schedule_batch).  K=None covers the longest path, its delay and (D-1) * stride more ticks, so that every
        path is at rest where the shifts end and the schedule leaves no conflict among the paths with slot >= 0
        (synchronises once to read the end times); with a K the call only enqueues.  Returns dict(slot, counts, delay float64
        [P] = slot * stride * dt_c seconds, NaN for slot < 0; tstatus, K; table with want_table; knots and knots_out with
        want_knots)."""
        return self._fleet_schedule(_on(sm["length"].device), sm, radius, t0, flags, group, T0, dt_c, K, D, stride, order, jmax, want_table,
                                    want_knots)

    def fleet_schedule_host(self, sm, radius, t0=None, flags=None, group=None, T0=0.0, dt_c=0.1, K=None, D=8, stride=1, order=None, jmax=None,
                            want_table=False, want_knots=False):
        """Host form of fleet_schedule (numpy in, numpy out; sc_fleet_schedule_batch_host)."""
        return self._fleet_schedule(_HOST, sm, radius, t0, flags, group, T0, dt_c, K, D, stride, order, jmax, want_table, want_knots)

    def _fleet_schedule(self, A, sm, radius, t0, flags, group, T0, dt_c, K, D, stride, order, jmax, want_table, want_knots):
        sm, P, t0, flags, radius, group, paths = self._fleet_args(A, sm, radius, t0, flags, group)
        order, jmax = self._priority(A, order, jmax, P)
        if K is None:
            K = min(self._traj_ticks(sm, t0, T0, dt_c) + (D - 1) * stride, TRAJ_MAX_TICKS)
        out = dict(slot=A.new(P, A.i32), counts=A.new(4, A.i32), tstatus=A.new(P, A.i32), K=K)
        if want_table:
            out["table"] = A.new((P, P), A.w64)
        if want_knots:
            out["knots"], out["knots_out"] = A.new((P, K + 1, 2), A.f64), A.new((P, K + 1, 2), A.f64)
        self._call("sc_fleet_schedule_batch" + A.suffix, *paths, P, _ptr(t0), _ptr(flags), T0, dt_c, K, _ptr(out.get("knots")),
                   _ptr(out["tstatus"]), _ptr(radius), _ptr(group), D, stride, _ptr(out.get("table")), _ptr(order), _ptr(jmax),
                   _ptr(out["slot"]), _ptr(out["counts"]), _ptr(out.get("knots_out")))
        out["delay"] = A.delay(out["slot"], stride, dt_c)
        return out

    # ---- re-planning in space-time around the scheduled fleet (sc_traj_reserve_batch, sc_tplan_batch, sc_fleet_replan_batch) ----
    @staticmethod
    def _tplan_out(A, B, L, H, W, want_knots, want_reach):
        """The result buffers of a plan; reach is w32 bit words."""
        out = dict(path=A.new((B, L), A.i32, fill=-1))
        for k in ("len", "arrive", "status"):
            out[k] = A.new(B, A.i32)
        if want_knots:
            out["knots_out"] = A.new((B, L, 2), A.f64)
        if want_reach:
            out["reach"] = A.new((B, L, H, (W + 31) // 32), A.w32)
        return out

    def traj_reserve(self, knots, tstatus, radius, W, H, frame, pad, select=None, res=None):
        """Rasterise knot rows into reservations (sc_traj_reserve_batch; the definition is in include/sea_current_hip.h): cell c
        is reserved at layers k and k+1 when a robot standing at c through interval k would come within radius[q] + pad of path
        q.  knots float64 [P,K+1,2], tstatus int32 [P] or None (all OK; updated like in traj_conflicts), radius float64 [P] or a
        number, frame = (x_min, y_min, res_x, res_y), select int32 [P] or None (0 = leave this path out).  res int32 [K+1, H,
        ceil(W/32)] bit words is ORed into (None: a zeroed one) and returned.  Only enqueues."""
        return self._traj_reserve(_on(knots.device), knots, tstatus, radius, W, H, frame, pad, select, res)[0]

    def traj_reserve_host(self, knots, tstatus, radius, W, H, frame, pad, select=None, res=None):
        """Host form of traj_reserve (numpy in, numpy out; sc_traj_reserve_batch_host).  Returns (res uint32 [K+1,H,ceil(W/32)],
        tstatus): copies, the arguments are not updated in place."""
        return self._traj_reserve(_HOST, knots, tstatus, radius, W, H, frame, pad, select, res)

    def _traj_reserve(self, A, knots, tstatus, radius, W, H, frame, pad, select, res):
        knots = A.arr(knots, A.f64)
        P, K = knots.shape[0], knots.shape[1] - 1
        radius, select = A.per_path(radius, P, A.f64), A.per_path(select, P, A.i32)
        tstatus = A.own(tstatus, A.i32)
        res = A.new((K + 1, H, (W + 31) // 32), A.w32, fill=0) if res is None else A.own(res, A.w32)
        self._call("sc_traj_reserve_batch" + A.suffix, _ptr(knots), _ptr(tstatus), P, K, _ptr(radius), _ptr(select), float(pad), W, H,
                   *(float(v) for v in frame), _ptr(res))
        return res, tstatus

    def tplan(self, d2, start, goal, res=None, L=None, t_start=None, hold=True, r2=0, frame=None, want_reach=False):
        """Earliest arrival on the time-expanded grid around reservations (sc_tplan_batch).  d2 int32 [H,W]; start, goal int32 [B]
        cells; res int32 [L,H,ceil(W/32)] as traj_reserve returned it, or None (nothing reserved; L must be given); t_start int32
        [B] layers or None = 0; hold: the robot stays at its goal, so it arrives only once the goal is never reserved again.
        Returns dict(path int32 [B,L] (-1 past len), len, arrive, status int32 [B] (TP_OK, TP_NO_PATH, TP_BAD_ENDPOINT,
        TP_START_BLOCKED); knots_out float64 [B,L,2] with a frame = (x_min, y_min, res_x, res_y): rows that traj_conflicts takes
        behind the fleet's; reach int32 [B,L,H,ceil(W/32)] with want_reach, otherwise the layers stay in the context's scratch).
        One stated earliest-arrival path, not the shortest in metres.  Only enqueues."""
        return self._tplan(_on(d2.device), d2, start, goal, res, L, t_start, hold, r2, frame, want_reach)

    def tplan_host(self, d2, start, goal, res=None, L=None, t_start=None, hold=True, r2=0, frame=None, want_reach=False):
        """Host form of tplan (numpy in, numpy out; sc_tplan_batch_host)."""
        return self._tplan(_HOST, d2, start, goal, res, L, t_start, hold, r2, frame, want_reach)

    def _tplan(self, A, d2, start, goal, res, L, t_start, hold, r2, frame, want_reach):
        d2, start, goal, t_start = (A.arr(a, A.i32) for a in (d2, start, goal, t_start))
        res = A.words(res, A.w32)
        H, W = d2.shape
        B = start.shape[0]
        L = res.shape[0] if L is None else L
        out = self._tplan_out(A, B, L, H, W, frame is not None, want_reach)
        fr = (0.0, 0.0, 1.0, 1.0) if frame is None else tuple(float(v) for v in frame)
        self._call("sc_tplan_batch" + A.suffix, _ptr(d2), W, H, r2, _ptr(res), L, _ptr(start), _ptr(goal), _ptr(t_start), B, int(bool(hold)),
                   _ptr(out["path"]), _ptr(out["len"]), _ptr(out["arrive"]), _ptr(out["status"]), _ptr(out.get("knots_out")), *fr,
                   _ptr(out.get("reach")))
        return out

    def fleet_replan(self, knots, tstatus, radius, d2, start, goal, frame, pad, r_new=None, select=None, t_start=None, hold=True, r2=0,
                     sequential=False, res=None, want_reach=False):
        """traj_reserve of the selected fleet rows, then tplan around them, in one call (sc_fleet_replan_batch): the fleet is knots
        / tstatus / radius / select as in traj_reserve (e.g. fleet_schedule's knots_out with select = slot >= 0), the robots are
        start / goal / t_start as in tplan.  pad: r_new + half the grid's diagonal move keeps a robot of radius r_new clear of
        every reserved path (see the header).  sequential=False plans all robots against the fleet at once; sequential=True
        plans robot i, reserves its row (radius r_new[i], the same pad) and goes on to robot i+1: prioritised planning in the
        caller's order (needs r_new, float64 [B] or a number).  Returns tplan's dict (knots_out always) plus res and tstatus.
        Only enqueues."""
        return self._fleet_replan(_on(knots.device), knots, tstatus, radius, d2, start, goal, frame, pad, r_new, select, t_start, hold, r2,
                                  sequential, res, want_reach)

    def fleet_replan_host(self, knots, tstatus, radius, d2, start, goal, frame, pad, r_new=None, select=None, t_start=None, hold=True, r2=0,
                          sequential=False, res=None, want_reach=False):
        """Host form of fleet_replan (numpy in, numpy out; sc_fleet_replan_batch_host); res and tstatus are copies."""
        return self._fleet_replan(_HOST, knots, tstatus, radius, d2, start, goal, frame, pad, r_new, select, t_start, hold, r2, sequential,
                                  res, want_reach)

    def _fleet_replan(self, A, knots, tstatus, radius, d2, start, goal, frame, pad, r_new, select, t_start, hold, r2, sequential, res,
                      want_reach):
        knots = A.arr(knots, A.f64)
        d2, start, goal, t_start = (A.arr(a, A.i32) for a in (d2, start, goal, t_start))
        P, K = knots.shape[0], knots.shape[1] - 1
        H, W = d2.shape
        B = start.shape[0]
        radius, select, r_new = A.per_path(radius, P, A.f64), A.per_path(select, P, A.i32), A.per_path(r_new, B, A.f64)
        tstatus = A.own(tstatus, A.i32)
        res = A.new((K + 1, H, (W + 31) // 32), A.w32, fill=0) if res is None else A.own(res, A.w32)
        out = self._tplan_out(A, B, K + 1, H, W, True, want_reach)
        self._call("sc_fleet_replan_batch" + A.suffix, _ptr(knots), _ptr(tstatus), P, K, _ptr(radius), _ptr(select), float(pad), W, H,
                   *(float(v) for v in frame), _ptr(res), _ptr(d2), r2, K + 1, _ptr(start), _ptr(goal), _ptr(t_start), B, int(bool(hold)),
                   _ptr(out["path"]), _ptr(out["len"]), _ptr(out["arrive"]), _ptr(out["status"]), _ptr(out["knots_out"]),
                   _ptr(out.get("reach")), _ptr(r_new), int(bool(sequential)))
        out["res"], out["tstatus"] = res, tstatus
        return out

    # ---- robots to goals (sc_field_cost_matrix, sc_assign_batch, sc_fleet_assign_batch) ----
    def field_cost_matrix(self, g, cells, col_cost=None, out=None):
        """The R x F cost matrix of robots at `cells` (int32 [R]) against the fields g (int32 [F,H,W], any of cost_fields' or
        cost_fields_multi's arrays): out[r][f] = g[f][cells[r]] (+ col_cost[f], int32 [F], 0 .. FIELD_SEED_COST_MAX), FIELD_INF
        kept; a cell out of range gives a row of FIELD_INF (sc_field_cost_matrix).  Returns int32 [R,F].  Only enqueues."""
        return self._field_cost_matrix(_on(g.device), g, cells, col_cost, out)

    def field_cost_matrix_host(self, g, cells, col_cost=None, out=None):
        """Host form of field_cost_matrix (numpy in, numpy out; sc_field_cost_matrix_host)."""
        return self._field_cost_matrix(_HOST, g, cells, col_cost, out)

    def _field_cost_matrix(self, A, g, cells, col_cost, out):
        g, cells, col_cost = A.arr(g, A.i32), A.arr(cells, A.i32), A.arr(col_cost, A.i32)
        F, H, W = g.shape
        R = cells.shape[0]
        if out is None:
            out = A.new((R, F), A.i32)
        self._call("sc_field_cost_matrix" + A.suffix, _ptr(g), F, W, H, _ptr(cells), R, _ptr(col_cost), _ptr(out))
        return out

    def assign(self, cost):
        """Optimal one-to-one matchings (sc_assign_batch; the definition is in include/sea_current_hip.h): cost int32 [B,R,C]
        or [R,C] (B = 1), FIELD_INF = forbidden.  Returns dict(col_of int32 [B,R], row_of int32 [B,C], u int64 [B,R], v int64
        [B,C], info int64 [B,4] = matched, total, steps, status), without the leading B for 2-D input.  Only enqueues."""
        return self._assign(_on(cost.device), cost)

    def assign_host(self, cost):
        """Host form of assign (numpy in, numpy out; sc_assign_batch_host)."""
        return self._assign(_HOST, cost)

    @staticmethod
    def _assign_out(A, lead, R, Cc):
        return dict(col_of=A.new(lead + (R,), A.i32), row_of=A.new(lead + (Cc,), A.i32), u=A.new(lead + (R,), A.i64),
                    v=A.new(lead + (Cc,), A.i64), info=A.new(lead + (4,), A.i64))

    def _assign(self, A, cost):
        cost = A.arr(cost, A.i32)
        B, R, Cc = _ghw(cost)
        out = self._assign_out(A, () if len(cost.shape) == 2 else (B,), R, Cc)
        self._call("sc_assign_batch" + A.suffix, _ptr(cost), B, R, Cc, *[_ptr(out[k]) for k in ("col_of", "row_of", "u", "v", "info")])
        return out

    def fleet_assign(self, g, cells, col_cost=None, want_cost=False):
        """field_cost_matrix and assign in one call (sc_fleet_assign_batch): robots at `cells` to the goals the fields g are
        rooted at, one goal per robot.  Returns assign's dict for one problem (col_of[r] = the field of robot r or -1: what
        field_paths takes as qfield with to_root=True), plus cost int32 [R,F] with want_cost.  Only enqueues."""
        return self._fleet_assign(_on(g.device), g, cells, col_cost, want_cost)

    def fleet_assign_host(self, g, cells, col_cost=None, want_cost=False):
        """Host form of fleet_assign (numpy in, numpy out; sc_fleet_assign_batch_host)."""
        return self._fleet_assign(_HOST, g, cells, col_cost, want_cost)

    def _fleet_assign(self, A, g, cells, col_cost, want_cost):
        g, cells, col_cost = A.arr(g, A.i32), A.arr(cells, A.i32), A.arr(col_cost, A.i32)
        F, H, W = g.shape
        R = cells.shape[0]
        out = self._assign_out(A, (), R, F)
        if want_cost:
            out["cost"] = A.new((R, F), A.i32)
        self._call("sc_fleet_assign_batch" + A.suffix, _ptr(g), F, W, H, _ptr(cells), R, _ptr(col_cost), _ptr(out.get("cost")),
                   *[_ptr(out[k]) for k in ("col_of", "row_of", "u", "v", "info")])
        return out

    # ---- exploration frontiers (sc_known_from_discs, sc_d2_known_i32, sc_frontier_batch, sc_frontier_cost_matrix,
    #      sc_fleet_explore_batch) ----
    def known_from_discs(self, discs, W, H, base=None, out=None):
        """The known-space mask of sensing discs (sc_known_from_discs): discs int32 [R,3] = (cx, cy, r2) on the GPU, base uint8
        [H,W] or None (may be `out`).  Returns uint8 [H,W], 1 where base is set or a disc covers the cell.  Only enqueues."""
        return self._known_from_discs(_on(discs.device), discs, W, H, base, out)

    def known_from_discs_host(self, discs, W, H, base=None):
        """Host form of known_from_discs (numpy in, numpy out)."""
        return self._known_from_discs(_HOST, discs, W, H, base)

    def _known_from_discs(self, A, discs, W, H, base, out=None):
        discs, base = A.rows(discs, A.i32, 3), A.arr(base, A.u8)
        if out is None:
            out = A.new((H, W), A.u8)
        self._call("sc_known_from_discs" + A.suffix, _ptr(base), _ptr(discs), discs.shape[0], W, H, _ptr(out))
        return out

    def d2_known(self, d2, known, out=None):
        """d2 where known, 0 elsewhere (sc_d2_known_i32): d2 int32 and known uint8, [H,W] or [G,H,W] on the GPU; every planner
        run on the result moves through known free space only.  out may be d2.  Only enqueues."""
        return self._d2_known(_on(d2.device), d2, known, out)

    def d2_known_host(self, d2, known):
        """Host form of d2_known (numpy in, numpy out)."""
        return self._d2_known(_HOST, d2, known)

    def _d2_known(self, A, d2, known, out=None):
        d2, known = A.arr(d2, A.i32), A.arr(known, A.u8)
        G, H, W = _ghw(d2)
        if out is None:
            out = A.new(tuple(d2.shape), d2.dtype)
        self._call("sc_d2_known_i32" + A.suffix, _ptr(d2), _ptr(known), G, W, H, _ptr(out))
        return out

    def frontiers(self, d2, known, r2=0, min_size=1, Cmax=128, want_label=True, want_slot=True, want_stats=True, out=None):
        """Frontier cells and their 8-connected clusters (sc_frontier_batch; the definition is in include/sea_current_hip.h).
        d2 int32 and known uint8, [H,W] or [G,H,W] on the GPU.  Returns dict(label, slot int32 shaped like d2 (None without
        want_label / want_slot), ncl int32 [G,2] = (listed, all), rep, csize int32 [G,Cmax], cbox int32 [G,Cmax,4] and csum int64
        [G,Cmax,2] (None without want_stats)).  `out`: the dict of an earlier call with the same shapes.  Only enqueues."""
        return self._frontiers(_on(d2.device), d2, known, r2, min_size, Cmax, want_label, want_slot, want_stats, out)

    def frontiers_host(self, d2, known, r2=0, min_size=1, Cmax=128, want_label=True, want_slot=True, want_stats=True):
        """Host form of frontiers (numpy in, numpy out)."""
        return self._frontiers(_HOST, d2, known, r2, min_size, Cmax, want_label, want_slot, want_stats)

    def _frontiers(self, A, d2, known, r2, min_size, Cmax, want_label, want_slot, want_stats, out=None):
        d2, known = A.arr(d2, A.i32), A.arr(known, A.u8)
        G, H, W = _ghw(d2)
        if out is None:
            shape = tuple(d2.shape)
            out = dict(label=A.new(shape, A.i32) if want_label else None, slot=A.new(shape, A.i32) if want_slot else None,
                       ncl=A.new((G, 2), A.i32), rep=A.new((G, Cmax), A.i32), csize=A.new((G, Cmax), A.i32),
                       cbox=A.new((G, Cmax, 4), A.i32) if want_stats else None, csum=A.new((G, Cmax, 2), A.i64) if want_stats else None)
        self._call("sc_frontier_batch" + A.suffix, _ptr(d2), _ptr(known), G, W, H, r2, min_size, Cmax,
                   *[_ptr(out[k]) for k in ("label", "slot", "ncl", "rep", "csize", "cbox", "csum")])
        return out

    def frontier_cost_matrix(self, g, fr, gain=0, size_cap=0, fgrid=None):
        """The robots x clusters matrix (sc_frontier_cost_matrix): g int32 [F,H,W] fields rooted at the robots, fr the dict of
        frontiers (its slot and csize), fgrid int32 [F] (None only with one grid).  Returns dict(cost, cell int32 [F,Cmax]):
        assign's layout.  Only enqueues."""
        return self._frontier_cost_matrix(_on(g.device), g, fr, gain, size_cap, fgrid)

    def frontier_cost_matrix_host(self, g, fr, gain=0, size_cap=0, fgrid=None):
        """Host form of frontier_cost_matrix (numpy in, numpy out)."""
        return self._frontier_cost_matrix(_HOST, g, fr, gain, size_cap, fgrid)

    def _frontier_cost_matrix(self, A, g, fr, gain, size_cap, fgrid):
        g, slot, csize, fgrid = (A.arr(a, A.i32) for a in (g, fr["slot"], fr["csize"], fgrid))
        F, H, W = g.shape
        G, Cmax = csize.shape
        out = dict(cost=A.new((F, Cmax), A.i32), cell=A.new((F, Cmax), A.i32))
        self._call("sc_frontier_cost_matrix" + A.suffix, _ptr(g), F, _ptr(fgrid), _ptr(slot), _ptr(csize), G, W, H, Cmax, gain, size_cap,
                   _ptr(out["cost"]), _ptr(out["cell"]))
        return out

    def fleet_explore(self, d2, known, g, r2=0, min_size=1, Cmax=128, gain=0, size_cap=0, want_all=False):
        """A frontier goal per robot (sc_fleet_explore_batch): frontiers of (d2, known) [H,W], the matrix of the robots' fields g
        int32 [F,H,W], an optimal matching.  Returns dict(goal int32 [F]: the cell to drive to or -1, gcost int32 [F]); with
        want_all also every intermediate array (frontiers' without the leading G, cost, cell, col_of, row_of, info).  goal is what
        field_paths takes as targets with qfield = arange(F).  Only enqueues."""
        return self._fleet_explore(_on(d2.device), d2, known, g, r2, min_size, Cmax, gain, size_cap, want_all)

    def fleet_explore_host(self, d2, known, g, r2=0, min_size=1, Cmax=128, gain=0, size_cap=0, want_all=False):
        """Host form of fleet_explore (numpy in, numpy out)."""
        return self._fleet_explore(_HOST, d2, known, g, r2, min_size, Cmax, gain, size_cap, want_all)

    def _fleet_explore(self, A, d2, known, g, r2, min_size, Cmax, gain, size_cap, want_all):
        d2, known, g = A.arr(d2, A.i32), A.arr(known, A.u8), A.arr(g, A.i32)
        H, W = d2.shape
        F = g.shape[0]
        e = lambda s, t=A.i32: A.new(s, t)
        out = dict(goal=e(F), gcost=e(F))
        if want_all:
            out.update(label=e((H, W)), slot=e((H, W)), ncl=e(2), rep=e(Cmax), csize=e(Cmax), cbox=e((Cmax, 4)), csum=e((Cmax, 2), A.i64),
                       cost=e((F, Cmax)), cell=e((F, Cmax)), col_of=e(F), row_of=e(Cmax), info=e(4, A.i64))
        self._call("sc_fleet_explore_batch" + A.suffix, _ptr(d2), _ptr(known), W, H, r2, min_size, Cmax, _ptr(g), F, gain, size_cap,
                   *(_ptr(out.get(k)) for k in ("label", "slot", "ncl", "rep", "csize", "cbox", "csum", "cost", "cell", "col_of", "row_of",
                                                "info")), _ptr(out["goal"]), _ptr(out["gcost"]))
        return out

    # ---- line-of-sight sensing (sc_known_from_views, sc_view_gain_batch) ----
    def known_from_views(self, views, occ, base=None, out=None, occ_seen=None):
        """The known-space mask of views that walls block (sc_known_from_views): views int32 [R,3] = (cx, cy, r2) and occ uint8
        [H,W] (the map the sensor meets) on the GPU, base uint8 [H,W] or None (may be `out`).  Returns known uint8 [H,W]: base,
        the free cells a view sees along a clear ray, and the occupied cells that border one.  occ_seen: a uint8 [H,W] tensor,
        or True to have it allocated; then (known, occ_seen) is returned, occ_seen = occ where known, 0 elsewhere.  Only
        enqueues."""
        return self._known_from_views(_on(occ.device), views, occ, base, out, occ_seen)

    def known_from_views_host(self, views, occ, base=None, occ_seen=None):
        """Host form of known_from_views (numpy in, numpy out)."""
        return self._known_from_views(_HOST, views, occ, base, None, occ_seen)

    def _known_from_views(self, A, views, occ, base, out, occ_seen):
        views, occ, base = A.rows(views, A.i32, 3), A.arr(occ, A.u8), A.arr(base, A.u8)
        H, W = occ.shape
        if out is None:
            out = A.new((H, W), A.u8)
        if occ_seen is True:
            occ_seen = A.new((H, W), A.u8)
        self._call("sc_known_from_views" + A.suffix, _ptr(base), _ptr(occ), _ptr(views), views.shape[0], W, H, _ptr(out), _ptr(occ_seen))
        return out if occ_seen is None else (out, occ_seen)

    def view_gain(self, views, occ, known, out=None):
        """The unknown cells every candidate pose would see (sc_view_gain_batch): views int32 [N,3], occ and known uint8 [H,W]
        on the GPU.  Returns gain int32 [N]: for view i alone, the cells with known == 0 it sees.  Only enqueues."""
        return self._view_gain(_on(occ.device), views, occ, known, out)

    def view_gain_host(self, views, occ, known):
        """Host form of view_gain (numpy in, numpy out)."""
        return self._view_gain(_HOST, views, occ, known)

    def _view_gain(self, A, views, occ, known, out=None):
        views, occ, known = A.rows(views, A.i32, 3), A.arr(occ, A.u8), A.arr(known, A.u8)
        H, W = occ.shape
        if out is None:
            out = A.new(views.shape[0], A.i32)
        self._call("sc_view_gain_batch" + A.suffix, _ptr(occ), _ptr(known), _ptr(views), views.shape[0], W, H, _ptr(out))
        return out

    # ---- sensors with a field of view (sc_known_from_sectors, sc_sector_gain_batch, sc_view_gain_headings_batch) ----
    def known_from_sectors(self, sviews, occ, base=None, out=None, occ_seen=None):
        """known_from_views for sector views (sc_known_from_sectors): sviews int32 [R,7] = (cx, cy, r2, ax, ay, bx, by), the
        sector counter-clockwise from direction a (inclusive) to b (exclusive); a = b = 0 is the full circle.  The other
        arguments and the result are known_from_views'.  Only enqueues."""
        return self._known_from_sectors(_on(occ.device), sviews, occ, base, out, occ_seen)

    def known_from_sectors_host(self, sviews, occ, base=None, occ_seen=None):
        """Host form of known_from_sectors (numpy in, numpy out)."""
        return self._known_from_sectors(_HOST, sviews, occ, base, None, occ_seen)

    def _known_from_sectors(self, A, sviews, occ, base, out, occ_seen):
        sviews, occ, base = A.rows(sviews, A.i32, 7), A.arr(occ, A.u8), A.arr(base, A.u8)
        H, W = occ.shape
        if out is None:
            out = A.new((H, W), A.u8)
        if occ_seen is True:
            occ_seen = A.new((H, W), A.u8)
        for what, x in (("base", base), ("out", out), ("occ_seen", occ_seen)):
            _sized(what, x, W * H)
        _sized("sviews", sviews, 7 * sviews.shape[0])
        self._call("sc_known_from_sectors" + A.suffix, _ptr(base), _ptr(occ), _ptr(sviews), sviews.shape[0], W, H, _ptr(out), _ptr(occ_seen))
        return out if occ_seen is None else (out, occ_seen)

    def sector_gain(self, sviews, occ, known, out=None):
        """The unknown cells every sector pose would see (sc_sector_gain_batch): sviews int32 [N,7], occ and known uint8 [H,W]
        on the GPU.  Returns gain int32 [N].  Only enqueues."""
        return self._sector_gain(_on(occ.device), sviews, occ, known, out)

    def sector_gain_host(self, sviews, occ, known):
        """Host form of sector_gain (numpy in, numpy out)."""
        return self._sector_gain(_HOST, sviews, occ, known)

    def _sector_gain(self, A, sviews, occ, known, out=None):
        sviews, occ, known = A.rows(sviews, A.i32, 7), A.arr(occ, A.u8), A.arr(known, A.u8)
        H, W = occ.shape
        N = sviews.shape[0]
        if out is None:
            out = A.new(N, A.i32)
        _sized("known", known, W * H)
        _sized("sviews", sviews, 7 * N)
        _sized("out", out, N)
        self._call("sc_sector_gain_batch" + A.suffix, _ptr(occ), _ptr(known), _ptr(sviews), N, W, H, _ptr(out))
        return out

    def view_gain_headings(self, views, occ, known, dirs, span, hist=None, gainh=None, out=None):
        """The gain of every heading of every candidate pose at the cost of one pass of rays (sc_view_gain_headings_batch):
        views int32 [N,3], occ and known uint8 [H,W] on the GPU; dirs int32 [B,2] on the HOST (heading_dirs(B)), the table whose
        consecutive entries bound the bins; span: the bins a sensor covers.  Returns best int32 [N,2] = (the largest gain over
        the headings, the smallest heading that attains it); heading h is the sector from dirs[h] to dirs[(h + span) % B].
        hist / gainh: an int32 [N,B] tensor, or True to have it allocated; then dict(best, hist, gainh) with what was asked for
        is returned.  Only enqueues."""
        return self._view_gain_headings(_on(occ.device), views, occ, known, dirs, span, hist, gainh, out)

    def view_gain_headings_host(self, views, occ, known, dirs, span, hist=None, gainh=None):
        """Host form of view_gain_headings (numpy in, numpy out)."""
        return self._view_gain_headings(_HOST, views, occ, known, dirs, span, hist, gainh)

    def _view_gain_headings(self, A, views, occ, known, dirs, span, hist, gainh, out=None):
        views, occ, known = A.rows(views, A.i32, 3), A.arr(occ, A.u8), A.arr(known, A.u8)
        dirs = np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 2)         # a host table in both forms
        H, W = occ.shape
        N, B = views.shape[0], dirs.shape[0]
        if out is None:
            out = A.new((N, 2), A.i32)
        plain = hist is None and gainh is None
        hist = A.new((N, B), A.i32) if hist is True else hist
        gainh = A.new((N, B), A.i32) if gainh is True else gainh
        _sized("known", known, W * H)
        _sized("views", views, 3 * N)
        _sized("out", out, 2 * N)
        _sized("hist", hist, N * B)
        _sized("gainh", gainh, N * B)
        self._call("sc_view_gain_headings_batch" + A.suffix, _ptr(occ), _ptr(known), _ptr(views), N, W, H, _ptr(dirs), B, int(span), _ptr(hist),
                   _ptr(gainh), _ptr(out))
        if plain:
            return out
        res = dict(best=out)
        if hist is not None:
            res["hist"] = hist
        if gainh is not None:
            res["gainh"] = gainh
        return res

    def views_from_cells(self, cell, W, H, r2, out=None):
        """View rows from cells (sc_views_from_cells): cell int32 [N] on the GPU -> views int32 [N,3] = (cell % W, cell // W, r2),
        (0, 0, -1), an ignored view, for a cell outside the grid (the -1 of fleet_explore's unmatched robot).  Only enqueues."""
        return self._views_from_cells(_on(cell.device), cell, W, H, r2, out)

    def views_from_cells_host(self, cell, W, H, r2):
        """Host form of views_from_cells (numpy in, numpy out)."""
        return self._views_from_cells(_HOST, cell, W, H, r2)

    def _views_from_cells(self, A, cell, W, H, r2, out=None):
        cell = A.arr(cell, A.i32)
        N = _count(cell)
        if out is None:
            out = A.new((N, 3), A.i32)
        _sized("out", out, 3 * N)
        self._call("sc_views_from_cells" + A.suffix, _ptr(cell), N, W, H, r2, _ptr(out))
        return out

    # ---- coordinated goals by gain (sc_explore_gain_batch, sc_frontier_centres, sc_fleet_explore_gain_batch) ----
    def explore_gain(self, occ, known, g, cand, r2, dirs=None, span=0, wg=1, wc=1, min_gain=1, rounds=None, known_out=None, want_all=True):
        """Greedy (robot, candidate) picks by what each view reveals (sc_explore_gain_batch; the definition is in
        include/sea_current_hip.h).  occ, known uint8 [H,W], g int32 [R,H,W] (fields rooted at the robots) and cand int32 [N]
        (candidate cells) on the GPU; r2 the sensing radius squared; dirs int32 [B,2] on the HOST (heading_dirs(B)) with span <
        B for a sensor with a field of view, None for the full circle.  The pair of largest wg * gain - wc * g[r][cand] is taken
        `rounds` times at most (None: min(R, N)); every pick's view is applied to a working copy of known before the next.
        Returns dict(goal, gcost int32 [R] (-1: no pick), npick int32 [1]); with want_all also ggain, head, cand_of, pick int32
        [R], gain0, gain_end int32 [N] and known_out uint8 [H,W] (the predicted known map; pass `known` itself as known_out to
        update it in place).  head[r] is a bin of dirs: the sensor covers dirs[head] .. dirs[(head + span) % B], so its axis
        points along angle (head + span / 2) * 2 pi / B; with dirs = heading_dirs(8) and an even span that is pose_fields' heading
        (head + span // 2) % 8 (heading k points along k * 45 degrees); for an odd span, or any other table, rounding the axis to
        a pose heading is the caller's job.  goal is what field_paths takes as
        targets with qfield = arange(R).  Only enqueues."""
        return self._explore_gain(_on(occ.device), occ, known, g, cand, r2, dirs, span, wg, wc, min_gain, rounds, known_out, want_all)

    def explore_gain_host(self, occ, known, g, cand, r2, dirs=None, span=0, wg=1, wc=1, min_gain=1, rounds=None, want_all=True):
        """Host form of explore_gain (numpy in, numpy out)."""
        return self._explore_gain(_HOST, occ, known, g, cand, r2, dirs, span, wg, wc, min_gain, rounds, None, want_all)

    @staticmethod
    def _gain_out(A, R, N, H, W, known_out, want_all):
        """The result dict of the picks by gain: what want_all adds is None without it."""
        e = lambda s, t=A.i32: A.new(s, t)
        out = dict(goal=e(R), gcost=e(R), npick=e(1))
        for k in ("ggain", "head", "cand_of", "pick"):
            out[k] = e(R) if want_all else None
        out.update(gain0=e(N) if want_all else None, gain_end=e(N) if want_all else None,
                   known_out=known_out if known_out is not None else (e((H, W), A.u8) if want_all else None))
        return out

    _GAIN_KEYS = ("goal", "gcost", "ggain", "head", "cand_of", "pick", "npick", "gain0", "gain_end", "known_out")

    def _explore_gain(self, A, occ, known, g, cand, r2, dirs, span, wg, wc, min_gain, rounds, known_out, want_all):
        occ, known, g, cand = A.arr(occ, A.u8), A.arr(known, A.u8), A.arr(g, A.i32), A.arr(cand, A.i32)
        dirs = None if dirs is None else np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 2)    # a host table in both forms
        H, W = occ.shape
        R, N, B = g.shape[0], _count(cand), 0 if dirs is None else dirs.shape[0]
        rounds = min(R, N) if rounds is None else int(rounds)
        out = self._gain_out(A, R, N, H, W, known_out, want_all)
        _sized("known", known, W * H)
        _sized("g", g, R * W * H)
        _sized("known_out", out["known_out"], W * H)
        self._call("sc_explore_gain_batch" + A.suffix, _ptr(occ), _ptr(known), _ptr(g), R, _ptr(cand), N, W, H, int(r2), _ptr(dirs), B, int(span),
                   int(wg), int(wc), int(min_gain), rounds, *(_ptr(out[k]) for k in self._GAIN_KEYS))
        return {k: v for k, v in out.items() if v is not None}

    def frontier_centres(self, fr, W, H, out=None):
        """A central cell per listed frontier cluster (sc_frontier_centres): fr the dict of frontiers (its slot, csize and csum;
        want_slot and want_stats).  Returns centre int32 [G,Cmax]: the cluster's cell nearest its centroid in the 1-norm (ties:
        the smallest cell), -1 for the rows beyond the listed clusters.  Only enqueues."""
        return self._frontier_centres(_on(fr["slot"].device), fr, W, H, out)

    def frontier_centres_host(self, fr, W, H):
        """Host form of frontier_centres (numpy in, numpy out)."""
        return self._frontier_centres(_HOST, fr, W, H)

    def _frontier_centres(self, A, fr, W, H, out=None):
        slot, csize, csum = A.arr(fr["slot"], A.i32), A.arr(fr["csize"], A.i32), A.arr(fr["csum"], A.i64)
        G, Cmax = csize.shape
        if out is None:
            out = A.new((G, Cmax), A.i32)
        _sized("slot", slot, G * W * H)
        _sized("csum", csum, 2 * G * Cmax)
        _sized("out", out, G * Cmax)
        self._call("sc_frontier_centres" + A.suffix, _ptr(slot), _ptr(csize), _ptr(csum), G, W, H, Cmax, _ptr(out))
        return out

    def fleet_explore_gain(self, d2, known, occ, g, r2_sense, r2=0, min_size=1, Cmax=128, dirs=None, span=0, wg=1, wc=1, min_gain=1, rounds=None,
                           known_out=None, want_all=False):
        """A goal per robot by what its view reveals (sc_fleet_explore_gain_batch): frontiers of (d2, known) [H,W], a central cell
        per cluster, then explore_gain over those cells with occ the observed map, g int32 [R,H,W] the robots' fields and
        r2_sense the sensing radius squared (r2: the clearance of the frontier cells).  Returns explore_gain's dict with every
        output; with want_all also label, slot, ncl, rep, csize, cbox, csum (frontiers' without the leading G) and centre int32
        [Cmax].  goal is what field_paths takes as targets with qfield = arange(R); with dirs = heading_dirs(8), (goal, head)
        gives a goal pose for pose_fields as explore_gain's docstring says.  Only enqueues."""
        return self._fleet_explore_gain(_on(d2.device), d2, known, occ, g, r2_sense, r2, min_size, Cmax, dirs, span, wg, wc, min_gain, rounds,
                                        known_out, want_all)

    def fleet_explore_gain_host(self, d2, known, occ, g, r2_sense, r2=0, min_size=1, Cmax=128, dirs=None, span=0, wg=1, wc=1, min_gain=1,
                                rounds=None, want_all=False):
        """Host form of fleet_explore_gain (numpy in, numpy out)."""
        return self._fleet_explore_gain(_HOST, d2, known, occ, g, r2_sense, r2, min_size, Cmax, dirs, span, wg, wc, min_gain, rounds, None,
                                        want_all)

    def _fleet_explore_gain(self, A, d2, known, occ, g, r2_sense, r2, min_size, Cmax, dirs, span, wg, wc, min_gain, rounds, known_out, want_all):
        d2, known, occ, g = A.arr(d2, A.i32), A.arr(known, A.u8), A.arr(occ, A.u8), A.arr(g, A.i32)
        dirs = None if dirs is None else np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 2)
        H, W = d2.shape
        R, B = g.shape[0], 0 if dirs is None else dirs.shape[0]
        rounds = min(R, Cmax, ASSIGN_MAX_DIM) if rounds is None else int(rounds)
        out = self._gain_out(A, R, Cmax, H, W, known_out, True)
        e = lambda s, t=A.i32: A.new(s, t)
        mid = dict(label=e((H, W)), slot=e((H, W)), ncl=e(2), rep=e(Cmax), csize=e(Cmax), cbox=e((Cmax, 4)), csum=e((Cmax, 2), A.i64),
                   centre=e(Cmax)) if want_all else {}
        for what, x in (("known", known), ("occ", occ), ("known_out", out["known_out"])):
            _sized(what, x, W * H)
        _sized("g", g, R * W * H)
        self._call("sc_fleet_explore_gain_batch" + A.suffix, _ptr(d2), _ptr(known), W, H, r2, min_size, Cmax, _ptr(occ), _ptr(g), R, int(r2_sense),
                   _ptr(dirs), B, int(span), int(wg), int(wc), int(min_gain), rounds,
                   *(_ptr(mid.get(k)) for k in ("label", "slot", "ncl", "rep", "csize", "cbox", "csum", "centre")),
                   *(_ptr(out[k]) for k in self._GAIN_KEYS))
        out.update(mid)
        return out

    # ---- planning in poses (sc_footprint_mask_u8, sc_pose_field_batch, sc_pose_paths_batch) ----
    def footprint_mask(self, d2, front, back, left, right, r2=0, out=None):
        """The per-heading collision mask of a rectangular body (sc_footprint_mask_u8): d2 int32 [H,W] or [B,H,W] on the GPU,
        the extents in whole cells, 0 .. FOOTPRINT_MAX, left counter-clockwise of the heading.  Returns uint8 shaped like d2:
        bit k set where the body, at heading k (POSE_HX, POSE_HY) and inflated by the disc r2 stands for, covers no blocked
        cell.  Only enqueues."""
        return self._footprint_mask(_on(d2.device), d2, front, back, left, right, r2, out)

    def footprint_mask_host(self, d2, front, back, left, right, r2=0):
        """Host form of footprint_mask (numpy in, numpy out)."""
        return self._footprint_mask(_HOST, d2, front, back, left, right, r2)

    def _footprint_mask(self, A, d2, front, back, left, right, r2, out=None):
        d2 = A.arr(d2, A.i32)
        B, H, W = _ghw(d2)
        if out is None:
            out = A.new(tuple(d2.shape), A.u8)
        _sized("out", out, B * H * W)
        self._call("sc_footprint_mask_u8" + A.suffix, _ptr(d2), W, H, B, r2, int(front), int(back), int(left), int(right), _ptr(out))
        return out

    def pose_fields(self, d2, roots, rhead, turn_cost, rev_cost=-1, toward=False, r2=0, hmask=None, fgrid=None, rounds=-1, out=None):
        """Cost fields over poses (sc_pose_field_batch): field f is rooted at the pose (roots[f], rhead[f]) (rhead -1: every
        valid heading of the cell) on grid fgrid[f].  d2 int32 [H,W] or [G,H,W], roots / rhead / fgrid int32 [F], hmask uint8
        shaped like d2 (what footprint_mask returned) or None, all on the GPU.  A forward move costs 10 / 14, a reverse move
        rev_cost more (-1: none), a turn of 45 degrees on the spot turn_cost.  toward: the cost from every pose to the root
        pose instead of from it.  Returns dict(gp int32 [F,8,H,W], status int32 [F]).  Only enqueues."""
        return self._pose_fields(_on(d2.device), d2, roots, rhead, turn_cost, rev_cost, toward, r2, hmask, fgrid, rounds, out)

    def pose_fields_host(self, d2, roots, rhead, turn_cost, rev_cost=-1, toward=False, r2=0, hmask=None, fgrid=None, rounds=-1):
        """Host form of pose_fields (numpy in, numpy out)."""
        return self._pose_fields(_HOST, d2, roots, rhead, turn_cost, rev_cost, toward, r2, hmask, fgrid, rounds)

    def _pose_fields(self, A, d2, roots, rhead, turn_cost, rev_cost, toward, r2, hmask, fgrid, rounds, out=None):
        d2, roots, rhead, fgrid, hmask = A.arr(d2, A.i32), A.arr(roots, A.i32), A.arr(rhead, A.i32), A.arr(fgrid, A.i32), A.arr(hmask, A.u8)
        G, H, W = _ghw(d2)
        F = _count(roots)
        if out is None:
            out = dict(gp=A.new((F, POSE_HEADINGS, H, W), A.i32), status=A.new(F, A.i32))
        _sized("rhead", rhead, F)
        _sized("fgrid", fgrid, F)
        _sized("hmask", hmask, G * H * W)
        _sized("out['gp']", out["gp"], F * POSE_HEADINGS * H * W)
        _sized("out['status']", out["status"], F)
        self._call("sc_pose_field_batch" + A.suffix, _ptr(d2), _ptr(hmask), G, _ptr(fgrid), W, H, r2, int(turn_cost), int(rev_cost),
                   int(bool(toward)), _ptr(roots), _ptr(rhead), F, rounds, _ptr(out["gp"]), _ptr(out["status"]))
        return out

    def pose_paths(self, d2, gp, roots, rhead, qfield, targets, thead, turn_cost, rev_cost=-1, toward=False, r2=0, hmask=None, Lmax=4096,
                   to_root=False, cells_only=False, fgrid=None, out=None):
        """Pose paths read from pose fields (sc_pose_paths_batch): query q follows field qfield[q] (gp, roots, rhead and the
        costs as pose_fields took and returned them) to the pose (targets[q], thead[q]); thead -1: the cheapest heading there.
        Returns dict(path int32 [Q,Lmax] cells, head uint8 [Q,Lmax] headings, len, cost, status int32 [Q]), one entry per
        pose; to_root writes target..root (the driving order of a toward field); cells_only keeps the first pose of every
        cell, which makes path a cell path path_waypoints takes.  turn_cost 0 is refused.  Only enqueues."""
        return self._pose_paths(_on(d2.device), d2, gp, roots, rhead, qfield, targets, thead, turn_cost, rev_cost, toward, r2, hmask, Lmax,
                                to_root, cells_only, fgrid, out)

    def pose_paths_host(self, d2, gp, roots, rhead, qfield, targets, thead, turn_cost, rev_cost=-1, toward=False, r2=0, hmask=None, Lmax=4096,
                        to_root=False, cells_only=False, fgrid=None):
        """Host form of pose_paths (numpy in, numpy out)."""
        return self._pose_paths(_HOST, d2, gp, roots, rhead, qfield, targets, thead, turn_cost, rev_cost, toward, r2, hmask, Lmax, to_root,
                                cells_only, fgrid)

    def _pose_paths(self, A, d2, gp, roots, rhead, qfield, targets, thead, turn_cost, rev_cost, toward, r2, hmask, Lmax, to_root, cells_only,
                    fgrid, out=None):
        d2, gp, roots, rhead, qfield, targets, thead, fgrid = (A.arr(a, A.i32) for a in (d2, gp, roots, rhead, qfield, targets, thead, fgrid))
        hmask = A.arr(hmask, A.u8)
        G, H, W = _ghw(d2)
        F, Q = _count(roots), _count(targets)
        if out is None:
            out = A.paths_out(Q, Lmax)
            out["head"] = A.new((Q, Lmax), A.u8)
        _sized("gp", gp, F * POSE_HEADINGS * H * W)
        _sized("rhead", rhead, F)
        _sized("fgrid", fgrid, F)
        _sized("hmask", hmask, G * H * W)
        _sized("qfield", qfield, Q)
        _sized("thead", thead, Q)
        _sized("out['path']", out["path"], Q * Lmax)
        _sized("out['head']", out["head"], Q * Lmax)
        self._call("sc_pose_paths_batch" + A.suffix, _ptr(d2), _ptr(hmask), G, _ptr(fgrid), W, H, r2, int(turn_cost), int(rev_cost),
                   int(bool(toward)), _ptr(gp), _ptr(roots), _ptr(rhead), F, _ptr(qfield), _ptr(targets), _ptr(thead), Q, Lmax,
                   int(bool(to_root)), int(bool(cells_only)), _ptr(out["path"]), _ptr(out["head"]), _ptr(out["len"]), _ptr(out["cost"]),
                   _ptr(out["status"]))
        return out

    # ---- car-like pose planning (sc_arc_mask_u16, sc_car_field_batch, sc_car_paths_batch) ----
    def arc_mask(self, d2, arc_n, r2=0, hmask=None, out=None):
        """The legal arcs of every pose (sc_arc_mask_u16): d2 int32 [H,W] or [B,H,W] on the GPU, hmask uint8 shaped like d2
        (what footprint_mask returned) or None, arc_n 1 .. ARC_MAX.  An arc is arc_n cells straight, 45 degrees, arc_n cells
        straight.  Returns int16 shaped like d2 (the bits of uint16): bit 2k of a cell is set where the arc from heading k to
        k + 1 is legal, bit 2k + 1 where the one to k - 1 is.  Only enqueues."""
        return self._arc_mask(_on(d2.device), d2, arc_n, r2, hmask, out)

    def arc_mask_host(self, d2, arc_n, r2=0, hmask=None):
        """Host form of arc_mask (numpy in, numpy uint16 out)."""
        return self._arc_mask(_HOST, d2, arc_n, r2, hmask)

    def _arc_mask(self, A, d2, arc_n, r2, hmask, out=None):
        d2, hmask = A.arr(d2, A.i32), A.arr(hmask, A.u8)
        B, H, W = _ghw(d2)
        _car_ranges(arc_n, 0, -1)
        if out is None:
            out = A.new(tuple(d2.shape), A.w16)
        _sized("hmask", hmask, B * H * W)
        _sized("out", out, B * H * W)
        self._call("sc_arc_mask_u16" + A.suffix, _ptr(d2), _ptr(hmask), W, H, B, r2, int(arc_n), _ptr(out))
        return out

    def car_fields(self, d2, amask, roots, rhead, arc_n, arc_cost=0, rev_cost=-1, toward=False, r2=0, hmask=None, fgrid=None, rounds=-1,
                   out=None):
        """Cost fields over poses for a car-like body (sc_car_field_batch): pose_fields' arguments, but the heading changes
        only along the arcs of amask (what arc_mask returned for the same d2, hmask, r2 and arc_n), never on the spot.  A
        forward move costs 10 / 14, an arc 24 arc_n + arc_cost, reversing rev_cost more per cell (-1: none).  toward: the cost
        from every pose to the root pose.  Returns dict(gp int32 [F,8,H,W], status int32 [F]).  Only enqueues."""
        return self._car_fields(_on(d2.device), d2, amask, roots, rhead, arc_n, arc_cost, rev_cost, toward, r2, hmask, fgrid, rounds, out)

    def car_fields_host(self, d2, amask, roots, rhead, arc_n, arc_cost=0, rev_cost=-1, toward=False, r2=0, hmask=None, fgrid=None,
                        rounds=-1):
        """Host form of car_fields (numpy in, numpy out)."""
        return self._car_fields(_HOST, d2, amask, roots, rhead, arc_n, arc_cost, rev_cost, toward, r2, hmask, fgrid, rounds)

    def _car_fields(self, A, d2, amask, roots, rhead, arc_n, arc_cost, rev_cost, toward, r2, hmask, fgrid, rounds, out=None):
        d2, roots, rhead, fgrid, hmask = A.arr(d2, A.i32), A.arr(roots, A.i32), A.arr(rhead, A.i32), A.arr(fgrid, A.i32), A.arr(hmask, A.u8)
        amask = A.words(amask, A.w16)
        G, H, W = _ghw(d2)
        F = _count(roots)
        _car_ranges(arc_n, arc_cost, rev_cost)
        if amask is None:
            raise SeaCurrentError("amask is mandatory: pass what arc_mask returned")
        if out is None:
            out = dict(gp=A.new((F, POSE_HEADINGS, H, W), A.i32), status=A.new(F, A.i32))
        _sized("amask", amask, G * H * W)
        _sized("rhead", rhead, F)
        _sized("fgrid", fgrid, F)
        _sized("hmask", hmask, G * H * W)
        _sized("out['gp']", out["gp"], F * POSE_HEADINGS * H * W)
        _sized("out['status']", out["status"], F)
        self._call("sc_car_field_batch" + A.suffix, _ptr(d2), _ptr(hmask), _ptr(amask), G, _ptr(fgrid), W, H, r2, int(arc_n), int(arc_cost),
                   int(rev_cost), int(bool(toward)), _ptr(roots), _ptr(rhead), F, rounds, _ptr(out["gp"]), _ptr(out["status"]))
        return out

    def car_paths(self, d2, amask, gp, roots, rhead, qfield, targets, thead, arc_n, arc_cost=0, rev_cost=-1, toward=False, r2=0, hmask=None,
                  Lmax=4096, to_root=False, fgrid=None, out=None):
        """Car paths read from car fields (sc_car_paths_batch): query q follows field qfield[q] (gp, roots, rhead, amask and the
        costs as car_fields took and returned them) to the pose (targets[q], thead[q]); thead -1: the cheapest heading there.
        Returns astar_batch's dict plus head uint8 [Q,Lmax]: one entry per cell, the cells of an arc included, so path is
        8-connected and goes straight into path_waypoints; to_root writes target..root (the driving order of a toward field).
        Only enqueues."""
        return self._car_paths(_on(d2.device), d2, amask, gp, roots, rhead, qfield, targets, thead, arc_n, arc_cost, rev_cost, toward, r2,
                               hmask, Lmax, to_root, fgrid, out)

    def car_paths_host(self, d2, amask, gp, roots, rhead, qfield, targets, thead, arc_n, arc_cost=0, rev_cost=-1, toward=False, r2=0,
                       hmask=None, Lmax=4096, to_root=False, fgrid=None):
        """Host form of car_paths (numpy in, numpy out)."""
        return self._car_paths(_HOST, d2, amask, gp, roots, rhead, qfield, targets, thead, arc_n, arc_cost, rev_cost, toward, r2, hmask, Lmax,
                               to_root, fgrid)

    def _car_paths(self, A, d2, amask, gp, roots, rhead, qfield, targets, thead, arc_n, arc_cost, rev_cost, toward, r2, hmask, Lmax, to_root,
                   fgrid, out=None):
        d2, gp, roots, rhead, qfield, targets, thead, fgrid = (A.arr(a, A.i32) for a in (d2, gp, roots, rhead, qfield, targets, thead, fgrid))
        hmask, amask = A.arr(hmask, A.u8), A.words(amask, A.w16)
        G, H, W = _ghw(d2)
        F, Q = _count(roots), _count(targets)
        _car_ranges(arc_n, arc_cost, rev_cost)
        if amask is None:
            raise SeaCurrentError("amask is mandatory: pass what arc_mask returned")
        if Lmax < 1:
            raise SeaCurrentError(f"Lmax is {Lmax}, the call needs at least 1")
        if out is None:
            out = A.paths_out(Q, Lmax)
            out["head"] = A.new((Q, Lmax), A.u8)
        _sized("amask", amask, G * H * W)
        _sized("gp", gp, F * POSE_HEADINGS * H * W)
        _sized("rhead", rhead, F)
        _sized("fgrid", fgrid, F)
        _sized("hmask", hmask, G * H * W)
        _sized("qfield", qfield, Q)
        _sized("thead", thead, Q)
        _sized("out['path']", out["path"], Q * Lmax)
        _sized("out['head']", out["head"], Q * Lmax)
        self._call("sc_car_paths_batch" + A.suffix, _ptr(d2), _ptr(hmask), _ptr(amask), G, _ptr(fgrid), W, H, r2, int(arc_n), int(arc_cost),
                   int(rev_cost), int(bool(toward)), _ptr(gp), _ptr(roots), _ptr(rhead), F, _ptr(qfield), _ptr(targets), _ptr(thead), Q, Lmax,
                   int(bool(to_root)), _ptr(out["path"]), _ptr(out["head"]), _ptr(out["len"]), _ptr(out["cost"]), _ptr(out["status"]))
        return out

    # ---- occupancy from range scans (sc_scan_cast_batch, sc_logodds_update) ----
    def scan_cast(self, rays, occ, out=None):
        """The simulated range sensor (sc_scan_cast_batch): rays int32 [N,4] = (ax, ay, bx, by) and occ uint8 [H,W] (the true
        map) on the GPU.  Returns hit int32 [N]: the first occupied cell of the walk from a to b, SCAN_NO_RETURN when there is
        none, SCAN_IGNORED for a ray that is ignored (a outside the grid, a reach above SCAN_MAX_REACH) or whose sensor stands
        on an occupied cell.  b may lie outside the grid.  Only enqueues."""
        return self._scan_cast(_on(occ.device), rays, occ, out)

    def scan_cast_host(self, rays, occ):
        """Host form of scan_cast (numpy in, numpy out)."""
        return self._scan_cast(_HOST, rays, occ)

    def _scan_cast(self, A, rays, occ, out=None):
        rays, occ = A.rows(rays, A.i32, 4), A.arr(occ, A.u8)
        H, W = occ.shape
        if out is None:
            out = A.new(rays.shape[0], A.i32)
        _sized("scan_cast: rays", rays, 4 * rays.shape[0])
        _sized("scan_cast: out", out, rays.shape[0])
        self._call("sc_scan_cast_batch" + A.suffix, _ptr(occ), _ptr(rays), rays.shape[0], W, H, _ptr(out))
        return out

    def logodds_update(self, rays, hit, W, H, L=None, l_hit=LOGODDS_HIT, l_miss=LOGODDS_MISS, l_clamp=LOGODDS_CLAMP, t_occ=LOGODDS_T_OCC,
                       t_free=LOGODDS_T_FREE, out=None, occ_est=None, known=None):
        """The occupancy-grid update from beams (sc_logodds_update): rays int32 [N,4] and hit int32 [N] (what scan_cast wrote, or
        recorded ends) on the GPU, L int32 [H,W] the map so far (None: all zeros; may be `out`).  Every cell some beam hits
        gains l_hit, every other cell some beam passes loses l_miss -- once per call however many beams cross it -- and the
        result is clamped to +-l_clamp.  occ_est / known: a uint8 [H,W] tensor, or True to have one allocated; occ_est = L >=
        t_occ, known = occ_est or L <= -t_free: the (occ_seen, known) pair the exploration calls take.  Returns L alone, or a
        tuple in the order (L, occ_est, known) of those requested.  rays and hit may be None (or empty): no beam, the stored
        map is clamped and turned into masks.  The defaults make one look decide a cell (l_hit >= t_occ, l_miss >= t_free: the
        estimate never contradicts a static true map) and the clamp four hits or eight misses deep, so that a cell that
        changed is taken back after a few scans.  Only enqueues."""
        src = next((x for x in (L, rays, out) if x is not None), None)
        A = _on(src.device if src is not None else "cuda:%d" % self.device)
        return self._logodds_update(A, rays, hit, W, H, L, l_hit, l_miss, l_clamp, t_occ, t_free, out, occ_est, known)

    def logodds_update_host(self, rays, hit, W, H, L=None, l_hit=LOGODDS_HIT, l_miss=LOGODDS_MISS, l_clamp=LOGODDS_CLAMP,
                            t_occ=LOGODDS_T_OCC, t_free=LOGODDS_T_FREE, occ_est=None, known=None):
        """Host form of logodds_update (numpy in, numpy out); a hit below SCAN_IGNORED or >= W * H is an error."""
        return self._logodds_update(_HOST, rays, hit, W, H, L, l_hit, l_miss, l_clamp, t_occ, t_free, None, occ_est, known)

    def _logodds_update(self, A, rays, hit, W, H, L, l_hit, l_miss, l_clamp, t_occ, t_free, out, occ_est, known):
        rays, hit, L = A.rows(rays, A.i32, 4), A.arr(hit, A.i32), A.arr(L, A.i32)
        N = 0 if rays is None else rays.shape[0]
        if out is None:
            out = A.new((H, W), A.i32)
        if occ_est is True:
            occ_est = A.new((H, W), A.u8)
        if known is True:
            known = A.new((H, W), A.u8)
        for what, x in (("L", L), ("out", out), ("occ_est", occ_est), ("known", known)):
            _sized("logodds_update: " + what, x, W * H)
        _sized("logodds_update: rays", rays, 4 * N)
        _sized("logodds_update: hit", hit if N else None, N)
        self._call("sc_logodds_update" + A.suffix, _ptr(L), _ptr(rays) if N else None, _ptr(hit) if N else None, N, W, H, l_hit, l_miss, l_clamp,
                   t_occ, t_free, _ptr(out), _ptr(occ_est), _ptr(known))
        res = (out,) + tuple(x for x in (occ_est, known) if x is not None)
        return out if len(res) == 1 else res

    # ---- scan matching (sc_scan_match_batch) ----
    def scan_match(self, pts, centre, d2, known=None, wx=8, wy=8, d2_cap=64, unk=1, out=None, score=None):
        """The pose of a scan against the map (sc_scan_match_batch): pts int32 [S,R,N,2], the scan's end points as cell offsets
        from the sensor, one set per scan and candidate rotation (points_from_hits, rotate_points; SCAN_MATCH_ABSENT where a
        beam has no end), centre int32 [S,2] the prior sensor cell, d2 int32 [H,W] the EDT of the estimated obstacles and
        known uint8 [H,W] (None: every cell), all on the GPU.  A cell costs min(d2, d2_cap), or unk where it is unknown or
        outside the grid; a pose scores the sum over its points.  Returns best int32 [S,6] = (r, dx, dy, score, n_points,
        n_ties): the smallest (score, dx^2 + dy^2, r, dy, dx) over the window +-wx, +-wy, and how many poses reach that score
        (1: the answer is unique); a scan whose centre is out of range reads (SCAN_MATCH_IGNORED, 0, ...).  score: an int32
        [S,R,2wy+1,2wx+1] tensor, or True to have one allocated; then the result is (best, score).  Only enqueues."""
        return self._scan_match(_on(d2.device), pts, centre, d2, known, wx, wy, d2_cap, unk, out, score)

    def scan_match_host(self, pts, centre, d2, known=None, wx=8, wy=8, d2_cap=64, unk=1, score=None):
        """Host form of scan_match (numpy in, numpy out); a centre out of range is an error."""
        return self._scan_match(_HOST, pts, centre, d2, known, wx, wy, d2_cap, unk, None, score)

    def _scan_match(self, A, pts, centre, d2, known, wx, wy, d2_cap, unk, out, score):
        pts, centre, d2, known = A.arr(pts, A.i32), A.rows(centre, A.i32, 2), A.arr(d2, A.i32), A.arr(known, A.u8)
        if len(pts.shape) != 4 or pts.shape[3] != 2 or len(d2.shape) != 2:
            raise SeaCurrentError(f"scan_match: pts is [S,R,N,2] and d2 [H,W], got {tuple(pts.shape)} and {tuple(d2.shape)}")
        S, R, N = (int(v) for v in pts.shape[:3])
        H, W = d2.shape
        vol = S * R * (2 * wy + 1) * (2 * wx + 1)
        if out is None:
            out = A.new((S, 6), A.i32)
        if score is True:
            score = A.new((S, R, 2 * wy + 1, 2 * wx + 1), A.i32)
        _sized("scan_match: centre", centre, 2 * S)
        _sized("scan_match: known", known, W * H)
        _sized("scan_match: out", out, 6 * S)
        _sized("scan_match: score", score, vol)
        self._call("sc_scan_match_batch" + A.suffix, _ptr(d2), _ptr(known), _ptr(pts), _ptr(centre), S, R, N, W, H, wx, wy, d2_cap, unk,
                   _ptr(out), _ptr(score))
        return out if score is None else (out, score)

    # ---- wide-window scan matching (sc_scan_match_wide_batch) ----
    def scan_match_wide(self, pts, centre, d2, known=None, wx=256, wy=256, d2_cap=64, unk=1, top=3, max_nodes=1 << 16, out=None, stats=None):
        """The pose of a scan in a wide window (sc_scan_match_wide_batch): the inputs and the result best int32 [S,6] of
        scan_match, for windows of up to +-SCAN_MATCH_WIDE_MAX_HALF cells, by an exact pruned search over a min-pooled
        pyramid of the cost map whose top nodes stand for 4^top x 4^top poses; best equals what the dense volume would give,
        ties included.  A scan whose search needs more than max_nodes nodes at a level reads (SCAN_MATCH_OVERFLOW, 0, ...).
        stats: an int32 [S,8] tensor = (n_0 .. n_5 nodes bounded per level, n_dive, U), or True to have one allocated; then
        the result is (best, stats).  Only enqueues."""
        return self._scan_match_wide(_on(d2.device), pts, centre, d2, known, wx, wy, d2_cap, unk, top, max_nodes, out, stats)

    def scan_match_wide_host(self, pts, centre, d2, known=None, wx=256, wy=256, d2_cap=64, unk=1, top=3, max_nodes=1 << 16, stats=None):
        """Host form of scan_match_wide (numpy in, numpy out); a centre out of range is an error."""
        return self._scan_match_wide(_HOST, pts, centre, d2, known, wx, wy, d2_cap, unk, top, max_nodes, None, stats)

    def _scan_match_wide(self, A, pts, centre, d2, known, wx, wy, d2_cap, unk, top, max_nodes, out, stats):
        pts, centre, d2, known = A.arr(pts, A.i32), A.rows(centre, A.i32, 2), A.arr(d2, A.i32), A.arr(known, A.u8)
        if len(pts.shape) != 4 or pts.shape[3] != 2 or len(d2.shape) != 2:
            raise SeaCurrentError(f"scan_match_wide: pts is [S,R,N,2] and d2 [H,W], got {tuple(pts.shape)} and {tuple(d2.shape)}")
        S, R, N = (int(v) for v in pts.shape[:3])
        H, W = d2.shape
        if out is None:
            out = A.new((S, 6), A.i32)
        if stats is True:
            stats = A.new((S, 8), A.i32)
        _sized("scan_match_wide: centre", centre, 2 * S)
        _sized("scan_match_wide: known", known, W * H)
        _sized("scan_match_wide: out", out, 6 * S)
        _sized("scan_match_wide: stats", stats, 8 * S)
        self._call("sc_scan_match_wide_batch" + A.suffix, _ptr(d2), _ptr(known), _ptr(pts), _ptr(centre), S, R, N, W, H, wx, wy, d2_cap, unk,
                   top, max_nodes, _ptr(out), _ptr(stats))
        return out if stats is None else (out, stats)

    # ---- multi-GPU gather (RCCL through the C ABI) ----
    @staticmethod
    def comm_unique_id():
        """128 bytes of an ncclUniqueId (call on one rank, hand to all)."""
        buf = C.create_string_buffer(128)
        st = lib().sc_comm_unique_id(buf)
        if st != 0:
            raise SeaCurrentError(f"sc_comm_unique_id: {lib().sc_status_string(st).decode()}")
        return buf.raw

    def comm_init(self, unique_id, world, rank):
        self._ck(self._l.sc_comm_init(self._h, C.c_char_p(unique_id), world, rank), "sc_comm_init")
        self.world, self.rank = world, rank

    def allgather_paths(self, out, Q_total, cap_cells, want_path=False, bufs=None):
        """Every rank's astar_batch results on every rank, in query order (sc_allgather_paths).  `out` = this rank's dict;
        returns dict(len, cost, status [Q_total], offsets int64 [Q_total+1], cells [world*cap_cells], truncated [1], path?)."""
        import torch
        dev = out["len"].device
        Ql, Lmax = out["path"].shape
        world = getattr(self, "world", 1)
        if bufs is None:
            bufs = dict(len=torch.empty(Q_total, dtype=torch.int32, device=dev), cost=torch.empty(Q_total, dtype=torch.int32, device=dev),
                        status=torch.empty(Q_total, dtype=torch.int32, device=dev),
                        offsets=torch.empty(Q_total + 1, dtype=torch.int64, device=dev),
                        cells=torch.empty(world * cap_cells, dtype=torch.int32, device=dev),
                        truncated=torch.zeros(1, dtype=torch.int32, device=dev))
            if want_path:
                bufs["path"] = torch.empty((Q_total, Lmax), dtype=torch.int32, device=dev)
        self._ck(self._l.sc_allgather_paths(self._h, _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]), _ptr(out["status"]), Ql, Q_total, Lmax,
                                            cap_cells, _ptr(bufs["len"]), _ptr(bufs["cost"]), _ptr(bufs["status"]), _ptr(bufs["offsets"]),
                                            _ptr(bufs["cells"]), bufs["cells"].numel(), _ptr(bufs.get("path")), _ptr(bufs["truncated"])),
                 "sc_allgather_paths")
        return bufs

    def gather_pack(self, out, Q_total, world, rank, cap_cells, msg=None, Lmax=None):
        """This rank's message of the gather (sc_gather_pack): int32 [sc_gather_msg_words].  `out` = the rank's astar_batch
        dict (may hold zero queries)."""
        import torch
        Ql = int(out["len"].shape[0])
        if Lmax is None:
            Lmax = int(out["path"].shape[1])
        words = int(self._l.sc_gather_msg_words(Q_total, world, cap_cells))
        if msg is None:
            msg = torch.empty(words, dtype=torch.int32, device=out["len"].device)
        assert msg.numel() == words
        nz = Ql > 0
        self._ck(self._l.sc_gather_pack(self._h, _ptr(out["path"]) if nz else None, _ptr(out["len"]) if nz else None,
                                        _ptr(out["cost"]) if nz else None, _ptr(out["status"]) if nz else None, Ql, Q_total, world, rank,
                                        Lmax, cap_cells, _ptr(msg)), "sc_gather_pack")
        return msg

    def gather_unpack(self, msgs, world, Q_total, Lmax, cap_cells, want_path=False, cells_capacity=None):
        """sc_gather_unpack: `msgs` = the world messages back to back in rank order -> the dict allgather_paths returns."""
        import torch
        dev = msgs.device
        cc = world * cap_cells if cells_capacity is None else cells_capacity
        bufs = dict(len=torch.empty(Q_total, dtype=torch.int32, device=dev), cost=torch.empty(Q_total, dtype=torch.int32, device=dev),
                    status=torch.empty(Q_total, dtype=torch.int32, device=dev), offsets=torch.empty(Q_total + 1, dtype=torch.int64, device=dev),
                    cells=torch.full((cc,), -7, dtype=torch.int32, device=dev), truncated=torch.zeros(1, dtype=torch.int32, device=dev))
        if want_path:
            bufs["path"] = torch.full((Q_total, Lmax), -7, dtype=torch.int32, device=dev)
        self._ck(self._l.sc_gather_unpack(self._h, _ptr(msgs), world, Q_total, Lmax, cap_cells, _ptr(bufs["len"]), _ptr(bufs["cost"]),
                                          _ptr(bufs["status"]), _ptr(bufs["offsets"]), _ptr(bufs["cells"]), cc, _ptr(bufs.get("path")),
                                          _ptr(bufs["truncated"])), "sc_gather_unpack")
        return bufs

    def allgather_last_bytes(self):
        n = C.c_int64()
        self._ck(self._l.sc_allgather_last_bytes(self._h, C.byref(n)), "sc_allgather_last_bytes")
        return n.value

    def astar_last_expansions(self):
        n = C.c_int64(0)
        self._ck(self._l.sc_astar_last_expansions(self._h, C.byref(n)), "sc_astar_last_expansions")
        return n.value

    def astar_debug_stats(self, Q):
        """Per-query (expansions, popped entries, kilo-cycles, steps) of the last astar_batch (synchronises)."""
        out = np.zeros((4, Q), dtype=np.int32)
        self._ck(self._l.sc_astar_debug_stats(self._h, _ptr(out), Q), "sc_astar_debug_stats")
        return out[0], out[1], out[2], out[3]

    def astar_gfield(self, d2, start, goal, r2=0):
        import torch
        H, W = d2.shape
        g = torch.empty((H, W), dtype=torch.int32, device=d2.device)
        cs = torch.empty(2, dtype=torch.int32, device=d2.device)
        self._ck(self._l.sc_astar_gfield(self._h, _ptr(d2), W, H, r2, int(start), int(goal), _ptr(g),
                                         cs.data_ptr(), cs.data_ptr() + 4), "sc_astar_gfield")
        self.synchronize()
        cost, status = cs.cpu().tolist()
        if status == Q_TRUNCATED:  # the path itself is not requested (Lmax = 1)
            status = Q_OK
        return g.cpu().numpy().view(np.uint32), cost, status

    def toppra(self, p0, p1, v0, v1, vlim_lo, vlim_hi, alim_lo, alim_hi, N=100, sd_start=0.0, sd_end=0.0):
        """All inputs float64 GPU tensors [P,dof] (vlim may be [P,N+1,dof])."""
        import torch
        P, dof = p0.shape
        per_stage = int(vlim_lo.dim() == 3)
        dev = p0.device
        out = dict(K=torch.empty((P, N + 1, 2), dtype=torch.float64, device=dev),
                   x=torch.empty((P, N + 1), dtype=torch.float64, device=dev),
                   u=torch.empty((P, N), dtype=torch.float64, device=dev),
                   t=torch.empty((P, N + 1), dtype=torch.float64, device=dev),
                   status=torch.empty(P, dtype=torch.int32, device=dev))
        self._ck(self._l.sc_toppra_hermite_batch(self._h, P, dof, N, _ptr(p0), _ptr(p1), _ptr(v0), _ptr(v1),
                                                 _ptr(vlim_lo), _ptr(vlim_hi), per_stage, _ptr(alim_lo), _ptr(alim_hi),
                                                 sd_start, sd_end, _ptr(out["K"]), _ptr(out["x"]), _ptr(out["u"]),
                                                 _ptr(out["t"]), _ptr(out["status"])), "sc_toppra_hermite_batch")
        return out

    def toppra_sample(self, p0, p1, v0, v1, x, t, dt, max_len):
        import torch
        P, dof = p0.shape
        N = x.shape[1] - 1
        dev = p0.device
        out = dict(pos=torch.zeros((P, dof, max_len), dtype=torch.float32, device=dev),
                   vel=torch.zeros((P, dof, max_len), dtype=torch.float32, device=dev),
                   acc=torch.zeros((P, dof, max_len), dtype=torch.float32, device=dev),
                   time=torch.zeros((P, max_len), dtype=torch.float64, device=dev),
                   length=torch.empty(P, dtype=torch.int32, device=dev))
        self._ck(self._l.sc_toppra_sample_batch(self._h, P, dof, N, _ptr(p0), _ptr(p1), _ptr(v0), _ptr(v1), _ptr(x),
                                                _ptr(t), float(dt), max_len, _ptr(out["pos"]), _ptr(out["vel"]),
                                                _ptr(out["acc"]), _ptr(out["time"]), _ptr(out["length"])),
                 "sc_toppra_sample_batch")
        return out

    def fmt_star(self, samples, starts, goals, rn, lines, Lmax=256):
        """FMT* (the reference's planner) for Q queries over shared samples.  GPU float32 tensors: samples [n,2], starts / goals
        [Q,2], lines [E,4] -> dict(path [Q,Lmax,2], len, cost, status)."""
        import torch
        Q = starts.shape[0]
        dev = starts.device
        out = dict(path=torch.zeros((Q, Lmax, 2), dtype=torch.float32, device=dev), len=torch.zeros(Q, dtype=torch.int32, device=dev),
                   cost=torch.zeros(Q, dtype=torch.float32, device=dev), status=torch.zeros(Q, dtype=torch.int32, device=dev))
        E = 0 if lines is None else lines.shape[0]
        self._ck(self._l.sc_fmt_star_batch(self._h, _ptr(samples), samples.shape[0], _ptr(starts), _ptr(goals), Q, float(rn),
                                           _ptr(lines) if E else None, E, Lmax, _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]),
                                           _ptr(out["status"])), "sc_fmt_star_batch")
        return out

    def edt_nearest(self, occ, d2):
        """occ uint8 [B,H,W] or [H,W] and its d2 (GPU) -> int32 index of the nearest occupied cell per cell (-1: none)."""
        import torch
        o3 = occ if occ.dim() == 3 else occ[None]
        B, H, W = o3.shape
        out = torch.empty((B, H, W), dtype=torch.int32, device=occ.device)
        self._ck(self._l.sc_edt_nearest_i32(self._h, _ptr(o3), _ptr(d2), W, H, B, _ptr(out)), "sc_edt_nearest_i32")
        return out if occ.dim() == 3 else out[0]

    def occ_from_rects(self, rects, W, H, base=None, free_border=True, out=None):
        """rects int32 [R,4] (x0,y0,x1,y1 exclusive; GPU) painted over `base` uint8 [H,W] (or an empty grid) -> occ uint8 [H,W]."""
        import torch
        occ = out if out is not None else torch.empty((H, W), dtype=torch.uint8, device=rects.device)
        self._ck(self._l.sc_occ_from_rects(self._h, _ptr(base) if base is not None else None, _ptr(rects), rects.shape[0], W, H,
                                           1 if free_border else 0, _ptr(occ)), "sc_occ_from_rects")
        return occ

    def occ_from_polygons(self, lines, obs_off, W, H, x_min, y_min, res_x, res_y, closed=None, box=None, grid_off=None, base=None,
                          out=None):
        """Polygon obstacles -> occupancy grids (sc_occ_from_polygons), GPU tensors: lines float32 [E,4] (x0,y0,x1,y1),
        obs_off int32 [n_obs+1], closed uint8 [n_obs] (None: all closed), box float32 [n_obs,4] in bound_rect order
        (x_max, x_min, y_max, y_min; None: each obstacle's own lines), grid_off int32 [G+1] (None: one grid).  Returns uint8
        [H,W] without grid_off, else [G,H,W]; base (same shape) is painted over, base is out paints in place."""
        return self._occ_from_polygons(_on(obs_off.device), lines, obs_off, W, H, x_min, y_min, res_x, res_y, closed, box, grid_off, base, out)

    def occ_from_polygons_host(self, lines, obs_off, W, H, x_min, y_min, res_x, res_y, closed=None, box=None, grid_off=None,
                               base=None):
        """Host form of occ_from_polygons (numpy in, numpy out; sc_occ_from_polygons_host checks the contract first)."""
        return self._occ_from_polygons(_HOST, lines, obs_off, W, H, x_min, y_min, res_x, res_y, closed, box, grid_off, base)

    def _occ_from_polygons(self, A, lines, obs_off, W, H, x_min, y_min, res_x, res_y, closed, box, grid_off, base, out=None):
        lines, box, closed = A.rows(lines, A.f32, 4), A.rows(box, A.f32, 4), A.arr(closed, A.u8)
        obs_off, grid_off = A.arr(obs_off, A.i32), A.arr(grid_off, A.i32)
        G = 1 if grid_off is None else grid_off.shape[0] - 1
        shape = (H, W) if grid_off is None else (G, H, W)
        if A is _HOST and base is not None:
            base = out = A.own(base, A.u8).reshape(shape)         # the host form paints over a copy of base, in place
        elif out is None:
            out = A.new(shape, A.u8)
        self._call("sc_occ_from_polygons" + A.suffix, _ptr(base), G, W, H, x_min, y_min, res_x, res_y, _ptr(lines) if lines.shape[0] else None,
                   lines.shape[0], _ptr(obs_off), obs_off.shape[0] - 1, _ptr(box), _ptr(closed), _ptr(grid_off), _ptr(out))
        return out

    def bezier_from_path(self, path, npts, start_angle=float("nan"), lines=None):
        """path float32 [P,n_max,2], npts int32 [P] (GPU) -> ctrl float32 [P,n_max-1,4,2]."""
        import torch
        P, n_max, _ = path.shape
        ctrl = torch.empty((P, n_max - 1, 4, 2), dtype=torch.float32, device=path.device)
        nl = 0 if lines is None else lines.shape[0]
        self._ck(self._l.sc_bezier_from_path_batch(self._h, _ptr(path), _ptr(npts), P, n_max, start_angle,
                                                   _ptr(lines) if nl else None, nl, _ptr(ctrl)), "sc_bezier_from_path_batch")
        return ctrl

    def bezier_eval(self, ctrl, seg, t, order=0):
        import torch
        M = t.shape[0]
        out = torch.empty((M, 2), dtype=torch.float32, device=t.device)
        self._ck(self._l.sc_bezier_eval_batch(self._h, _ptr(ctrl), _ptr(seg), _ptr(t), M, order, _ptr(out)), "sc_bezier_eval_batch")
        return out

    def bezier_curve(self, ctrl, seg, t):
        """General degree: ctrl float32 [S, degree+1, 2] (GPU), seg int32 [M], t float32 [M] -> points float32 [M, 2]."""
        import torch
        M = t.shape[0]
        out = torch.empty((M, 2), dtype=torch.float32, device=t.device)
        self._ck(self._l.sc_bezier_curve_batch(self._h, _ptr(ctrl), ctrl.shape[1] - 1, _ptr(seg), _ptr(t), M, _ptr(out)), "sc_bezier_curve_batch")
        return out

    def chebfit(self, x, y, off, degree):
        """B least-squares Chebyshev fits; x, y float32 [total], off int32 [B+1] (all GPU) -> (coef [B, degree], xrange [B, 2])."""
        import torch
        B = off.shape[0] - 1
        coef = torch.empty((B, degree), dtype=torch.float32, device=x.device)
        xr = torch.empty((B, 2), dtype=torch.float32, device=x.device)
        self._ck(self._l.sc_chebfit_batch(self._h, _ptr(x), _ptr(y), _ptr(off), B, x.shape[0], degree, _ptr(coef), _ptr(xr)), "sc_chebfit_batch")
        return coef, xr

    def chebeval(self, x, off, coef, xr):
        import torch
        B, degree = coef.shape
        y = torch.empty_like(x)
        self._ck(self._l.sc_chebeval_batch(self._h, _ptr(x), _ptr(off), B, degree, _ptr(coef), _ptr(xr), _ptr(y)), "sc_chebeval_batch")
        return y

    def bezier_arclength(self, ctrl, nsub=100):
        """ctrl float32 [...,4,2] (GPU) -> (cum float32 [S,nsub+1], seg_len float32 [S])."""
        import torch
        c = ctrl.reshape(-1, 4, 2)
        S = c.shape[0]
        cum = torch.empty((S, nsub + 1), dtype=torch.float32, device=ctrl.device)
        seg_len = torch.empty(S, dtype=torch.float32, device=ctrl.device)
        self._ck(self._l.sc_bezier_arclength_batch(self._h, _ptr(c), S, nsub, _ptr(cum), _ptr(seg_len)), "sc_bezier_arclength_batch")
        return cum, seg_len

    def bezier_resample(self, ctrl, cum, arclength, seg_off, profile_pos, prof_off, nudge=True, want_curvature=True):
        """B splines (GPU tensors): ctrl float32 [S,4,2], cum float32 [S,nsub+1], arclength float32 [B], seg_off int32 [B+1],
        profile_pos float32 [M] (nudged IN PLACE when `nudge`), prof_off int32 [B+1] -> dict(pts [M,2], t [M], seg [M],
        curvature [M], status [B])."""
        import torch
        S, m = cum.shape
        B = arclength.shape[0]
        M = profile_pos.shape[0]
        dev = profile_pos.device
        out = dict(pts=torch.zeros((M, 2), dtype=torch.float32, device=dev), t=torch.zeros(M, dtype=torch.float32, device=dev),
                   seg=torch.zeros(M, dtype=torch.int32, device=dev), status=torch.zeros(B, dtype=torch.int32, device=dev),
                   curvature=torch.zeros(M, dtype=torch.float32, device=dev) if want_curvature else None)
        self._ck(self._l.sc_bezier_resample_batch(self._h, _ptr(ctrl), _ptr(cum), _ptr(arclength), _ptr(seg_off), B, S, m - 1,
                                                  _ptr(profile_pos), _ptr(prof_off), 1 if nudge else 0, _ptr(out["pts"]), _ptr(out["t"]),
                                                  _ptr(out["seg"]), _ptr(out["curvature"]) if want_curvature else None,
                                                  _ptr(out["status"])), "sc_bezier_resample_batch")
        return out


# ---- host helpers of scan matching (numpy) ----
def points_from_hits(rays, hit, W):
    """scan_cast's output as scan_match's points: int32 [N,2], the hit cell of every beam as a cell offset from its ray's
    origin (rays int32 [N,4], hit int32 [N], W the grid's width).  Integer and exact.  A beam without a return or an ignored
    one (hit < 0) becomes SCAN_MATCH_ABSENT."""
    rays, hit = np.asarray(rays, dtype=np.int64).reshape(-1, 4), np.asarray(hit, dtype=np.int64).reshape(-1)
    if len(rays) != len(hit):
        raise SeaCurrentError(f"points_from_hits: {len(rays)} rays and {len(hit)} hits")
    out = np.full((len(hit), 2), SCAN_MATCH_ABSENT, np.int64)
    ok = hit >= 0
    out[ok, 0], out[ok, 1] = hit[ok] % W - rays[ok, 0], hit[ok] // W - rays[ok, 1]
    return out.astype(np.int32)


def rotate_points(pts, angles):
    """Candidate rotations of a scan: pts int32 [..., N, 2] and angles [R] in radians -> int32 [..., R, N, 2], every point
    turned by each angle about the sensor ((x, y) -> (x cos a - y sin a, x sin a + y cos a), in float64 on the host) and
    rounded to the nearest cell.  Absent points stay SCAN_MATCH_ABSENT.  No bit-exactness is claimed but at multiples of a
    quarter turn, where the result is the integer rotation (x, y) -> (-y, x) applied that many times."""
    p = np.asarray(pts, dtype=np.int64)
    a = np.asarray(angles, dtype=np.float64).reshape(-1)
    ok = (np.abs(p) <= SCAN_MAX_REACH).all(-1)
    x, y = np.where(ok, p[..., 0], 0).astype(np.float64)[..., None, :], np.where(ok, p[..., 1], 0).astype(np.float64)[..., None, :]
    # at a multiple of a quarter turn cos and sin are within 1e-15 of 0 and +-1 and |x|, |y| <= 2^14: the sums lie within
    # 1e-10 of the integers they stand for, and rounding gives exactly those
    c, s = np.cos(a)[:, None], np.sin(a)[:, None]
    out = np.stack([np.rint(x * c - y * s), np.rint(x * s + y * c)], -1).astype(np.int64)
    return np.where(ok[..., None, :, None], out, SCAN_MATCH_ABSENT).astype(np.int32)


# ---- host helpers of sensors with a field of view (numpy) ----
def heading_dirs(B, phase=0.0):
    """The heading table of B evenly spaced directions, counter-clockwise: int32 [B,2] =
    round(32767 (cos, sin)(2 pi (b + phase) / B)), 3 <= B <= VIEW_MAX_BINS, computed in float64.  Valid for
    view_gain_headings; no bit claim beyond that."""
    if not 3 <= int(B) <= VIEW_MAX_BINS:
        raise SeaCurrentError(f"heading_dirs: B = {B} outside 3 .. {VIEW_MAX_BINS}")
    t = 2.0 * np.pi * (np.arange(int(B), dtype=np.float64) + float(phase)) / int(B)
    return np.rint(32767.0 * np.stack([np.cos(t), np.sin(t)], 1)).astype(np.int32)


def sector_views(views, dirs, h, span):
    """Views with a heading as sector rows: views int32 [N,3], dirs int32 [B,2], h a heading or [N] headings, span the bins the
    sensor covers -> int32 [N,7] = (cx, cy, r2, dirs[h], dirs[(h + span) % B]); span == B gives a = b = 0, the full circle."""
    views = np.asarray(views, dtype=np.int32).reshape(-1, 3)
    dirs = np.asarray(dirs, dtype=np.int32).reshape(-1, 2)
    B = len(dirs)
    if not 1 <= int(span) <= B:
        raise SeaCurrentError(f"sector_views: span = {span} outside 1 .. {B}")
    h = np.broadcast_to(np.asarray(h, dtype=np.int64), (len(views),)) % B
    out = np.zeros((len(views), 7), np.int32)
    out[:, :3] = views
    if int(span) < B:
        out[:, 3:5], out[:, 5:7] = dirs[h], dirs[(h + int(span)) % B]
    return out
