"""The space-time re-planning at the drop-in boundary: the six C functions are declared in include/sea_current_hip.h and
exported by the built library, the binding's signatures match them in count and kind, the combined call takes the reserving
call's arguments followed by the search's and r_new, sequential, nothing older moved, and the Python methods exist with their
defaults.  No GPU."""
import ctypes
import inspect
import re

import pytest

import sea_current_amd as sc

BASE = ("sc_traj_reserve_batch", "sc_tplan_batch", "sc_fleet_replan_batch")
NEW = BASE + tuple(n + "_host" for n in BASE)


@pytest.fixture(scope="module")
def built():
    sc.build()
    return ctypes.CDLL(sc.LIB_PATH)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(sc.HEADER_PATH).read(), flags=re.S)


def _params(name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S)
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_declared_and_exported(built):
    src = _header()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), f"{n} not declared"
        assert hasattr(built, n), f"{n} not exported"
        assert n in sc.EXPORTS
    assert re.search(r"SC_TP_OK = 0,\s*SC_TP_NO_PATH = 1,\s*SC_TP_BAD_ENDPOINT = 2,\s*SC_TP_START_BLOCKED = 3\s*}\s*sc_tplan_status;", src)
    assert (sc.TP_OK, sc.TP_NO_PATH, sc.TP_BAD_ENDPOINT, sc.TP_START_BLOCKED) == (0, 1, 2, 3)


def test_additive(built):
    src = _header()
    assert re.search(r"SC_K_COUNT = 15\b", src) and re.search(r"SC_K_ASTAR = 3\b", src) and re.search(r"SC_K_SMOOTH = 14\b", src)
    assert re.search(r"#define\s+SC_ABI_VERSION\s+1\b", src)
    assert re.search(r"SC_TRAJ_OK = 0,\s*SC_TRAJ_SKIPPED = 1,\s*SC_TRAJ_BAD = 2\s*}\s*sc_traj_status;", src)
    assert re.search(r"#define\s+SC_SLOT_UNRESOLVED\s+\(-1\)", src)
    built.sc_abi_version.restype = ctypes.c_int
    assert built.sc_abi_version() == 1


def test_parameter_counts_and_order():
    kinds = (("double ", ctypes.c_double), ("float ", ctypes.c_float), ("int32_t ", ctypes.c_int32), ("int ", ctypes.c_int))
    for suffix in ("", "_host"):
        rs, tp, fl = (_params(n + suffix) for n in BASE)
        assert rs == ["sc_ctx* ctx", "const double* knots", "int32_t* tstatus", "int P", "int K", "const double* radius", "const int32_t* select",
                      "double pad", "int W", "int H", "float x_min", "float y_min", "float res_x", "float res_y", "uint32_t* res"]
        assert tp == ["sc_ctx* ctx", "const int32_t* d2", "int W", "int H", "int32_t r2_clear", "const uint32_t* res", "int L",
                      "const int32_t* start", "const int32_t* goal", "const int32_t* t_start", "int B", "int hold", "int32_t* path", "int32_t* len",
                      "int32_t* arrive", "int32_t* status", "double* knots_out", "float x_min", "float y_min", "float res_x", "float res_y",
                      "uint32_t* reach"]
        assert len(fl) == 31
        assert fl[:15] == rs                                            # the combined call: the reserving call's arguments ...
        assert fl[15:17] == [tp[1], tp[4]]                              # ... d2 and r2_clear (W, H, res and the frame are already there) ...
        assert fl[17:29] == tp[6:17] + tp[21:]                          # ... L, the queries, the outputs, reach ...
        assert fl[29:] == ["const double* r_new", "int sequential"]     # ... and what only the combined call has
        for n, params in zip(BASE, (rs, tp, fl)):
            assert len(sc._SIGNATURES[n + suffix][1]) == len(params), n + suffix
            for ctype, decl in zip(sc._SIGNATURES[n + suffix][1], params):
                want = next((t for prefix, t in kinds if decl.startswith(prefix)), ctypes.c_void_p)
                assert ctype is want, (n + suffix, decl)


def test_binding_has_the_methods_and_keywords():
    for name in ("traj_reserve", "traj_reserve_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[:8] == ["self", "knots", "tstatus", "radius", "W", "H", "frame", "pad"], name
        assert p["select"].default is None and p["res"].default is None, name
    for name in ("tplan", "tplan_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[:4] == ["self", "d2", "start", "goal"], name
        assert p["res"].default is None and p["L"].default is None and p["t_start"].default is None and p["hold"].default is True, name
        assert p["r2"].default == 0 and p["frame"].default is None and p["want_reach"].default is False, name
    for name in ("fleet_replan", "fleet_replan_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[:9] == ["self", "knots", "tstatus", "radius", "d2", "start", "goal", "frame", "pad"], name
        assert p["r_new"].default is None and p["select"].default is None and p["t_start"].default is None and p["hold"].default is True, name
        assert p["r2"].default == 0 and p["sequential"].default is False and p["res"].default is None and p["want_reach"].default is False, name
