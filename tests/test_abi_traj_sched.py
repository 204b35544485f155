"""The delay schedules at the drop-in boundary: the eight C functions are declared in include/sea_current_hip.h and exported by
the built library, the binding's signatures match them in count and kind, the combined call takes the knots call's arguments
followed by the three calls', nothing older moved, and the Python methods exist with their defaults.  No GPU."""
import ctypes
import inspect
import re

import pytest

import sea_current_amd as sc

BASE = ("sc_traj_shift_table_batch", "sc_traj_schedule_batch", "sc_traj_shift_knots_batch", "sc_fleet_schedule_batch")
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
    for name, val in (("SC_SLOT_UNRESOLVED", -1), ("SC_SLOT_NOT_OK", -2), ("SC_SLOT_UNNAMED", -3)):
        assert re.search(r"#define\s+%s\s+\(%d\)" % (name, val), src), name
    assert (sc.SLOT_UNRESOLVED, sc.SLOT_NOT_OK, sc.SLOT_UNNAMED) == (-1, -2, -3)


def test_additive(built):
    src = _header()
    assert re.search(r"SC_K_COUNT = 15\b", src) and re.search(r"SC_K_SMOOTH = 14\b", src)
    assert re.search(r"#define\s+SC_ABI_VERSION\s+1\b", src)
    assert re.search(r"SC_TRAJ_OK = 0,\s*SC_TRAJ_SKIPPED = 1,\s*SC_TRAJ_BAD = 2\s*}\s*sc_traj_status;", src)
    built.sc_abi_version.restype = ctypes.c_int
    assert built.sc_abi_version() == 1


def test_parameter_counts_and_order():
    for suffix in ("", "_host"):
        kn = _params("sc_traj_knots_batch" + suffix)
        tb, sd, sh, fl = (_params(n + suffix) for n in BASE)
        assert len(tb) == 10 and len(sd) == 9 and len(sh) == 7 and len(fl) == 24
        assert tb == ["sc_ctx* ctx", "const double* knots", "int32_t* tstatus", "int P", "int K", "const double* radius", "const int32_t* group",
                      "int D", "int stride", "uint64_t* table"]
        assert sd == ["sc_ctx* ctx", "const uint64_t* table", "const int32_t* tstatus", "int P", "int D", "const int32_t* order",
                      "const int32_t* jmax", "int32_t* slot", "int32_t* counts"]
        assert sh == ["sc_ctx* ctx", "const double* knots", "int P", "int K", "const int32_t* slot", "int stride", "double* knots_out"]
        assert fl[:14] == kn                                       # the combined call: the knots call's arguments ...
        assert fl[14:19] == tb[5:]                                 # ... then what the table call takes after knots, tstatus, P, K ...
        assert fl[19:23] == sd[5:]                                 # ... what the schedule call takes after table, tstatus, P, D ...
        assert fl[23:] == sh[6:]                                   # ... and the shifted knots
        for n, params in zip(BASE, (tb, sd, sh, fl)):
            assert len(sc._SIGNATURES[n + suffix][1]) == len(params), n + suffix
            for ctype, decl in zip(sc._SIGNATURES[n + suffix][1], params):
                want = ctypes.c_double if decl.startswith("double ") else ctypes.c_int if decl.startswith("int ") else ctypes.c_void_p
                assert ctype is want, (n + suffix, decl)


def test_binding_has_the_methods_and_keywords():
    for name in ("fleet_schedule", "fleet_schedule_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[:3] == ["self", "sm", "radius"], name
        assert p["t0"].default is None and p["flags"].default is None and p["group"].default is None, name
        assert p["T0"].default == 0.0 and p["dt_c"].default == 0.1 and p["K"].default is None, name
        assert p["D"].default == 8 and p["stride"].default == 1 and p["order"].default is None and p["jmax"].default is None, name
        assert p["want_table"].default is False and p["want_knots"].default is False, name
    for name in ("traj_shift_table", "traj_shift_table_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[:4] == ["self", "knots", "tstatus", "radius"] and p["group"].default is None, name
        assert p["D"].default == 8 and p["stride"].default == 1, name
    for name in ("traj_schedule", "traj_schedule_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[:3] == ["self", "table", "tstatus"] and p["D"].default == 8 and p["order"].default is None and p["jmax"].default is None, name
    for name in ("traj_shift_knots", "traj_shift_knots_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[:3] == ["self", "knots", "slot"] and p["stride"].default == 1, name
