"""The assignment at the drop-in boundary: the six C functions are declared in include/sea_current_hip.h and exported by the
built library, the binding's signatures match them in count and kind, the combined call takes the matrix call's arguments
followed by the matching's, the constants hold, nothing older moved, and the Python methods exist with their defaults.  No GPU."""
import ctypes
import inspect
import re

import pytest

import sea_current_amd as sc

BASE = ("sc_field_cost_matrix", "sc_assign_batch", "sc_fleet_assign_batch")
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


def test_constants():
    src = _header()
    assert re.search(r"#define\s+SC_ASSIGN_MAX_DIM\s+1024\b", src) and sc.ASSIGN_MAX_DIM == 1024
    assert re.search(r"#define\s+SC_ASSIGN_BIG\s+\(1ll << 42\)", src) and sc.ASSIGN_BIG == 1 << 42
    assert re.search(r"#define\s+SC_ASSIGN_OK\s+0\b", src) and re.search(r"#define\s+SC_ASSIGN_BAD\s+1\b", src)
    assert (sc.ASSIGN_OK, sc.ASSIGN_BAD) == (0, 1)
    assert sc.ASSIGN_BIG > sc.ASSIGN_MAX_DIM * 2**31 and sc.ASSIGN_MAX_DIM * sc.ASSIGN_BIG <= 2**52


def test_additive(built):
    src = _header()
    assert re.search(r"SC_K_COUNT = 15\b", src) and re.search(r"SC_K_ASTAR = 3\b", src) and re.search(r"SC_K_SMOOTH = 14\b", src)
    assert re.search(r"#define\s+SC_ABI_VERSION\s+1\b", src)
    assert re.search(r"#define\s+SC_FIELD_INF\s+INT32_MAX\b", src) and re.search(r"#define\s+SC_FIELD_SEED_COST_MAX\s+\(1 << 24\)", src)
    built.sc_abi_version.restype = ctypes.c_int
    assert built.sc_abi_version() == 1
    full = open(sc.HEADER_PATH).read()
    assert "sc_field_cost_matrix, sc_assign_batch, sc_fleet_assign_batch" in full[full.index("SC_K_ASTAR = 3"):full.index("SC_K_TOPPRA = 4")]


def test_parameter_counts_and_order():
    for suffix in ("", "_host"):
        mx, asg, fl = (_params(n + suffix) for n in BASE)
        assert mx == ["sc_ctx* ctx", "const int32_t* g", "int F", "int W", "int H", "const int32_t* cell", "int R", "const int32_t* col_cost",
                      "int32_t* cost"]
        assert asg == ["sc_ctx* ctx", "const int32_t* cost", "int B", "int R", "int C", "int32_t* col_of", "int32_t* row_of", "int64_t* u",
                       "int64_t* v", "int64_t* info"]
        assert len(fl) == 14
        assert fl[:9] == mx                                        # the combined call: the matrix call's arguments ...
        assert fl[9:] == asg[5:]                                   # ... then what the matching takes after cost, B, R, C
        for n, params in zip(BASE, (mx, asg, fl)):
            assert len(sc._SIGNATURES[n + suffix][1]) == len(params), n + suffix
            for ctype, decl in zip(sc._SIGNATURES[n + suffix][1], params):
                want = ctypes.c_int if decl.startswith("int ") else ctypes.c_void_p
                assert ctype is want, (n + suffix, decl)
            assert sc._SIGNATURES[n + suffix][0] is ctypes.c_int


def test_binding_has_the_methods_and_defaults():
    for name in ("field_cost_matrix", "field_cost_matrix_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p) == ["self", "g", "cells", "col_cost", "out"] and p["col_cost"].default is None and p["out"].default is None, name
    for name in ("assign", "assign_host"):
        assert list(inspect.signature(getattr(sc.Context, name)).parameters) == ["self", "cost"], name
    for name in ("fleet_assign", "fleet_assign_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p) == ["self", "g", "cells", "col_cost", "want_cost"] and p["col_cost"].default is None and p["want_cost"].default is False, name
