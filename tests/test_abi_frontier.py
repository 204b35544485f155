"""The frontier entry points at the drop-in boundary: the ten C functions are declared in include/sea_current_hip.h and exported
by the built library, their ctypes signatures match the declarations, the Python binding has the new methods, and without a
device the calls fail with a status.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

STEMS = ("sc_known_from_discs", "sc_d2_known_i32", "sc_frontier_batch", "sc_frontier_cost_matrix", "sc_fleet_explore_batch")
NEW = tuple(s + h for s in STEMS for h in ("", "_host"))


@pytest.fixture(scope="module")
def built():
    sc.build()
    return ctypes.CDLL(sc.LIB_PATH)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(sc.HEADER_PATH).read(), flags=re.S)


def _params(name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S)
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype(param):
    if "*" in param:
        return ctypes.c_void_p
    return ctypes.c_int32 if param.startswith("int32_t") else ctypes.c_int


def test_declared_and_exported(built):
    src = _header()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), f"{n} not declared"
        assert hasattr(built, n), f"{n} not exported"
        assert n in sc.EXPORTS
        res, args = sc._SIGNATURES[n]
        assert res is ctypes.c_int and args == [_ctype(p) for p in _params(n)], n
    built.sc_abi_version.restype = ctypes.c_int
    assert built.sc_abi_version() == 1                                # additive: the ABI version stays
    assert re.search(r"SC_K_COUNT\s*=\s*15\b", src)                   # and so does sc_kernel_id
    assert re.search(r"#define\s+SC_FRONTIER_MAX_CLUSTERS\s+65536\b", src)


def test_parameter_lists():
    for h in ("", "_host"):
        assert _params("sc_known_from_discs" + h) == ["sc_ctx* ctx", "const uint8_t* base", "const int32_t* discs", "int R", "int W", "int H",
                                                      "uint8_t* known"]
        assert _params("sc_d2_known_i32" + h) == ["sc_ctx* ctx", "const int32_t* d2", "const uint8_t* known", "int G", "int W", "int H",
                                                  "int32_t* d2k"]
        fr = _params("sc_frontier_batch" + h)
        assert fr == ["sc_ctx* ctx", "const int32_t* d2", "const uint8_t* known", "int G", "int W", "int H", "int32_t r2_clear", "int min_size",
                      "int Cmax", "int32_t* label", "int32_t* slot", "int32_t* ncl", "int32_t* rep", "int32_t* csize", "int32_t* cbox",
                      "int64_t* csum"]
        assert _params("sc_frontier_cost_matrix" + h) == ["sc_ctx* ctx", "const int32_t* g", "int F", "const int32_t* fgrid",
                                                          "const int32_t* slot", "const int32_t* csize", "int G", "int W", "int H", "int Cmax",
                                                          "int32_t gain", "int32_t size_cap", "int32_t* cost", "int32_t* cell"]
        # the combined call: one grid, then the fields and the weights, frontier's outputs, the matrix's, the matching's, the goals
        ex = _params("sc_fleet_explore_batch" + h)
        assert ex == fr[:3] + fr[4:9] + ["const int32_t* g", "int F", "int32_t gain", "int32_t size_cap"] + fr[9:] + \
            ["int32_t* cost", "int32_t* cell", "int32_t* col_of", "int32_t* row_of", "int64_t* info", "int32_t* goal", "int32_t* gcost"]


def test_binding_has_the_methods():
    p = inspect.signature(sc.Context.known_from_discs).parameters
    assert list(p)[1:] == ["discs", "W", "H", "base", "out"] and p["base"].default is None
    assert list(inspect.signature(sc.Context.d2_known).parameters)[1:] == ["d2", "known", "out"]
    p = inspect.signature(sc.Context.frontiers).parameters
    assert list(p)[1:6] == ["d2", "known", "r2", "min_size", "Cmax"] and (p["r2"].default, p["min_size"].default, p["Cmax"].default) == (0, 1, 128)
    p = inspect.signature(sc.Context.frontier_cost_matrix).parameters
    assert list(p)[1:] == ["g", "fr", "gain", "size_cap", "fgrid"] and p["gain"].default == 0
    p = inspect.signature(sc.Context.fleet_explore).parameters
    assert list(p)[1:] == ["d2", "known", "g", "r2", "min_size", "Cmax", "gain", "size_cap", "want_all"]
    for name in ("known_from_discs", "d2_known", "frontiers", "frontier_cost_matrix", "fleet_explore"):
        assert callable(getattr(sc.Context, name + "_host")), name


def test_calls_fail_with_a_status_without_a_context(built):
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES[n]
    p = sc._ptr
    d2, known = np.ones((8, 8), np.int32), np.ones((8, 8), np.uint8)
    i32 = lambda *s: np.zeros(s, np.int32)
    label, slot, ncl, rep, csize, g, cost, cell, one = i32(8, 8), i32(8, 8), i32(2), i32(4), i32(4), i32(1, 8, 8), i32(4), i32(4), i32(1)
    info = np.zeros(4, np.int64)
    for h in ("", "_host"):
        f = lambda stem: getattr(built, stem + h)
        assert f("sc_known_from_discs")(None, None, p(i32(3)), 1, 8, 8, p(known)) == 1
        assert f("sc_d2_known_i32")(None, p(d2), p(known), 1, 8, 8, p(label)) == 1
        assert f("sc_frontier_batch")(None, p(d2), p(known), 1, 8, 8, 0, 1, 4, p(label), p(slot), p(ncl), p(rep), p(csize), None, None) == 1
        assert f("sc_frontier_cost_matrix")(None, p(g), 1, None, p(slot), p(csize), 1, 8, 8, 4, 0, 0, p(cost), p(cell)) == 1
        assert f("sc_fleet_explore_batch")(None, p(d2), p(known), 8, 8, 0, 1, 4, p(g), 1, 0, 0, None, None, None, None, None, None, None, None,
                                           None, None, None, p(info), p(one), p(one)) == 1
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        built.sc_ctx_create.restype = ctypes.c_int
        assert built.sc_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
