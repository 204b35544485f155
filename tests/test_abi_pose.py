"""The pose entry points at the drop-in boundary: the six C functions are declared in include/sea_current_hip.h and exported by
the built library, their ctypes signatures match the declarations, the parameter lists match by name, the Python binding has
the methods with their defaults and the constants, sizes are refused in Python before the call, without a context the calls
return a status, and the ABI version and SC_K_COUNT are unchanged.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

STEMS = ("sc_footprint_mask_u8", "sc_pose_field_batch", "sc_pose_paths_batch")
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
    assert re.search(r"#define\s+SC_POSE_HEADINGS\s+8\b", src) and sc.POSE_HEADINGS == 8
    assert re.search(r"#define\s+SC_FOOTPRINT_MAX\s+32\b", src) and sc.FOOTPRINT_MAX == 32
    assert sc.POSE_HX == (1, 1, 0, -1, -1, -1, 0, 1) and sc.POSE_HY == (0, 1, 1, 1, 0, -1, -1, -1)
    # heading k is A*'s move {0,4,2,5,1,7,3,6}[k] (dx = {1,-1,0,0,1,-1,1,-1}, dy = {0,0,1,-1,1,1,-1,-1})
    dx, dy = (1, -1, 0, 0, 1, -1, 1, -1), (0, 0, 1, -1, 1, 1, -1, -1)
    assert all((dx[d], dy[d]) == (sc.POSE_HX[k], sc.POSE_HY[k]) for k, d in enumerate((0, 4, 2, 5, 1, 7, 3, 6)))


def test_parameter_lists():
    for h in ("", "_host"):
        assert _params("sc_footprint_mask_u8" + h) == ["sc_ctx* ctx", "const int32_t* d2", "int W", "int H", "int batch", "int32_t r2_clear",
                                                       "int front", "int back", "int left", "int right", "uint8_t* hmask"]
        assert _params("sc_pose_field_batch" + h) == ["sc_ctx* ctx", "const int32_t* d2", "const uint8_t* hmask", "int G", "const int32_t* fgrid",
                                                      "int W", "int H", "int32_t r2_clear", "int turn_cost", "int rev_cost", "int toward",
                                                      "const int32_t* root", "const int32_t* rhead", "int F", "int rounds", "int32_t* gp",
                                                      "int32_t* fstatus"]
        assert _params("sc_pose_paths_batch" + h) == ["sc_ctx* ctx", "const int32_t* d2", "const uint8_t* hmask", "int G", "const int32_t* fgrid",
                                                      "int W", "int H", "int32_t r2_clear", "int turn_cost", "int rev_cost", "int toward",
                                                      "const int32_t* gp", "const int32_t* root", "const int32_t* rhead", "int F",
                                                      "const int32_t* qfield", "const int32_t* target", "const int32_t* thead", "int Q",
                                                      "int Lmax", "int to_root", "int cells_only", "int32_t* path", "uint8_t* head",
                                                      "int32_t* len", "int32_t* cost", "int32_t* status"]
    # the plain fields keep their lists
    assert _params("sc_cost_field_batch") == ["sc_ctx* ctx", "const int32_t* d2", "int G", "const int32_t* fgrid", "int W", "int H",
                                              "int32_t r2_clear", "const int32_t* root", "int F", "int rounds", "int32_t* g", "int32_t* fstatus"]


def test_binding_has_the_methods():
    C = sc.Context
    p = inspect.signature(C.footprint_mask).parameters
    assert list(p)[1:] == ["d2", "front", "back", "left", "right", "r2", "out"] and p["r2"].default == 0 and p["out"].default is None
    assert list(inspect.signature(C.footprint_mask_host).parameters)[1:] == ["d2", "front", "back", "left", "right", "r2"]
    p = inspect.signature(C.pose_fields).parameters
    assert list(p)[1:] == ["d2", "roots", "rhead", "turn_cost", "rev_cost", "toward", "r2", "hmask", "fgrid", "rounds", "out"]
    assert (p["rev_cost"].default, p["toward"].default, p["r2"].default, p["hmask"].default, p["fgrid"].default, p["rounds"].default,
            p["out"].default) == (-1, False, 0, None, None, -1, None)
    p = inspect.signature(C.pose_fields_host).parameters
    assert list(p)[1:] == ["d2", "roots", "rhead", "turn_cost", "rev_cost", "toward", "r2", "hmask", "fgrid", "rounds"]
    p = inspect.signature(C.pose_paths).parameters
    assert list(p)[1:] == ["d2", "gp", "roots", "rhead", "qfield", "targets", "thead", "turn_cost", "rev_cost", "toward", "r2", "hmask", "Lmax",
                           "to_root", "cells_only", "fgrid", "out"]
    assert (p["rev_cost"].default, p["toward"].default, p["r2"].default, p["hmask"].default, p["Lmax"].default, p["to_root"].default,
            p["cells_only"].default, p["fgrid"].default, p["out"].default) == (-1, False, 0, None, 4096, False, False, None, None)
    p = inspect.signature(C.pose_paths_host).parameters
    assert list(p)[1:] == ["d2", "gp", "roots", "rhead", "qfield", "targets", "thead", "turn_cost", "rev_cost", "toward", "r2", "hmask", "Lmax",
                           "to_root", "cells_only", "fgrid"]


def test_binding_checks_sizes_before_the_call():
    """A wrong size raises in Python: the library is never reached (the stand-in context has none)."""
    ctx = object.__new__(sc.Context)
    ctx._l, ctx._h = None, None
    d2 = np.ones((8, 8), np.int32)
    gp = np.zeros((1, 8, 8, 8), np.int32)
    one = np.zeros(1, np.int32)
    E = sc.SeaCurrentError
    with pytest.raises(E):
        ctx._footprint_mask(sc._HOST, d2, 1, 1, 1, 1, 0, out=np.zeros((8, 7), np.uint8))
    with pytest.raises(E):
        ctx.pose_fields_host(d2, one, np.zeros(2, np.int32), 1)                       # rhead
    with pytest.raises(E):
        ctx.pose_fields_host(d2, one, one, 1, hmask=np.zeros((8, 7), np.uint8))
    with pytest.raises(E):
        ctx.pose_fields_host(d2, one, one, 1, fgrid=np.zeros(2, np.int32))
    with pytest.raises(E):
        ctx._pose_fields(sc._HOST, d2, one, one, 1, -1, False, 0, None, None, -1, out=dict(gp=gp[:, :7], status=one))
    with pytest.raises(E):
        ctx.pose_paths_host(d2, gp[:, :7], one, one, one, one, one, 1)                # gp
    with pytest.raises(E):
        ctx.pose_paths_host(d2, gp, one, one, one, one, np.zeros(2, np.int32), 1)     # thead
    with pytest.raises(E):
        ctx.pose_paths_host(d2, gp, one, one, np.zeros(2, np.int32), one, one, 1)     # qfield
    with pytest.raises(E):
        ctx.pose_paths_host(d2, gp, one, np.zeros(2, np.int32), one, one, one, 1)     # rhead
    with pytest.raises(E):
        ctx.pose_paths_host(d2, gp, one, one, one, one, one, 1, hmask=np.zeros(3, np.uint8))


def test_calls_fail_with_a_status_without_a_context(built):
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES[n]
    p = sc._ptr
    d2, hm, gp = np.ones((8, 8), np.int32), np.zeros((8, 8), np.uint8), np.zeros((1, 8, 8, 8), np.int32)
    one, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
    path, head = np.zeros((1, 16), np.int32), np.zeros((1, 16), np.uint8)
    for h in ("", "_host"):
        f = lambda stem: getattr(built, stem + h)
        assert f("sc_footprint_mask_u8")(None, p(d2), 8, 8, 1, 0, 1, 1, 1, 1, p(hm)) == 1
        assert f("sc_pose_field_batch")(None, p(d2), None, 1, None, 8, 8, 0, 1, -1, 0, p(one), p(one), 1, -1, p(gp), p(st)) == 1
        assert f("sc_pose_paths_batch")(None, p(d2), None, 1, None, 8, 8, 0, 1, -1, 0, p(gp), p(one), p(one), 1, p(one), p(one), p(one), 1, 16, 0, 0,
                                        p(path), p(head), p(st), p(st), p(st)) == 1
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        built.sc_ctx_create.restype = ctypes.c_int
        assert built.sc_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
