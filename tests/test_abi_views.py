"""The line-of-sight entry points at the drop-in boundary: the four C functions are declared in include/sea_current_hip.h and
exported by the built library, their ctypes signatures match the declarations, the Python binding has the new methods with
their defaults, and without a device the calls fail with a status.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

STEMS = ("sc_known_from_views", "sc_view_gain_batch")
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


def test_parameter_lists():
    for h in ("", "_host"):
        assert _params("sc_known_from_views" + h) == ["sc_ctx* ctx", "const uint8_t* base", "const uint8_t* occ", "const int32_t* views", "int R",
                                                      "int W", "int H", "uint8_t* known", "uint8_t* occ_seen"]
        assert _params("sc_view_gain_batch" + h) == ["sc_ctx* ctx", "const uint8_t* occ", "const uint8_t* known", "const int32_t* views", "int N",
                                                     "int W", "int H", "int32_t* gain"]
    # the disc call keeps its list
    assert _params("sc_known_from_discs") == ["sc_ctx* ctx", "const uint8_t* base", "const int32_t* discs", "int R", "int W", "int H",
                                              "uint8_t* known"]


def test_binding_has_the_methods():
    p = inspect.signature(sc.Context.known_from_views).parameters
    assert list(p)[1:] == ["views", "occ", "base", "out", "occ_seen"]
    assert p["base"].default is None and p["out"].default is None and p["occ_seen"].default is None
    p = inspect.signature(sc.Context.view_gain).parameters
    assert list(p)[1:] == ["views", "occ", "known", "out"] and p["out"].default is None
    p = inspect.signature(sc.Context.known_from_views_host).parameters
    assert list(p)[1:] == ["views", "occ", "base", "occ_seen"] and p["base"].default is None and p["occ_seen"].default is None
    assert list(inspect.signature(sc.Context.view_gain_host).parameters)[1:] == ["views", "occ", "known"]


def test_calls_fail_with_a_status_without_a_context(built):
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES[n]
    p = sc._ptr
    occ, known, seen = np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)
    views, gain = np.array([[4, 4, 9]], np.int32), np.zeros(1, np.int32)
    for h in ("", "_host"):
        f = lambda stem: getattr(built, stem + h)
        assert f("sc_known_from_views")(None, None, p(occ), p(views), 1, 8, 8, p(known), p(seen)) == 1
        assert f("sc_view_gain_batch")(None, p(occ), p(known), p(views), 1, 8, 8, p(gain)) == 1
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        built.sc_ctx_create.restype = ctypes.c_int
        assert built.sc_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
