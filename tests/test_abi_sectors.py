"""The field-of-view entry points at the drop-in boundary: the eight C functions are declared in include/sea_current_hip.h and
exported by the built library, their ctypes signatures match the declarations, the parameter lists match by name, the Python
binding has the new methods with their defaults and the constant, and without a device the calls fail with a status.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

STEMS = ("sc_known_from_sectors", "sc_sector_gain_batch", "sc_view_gain_headings_batch", "sc_views_from_cells")
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
    assert re.search(r"#define\s+SC_VIEW_MAX_BINS\s+64\b", src) and sc.VIEW_MAX_BINS == 64


def test_parameter_lists():
    for h in ("", "_host"):
        assert _params("sc_known_from_sectors" + h) == ["sc_ctx* ctx", "const uint8_t* base", "const uint8_t* occ", "const int32_t* sviews",
                                                        "int R", "int W", "int H", "uint8_t* known", "uint8_t* occ_seen"]
        assert _params("sc_sector_gain_batch" + h) == ["sc_ctx* ctx", "const uint8_t* occ", "const uint8_t* known", "const int32_t* sviews",
                                                       "int N", "int W", "int H", "int32_t* gain"]
        assert _params("sc_view_gain_headings_batch" + h) == ["sc_ctx* ctx", "const uint8_t* occ", "const uint8_t* known",
                                                              "const int32_t* views", "int N", "int W", "int H", "const int32_t* dirs", "int B",
                                                              "int span", "int32_t* hist", "int32_t* gainh", "int32_t* best"]
        assert _params("sc_views_from_cells" + h) == ["sc_ctx* ctx", "const int32_t* cell", "int N", "int W", "int H", "int32_t r2",
                                                      "int32_t* views"]
    # the full-circle calls keep their lists
    assert _params("sc_known_from_views") == ["sc_ctx* ctx", "const uint8_t* base", "const uint8_t* occ", "const int32_t* views", "int R",
                                              "int W", "int H", "uint8_t* known", "uint8_t* occ_seen"]
    assert _params("sc_view_gain_batch") == ["sc_ctx* ctx", "const uint8_t* occ", "const uint8_t* known", "const int32_t* views", "int N",
                                             "int W", "int H", "int32_t* gain"]


def test_binding_has_the_methods():
    C = sc.Context
    p = inspect.signature(C.known_from_sectors).parameters
    assert list(p)[1:] == ["sviews", "occ", "base", "out", "occ_seen"]
    assert p["base"].default is None and p["out"].default is None and p["occ_seen"].default is None
    p = inspect.signature(C.known_from_sectors_host).parameters
    assert list(p)[1:] == ["sviews", "occ", "base", "occ_seen"] and p["base"].default is None and p["occ_seen"].default is None
    p = inspect.signature(C.sector_gain).parameters
    assert list(p)[1:] == ["sviews", "occ", "known", "out"] and p["out"].default is None
    assert list(inspect.signature(C.sector_gain_host).parameters)[1:] == ["sviews", "occ", "known"]
    p = inspect.signature(C.view_gain_headings).parameters
    assert list(p)[1:] == ["views", "occ", "known", "dirs", "span", "hist", "gainh", "out"]
    assert p["hist"].default is None and p["gainh"].default is None and p["out"].default is None
    p = inspect.signature(C.view_gain_headings_host).parameters
    assert list(p)[1:] == ["views", "occ", "known", "dirs", "span", "hist", "gainh"] and p["hist"].default is None and p["gainh"].default is None
    p = inspect.signature(C.views_from_cells).parameters
    assert list(p)[1:] == ["cell", "W", "H", "r2", "out"] and p["out"].default is None
    assert list(inspect.signature(C.views_from_cells_host).parameters)[1:] == ["cell", "W", "H", "r2"]
    p = inspect.signature(sc.heading_dirs).parameters
    assert list(p) == ["B", "phase"] and p["phase"].default == 0.0
    assert list(inspect.signature(sc.sector_views).parameters) == ["views", "dirs", "h", "span"]


def test_binding_checks_sizes_before_the_call():
    """A wrong size raises in Python: the library is never reached (the stand-in context has none)."""
    ctx = object.__new__(sc.Context)
    ctx._l, ctx._h = None, None
    occ, known = np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)
    views, sviews = np.array([[4, 4, 9]], np.int32), np.array([[4, 4, 9, 1, 0, 0, 1]], np.int32)
    d = sc.heading_dirs(8)
    with pytest.raises(sc.SeaCurrentError):
        ctx.known_from_sectors_host(sviews, occ, base=np.zeros((8, 7), np.uint8))
    with pytest.raises(sc.SeaCurrentError):
        ctx.sector_gain_host(sviews, occ, known[:7])
    with pytest.raises(sc.SeaCurrentError):
        ctx.view_gain_headings_host(views, occ, known, d, 2, hist=np.zeros((1, 7), np.int32))
    with pytest.raises(sc.SeaCurrentError):
        ctx.view_gain_headings_host(views, occ, known[:7], d, 2)


def test_calls_fail_with_a_status_without_a_context(built):
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES[n]
    p = sc._ptr
    occ, known, seen = np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)
    sviews, views, gain = np.array([[4, 4, 9, 1, 0, 0, 1]], np.int32), np.array([[4, 4, 9]], np.int32), np.zeros(1, np.int32)
    dirs, hist, best, cell = sc.heading_dirs(8), np.zeros((1, 8), np.int32), np.zeros((1, 2), np.int32), np.array([5], np.int32)
    for h in ("", "_host"):
        f = lambda stem: getattr(built, stem + h)
        assert f("sc_known_from_sectors")(None, None, p(occ), p(sviews), 1, 8, 8, p(known), p(seen)) == 1
        assert f("sc_sector_gain_batch")(None, p(occ), p(known), p(sviews), 1, 8, 8, p(gain)) == 1
        assert f("sc_view_gain_headings_batch")(None, p(occ), p(known), p(views), 1, 8, 8, p(dirs), 8, 2, p(hist), None, p(best)) == 1
        assert f("sc_views_from_cells")(None, p(cell), 1, 8, 8, 9, p(views)) == 1
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        built.sc_ctx_create.restype = ctypes.c_int
        assert built.sc_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
