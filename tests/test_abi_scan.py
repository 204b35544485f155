"""The range-scan entry points at the drop-in boundary: the four C functions are declared in include/sea_current_hip.h and
exported by the built library, their ctypes signatures match the declarations, the three constants are defined, the Python
binding has the new methods with their defaults, and without a device the calls fail with a status.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

STEMS = ("sc_scan_cast_batch", "sc_logodds_update")
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


def test_constants():
    src = _header()
    for name, value, mine in (("SC_SCAN_NO_RETURN", r"\(-1\)", sc.SCAN_NO_RETURN), ("SC_SCAN_IGNORED", r"\(-2\)", sc.SCAN_IGNORED),
                              ("SC_SCAN_MAX_REACH", "16384", sc.SCAN_MAX_REACH)):
        m = re.search(r"#define\s+%s\s+(%s)\s" % (name, value), src)
        assert m, name
        assert int(m.group(1).strip("()")) == mine
    # the bound the walk's int32 products rest on
    D = m_ = sc.SCAN_MAX_REACH
    assert (2 * D + 1) * m_ + D < 2**30


def test_parameter_lists():
    for h in ("", "_host"):
        assert _params("sc_scan_cast_batch" + h) == ["sc_ctx* ctx", "const uint8_t* occ", "const int32_t* rays", "int N", "int W", "int H",
                                                     "int32_t* hit"]
        assert _params("sc_logodds_update" + h) == ["sc_ctx* ctx", "const int32_t* L", "const int32_t* rays", "const int32_t* hit", "int N",
                                                    "int W", "int H", "int32_t l_hit", "int32_t l_miss", "int32_t l_clamp", "int32_t t_occ",
                                                    "int32_t t_free", "int32_t* Lout", "uint8_t* occ_est", "uint8_t* known"]
    # the line-of-sight calls keep their lists
    assert _params("sc_known_from_views") == ["sc_ctx* ctx", "const uint8_t* base", "const uint8_t* occ", "const int32_t* views", "int R",
                                              "int W", "int H", "uint8_t* known", "uint8_t* occ_seen"]


def test_binding_has_the_methods():
    p = inspect.signature(sc.Context.scan_cast).parameters
    assert list(p)[1:] == ["rays", "occ", "out"] and p["out"].default is None
    assert list(inspect.signature(sc.Context.scan_cast_host).parameters)[1:] == ["rays", "occ"]
    names = ["rays", "hit", "W", "H", "L", "l_hit", "l_miss", "l_clamp", "t_occ", "t_free"]
    p = inspect.signature(sc.Context.logodds_update).parameters
    assert list(p)[1:] == names + ["out", "occ_est", "known"]
    q = inspect.signature(sc.Context.logodds_update_host).parameters
    assert list(q)[1:] == names + ["occ_est", "known"]
    for s in (p, q):
        assert s["L"].default is None and s["occ_est"].default is None and s["known"].default is None
        d = {k: s[k].default for k in names[5:]}
        # one look decides a cell, and the clamp is a few updates deep
        assert d["l_hit"] >= d["t_occ"] >= 1 and d["l_miss"] >= d["t_free"] >= 1
        assert 2 * max(d["l_hit"], d["l_miss"]) <= d["l_clamp"] <= 16 * min(d["l_hit"], d["l_miss"])


def test_calls_fail_with_a_status_without_a_context(built):
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES[n]
    p = sc._ptr
    occ, est, known = np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)
    rays, hit, L = np.array([[4, 4, 7, 7]], np.int32), np.zeros(1, np.int32), np.zeros((8, 8), np.int32)
    for h in ("", "_host"):
        f = lambda stem: getattr(built, stem + h)
        assert f("sc_scan_cast_batch")(None, p(occ), p(rays), 1, 8, 8, p(hit)) == 1
        assert f("sc_logodds_update")(None, p(L), p(rays), p(hit), 1, 8, 8, 2, 1, 8, 2, 1, p(L), p(est), p(known)) == 1
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        built.sc_ctx_create.restype = ctypes.c_int
        assert built.sc_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
