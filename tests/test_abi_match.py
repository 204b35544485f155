"""The scan-matching entry points at the drop-in boundary: the two C functions are declared in include/sea_current_hip.h and
exported by the built library, their ctypes signatures match the declarations, the constants are defined, the Python binding
has the new methods with their defaults and the two host helpers, and without a device the calls fail with a status.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

NEW = ("sc_scan_match_batch", "sc_scan_match_batch_host")
PARAMS = ["sc_ctx* ctx", "const int32_t* d2", "const uint8_t* known", "const int32_t* pts", "const int32_t* centre", "int S", "int R", "int N",
          "int W", "int H", "int wx", "int wy", "int32_t d2_cap", "int32_t unk", "int32_t* best", "int32_t* score"]


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
    for name, value, mine in (("SC_MATCH_ABSENT", "INT32_MIN", sc.SCAN_MATCH_ABSENT), ("SC_MATCH_IGNORED", r"\(-1\)", sc.SCAN_MATCH_IGNORED),
                              ("SC_MATCH_MAX_HALF", "64", sc.SCAN_MATCH_MAX_HALF), ("SC_MATCH_MAX_POINTS", "65536", sc.SCAN_MATCH_MAX_POINTS),
                              ("SC_MATCH_MAX_ROT", "256", sc.SCAN_MATCH_MAX_ROT)):
        m = re.search(r"#define\s+%s\s+(%s)\s" % (name, value), src)
        assert m, name
        assert (-2**31 if m.group(1) == "INT32_MIN" else int(m.group(1).strip("()"))) == mine
    # the bounds the kernels rest on: a score is an int32, a key's fields hold a window's displacement and indices, and an
    # absent point is one by the reach test
    assert 32767 * sc.SCAN_MATCH_MAX_POINTS == 2147418112 < 2**31
    assert 2 * sc.SCAN_MATCH_MAX_HALF**2 < 2**16 and 2 * sc.SCAN_MATCH_MAX_HALF + 1 <= 256 and sc.SCAN_MATCH_MAX_ROT <= 256
    assert abs(sc.SCAN_MATCH_ABSENT) > sc.SCAN_MAX_REACH


def test_parameter_lists():
    for n in NEW:
        assert _params(n) == PARAMS
    # the range-scan calls keep their lists
    assert _params("sc_scan_cast_batch") == ["sc_ctx* ctx", "const uint8_t* occ", "const int32_t* rays", "int N", "int W", "int H", "int32_t* hit"]


def test_binding_has_the_methods():
    names = ["pts", "centre", "d2", "known", "wx", "wy", "d2_cap", "unk"]
    p = inspect.signature(sc.Context.scan_match).parameters
    q = inspect.signature(sc.Context.scan_match_host).parameters
    assert list(p)[1:] == names + ["out", "score"] and list(q)[1:] == names + ["score"]
    for s in (p, q):
        assert s["known"].default is None and s["score"].default is None
        assert {k: s[k].default for k in names[4:]} == dict(wx=8, wy=8, d2_cap=64, unk=1)
    assert p["out"].default is None
    assert list(inspect.signature(sc.points_from_hits).parameters) == ["rays", "hit", "W"]
    assert list(inspect.signature(sc.rotate_points).parameters) == ["pts", "angles"]


def test_calls_fail_with_a_status_without_a_context(built):
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES[n]
    p = sc._ptr
    d2, pts, centre, best = np.zeros((8, 8), np.int32), np.zeros((1, 1, 1, 2), np.int32), np.array([[4, 4]], np.int32), np.zeros((1, 6), np.int32)
    for n in NEW:
        assert getattr(built, n)(None, p(d2), None, p(pts), p(centre), 1, 1, 1, 8, 8, 1, 1, 64, 1, p(best), None) == 1
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        built.sc_ctx_create.restype = ctypes.c_int
        assert built.sc_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
