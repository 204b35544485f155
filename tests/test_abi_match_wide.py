"""The wide-window scan-matching entry points at the drop-in boundary: the two C functions are declared in
include/sea_current_hip.h and exported by the built library, their ctypes signatures match the declarations, the constants are
defined, the Python binding has the new methods with their defaults, and without a device the calls fail with a status.  The
ABI version and the kernel ids stay.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

NEW = ("sc_scan_match_wide_batch", "sc_scan_match_wide_batch_host")
PARAMS = ["sc_ctx* ctx", "const int32_t* d2", "const uint8_t* known", "const int32_t* pts", "const int32_t* centre", "int S", "int R", "int N",
          "int W", "int H", "int wx", "int wy", "int32_t d2_cap", "int32_t unk", "int top", "int max_nodes", "int32_t* best", "int32_t* stats"]


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
    for name, value, mine in (("SC_MATCH_OVERFLOW", r"\(-2\)", sc.SCAN_MATCH_OVERFLOW), ("SC_MATCH_WIDE_MAX_HALF", "2048", sc.SCAN_MATCH_WIDE_MAX_HALF),
                              ("SC_MATCH_WIDE_MAX_TOP", "5", sc.SCAN_MATCH_WIDE_MAX_TOP), ("SC_MATCH_WIDE_MIN_NODES", "64", 64),
                              ("SC_MATCH_WIDE_MAX_NODES", r"\(1 << 22\)", 1 << 22), ("SC_MATCH_WIDE_MAX_TOTAL", r"\(1 << 26\)", 1 << 26)):
        m = re.search(r"#define\s+%s\s+(%s)\s" % (name, value), src)
        assert m, name
        assert eval(m.group(1)) == mine
    # the bounds the kernels rest on: a node's coordinates (origin + half window, 0 .. 4096) take 13 bits, a displacement 24,
    # a bound 31; a parent's offset into a level's bounds (at most 16 children per node of a full list) 27
    assert 2 * sc.SCAN_MATCH_WIDE_MAX_HALF < 2**13 and 2 * sc.SCAN_MATCH_WIDE_MAX_HALF**2 < 2**24 and 32767 * sc.SCAN_MATCH_MAX_POINTS < 2**31
    assert 16 * (1 << 22) < 2**27 and 4**sc.SCAN_MATCH_WIDE_MAX_TOP * 4 <= 2 * sc.SCAN_MATCH_WIDE_MAX_HALF
    assert sc.SCAN_MATCH_OVERFLOW != sc.SCAN_MATCH_IGNORED and sc.SCAN_MATCH_OVERFLOW < 0


def test_parameter_lists():
    for n in NEW:
        assert _params(n) == PARAMS
    dense = _params("sc_scan_match_batch")                             # the dense call keeps its list; the wide one is it without
    assert PARAMS[:14] == dense[:14] and dense[14:] == ["int32_t* best", "int32_t* score"]   # score, plus top, max_nodes, stats


def test_binding_has_the_methods():
    names = ["pts", "centre", "d2", "known", "wx", "wy", "d2_cap", "unk", "top", "max_nodes"]
    p = inspect.signature(sc.Context.scan_match_wide).parameters
    q = inspect.signature(sc.Context.scan_match_wide_host).parameters
    assert list(p)[1:] == names + ["out", "stats"] and list(q)[1:] == names + ["stats"]
    for s in (p, q):
        assert s["known"].default is None and s["stats"].default is None
        assert {k: s[k].default for k in names[4:]} == dict(wx=256, wy=256, d2_cap=64, unk=1, top=3, max_nodes=1 << 16)
    assert p["out"].default is None


def test_calls_fail_with_a_status_without_a_context(built):
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES[n]
    p = sc._ptr
    d2, pts, centre, best = np.zeros((8, 8), np.int32), np.zeros((1, 1, 1, 2), np.int32), np.array([[4, 4]], np.int32), np.zeros((1, 6), np.int32)
    for n in NEW:
        assert getattr(built, n)(None, p(d2), None, p(pts), p(centre), 1, 1, 1, 8, 8, 1, 1, 64, 1, 1, 64, p(best), None) == 1
