"""The goals-by-gain entry points at the drop-in boundary: the six C functions are declared in include/sea_current_hip.h and
exported by the built library, their ctypes signatures match the declarations, the parameter lists match by name, the Python
binding has the new methods with their defaults, and without a device the calls fail with a status.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

STEMS = ("sc_explore_gain_batch", "sc_frontier_centres", "sc_fleet_explore_gain_batch")
NEW = tuple(s + h for s in STEMS for h in ("", "_host"))
GAIN_IN = ["int32_t r2", "const int32_t* dirs", "int B", "int span", "int32_t wg", "int32_t wc", "int32_t min_gain", "int rounds"]
GAIN_OUT = ["int32_t* goal", "int32_t* gcost", "int32_t* ggain", "int32_t* head", "int32_t* cand_of", "int32_t* pick", "int32_t* npick",
            "int32_t* gain0", "int32_t* gain_end", "uint8_t* known_out"]


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
        assert _params("sc_explore_gain_batch" + h) == ["sc_ctx* ctx", "const uint8_t* occ", "const uint8_t* known", "const int32_t* g", "int R",
                                                        "const int32_t* cand", "int N", "int W", "int H"] + GAIN_IN + GAIN_OUT
        assert _params("sc_frontier_centres" + h) == ["sc_ctx* ctx", "const int32_t* slot", "const int32_t* csize", "const int64_t* csum", "int G",
                                                      "int W", "int H", "int Cmax", "int32_t* centre"]
        assert _params("sc_fleet_explore_gain_batch" + h) == [
            "sc_ctx* ctx", "const int32_t* d2", "const uint8_t* known", "int W", "int H", "int32_t r2_clear", "int min_size", "int Cmax",
            "const uint8_t* occ", "const int32_t* g", "int R"] + GAIN_IN + [
            "int32_t* label", "int32_t* slot", "int32_t* ncl", "int32_t* rep", "int32_t* csize", "int32_t* cbox", "int64_t* csum",
            "int32_t* centre"] + GAIN_OUT
    # the call it stands beside keeps its list
    assert _params("sc_fleet_explore_batch")[:8] == ["sc_ctx* ctx", "const int32_t* d2", "const uint8_t* known", "int W", "int H",
                                                     "int32_t r2_clear", "int min_size", "int Cmax"]


def test_binding_has_the_methods():
    C = sc.Context
    p = inspect.signature(C.explore_gain).parameters
    assert list(p)[1:] == ["occ", "known", "g", "cand", "r2", "dirs", "span", "wg", "wc", "min_gain", "rounds", "known_out", "want_all"]
    assert p["dirs"].default is None and p["wg"].default == 1 and p["wc"].default == 1 and p["min_gain"].default == 1
    assert p["rounds"].default is None and p["known_out"].default is None
    assert list(inspect.signature(C.explore_gain_host).parameters)[1:] == ["occ", "known", "g", "cand", "r2", "dirs", "span", "wg", "wc",
                                                                           "min_gain", "rounds", "want_all"]
    assert list(inspect.signature(C.frontier_centres).parameters)[1:] == ["fr", "W", "H", "out"]
    assert list(inspect.signature(C.frontier_centres_host).parameters)[1:] == ["fr", "W", "H"]
    p = inspect.signature(C.fleet_explore_gain).parameters
    assert list(p)[1:] == ["d2", "known", "occ", "g", "r2_sense", "r2", "min_size", "Cmax", "dirs", "span", "wg", "wc", "min_gain", "rounds",
                           "known_out", "want_all"]
    assert p["Cmax"].default == 128 and p["want_all"].default is False
    assert list(inspect.signature(C.fleet_explore_gain_host).parameters)[1:] == [k for k in list(p)[1:] if k != "known_out"]


def test_binding_checks_sizes_before_the_call():
    """A wrong size raises in Python: the library is never reached (the stand-in context has none)."""
    ctx = object.__new__(sc.Context)
    ctx._l, ctx._h = None, None
    occ, known, g = np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((2, 8, 8), np.int32)
    with pytest.raises(sc.SeaCurrentError):
        ctx.explore_gain_host(occ, known[:7], g, [5], 9)
    with pytest.raises(sc.SeaCurrentError):
        ctx.explore_gain_host(occ, known, g[:, :7], [5], 9)
    fr = dict(slot=np.zeros((8, 7), np.int32), csize=np.zeros((1, 4), np.int32), csum=np.zeros((1, 4, 2), np.int64))
    with pytest.raises(sc.SeaCurrentError):
        ctx.frontier_centres_host(fr, 8, 8)
    with pytest.raises(sc.SeaCurrentError):
        ctx.fleet_explore_gain_host(np.zeros((8, 8), np.int32), known, occ[:7], g, 9)


def test_calls_fail_with_a_status_without_a_context(built):
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES[n]
    p = sc._ptr
    occ, known, d2 = np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8), np.ones((8, 8), np.int32)
    g, cand = np.zeros((1, 8, 8), np.int32), np.array([5], np.int32)
    goal, gcost, npick = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    slot, csize, csum, centre = np.zeros((8, 8), np.int32), np.zeros(4, np.int32), np.zeros((4, 2), np.int64), np.zeros(4, np.int32)
    for h in ("", "_host"):
        f = lambda stem: getattr(built, stem + h)
        assert f("sc_explore_gain_batch")(None, p(occ), p(known), p(g), 1, p(cand), 1, 8, 8, 9, None, 0, 0, 1, 1, 1, 1, p(goal), p(gcost), None,
                                          None, None, None, p(npick), None, None, None) == 1
        assert f("sc_frontier_centres")(None, p(slot), p(csize), p(csum), 1, 8, 8, 4, p(centre)) == 1
        assert f("sc_fleet_explore_gain_batch")(None, p(d2), p(known), 8, 8, 0, 1, 4, p(occ), p(g), 1, 9, None, 0, 0, 1, 1, 1, 1, None, None, None,
                                                None, None, None, None, None, p(goal), p(gcost), None, None, None, None, p(npick), None, None,
                                                None) == 1
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        built.sc_ctx_create.restype = ctypes.c_int
        assert built.sc_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
