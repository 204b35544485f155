"""The field repair at the drop-in boundary: the four C functions are declared in include/sea_current_hip_update.h, exported
by the built library and bound in sc.EXPORTS_UPDATE with matching signatures; their parameter lists extend the build
entries' by name; the binding's methods and defaults exist and refuse wrong sizes before any call; EXPORTS, the ABI version
and SC_K_COUNT are what they were.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

NEW = ("sc_cost_field_update_batch", "sc_cost_field_update_batch_host", "sc_cost_field_weighted_update_batch",
       "sc_cost_field_weighted_update_batch_host")


@pytest.fixture(scope="module")
def built():
    sc.build()
    return ctypes.CDLL(sc.LIB_PATH)


def _strip(path):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))


def _params(name, path):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _strip(path), flags=re.S)
    assert m, f"{name} not declared in {path}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_declared_exported_and_bound(built):
    src = _strip(sc.HEADER_UPDATE_PATH)
    assert sorted(set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", src))) == sorted(NEW)
    assert sorted(sc.EXPORTS_UPDATE) == sorted(NEW)
    scalar = {"int": ctypes.c_int, "int32_t": ctypes.c_int32}
    for n in NEW:
        assert hasattr(built, n), f"{n} not exported"
        res, args = sc._SIGNATURES_UPDATE[n]
        params = _params(n, sc.HEADER_UPDATE_PATH)
        assert res is ctypes.c_int and len(args) == len(params), n
        for p, got in zip(params, args):
            assert got is (ctypes.c_void_p if "*" in p else scalar[p.split()[0]]), (n, p)
    assert '#include "sea_current_hip.h"' in open(sc.HEADER_UPDATE_PATH).read()
    hpp = open(sc.NATIVE_DIR + "/sea_current.hpp").read()
    assert "sea_current_hip_update.h" in hpp


def test_the_main_header_and_its_table_are_unchanged(built):
    main = _strip(sc.HEADER_PATH)
    for n in NEW:
        assert n not in main and n not in sc.EXPORTS
    assert not set(sc.EXPORTS) & set(sc.EXPORTS_UPDATE)
    assert sorted(sc.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", main)))
    built.sc_abi_version.restype = ctypes.c_int
    assert built.sc_abi_version() == 1
    assert re.search(r"SC_K_COUNT\s*=\s*15\b", main) and re.search(r"#define\s+SC_ABI_VERSION\s+1\b", main)


def test_parameter_lists_by_name():
    """d2 becomes d2_old, d2_new (weighted: d2_old, pen_old, d2_new, pen_new, pen_cap), g is in and out, stats comes last; the
    rest is the build entry's list in its order."""
    for suffix in ("", "_host"):
        o = _params("sc_cost_field_batch" + suffix, sc.HEADER_PATH)
        n = _params("sc_cost_field_update_batch" + suffix, sc.HEADER_UPDATE_PATH)
        assert n == [o[0], "const int32_t* d2_old", "const int32_t* d2_new"] + o[2:] + ["int32_t* stats"], suffix
        o = _params("sc_cost_field_weighted_batch" + suffix, sc.HEADER_PATH)
        n = _params("sc_cost_field_weighted_update_batch" + suffix, sc.HEADER_UPDATE_PATH)
        assert n == [o[0], "const int32_t* d2_old", "const uint8_t* pen_old", "const int32_t* d2_new", "const uint8_t* pen_new",
                     "int pen_cap"] + o[4:] + ["int32_t* stats"], suffix


def test_binding_methods_and_defaults():
    for name in ("cost_fields_update", "cost_fields_update_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[1:] == ["d2_old", "d2_new", "g", "roots", "r2", "fgrid", "rounds", "pen_old", "pen_new", "pen_cap", "stats"], name
        assert (p["r2"].default, p["fgrid"].default, p["rounds"].default, p["pen_old"].default, p["pen_new"].default,
                p["pen_cap"].default, p["stats"].default) == (0, None, -1, None, None, 255, True), name
    # one body for the pair
    assert "_cost_fields_update(" in inspect.getsource(sc.Context.cost_fields_update)
    assert "_cost_fields_update(_HOST" in inspect.getsource(sc.Context.cost_fields_update_host)


class _NoCall:
    """Stands in for a context: the body must refuse the sizes before it reaches the library."""

    def _call(self, *a):
        raise AssertionError("the library was called")


def test_sizes_are_refused_in_python():
    body = sc.Context._cost_fields_update
    d2 = np.ones((8, 8), np.int32)
    g = np.zeros((2, 8, 8), np.int32)
    roots = np.zeros(2, np.int32)
    pen = np.zeros((8, 8), np.uint8)
    args = dict(r2=0, fgrid=None, rounds=-1, pen_old=None, pen_new=None, pen_cap=255, stats=True)

    def refused(**kw):
        a = dict(args, d2_old=d2, d2_new=d2, g=g, roots=roots)
        a.update(kw)
        with pytest.raises(sc.SeaCurrentError):
            body(_NoCall(), sc._HOST, a["d2_old"], a["d2_new"], a["g"], a["roots"], a["r2"], a["fgrid"], a["rounds"], a["pen_old"],
                 a["pen_new"], a["pen_cap"], a["stats"])

    refused(d2_old=np.ones((8, 7), np.int32))
    refused(g=np.zeros((1, 8, 8), np.int32))
    refused(g=np.zeros((2, 8, 9), np.int32))
    refused(pen_old=pen)                                          # one costmap without the other
    refused(pen_old=pen, pen_new=np.zeros((4, 8), np.uint8))
    refused(pen_old=np.zeros((8, 4), np.uint8), pen_new=pen)
    refused(fgrid=np.zeros(3, np.int32))
    with pytest.raises(AssertionError, match="the library was called"):          # right sizes reach the call
        body(_NoCall(), sc._HOST, d2, d2, g, roots, 0, None, -1, pen, pen, 255, True)


def test_host_forms_fail_with_a_status_without_a_context(built):
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES_UPDATE[n]
    d2 = np.ones((8, 8), np.int32)
    pen = np.zeros((8, 8), np.uint8)
    root = np.zeros(1, np.int32)
    g = np.zeros((1, 8, 8), np.int32)
    st = np.zeros(2, np.int32)
    p = sc._ptr
    assert built.sc_cost_field_update_batch_host(None, p(d2), p(d2), 1, None, 8, 8, 0, p(root), 1, -1, p(g), p(st), p(st)) == 1
    assert built.sc_cost_field_update_batch(None, p(d2), p(d2), 1, None, 8, 8, 0, p(root), 1, -1, p(g), p(st), p(st)) == 1
    assert built.sc_cost_field_weighted_update_batch_host(None, p(d2), p(pen), p(d2), p(pen), 255, 1, None, 8, 8, 0, p(root), 1, -1, p(g),
                                                          p(st), p(st)) == 1
    assert built.sc_cost_field_weighted_update_batch(None, p(d2), p(pen), p(d2), p(pen), 255, 1, None, 8, 8, 0, p(root), 1, -1, p(g),
                                                     p(st), p(st)) == 1
