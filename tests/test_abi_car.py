"""Car-like pose planning at the drop-in boundary: the six C functions are declared in include/sea_current_hip_car.h, exported
by the built library and bound in sc.EXPORTS_CAR with matching signatures; their parameter lists follow the pose entries' by
name; the binding's methods, defaults and constant exist and refuse wrong sizes and ranges before any call; the entries fail
with a status without a context; EXPORTS, EXPORTS_UPDATE, the ABI version and SC_K_COUNT are what they were.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

NEW = ("sc_arc_mask_u16", "sc_arc_mask_u16_host", "sc_car_field_batch", "sc_car_field_batch_host", "sc_car_paths_batch",
       "sc_car_paths_batch_host")


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
    src = _strip(sc.HEADER_CAR_PATH)
    assert sorted(set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", src))) == sorted(NEW)
    assert sorted(sc.EXPORTS_CAR) == sorted(NEW)
    scalar = {"int": ctypes.c_int, "int32_t": ctypes.c_int32}
    for n in NEW:
        assert hasattr(built, n), f"{n} not exported"
        res, args = sc._SIGNATURES_CAR[n]
        params = _params(n, sc.HEADER_CAR_PATH)
        assert res is ctypes.c_int and len(args) == len(params), n
        for p, got in zip(params, args):
            assert got is (ctypes.c_void_p if "*" in p else scalar[p.split()[0]]), (n, p)
    text = open(sc.HEADER_CAR_PATH).read()
    assert '#include "sea_current_hip.h"' in text and re.search(r"#define\s+SC_ARC_MAX\s+4\b", text)
    hpp = open(sc.NATIVE_DIR + "/sea_current.hpp").read()
    assert "sea_current_hip_car.h" in hpp


def test_the_other_headers_and_their_tables_are_unchanged(built):
    main, update = _strip(sc.HEADER_PATH), _strip(sc.HEADER_UPDATE_PATH)
    for n in NEW:
        assert n not in main and n not in update and n not in sc.EXPORTS and n not in sc.EXPORTS_UPDATE
    assert not set(sc.EXPORTS_CAR) & (set(sc.EXPORTS) | set(sc.EXPORTS_UPDATE))
    assert sorted(sc.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", main)))
    assert sorted(sc.EXPORTS_UPDATE) == sorted(set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", update)))
    assert len(sc.EXPORTS) == 160 and len(sc.EXPORTS_UPDATE) == 4
    built.sc_abi_version.restype = ctypes.c_int
    assert built.sc_abi_version() == 1
    assert re.search(r"SC_K_COUNT\s*=\s*15\b", main) and re.search(r"#define\s+SC_ABI_VERSION\s+1\b", main)


def test_parameter_lists_by_name():
    """The field and the read-out take the pose entries' lists with amask after hmask and arc_n, arc_cost in the place of
    turn_cost; the read-out has no cells_only.  The mask takes d2, hmask, the grid, r2_clear, arc_n and its output."""
    for suffix in ("", "_host"):
        o = _params("sc_pose_field_batch" + suffix, sc.HEADER_PATH)
        n = _params("sc_car_field_batch" + suffix, sc.HEADER_CAR_PATH)
        i = o.index("int turn_cost")
        assert n == o[:3] + ["const uint16_t* amask"] + o[3:i] + ["int arc_n", "int arc_cost"] + o[i + 1:], suffix
        o = _params("sc_pose_paths_batch" + suffix, sc.HEADER_PATH)
        n = _params("sc_car_paths_batch" + suffix, sc.HEADER_CAR_PATH)
        i, j = o.index("int turn_cost"), o.index("int cells_only")
        assert n == o[:3] + ["const uint16_t* amask"] + o[3:i] + ["int arc_n", "int arc_cost"] + o[i + 1:j] + o[j + 1:], suffix
        assert _params("sc_arc_mask_u16" + suffix, sc.HEADER_CAR_PATH) == ["sc_ctx* ctx", "const int32_t* d2", "const uint8_t* hmask", "int W",
                                                                            "int H", "int batch", "int32_t r2_clear", "int arc_n",
                                                                            "uint16_t* amask"], suffix


def test_binding_methods_defaults_and_constant():
    assert sc.ARC_MAX == 4
    for name in ("arc_mask", "arc_mask_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[1:5] == ["d2", "arc_n", "r2", "hmask"] and (p["r2"].default, p["hmask"].default) == (0, None), name
    for name in ("car_fields", "car_fields_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[1:13] == ["d2", "amask", "roots", "rhead", "arc_n", "arc_cost", "rev_cost", "toward", "r2", "hmask", "fgrid", "rounds"], name
        assert (p["arc_cost"].default, p["rev_cost"].default, p["toward"].default, p["r2"].default, p["hmask"].default, p["fgrid"].default,
                p["rounds"].default) == (0, -1, False, 0, None, None, -1), name
    for name in ("car_paths", "car_paths_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[1:18] == ["d2", "amask", "gp", "roots", "rhead", "qfield", "targets", "thead", "arc_n", "arc_cost", "rev_cost", "toward",
                                 "r2", "hmask", "Lmax", "to_root", "fgrid"], name
        assert (p["arc_cost"].default, p["rev_cost"].default, p["toward"].default, p["Lmax"].default, p["to_root"].default) == \
            (0, -1, False, 4096, False), name
    # one body for each pair
    for stem in ("arc_mask", "car_fields", "car_paths"):
        assert f"_{stem}(_on(" in inspect.getsource(getattr(sc.Context, stem))
        assert f"_{stem}(_HOST" in inspect.getsource(getattr(sc.Context, stem + "_host"))


class _NoCall:
    """Stands in for a context: the body must refuse the sizes before it reaches the library."""

    def _call(self, *a):
        raise AssertionError("the library was called")


def test_sizes_and_ranges_are_refused_in_python():
    d2 = np.ones((8, 9), np.int32)
    am = np.zeros((8, 9), np.uint16)
    hm = np.zeros((8, 9), np.uint8)
    roots, rhead = np.zeros(2, np.int32), np.zeros(2, np.int32)
    gp = np.zeros((2, 8, 8, 9), np.int32)
    q = np.zeros(3, np.int32)
    E = sc.SeaCurrentError
    mask, field, paths = sc.Context._arc_mask, sc.Context._car_fields, sc.Context._car_paths
    nc = _NoCall()

    def fld(**kw):
        a = dict(d2=d2, amask=am, roots=roots, rhead=rhead, arc_n=1, arc_cost=0, rev_cost=-1, hmask=None, fgrid=None)
        a.update(kw)
        return field(nc, sc._HOST, a["d2"], a["amask"], a["roots"], a["rhead"], a["arc_n"], a["arc_cost"], a["rev_cost"], False, 0, a["hmask"],
                     a["fgrid"], -1)

    def pth(**kw):
        a = dict(d2=d2, amask=am, gp=gp, roots=roots, rhead=rhead, qfield=q, targets=q, thead=q, arc_n=1, arc_cost=0, rev_cost=-1, hmask=None,
                 Lmax=16, fgrid=None)
        a.update(kw)
        return paths(nc, sc._HOST, a["d2"], a["amask"], a["gp"], a["roots"], a["rhead"], a["qfield"], a["targets"], a["thead"], a["arc_n"],
                     a["arc_cost"], a["rev_cost"], False, 0, a["hmask"], a["Lmax"], False, a["fgrid"])

    for kw in (dict(arc_n=0), dict(arc_n=5), dict(arc_cost=-1), dict(arc_cost=256), dict(rev_cost=-2), dict(rev_cost=256), dict(amask=None),
               dict(amask=np.zeros((8, 8), np.uint16)), dict(rhead=np.zeros(3, np.int32)), dict(hmask=np.zeros((4, 9), np.uint8)),
               dict(fgrid=np.zeros(3, np.int32))):
        with pytest.raises(E):
            fld(**kw)
        with pytest.raises(E):
            pth(**kw)
    for kw in (dict(gp=np.zeros((1, 8, 8, 9), np.int32)), dict(qfield=np.zeros(2, np.int32)), dict(thead=np.zeros(4, np.int32)), dict(Lmax=0)):
        with pytest.raises(E):
            pth(**kw)
    for n in (0, 5):
        with pytest.raises(E):
            mask(nc, sc._HOST, d2, n, 0, None)
    with pytest.raises(E):
        mask(nc, sc._HOST, d2, 1, 0, np.zeros((8, 8), np.uint8))
    with pytest.raises(E):
        mask(nc, sc._HOST, d2, 1, 0, None, np.zeros((8, 8), np.uint16))
    for call in (lambda: fld(hmask=hm), lambda: pth(hmask=hm), lambda: mask(nc, sc._HOST, d2, 4, 0, hm)):      # right sizes reach the call
        with pytest.raises(AssertionError, match="the library was called"):
            call()


def test_entries_fail_with_a_status_without_a_context(built):
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES_CAR[n]
    d2 = np.ones((8, 8), np.int32)
    am = np.zeros((8, 8), np.uint16)
    root, rh, q = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    gp = np.zeros((1, 8, 8, 8), np.int32)
    path, head = np.zeros(16, np.int32), np.zeros(16, np.uint8)
    p = sc._ptr
    for suffix in ("", "_host"):
        assert getattr(built, "sc_arc_mask_u16" + suffix)(None, p(d2), None, 8, 8, 1, 0, 1, p(am)) == 1
        assert getattr(built, "sc_car_field_batch" + suffix)(None, p(d2), None, p(am), 1, None, 8, 8, 0, 1, 0, -1, 0, p(root), p(rh), 1, -1, p(gp),
                                                             p(q)) == 1
        assert getattr(built, "sc_car_paths_batch" + suffix)(None, p(d2), None, p(am), 1, None, 8, 8, 0, 1, 0, -1, 0, p(gp), p(root), p(rh), 1, p(q),
                                                             p(q), p(q), 1, 16, 0, p(path), p(head), p(q), p(q), p(q)) == 1
