"""The multi-source field entry points at the drop-in boundary: the four C functions are declared in
include/sea_current_hip.h with the parameter lists of the definition and exported by the built library, their ctypes
signatures match the declarations, the Python binding has the methods, a null context gives a status, and the ABI version
and SC_K_COUNT are unchanged.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

NEW = ("sc_cost_field_multi_batch", "sc_cost_field_multi_batch_host", "sc_field_paths_multi_batch", "sc_field_paths_multi_batch_host")


@pytest.fixture(scope="module")
def built():
    sc.build()
    return ctypes.CDLL(sc.LIB_PATH)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(sc.HEADER_PATH).read(), flags=re.S)


def _params(name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S)
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_declared_and_exported(built):
    src = _header()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), f"{n} not declared"
        assert hasattr(built, n), f"{n} not exported"
        assert n in sc.EXPORTS
        assert len(sc._SIGNATURES[n][1]) == len(_params(n)), n
    built.sc_abi_version.restype = ctypes.c_int
    assert built.sc_abi_version() == 1                                # additive: the ABI version stays
    assert re.search(r"SC_K_COUNT\s*=\s*15\b", src)                   # and so does sc_kernel_id
    assert re.search(r"#define\s+SC_FIELD_SEED_COST_MAX\s+\(1\s*<<\s*24\)", src) and sc.FIELD_SEED_COST_MAX == 1 << 24


def test_parameter_lists():
    for suffix in ("", "_host"):
        assert _params("sc_cost_field_multi_batch" + suffix) == [
            "sc_ctx* ctx", "const int32_t* d2", "const uint8_t* pen", "int pen_cap", "int G", "const int32_t* fgrid", "int W", "int H",
            "int32_t r2_clear", "const int32_t* seed", "const int32_t* seed_cost", "const int32_t* seed_off", "int n_seed", "int F",
            "int rounds", "int32_t* g", "int32_t* owner", "int32_t* fstatus"]
        assert _params("sc_field_paths_multi_batch" + suffix) == [
            "sc_ctx* ctx", "const int32_t* d2", "const uint8_t* pen", "int pen_cap", "int G", "const int32_t* fgrid", "int W", "int H",
            "int32_t r2_clear", "const int32_t* g", "const int32_t* owner", "const int32_t* seed", "int n_seed", "int F",
            "const int32_t* qfield", "const int32_t* target", "int Q", "int Lmax", "int to_seed", "int32_t* path", "int32_t* len",
            "int32_t* cost", "int32_t* status", "int32_t* which"]


def test_binding_signatures_match_the_declarations():
    ctype_of = {"int": ctypes.c_int, "int32_t": ctypes.c_int32}
    for n in NEW:
        res, args = sc._SIGNATURES[n]
        assert res is ctypes.c_int
        for decl, a in zip(_params(n), args):
            want = ctypes.c_void_p if "*" in decl else ctype_of[decl.split()[0]]
            assert a is want, (n, decl)


def test_binding_has_the_methods():
    p = inspect.signature(sc.Context.cost_fields_multi).parameters
    assert list(p)[1:] == ["d2", "seeds", "seed_off", "seed_cost", "r2", "fgrid", "rounds", "want_owner", "pen", "pen_cap", "out"]
    assert (p["seed_cost"].default is None and p["r2"].default == 0 and p["fgrid"].default is None and p["rounds"].default == -1 and
            p["want_owner"].default is True and p["pen"].default is None and p["pen_cap"].default == 255 and p["out"].default is None)
    p = inspect.signature(sc.Context.field_paths_multi).parameters
    assert list(p)[1:] == ["d2", "fields", "seeds", "qfield", "targets", "r2", "Lmax", "to_seed", "fgrid", "pen", "pen_cap", "out"]
    assert (p["r2"].default == 0 and p["Lmax"].default == 4096 and p["to_seed"].default is False and p["fgrid"].default is None and
            p["pen"].default is None and p["pen_cap"].default == 255 and p["out"].default is None)
    assert callable(sc.Context.cost_fields_multi_host) and callable(sc.Context.field_paths_multi_host)


def test_null_context_gives_a_status(built):
    """A null context, and (where there is no GPU) a failed sc_ctx_create: a status comes back, nothing crashes."""
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES[n]
    d2 = np.ones((8, 8), np.int32)
    g = np.zeros((1, 8, 8), np.int32)
    seed = np.zeros(1, np.int32)
    off = np.array([0, 1], np.int32)
    one = np.zeros(1, np.int32)
    path = np.zeros((1, 4), np.int32)
    p = sc._ptr
    for suffix in ("", "_host"):
        cf, fp = getattr(built, "sc_cost_field_multi_batch" + suffix), getattr(built, "sc_field_paths_multi_batch" + suffix)
        assert cf(None, p(d2), None, 0, 1, None, 8, 8, 0, p(seed), None, p(off), 1, 1, -1, p(g), p(g), p(one)) == 1
        assert fp(None, p(d2), None, 0, 1, None, 8, 8, 0, p(g), p(g), p(seed), 1, 1, p(one), p(one), 1, 4, 0, p(path), p(one), p(one), p(one),
                  p(one)) == 1
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        built.sc_ctx_create.restype = ctypes.c_int
        assert built.sc_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
