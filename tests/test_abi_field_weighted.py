"""The weighted cost fields at the drop-in boundary: the six C functions are declared in include/sea_current_hip.h and
exported by the built library, their ctypes signatures match the declarations, the Python binding has the new method and
keywords, and without a device the _host forms fail with a status.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

NEW = ("sc_clearance_penalty_u8", "sc_clearance_penalty_u8_host", "sc_cost_field_weighted_batch", "sc_cost_field_weighted_batch_host",
       "sc_field_paths_weighted_batch", "sc_field_paths_weighted_batch_host")


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


def test_weighted_calls_extend_the_unweighted_calls():
    """After ctx and d2 come pen and pen_cap; the rest is the unweighted call's list in its order."""
    for old, new in (("sc_cost_field_batch", "sc_cost_field_weighted_batch"), ("sc_field_paths_batch", "sc_field_paths_weighted_batch")):
        for suffix in ("", "_host"):
            o, n = _params(old + suffix), _params(new + suffix)
            assert n == o[:2] + ["const uint8_t* pen", "int pen_cap"] + o[2:], new + suffix
    for suffix in ("", "_host"):
        assert _params("sc_clearance_penalty_u8" + suffix) == ["sc_ctx* ctx", "const int32_t* d2", "int W", "int H", "int batch",
                                                               "int32_t r2_clear", "int32_t r2_soft", "int pen_max", "uint8_t* pen"]


def test_binding_has_the_method_and_keywords():
    p = inspect.signature(sc.Context.clearance_penalty).parameters
    assert list(p)[1:] == ["d2", "r2", "r2_soft", "pen_max", "out"] and p["r2"].default == 0 and p["out"].default is None
    for name in ("cost_fields", "field_paths", "cost_fields_host", "field_paths_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert p["pen"].default is None and p["pen_cap"].default == 255, name


def test_host_forms_fail_with_a_status_without_a_device(built):
    """A null context, and (where there is no GPU) a failed sc_ctx_create: a status comes back, nothing crashes."""
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES[n]
    d2 = np.ones((8, 8), np.int32)
    pen = np.zeros((8, 8), np.uint8)
    root = np.zeros(1, np.int32)
    g = np.zeros((1, 8, 8), np.int32)
    st = np.zeros(1, np.int32)
    path = np.zeros((1, 4), np.int32)
    p = sc._ptr
    assert built.sc_clearance_penalty_u8_host(None, p(d2), 8, 8, 1, 0, 36, 40, p(pen)) == 1
    assert built.sc_cost_field_weighted_batch_host(None, p(d2), p(pen), 255, 1, None, 8, 8, 0, p(root), 1, -1, p(g), p(st)) == 1
    assert built.sc_field_paths_weighted_batch_host(None, p(d2), p(pen), 255, 1, None, 8, 8, 0, p(g), p(root), 1, p(st), p(st), 1, 4, 0,
                                                    p(path), p(st), p(st), p(st)) == 1
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        built.sc_ctx_create.restype = ctypes.c_int
        assert built.sc_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
