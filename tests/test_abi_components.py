"""The component entry points at the drop-in boundary: the five C functions are declared in include/sea_current_hip.h and
exported by the built library, their ctypes signatures match the declarations, the Python binding has the new methods and
the `label` keyword, and without a device the _host forms fail with a status.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sea_current_amd as sc

NEW = ("sc_components_batch", "sc_components_batch_host", "sc_reachable_batch", "sc_reachable_batch_host", "sc_astar_batch_screened")


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


def test_parameter_lists():
    for suffix in ("", "_host"):
        assert _params("sc_components_batch" + suffix) == ["sc_ctx* ctx", "const int32_t* d2", "int G", "int W", "int H", "int32_t r2_clear",
                                                           "int32_t* label", "int32_t* size", "int32_t* ncomp", "int32_t* largest"]
        assert _params("sc_reachable_batch" + suffix) == ["sc_ctx* ctx", "const int32_t* label", "int G", "const int32_t* qgrid", "int W",
                                                          "int H", "const int32_t* start", "const int32_t* goal", "int Q", "int32_t* status"]
    # the screened search: sc_astar_batch_multi's list with the labels after d2
    o, n = _params("sc_astar_batch_multi"), _params("sc_astar_batch_screened")
    assert n == o[:2] + ["const int32_t* label"] + o[2:]


def test_binding_has_the_methods_and_the_keyword():
    p = inspect.signature(sc.Context.components).parameters
    assert list(p)[1:] == ["d2", "r2", "want_size", "out"]
    assert p["r2"].default == 0 and p["want_size"].default is False and p["out"].default is None
    p = inspect.signature(sc.Context.reachable).parameters
    assert list(p)[1:] == ["label", "start", "goal", "qgrid"] and p["qgrid"].default is None
    for name in ("astar_batch", "astar_batch_multi"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[-1] == "label" and p["label"].default is None, name
    assert callable(sc.Context.components_host) and callable(sc.Context.reachable_host)


def test_host_forms_fail_with_a_status_without_a_device(built):
    """A null context, and (where there is no GPU) a failed sc_ctx_create: a status comes back, nothing crashes."""
    for n in NEW:
        fn = getattr(built, n)
        fn.restype, fn.argtypes = sc._SIGNATURES[n]
    d2 = np.ones((8, 8), np.int32)
    label = np.zeros((8, 8), np.int32)
    one = np.zeros(1, np.int32)
    path = np.zeros((1, 4), np.int32)
    p = sc._ptr
    assert built.sc_components_batch_host(None, p(d2), 1, 8, 8, 0, p(label), None, p(one), p(one)) == 1
    assert built.sc_reachable_batch_host(None, p(label), 1, None, 8, 8, p(one), p(one), 1, p(one)) == 1
    assert built.sc_components_batch(None, p(d2), 1, 8, 8, 0, p(label), None, None, None) == 1
    assert built.sc_reachable_batch(None, p(label), 1, None, 8, 8, p(one), p(one), 1, p(one)) == 1
    assert built.sc_astar_batch_screened(None, p(d2), p(label), 1, None, 8, 8, 0, p(one), p(one), 1, 4, p(path), p(one), p(one), p(one)) == 1
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        built.sc_ctx_create.restype = ctypes.c_int
        assert built.sc_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
