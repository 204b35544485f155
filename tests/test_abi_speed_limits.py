"""The per-stage speed limits at the drop-in boundary: the four C functions are declared in include/sea_current_hip.h and
exported by the built library, and the Python binding has the new methods and the new smooth_paths keywords.  No GPU."""
import ctypes
import inspect
import re

import pytest

import sea_current_amd as sc

NEW = ("sc_speed_limits_batch", "sc_speed_limits_batch_host", "sc_smooth_paths_limited_batch", "sc_smooth_paths_limited_batch_host")


@pytest.fixture(scope="module")
def built():
    sc.build()
    return ctypes.CDLL(sc.LIB_PATH)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(sc.HEADER_PATH).read(), flags=re.S)


def test_declared_and_exported(built):
    src = _header()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), f"{n} not declared"
        assert hasattr(built, n), f"{n} not exported"
        assert n in sc.EXPORTS
    assert re.search(r"#define\s+SC_SPEED_MAX_J\s+32\b", src)
    built.sc_abi_version.restype = ctypes.c_int
    assert built.sc_abi_version() == 1                                # additive: the ABI version stays


def test_limited_call_extends_the_smooth_call():
    """sc_smooth_paths_limited_batch takes every argument of sc_smooth_paths_batch in the same order, then its own."""
    src = _header()

    def params(name):
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        return [" ".join(p.split()) for p in m.group(1).split(",")]

    for suffix in ("", "_host"):
        old, new = params("sc_smooth_paths_batch" + suffix), params("sc_smooth_paths_limited_batch" + suffix)
        assert new[:len(old)] == old
        assert new[len(old):] == ["const double* dyn", "int J", "const int32_t* d2", "int W", "int H", "float x_min", "float y_min",
                                  "float res_x", "float res_y", "double* vmax_stage", "float* min_clear"]
        assert len(sc._SIGNATURES["sc_smooth_paths_limited_batch" + suffix][1]) == len(new)
    for suffix in ("", "_host"):
        assert len(sc._SIGNATURES["sc_speed_limits_batch" + suffix][1]) == len(params("sc_speed_limits_batch" + suffix)) == 22


def test_binding_has_the_methods_and_keywords():
    assert callable(sc.Context.speed_limits) and callable(sc.Context.speed_limits_host)
    for name in ("smooth_paths", "smooth_paths_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert p["dyn"].default is None and p["J"].default == 4 and p["d2"].default is None and p["frame"].default is None, name
    p = inspect.signature(sc.Context.speed_limits).parameters
    assert p["J"].default == 4 and p["N"].default == 100
