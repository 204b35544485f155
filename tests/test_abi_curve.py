"""The curve check and repair at the drop-in boundary: the six C functions are declared in include/sea_current_hip.h with the
documented arguments and exported by the built library, SC_SMOOTH_COLLIDES is 6, and the Python binding has the new methods
and the new smooth_paths keywords.  No GPU."""
import ctypes
import inspect
import re

import pytest

import sea_current_amd as sc

NEW = ("sc_curve_clearance_batch", "sc_curve_clear_batch", "sc_smooth_paths_clear_batch")


@pytest.fixture(scope="module")
def built():
    sc.build()
    return ctypes.CDLL(sc.LIB_PATH)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(sc.HEADER_PATH).read(), flags=re.S)


def _params(src, name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
    assert m, f"{name} not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_declared_and_exported(built):
    src = _header()
    for n in NEW:
        for suffix in ("", "_host"):
            assert re.search(r"\bint\s+%s\s*\(" % (n + suffix), src), f"{n + suffix} not declared"
            assert hasattr(built, n + suffix), f"{n + suffix} not exported"
            assert n + suffix in sc.EXPORTS
    assert re.search(r"\bSC_SMOOTH_COLLIDES\s*=\s*6\b", src) and sc.SMOOTH_COLLIDES == 6
    assert re.search(r"#define\s+SC_CURVE_MAX_LEVEL\s+30\b", src) and sc.CURVE_MAX_LEVEL == 30
    m = re.search(r"#define\s+SC_CURVE_MAX_LEGS\s+(\d+)\b", src)
    assert m and int(m.group(1)) == sc.CURVE_MAX_LEGS
    built.sc_abi_version.restype = ctypes.c_int
    assert built.sc_abi_version() == 1                                # additive: the ABI version stays


def test_argument_lists():
    src = _header()
    frame = ["const int32_t* d2", "int W", "int H", "float x_min", "float y_min", "float res_x", "float res_y", "int32_t r2_clear"]
    for suffix in ("", "_host"):
        chk = _params(src, "sc_curve_clearance_batch" + suffix)
        assert chk == ["sc_ctx* ctx", "const float* ctrl", "const int32_t* seg_off", "const int32_t* status", "int P"] + frame + \
            ["int32_t* leg_min_d2", "int32_t* path_min_d2", "int32_t* hit_legs", "int32_t* hit_leg", "float* hit_t"]
        clr = _params(src, "sc_curve_clear_batch" + suffix)
        assert clr == ["sc_ctx* ctx", "const float* ctrl_in", "const int32_t* seg_off", "const int32_t* status", "int P"] + frame + \
            ["int max_level", "float* ctrl_out", "uint8_t* level", "int32_t* rounds", "int32_t* leg_min_d2", "int32_t* status_out"]
        assert len(sc._SIGNATURES["sc_curve_clearance_batch" + suffix][1]) == len(chk) == 18
        assert len(sc._SIGNATURES["sc_curve_clear_batch" + suffix][1]) == len(clr) == 19
        # the smoothing call takes every argument of the limited call in the same order, then its own
        old, new = _params(src, "sc_smooth_paths_limited_batch" + suffix), _params(src, "sc_smooth_paths_clear_batch" + suffix)
        assert new[:len(old)] == old
        assert new[len(old):] == ["int32_t r2_clear", "int max_level", "uint8_t* level", "int32_t* leg_min_d2", "int32_t* rounds"]
        assert len(sc._SIGNATURES["sc_smooth_paths_clear_batch" + suffix][1]) == len(new) == 45


def test_binding_has_the_methods_and_keywords():
    for name in ("curve_clearance", "curve_clearance_host", "curve_clear", "curve_clear_host"):
        assert callable(getattr(sc.Context, name)), name
    for name in ("smooth_paths", "smooth_paths_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert p["r2_clear"].default is None and p["max_level"].default == 6, name   # the default keeps the calls of before
    assert inspect.signature(sc.Context.curve_clear).parameters["max_level"].default == 6
