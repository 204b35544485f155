"""The timed-path conflicts at the drop-in boundary: the six C functions are declared in include/sea_current_hip.h and exported
by the built library, the binding's signatures have their parameter counts, and the Python methods exist with their
defaults.  No GPU."""
import ctypes
import inspect
import re

import pytest

import sea_current_amd as sc

NEW = ("sc_traj_knots_batch", "sc_traj_knots_batch_host", "sc_traj_conflicts_batch", "sc_traj_conflicts_batch_host",
       "sc_fleet_conflicts_batch", "sc_fleet_conflicts_batch_host")


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
    assert re.search(r"SC_TRAJ_OK = 0,\s*SC_TRAJ_SKIPPED = 1,\s*SC_TRAJ_BAD = 2\s*}\s*sc_traj_status;", src)
    assert (sc.TRAJ_OK, sc.TRAJ_SKIPPED, sc.TRAJ_BAD) == (0, 1, 2)


def test_additive(built):
    src = _header()
    assert re.search(r"SC_K_COUNT = 15\b", src) and re.search(r"SC_K_SMOOTH = 14\b", src)
    assert re.search(r"#define\s+SC_ABI_VERSION\s+1\b", src)
    built.sc_abi_version.restype = ctypes.c_int
    assert built.sc_abi_version() == 1


def test_parameter_counts_and_order():
    for suffix in ("", "_host"):
        kn, cf, fl = (_params(n + suffix) for n in ("sc_traj_knots_batch", "sc_traj_conflicts_batch", "sc_fleet_conflicts_batch"))
        assert len(kn) == 14 and len(cf) == 16 and len(fl) == 23
        assert fl[:14] == kn                                       # the combined call: the knots call's arguments ...
        assert fl[14:] == cf[7:]                                   # ... then what the conflicts call takes after the clock
        assert cf[:7] == ["sc_ctx* ctx", "const double* knots", "int32_t* tstatus", "int P", "int K", "double T0", "double dt_c"]
        for n, params in (("sc_traj_knots_batch", kn), ("sc_traj_conflicts_batch", cf), ("sc_fleet_conflicts_batch", fl)):
            assert len(sc._SIGNATURES[n + suffix][1]) == len(params), n + suffix
            for ctype, decl in zip(sc._SIGNATURES[n + suffix][1], params):
                want = ctypes.c_double if decl.startswith("double ") else ctypes.c_int if decl.startswith("int ") else ctypes.c_void_p
                assert ctype is want, (n + suffix, decl)


def test_binding_has_the_methods_and_keywords():
    inf = float("inf")
    for name in ("fleet_conflicts", "fleet_conflicts_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[:3] == ["self", "sm", "radius"], name
        assert p["t0"].default is None and p["flags"].default is None and p["group"].default is None, name
        assert p["T0"].default == 0.0 and p["dt_c"].default == 0.1 and p["K"].default is None and p["sep_cap"].default == inf, name
        assert p["want_matrix"].default is False, name
    for name in ("traj_knots", "traj_knots_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert p["t0"].default is None and p["flags"].default is None and p["dt_c"].default == 0.1 and p["K"].default is None, name
    for name in ("traj_conflicts", "traj_conflicts_host"):
        p = inspect.signature(getattr(sc.Context, name)).parameters
        assert list(p)[:4] == ["self", "knots", "tstatus", "radius"] and p["sep_cap"].default == inf and p["want_matrix"].default is False, name
