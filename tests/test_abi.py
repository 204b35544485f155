"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and
exports every symbol include/sea_current_hip.h declares.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

import sea_current_amd as sc


@pytest.fixture(scope="module")
def built():
    sc.build()
    return ctypes.CDLL(sc.LIB_PATH)


def _declared():
    src = open(sc.HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(built):
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(built, n), f"{n} declared in include/sea_current_hip.h but not exported"
    assert sorted(sc.EXPORTS) == names  # the Python binding covers the whole ABI


def _declarations():
    """{name: (result, [parameter, ..])} as the header spells them, read statement by statement (the binding reads the
    header with a parser of its own; this one shares nothing with it)."""
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(sc.HEADER_PATH).read(), flags=re.S))
    decls = {}
    for stmt in src.split(";"):
        m = re.search(r"\b(sc_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if m:
            result = stmt[:m.start(1)].split("\n")[-1].strip()
            params = [" ".join(p.split()) for p in m.group(2).split(",")]
            decls[m.group(1)] = (result, [] if params == ["void"] else params)
    return decls


def test_signatures_match_every_declaration():
    """Every function the header declares, not one feature's: the binding's argument count, per argument a pointer
    (c_void_p) or the exact scalar ctype, and the result type."""
    scalar = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
              "double": ctypes.c_double}
    result = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p, "void": None}
    decls = _declarations()
    assert sorted(decls) == _declared() and len(decls) >= 128
    assert sorted(sc._SIGNATURES) == sorted(decls)
    for name, (res, params) in decls.items():
        got_res, got_args = sc._SIGNATURES[name]
        assert got_res is result[res], (name, res, got_res)
        assert len(got_args) == len(params), (name, len(got_args), len(params))
        for k, (p, got) in enumerate(zip(params, got_args)):
            want = ctypes.c_void_p if "*" in p else scalar[p.split()[0]]
            assert got is want, (name, k, p, got)
    assert {res for res, _ in decls.values()} == set(result)       # each result type occurs, so each mapping is exercised


@pytest.mark.parametrize("decl", ["int sc_odd(sc_ctx* ctx, unsigned n);", "int sc_odd(sc_ctx* ctx, size_t n);", "int sc_odd(long);",
                                  "unsigned sc_odd(int n);", "float* sc_odd(int n);", "int sc_odd(int (*cb)(int));"])
def test_unreadable_declaration_raises_and_names_the_function(decl):
    """The binding never skips or guesses a declaration it cannot map to ctypes."""
    with pytest.raises(sc.SeaCurrentError, match="sc_odd"):
        sc._signatures("int sc_fine(int a, const float* b);\n" + decl)
    assert sc._signatures("int sc_fine(int a, const float* b);\nvoid sc_none(void);") == {
        "sc_fine": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p]), "sc_none": (None, [])}


def test_abi_version_and_strings(built):
    built.sc_abi_version.restype = ctypes.c_int
    assert built.sc_abi_version() == 1
    built.sc_status_string.restype = ctypes.c_char_p
    assert built.sc_status_string(0) == b"ok"
    assert built.sc_status_string(1) == b"invalid argument"


def test_no_gpu_fails_loudly(built):
    """Without a GPU the product path must fail, not fall back to the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = ctypes.c_void_p()
    built.sc_ctx_create.restype = ctypes.c_int
    st = built.sc_ctx_create(0, ctypes.byref(h))
    assert st != 0 and not h.value


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under sea-current_amd/ may reference it."""
    bad = []
    for root, _, files in os.walk(sc.NATIVE_DIR):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp", ".cpp", "Makefile")):
                txt = open(os.path.join(root, f), errors="ignore").read()
                if re.search(r"(import\s+oracle|from\s+oracle|libsc_oracle|sc_oracle\.h\"|sco_)", txt) and "sc_oracle.h)" not in txt:
                    for line in txt.splitlines():
                        if re.search(r"(import\s+oracle|from\s+oracle|libsc_oracle|#include.*sc_oracle|sco_[a-z])", line):
                            bad.append((f, line.strip()))
    assert not bad, bad
