"""The C reference of the assignment (tests/cpp/assign_ref.c) against the NumPy twin, bit for bit in all five outputs, the two
pinned 1024 x 1024 cases, and its stand-alone check program under AddressSanitizer and UndefinedBehaviorSanitizer (a program of
its own: nothing loaded into Python is sanitised).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import assign_twin as tw

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "assign_ref.c")
CHECK = os.path.join(HERE, "cpp", "assign_ref_check.c")
KEYS = ("col_of", "row_of", "u", "v", "info")


def build_ref(directory):
    so = os.path.join(str(directory), "libassign_ref.so")
    subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    lib.assign_ref.restype = lib.field_cost_matrix_ref.restype = None
    lib.assign_ref.argtypes = [vp, i, i, i, vp, vp, vp, vp, vp, vp]
    lib.field_cost_matrix_ref.argtypes = [vp, i, i, i, vp, i, vp, vp]
    return lib


def run_ref(lib, cost, max_raw=None):
    cost = np.ascontiguousarray(cost, np.int32)
    if cost.ndim == 2:
        cost = cost[None]
    B, R, Cc = cost.shape
    o = dict(col_of=np.full((B, R), 7, np.int32), row_of=np.full((B, Cc), 7, np.int32), u=np.full((B, R), 7, np.int64),
             v=np.full((B, Cc), 7, np.int64), info=np.full((B, 4), 7, np.int64))
    lib.assign_ref(cost.ctypes.data, B, R, Cc, *(o[k].ctypes.data for k in KEYS), None if max_raw is None else max_raw.ctypes.data)
    return o


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("assign_ref"))


def same(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_reference_equals_twin_on_every_small_shape(ref):
    rng = np.random.default_rng(1)
    for R in range(1, 7):
        for Cc in range(1, 8):
            for kind in ("tie", "small", "octile", "full"):
                for fb in (0.0, 0.1, 0.5, 0.9, 1.0):
                    cost = tw.random_cost(rng, R, Cc, kind, fb)
                    same(run_ref(ref, cost), tw.assign(cost))


@pytest.mark.parametrize("R,Cc", [(257, 300), (300, 257)])
@pytest.mark.parametrize("kind,fb", [("full", 0.0), ("octile", 0.1), ("small", 0.5)])
def test_reference_equals_twin_across_the_block_sizes(ref, R, Cc, kind, fb):
    cost = tw.random_cost(np.random.default_rng(R), R, Cc, kind, fb)
    raw = np.zeros(1, np.int64)
    got = run_ref(ref, cost, raw)
    same(got, tw.assign(cost))
    assert raw[0] < 2**53                       # the reduction key (minv << 10) | j of the kernels fits 64 bits
    tw.certificate(cost, {k: got[k][0] for k in KEYS})


def test_a_bad_problem_in_a_batch(ref):
    cost = tw.random_cost(np.random.default_rng(2), 4, 3, "small")[None].repeat(3, 0)
    cost[1, 0, 0] = -7
    same(run_ref(ref, cost), tw.assign(cost))


@pytest.mark.parametrize("name,total", [("i*j", 178433024), ("(1024-i)*j", 178956800)])
def test_pinned_1024(ref, name, total):
    i, j = np.mgrid[0:1024, 0:1024]
    cost = (i * j if name == "i*j" else (1024 - i) * j).astype(np.int32)
    raw = np.zeros(1, np.int64)
    got = run_ref(ref, cost, raw)
    assert got["info"][0].tolist() == [1024, total, 524800, 0] and 524800 == 1024 * 1025 // 2
    assert raw[0] < 2**53
    tw.certificate(cost, {k: got[k][0] for k in KEYS})


def test_field_cost_matrix_reference_equals_twin(ref):
    rng = np.random.default_rng(4)
    g = rng.integers(0, 2**31 - 1, (5, 9, 13)).astype(np.int32)
    g[rng.random(g.shape) < 0.2] = tw.INF
    g[0, 0, 0] = tw.INF - 1
    cells = rng.integers(-3, 9 * 13 + 3, 40).astype(np.int32)
    cells[0] = 0
    for cc in (None, rng.integers(0, tw.SEED_COST_MAX + 1, 5).astype(np.int32)):
        out = np.full((40, 5), 7, np.int32)
        ref.field_cost_matrix_ref(g.ctypes.data, 5, 13, 9, cells.ctypes.data, 40, None if cc is None else cc.ctypes.data, out.ctypes.data)
        assert np.array_equal(out, tw.field_cost_matrix(g, cells, cc))


def test_check_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "assign_ref_check")
    subprocess.check_call(["cc", "-g", "-O1", "-std=c11", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           CHECK, SRC, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("assign_ref OK") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
