"""The C reference of the space-time re-planning (tests/cpp/tplan_ref.c) against the NumPy twin, bit for bit: res, the reach
layers, every output; and its stand-alone check program under AddressSanitizer and UndefinedBehaviorSanitizer (a program of its
own: nothing loaded into Python is sanitised).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_tplan_twin as cases
import tplan_twin as tw

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "tplan_ref.c")
CHECK = os.path.join(HERE, "cpp", "tplan_ref_check.c")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("tplan_ref")), "libtplan_ref.so")
    subprocess.check_call(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", so, SRC, "-lm"])
    lib = C.CDLL(so)
    vp, i, d, f = C.c_void_p, C.c_int, C.c_double, C.c_float
    lib.tp_reserve.restype = lib.tp_plan.restype = lib.tp_fleet_replan.restype = None
    lib.tp_reserve.argtypes = [vp, vp, i, i, vp, vp, d, i, i, f, f, f, f, vp]
    lib.tp_plan.argtypes = [vp, i, i, C.c_int32, vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp, f, f, f, f, vp]
    lib.tp_fleet_replan.argtypes = [vp, vp, i, i, vp, vp, d, i, i, f, f, f, f, vp, vp, C.c_int32, vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp, i]
    return lib


def run_ref(lib, knots, tstatus, radius, select, pad, W, H, frame, d2, start, goal, t_start, hold, r_new, sequential):
    p = lambda a: None if a is None else a.ctypes.data
    knots = np.ascontiguousarray(knots, np.float64)
    P, L = knots.shape[:2]
    B, Wq = len(start), (W + 31) // 32
    a = lambda v, t: None if v is None else np.ascontiguousarray(v, t)
    radius, select, d2, start, goal, t_start, r_new = (a(radius, np.float64), a(select, np.int32), a(d2, np.int32), a(start, np.int32),
                                                        a(goal, np.int32), a(t_start, np.int32), a(r_new, np.float64))
    o = dict(tstatus=None if tstatus is None else np.array(tstatus, np.int32), res=np.zeros((L, H, Wq), np.uint32),
             path=np.full((B, L), -1, np.int32), len=np.zeros(B, np.int32), arrive=np.zeros(B, np.int32), status=np.zeros(B, np.int32),
             knots_out=np.zeros((B, L, 2)), reach=np.zeros((1 if sequential else B, L, H, Wq), np.uint32))
    lib.tp_fleet_replan(p(knots), p(o["tstatus"]), P, L - 1, p(radius), p(select), pad, W, H, *frame, p(o["res"]), p(d2), 0, p(start), p(goal),
                        p(t_start), B, hold, p(o["path"]), p(o["len"]), p(o["arrive"]), p(o["status"]), p(o["knots_out"]), p(o["reach"]), p(r_new),
                        int(sequential))
    return o


def same(got, want, reach=True):
    for k in ("status", "arrive", "len", "path"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["knots_out"].view(np.uint64), want["knots_out"].view(np.uint64))
    assert np.array_equal(got["res"], tw.pack(want["res"]))
    if got["tstatus"] is not None:
        assert np.array_equal(got["tstatus"], want["tstatus"])
    if reach:
        assert np.array_equal(got["reach"], tw.pack(want["reach"]))


@pytest.mark.parametrize("sequential", [False, True])
def test_reference_equals_twin_on_the_fleet(ref, sequential):
    f = cases.random_fleet()
    n = 40 if not sequential else 12
    pad = 0.02 + np.sqrt(np.float64(np.float32(0.05)) ** 2 * 2) / 2 * (1 + 2.0 ** -20)
    radius = f["radius"].copy()
    radius[3] = np.inf                                  # outside the contract: TRAJ_BAD, reserves nothing
    select = np.ones(len(radius), np.int32)
    select[5] = 0
    ts = np.zeros(len(radius), np.int32)
    ts[7] = 1
    args = (f["knots"], ts, radius, select, pad, f["W"], f["H"], f["frame"])
    want = tw.fleet_replan(*args, None, f["d2"], 0, f["start"][:n], f["goal"][:n], f["t_start"][:n], 1, r_new=f["r_new"][:n],
                           sequential=sequential, want_reach=True)
    got = run_ref(ref, *args, f["d2"], f["start"][:n], f["goal"][:n], f["t_start"][:n], 1, f["r_new"][:n], sequential)
    same(got, want, reach=not sequential)
    assert list(want["tstatus"][[3, 5, 7]]) == [2, 0, 1] and (want["status"] == tw.TP_OK).sum() >= n // 2


@pytest.mark.parametrize("W,H", [(1, 1), (31, 2), (32, 7), (33, 5), (65, 3)])
@pytest.mark.parametrize("hold", [0, 1])
def test_reference_equals_twin_on_word_edges(ref, W, H, hold):
    rng = np.random.default_rng(W * 10 + H)
    L = 20
    d2 = (rng.random((H, W)) >= 0.15).astype(np.int32)
    frame = (0.5, -0.25, 0.1, 0.07)
    knots = np.stack([rng.uniform(0.5, 0.5 + 0.1 * W, (3, L)), rng.uniform(-0.25, -0.25 + 0.07 * H, (3, L))], axis=2)
    knots[rng.random((3, L)) < 0.1] = np.nan
    start, goal = rng.integers(-1, W * H + 1, 12), rng.integers(0, W * H, 12)
    t_start = rng.integers(-1, L + 1, 12)
    args = (knots, None, np.full(3, 0.03), None, 0.08, W, H, frame)
    want = tw.fleet_replan(*args, None, d2, 0, start, goal, t_start, hold, want_reach=True)
    same(run_ref(ref, *args, d2, start, goal, t_start, hold, None, False), want)


def test_check_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tplan_ref_check")
    subprocess.check_call(["cc", "-g", "-O1", "-std=c11", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, CHECK, SRC, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("tplan_ref OK") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
