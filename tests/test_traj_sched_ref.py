"""The C reference of the delay schedules (tests/cpp/traj_sched_ref.c) against the NumPy twin, bit for bit, and its stand-alone
check program under AddressSanitizer and UndefinedBehaviorSanitizer (a program of its own: nothing loaded into Python is
sanitised).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import traj_cases as tc
import traj_sched_twin as sw

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = [os.path.join(HERE, "cpp", n) for n in ("traj_sched_ref.c", "traj_ref.c")]
CHECK = os.path.join(HERE, "cpp", "traj_sched_ref_check.c")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("traj_sched_ref")), "libtraj_sched_ref.so")
    subprocess.check_call(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", so, *SRC, "-lm"])
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    lib.ts_shift_table.restype = lib.ts_schedule.restype = lib.ts_shift_knots.restype = None
    lib.ts_shift_table.argtypes = [vp, vp, i, i, vp, vp, i, i, i, vp, vp]
    lib.ts_schedule.argtypes = [vp, vp, i, i, vp, vp, vp, vp]
    lib.ts_shift_knots.argtypes = [vp, i, i, vp, i, vp]
    return lib


def run_ref(lib, kn, ts, c, D, stride, order=None, jmax=None, skip=1):
    p = lambda a: None if a is None else a.ctypes.data
    P, K = kn.shape[0], kn.shape[1] - 1
    kn = np.ascontiguousarray(kn)
    o = dict(tstatus=np.array(ts, np.int32), table=np.full((P, P), 7, np.uint64), slot=np.zeros(P, np.int32), counts=np.zeros(4, np.int32),
             knots_out=np.zeros_like(kn), stats=np.zeros(2, np.int64))
    order = None if order is None else np.ascontiguousarray(order, np.int32)
    jmax = None if jmax is None else np.ascontiguousarray(jmax, np.int32)
    lib.ts_shift_table(p(kn), p(o["tstatus"]), P, K, p(c["radius"]), p(c["group"]), D, stride, skip, p(o["table"]), p(o["stats"]))
    lib.ts_schedule(p(o["table"]), p(o["tstatus"]), P, D, p(order), p(jmax), p(o["slot"]), p(o["counts"]))
    lib.ts_shift_knots(p(kn), P, K, p(o["slot"]), stride, p(o["knots_out"]))
    return o


def same(got, want):
    for k in ("tstatus", "table", "slot", "counts"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(tc.bits(got["knots_out"]), tc.bits(want["knots_out"]))


@pytest.mark.parametrize("D,stride,K", [(8, 1, 300), (32, 2, 400)])
def test_reference_equals_twin_on_the_fleet(ref, D, stride, K):
    c = tc.random_fleet(K=K)
    rng = np.random.default_rng(D)
    P = len(c["length"])
    order = rng.integers(-1, P + 1, P)
    jmax = rng.integers(-2, D + 3, P)
    st = {}
    want = sw.fleet_schedule(**c, D=D, stride=stride, stats=st)
    from traj_twin import knots
    kn, ts = knots(c["time"], c["pts"], c["offsets"], c["length"], c["status"], c["t0"], c["flags"], c["T0"], c["dt_c"], K)
    got = run_ref(ref, kn, ts, c, D, stride)
    same(got, want)
    assert got["stats"].tolist() == [st["compared"], st["skipped"]] == [6722, 5678]
    same(run_ref(ref, kn, ts, c, D, stride, order, jmax, skip=0), sw.fleet_schedule(**c, D=D, stride=stride, order=order, jmax=jmax))


HAND = {
    "crossing": (lambda: tc.crossing(), 8, 1), "crossing_stride": (lambda: tc.crossing(), 4, 2), "head_on": (lambda: tc.head_on(), 8, 1),
    "head_on_vanishing": (lambda: {**tc.head_on(), "flags": np.zeros(2, np.int32), "T0": -0.5, "K": 40}, 20, 1),
    "parked": (lambda: tc.parked(True), 6, 1), "vanishing": (lambda: tc.parked(False), 6, 1), "tie": (tc.mirror_tie, 4, 1),
    "one_slot": (lambda: tc.crossing(), 1, 1), "whole_horizon": (lambda: tc.crossing(), 3, 11),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_reference_equals_twin_on_hand_cases(ref, name):
    make, D, stride = HAND[name]
    c = make()
    want = sw.fleet_schedule(**c, D=D, stride=stride)
    same(run_ref(ref, want["knots"], np.zeros(len(c["length"]), np.int32), c, D, stride), want)


def test_check_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "traj_sched_ref_check")
    subprocess.check_call(["cc", "-g", "-O1", "-std=c11", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, CHECK, *SRC, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("traj_sched_ref OK") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
