"""The C reference of the timed-path conflicts (tests/cpp/traj_ref.c) against the NumPy twin, bit for bit.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import traj_cases as tc
import traj_twin as tw

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "traj_ref.c")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("traj_ref")), "libtraj_ref.so")
    subprocess.check_call(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", so, SRC, "-lm"])
    lib = C.CDLL(so)
    lib.tr_knots.restype = lib.tr_conflicts.restype = None
    lib.tr_knots.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.tr_conflicts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_double] + \
        [C.c_void_p] * 6
    return lib


def run_ref(lib, c):
    p = lambda a: None if a is None else a.ctypes.data
    P, K = len(c["length"]), c["K"]
    kn = np.zeros((P, K + 1, 2))
    o = dict(knots=kn, tstatus=np.zeros(P, np.int32), first_t=np.zeros(P), first_with=np.zeros(P, np.int32), min_sep=np.zeros(P),
             min_with=np.zeros(P, np.int32), n_conf=np.zeros(P, np.int32), conflict=np.full((P, (P + 31) // 32), 7, np.uint32))
    lib.tr_knots(p(c["time"]), p(c["pts"]), p(c["offsets"]), p(c["length"]), p(c["status"]), P, p(c["t0"]), p(c["flags"]), c["T0"], c["dt_c"],
                 K, p(kn), p(o["tstatus"]))
    lib.tr_conflicts(p(kn), p(o["tstatus"]), P, K, c["T0"], c["dt_c"], p(c["radius"]), p(c["group"]), c["sep_cap"], p(o["first_t"]),
                     p(o["first_with"]), p(o["min_sep"]), p(o["min_with"]), p(o["n_conf"]), p(o["conflict"]))
    return o


def same_bits(got, ref):
    for k in ("knots", "first_t", "min_sep"):
        assert np.array_equal(tc.bits(got[k]), tc.bits(ref[k])), k
    for k in ("tstatus", "first_with", "min_with", "n_conf", "conflict"):
        assert np.array_equal(got[k], ref[k]), k


CASES = {
    "fleet": lambda: tc.random_fleet(),
    "fleet_capped": lambda: {**tc.random_fleet(), "sep_cap": 2.0},
    "fleet_defaults": lambda: {**tc.random_fleet(seed=3, P=40, K=65, broken=False), "t0": None, "flags": None, "group": None, "status": None},
    "head_on": lambda: tc.head_on(3.0),
    "crossing": lambda: tc.crossing(1.0),
    "parked": lambda: tc.parked(True),
    "vanishing": lambda: tc.parked(False),
    "tie": lambda: tc.mirror_tie(),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_equals_twin(ref, name):
    c = CASES[name]()
    same_bits(run_ref(ref, c), tw.fleet(**c))
