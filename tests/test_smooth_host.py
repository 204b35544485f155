"""CPU-side checks of sc_smooth_paths_batch: the library exports the new entries, and the sample-count rule it applies
before sampling (so that the ragged profiles can be packed without a host round trip) is the sampler's own: knots whose
time increment is below 1e-8 are dropped, T is the time of the last knot kept, length = ceil(T / dt).  This pins the RULE:
a Python twin of it is checked against the CPU oracle's sampler on random 1-dof TOPP-RA problems, some with near-zero
stages.  The kernel that applies it (smooth_count_scan_kernel) is checked on the GPU (tests/test_gpu_smooth.py: counts
bit-equal to the sampler's on the bench batch, the recorded run and the capacity test)."""
import ctypes
import math

import numpy as np
import pytest

import sea_current_amd as sc

NEARLY_ZERO = 1e-8


def sample_count(t, dt):
    """The rule of smooth_count_scan_kernel (csrc/smooth.hip) and toppra_sample_kernel (csrc/toppra.hip)."""
    i = len(t) - 1
    while i > 0 and not (t[i] - t[i - 1] >= NEARLY_ZERO):
        i -= 1
    return int(math.ceil(t[i] / dt))


def test_smooth_entries_exported():
    sc.build()
    lib = ctypes.CDLL(sc.LIB_PATH)
    for name in ("sc_smooth_paths_batch", "sc_smooth_paths_batch_host", "sc_cells_to_points_batch"):
        assert hasattr(lib, name), name
        assert name in sc.EXPORTS
    assert sc.K_SMOOTH == 14
    assert (sc.SMOOTH_OK, sc.SMOOTH_BAD_INPUT, sc.SMOOTH_NONFINITE, sc.SMOOTH_TOPPRA_FAILED, sc.SMOOTH_TRUNCATED,
            sc.SMOOTH_EMPTY_SEGMENT) == (0, 1, 2, 3, 4, 5)
    hdr = open(sc.HEADER_PATH).read()
    assert "SC_K_SMOOTH = 14" in hdr and "SC_K_COUNT = 15" in hdr


def _problems(n, seed=3):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        L = float(rng.choice([rng.uniform(0.01, 0.5), rng.uniform(0.5, 30.0), rng.uniform(30.0, 200.0)]))
        v = float(rng.uniform(0.05, 3.0))
        a = float(rng.uniform(0.05, 3.0))
        dt = float(np.float32(rng.choice([0.02, 0.01, 0.05, 0.1, 0.013])))
        N = int(rng.choice([20, 50, 100]))
        yield L, v, a, dt, N, rng


def test_sample_count_rule_matches_the_sampler(oracle):
    checked = dropped = 0
    for L, v, a, dt, N, rng in _problems(500):
        r = oracle.toppra([0.0], [L], [0.0], [0.0], [-v], [v], [-a], [a], N=N)
        if r["status"] != 0:
            continue
        t = r["t"].copy()
        kind = rng.integers(0, 4)
        if kind == 1:      # stages that take (nearly) no time: inner ones, and the last ones
            for i in rng.choice(np.arange(1, N + 1), size=3, replace=False):
                t[i:] -= (t[i] - t[i - 1]) - rng.choice([0.0, 1e-9, 9.9e-9])
        elif kind == 2:    # the last stages: their increments drop and T is an earlier knot's time
            k = int(rng.integers(1, 5))
            t[N - k + 1:] = t[N - k] + rng.choice([0.0, 5e-9]) * np.arange(1, k + 1)
        elif kind == 3:    # an increment just at the threshold
            i = int(rng.integers(1, N + 1))
            t[i:] -= (t[i] - t[i - 1]) - 1e-8
        expect = oracle.toppra_sample([0.0], [L], [0.0], [0.0], r["x"], t, dt, max_len=1)["length"]
        got = sample_count(t, dt)
        assert got == expect, (L, v, a, dt, N, kind)
        checked += 1
        dropped += int(not (t[-1] - t[-2] >= NEARLY_ZERO))
    assert checked >= 450
    assert dropped >= 50       # problems whose last knot is dropped
    # where that moves the count: T = 1.0, not t[N] = 1.0 + 5e-9 (ceil(t[N] / dt) would give 3)
    t = np.array([0.0, 0.5, 1.0, 1.0 + 5e-9])
    got = sample_count(t, 0.5)
    assert got == 2 == oracle.toppra_sample([0.0], [1.0], [0.0], [0.0], np.ones(4), t, 0.5, max_len=1)["length"]
