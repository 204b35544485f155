"""The NumPy twin of the delay schedules (tests/traj_sched_twin.py) against hand cases with exact answers, against its own
properties (symmetry, the r = 0 bit, the window formula against a brute-force greedy on absolutely shifted knots, no residual
conflict) and on the seeded fleet, whose counts are asserted so that the GPU tests are known not to be vacuous.  No GPU."""
import numpy as np
import pytest

import traj_cases as tc
import traj_sched_twin as sw
import traj_twin as tw

CONFIGS = {(8, 1, 300): dict(counts=[67, 4, 52, 7], full=118, some=57), (32, 2, 400): dict(counts=[65, 15, 43, 7], full=63, some=354)}
_cache = {}


def fleet(D, stride, K):
    if (D, stride, K) not in _cache:
        c = tc.random_fleet(K=K)
        st = {}
        _cache[(D, stride, K)] = (c, sw.fleet_schedule(**c, D=D, stride=stride, stats=st), st)
    return _cache[(D, stride, K)]


def run(c, D, stride=1, **kw):
    return sw.fleet_schedule(**c, D=D, stride=stride, **kw)


def reverse(w, nb):
    return sum(((int(w) >> b) & 1) << (nb - 1 - b) for b in range(nb))


# ---- hand cases ----
def test_crossing_waits_three_ticks():
    """(0,0) -> (8,0) and (4,-4) -> (4,4) at 1 m/s, radius 0.5 each, dt_c 0.5: with the second path delta seconds behind, the
    closest approach is delta / sqrt(2), so they meet iff |delta| < sqrt(2) s = 2.83 ticks: relative shifts -2 .. 2."""
    o = run(tc.crossing(), 8)
    want = sum(1 << (r + 7) for r in range(-2, 3))
    assert o["table"].tolist() == [[0, want], [want, 0]]
    assert o["slot"].tolist() == [0, 3] and o["counts"].tolist() == [1, 1, 0, 0] and o["delay"].tolist() == [0.0, 1.5]
    assert np.array_equal(tc.bits(o["knots_out"][1, 3:]), tc.bits(o["knots"][1, :-3])) and (o["knots_out"][1, :3] == [4.0, -4.0]).all()
    assert run(tc.crossing(), 8, order=[1, 0])["slot"].tolist() == [3, 0]
    assert run(tc.crossing(), 4, stride=2)["slot"].tolist() == [0, 2]           # 2 ticks still meet, 4 do not


def test_head_on_is_unresolved_until_the_other_has_vanished():
    o = run(tc.head_on(), 8)                                                  # both stand at their ends for ever (flags 3)
    assert o["table"].tolist() == [[0, 2 ** 15 - 1], [2 ** 15 - 1, 0]]
    assert o["slot"].tolist() == [0, -1] and o["counts"].tolist() == [1, 0, 1, 0] and np.isnan(o["delay"][1])
    assert np.isnan(o["knots_out"][1]).all() and np.array_equal(o["knots_out"][0], o["knots"][0])
    # flags 0 and the clock half a second early: both are absent at tick 0, path 0 is there on ticks 1 .. 17.  Path 1, s ticks
    # late, appears on tick s + 1: at s = 15 both are present on interval 16 .. 17, at s = 16 on no interval.
    c = {**tc.head_on(), "flags": np.zeros(2, np.int32), "T0": -0.5, "K": 40}
    o = run(c, 20)
    assert o["slot"].tolist() == [0, 16]
    assert run(c, 16)["slot"].tolist() == [0, -1]


def test_parked_is_unresolved_unless_pinned():
    c = tc.parked(True)                                                       # path 0 stays where path 1 ends; 6 slots end inside the horizon
    o = run(c, 6)
    assert o["table"][0, 1] == 2 ** 11 - 1 and o["slot"].tolist() == [0, -1]
    assert run(c, 6, jmax=[5, -1])["slot"].tolist() == [0, 0]
    assert run(c, 6, jmax=[5, -1])["counts"].tolist() == [2, 0, 0, 0]
    assert run(tc.parked(False), 6)["slot"].tolist() == [0, 0]               # path 0 vanishes at its end: nothing to wait for


def test_same_group_pairs_stay_zero():
    o = run(tc.mirror_tie(), 4)
    assert o["table"][0, 2] == 0 and o["table"][2, 0] == 0 and o["table"][0, 1] != 0 and o["table"][1, 2] != 0
    # 0 and 2 are one group.  Path 1, delta seconds late, is delta short of (8, 0), where 0 and 2 arrive, when the horizon ends at
    # 8 s: 0.5 < R = 1 still meets, 1.0 does not.
    assert o["slot"].tolist() == [0, 2, 0]


# ---- properties ----
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_fleet_counts_and_no_residual_conflict(cfg):
    D, stride, K = cfg
    c, o, st = fleet(*cfg)
    want = CONFIGS[cfg]
    assert o["counts"].tolist() == want["counts"]
    assert st == dict(compared=6722, skipped=5678, full=want["full"], some=want["some"])
    ok = o["tstatus"] == tw.TRAJ_OK
    assert ok.sum() == 123 and sw.at_rest(o["knots"], D, stride)[ok].all()     # the condition of the equivalence note
    args = (c["T0"], c["dt_c"], c["radius"], c["group"])
    before = tw.conflicts(o["knots"], o["tstatus"], *args)
    after = tw.conflicts(o["knots_out"], o["tstatus"], *args)
    assert before["n_conf"].sum() == 280 and after["n_conf"].sum() == 0
    assert np.isnan(o["knots_out"][o["slot"] < 0]).all()
    T, nb = o["table"], 2 * D - 1
    lo, hi = np.triu_indices(len(ok), 1)
    w = T[lo, hi]
    pos_full = (w >> np.uint64(D - 1)) == np.uint64(2 ** D - 1)                # p cannot follow q at any delay ...
    neg_free = (w & np.uint64(2 ** (D - 1) - 1)) != np.uint64(2 ** (D - 1) - 1)  # ... but q can follow p
    assert (pos_full & neg_free).sum() == {(8, 1, 300): 9, (32, 2, 400): 26}[cfg]
    assert (T >> np.uint64(nb)).max() == 0 and (np.diag(T) == 0).all()
    slot2, _ = sw.schedule(T, o["tstatus"], D, np.random.default_rng(1).permutation(len(ok)))
    assert (slot2 != o["slot"]).sum() == {(8, 1, 300): 46, (32, 2, 400): 54}[cfg]


def test_symmetry_and_zero_shift_bit():
    c, o, _ = fleet(8, 1, 300)
    T = o["table"]
    P = T.shape[0]
    for p in range(P):
        for q in range(p + 1, P):
            assert int(T[q, p]) == reverse(T[p, q], 15)
    m = tw.conflicts(o["knots"], o["tstatus"], c["T0"], c["dt_c"], c["radius"], c["group"])["conflict"]
    bit0 = ((T >> np.uint64(7)) & np.uint64(1)).astype(bool)
    dense = ((m[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(P, -1)[:, :P].astype(bool)
    assert np.array_equal(bit0, dense) and bit0.sum() == 280


def test_box_skip_changes_nothing():
    c, o, _ = fleet(8, 1, 300)
    dense, _ = sw.shift_table(o["knots"], o["tstatus"], c["radius"], c["group"], 8, 1, skip=False)
    assert np.array_equal(dense, o["table"])
    far = np.array([[0.0, 1.0, 0.0, 1.0], [np.inf, -np.inf, np.inf, -np.inf]])
    assert sw.gap2(far[0], far[1]) == np.inf and sw.gap2(far[1], far[1]) == np.inf and sw.gap2(far[0], far[0]) == 0.0


def brute_greedy(kn, ts, c, D, stride, order, jmax):
    """The schedule by its meaning: every candidate slot is tried by shifting the path absolutely and asking
    traj_twin.conflicts whether it meets one of the paths placed (and shifted) before it."""
    P = kn.shape[0]
    slot = np.full(P, sw.SLOT_UNNAMED, np.int32)
    rows = {}
    for p in (range(P) if order is None else order):
        if p < 0 or p >= P or slot[p] != sw.SLOT_UNNAMED:
            continue
        jm = D - 1 if jmax is None else jmax[p]
        if ts[p] != tw.TRAJ_OK:
            slot[p] = sw.SLOT_NOT_OK
            continue
        others = [q for q in rows if not (c["group"][q] >= 0 and c["group"][q] == c["group"][p])]
        found = sw.SLOT_UNRESOLVED
        for j in ([0] if jm < 0 else range(min(jm, D - 1) + 1)):
            row = sw.shifted(kn[p], [j * stride])[0]
            arr = np.stack([rows[q] for q in others] + [row])
            out = tw.conflicts(arr, np.zeros(len(arr), np.int32), c["T0"], c["dt_c"], np.append(c["radius"][others], c["radius"][p]),
                               np.array([0] * len(others) + [-1], np.int32))
            if jm < 0 or out["n_conf"][-1] == 0:
                found = j
                break
        slot[p] = found
        if found >= 0:
            rows[p] = sw.shifted(kn[p], [found * stride])[0]
    return slot


@pytest.mark.parametrize("variant", ["natural", "random_order", "pins_and_limits"])
def test_window_formula_equals_brute_force(variant):
    D, stride = 6, 8
    c = tc.random_fleet(seed=11, P=40, K=360, box=20.0)
    rng = np.random.default_rng(5)
    order = None if variant == "natural" else rng.permutation(40)
    jmax = rng.integers(-1, D + 2, 40) if variant == "pins_and_limits" else None
    o = run(c, D, stride, order=order, jmax=jmax)
    ok = o["tstatus"] == tw.TRAJ_OK
    assert sw.at_rest(o["knots"], D, stride)[ok].all()
    want = brute_greedy(o["knots"], o["tstatus"], c, D, stride, order, jmax)
    assert np.array_equal(o["slot"], want)
    assert (o["slot"] > 0).any() and (o["slot"] == -1).any() and (o["slot"] == 0).any()


# ---- arguments ----
def test_order_with_repeats_out_of_range_and_omissions():
    c, o, _ = fleet(8, 1, 300)
    T, ts = o["table"], o["tstatus"]
    P = len(ts)
    order = np.arange(P)[::-1].copy()
    order[3], order[4], order[5], order[6] = order[0], -1, P, 2 ** 31 - 1       # a repeat, three outside; paths P-4 .. P-7 are never named
    slot, counts = sw.schedule(T, ts, 8, order)
    assert (slot[[P - 4, P - 5, P - 6, P - 7]] == sw.SLOT_UNNAMED).all() and (slot[: P - 7] != sw.SLOT_UNNAMED).all()
    keep = [p for i, p in enumerate(order.tolist()) if i not in (3, 4, 5, 6)]
    full = np.array(keep + [keep[0]] * (P - len(keep)), np.int32)             # the same walk with the skipped entries as repeats at the end
    assert np.array_equal(sw.schedule(T, ts, 8, full)[0], slot)
    assert counts.sum() == P and counts[3] == 7 + 4 - int((ts[[P - 4, P - 5, P - 6, P - 7]] != 0).sum())


def test_jmax_zero_negative_and_large():
    c, o, _ = fleet(8, 1, 300)
    T, ts = o["table"], o["tstatus"]
    ok = ts == tw.TRAJ_OK
    s0, c0 = sw.schedule(T, ts, 8, jmax=np.zeros(len(ts), np.int32))
    assert set(s0[ok].tolist()) == {0, -1} and c0[1] == 0 and c0[2] > 0 and c0[0] + c0[2] == 123   # nobody may wait
    sp, cp = sw.schedule(T, ts, 8, jmax=np.full(len(ts), -5, np.int32))
    assert (sp[ok] == 0).all() and (sp[~ok] == sw.SLOT_NOT_OK).all() and cp.tolist() == [123, 0, 0, 7]
    sl, _ = sw.schedule(T, ts, 8, jmax=np.full(len(ts), 1000, np.int32))
    assert np.array_equal(sl, o["slot"])                                       # clamped to D - 1


def test_one_slot():
    c = tc.random_fleet()
    o = run(c, 1)
    m = tw.conflicts(o["knots"], o["tstatus"], c["T0"], c["dt_c"], c["radius"], c["group"])
    assert set(np.unique(o["table"]).tolist()) == {0, 1} and o["table"].sum() == m["n_conf"].sum() == 280
    assert o["counts"][1] == 0 and o["counts"][2] > 0 and np.array_equal(tc.bits(o["knots_out"][o["slot"] == 0]), tc.bits(o["knots"][o["slot"] == 0]))
