"""The range-scan definitions on the CPU: the NumPy twin (tests/scan_twin.py) against the C statement (tests/cpp/scan_ref.c) in
hit, Lout, occ_est and known; the walk as a set against the brute-force supercover, its order, the corner rule; hit = -1 <=>
Clear; fan coverage; soundness of cast -> update; the update rules; every ignored kind and ends outside the grid; the door
map's recorded figures; the exploration loop with a log-odds map; the C statement under AddressSanitizer and UBSan as a
program of its own, and the walker the kernels run (csrc/ray_walk.h) compiled for the host against the C statement.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import frontier_twin as ft
import scan_twin as st
import views_twin as vt
from field_twin import Twin as FieldTwin

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = os.path.join(HERE, "cpp", "scan_ref_check.c")
WALK_CHECK = os.path.join(HERE, "cpp", "scan_walk_check.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "sea-current_amd", "csrc")
P = dict(l_hit=5, l_miss=3, l_clamp=8, t_occ=5, t_free=3)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return st.Ref(tmp_path_factory.mktemp("scan_ref"))


@pytest.fixture(scope="module")
def fields(tmp_path_factory):
    return FieldTwin(tmp_path_factory.mktemp("field_ref"))


def _line():
    line = np.zeros((1, 200), np.uint8)
    line[0, [80, 150]] = 1
    return line


def _maps():
    return {"salt0.05": vt.salt(130, 70, 0.05, 2), "blocks": vt.blocks(), "door": vt.door_map(), "row": _line(),
            "column": np.ascontiguousarray(_line().T)}


NAMES = ["salt0.05", "blocks", "door", "row", "column"]


def _free_near(occ, x, y):
    H, W = occ.shape
    free = np.flatnonzero(occ.ravel() == 0)
    c = int(free[np.argmin((free % W - x) ** 2 + (free // W - y) ** 2)])
    return c % W, c // W


def odd_rays(W, H, x, y):
    """From the free cell (x, y): length 0, every ignored kind (origin outside on each side, reach exceeded in x and y, int32
    extremes), the reach limit itself, and ends beyond each side and each corner of the grid."""
    R = st.MAX_REACH
    ignored = [(-1, y, x, y), (W, y, x, y), (x, -1, x, y), (x, H, x, y), (x, y, x + R + 1, y), (x, y, x, y - R - 1),
               (x, y, 2**31 - 1, -2**31), (-2**31, 2**31 - 1, x, y)]
    outside = [(x, y, -5, y), (x, y, W + 4, y), (x, y, x, -3), (x, y, x, H + 6), (x, y, -4, -7), (x, y, W + 9, -2), (x, y, -3, H + 8),
               (x, y, W + 5, H + 5), (x, y, W, H), (x, y, -1, -1), (x, y, x + R, y + R), (x, y, x - R, y + 3)]
    return np.array([(x, y, x, y)] + ignored + outside, np.int32), 1 + np.arange(len(ignored))


def _rays_for(occ, seed=0):
    """Two fans (one clipped by the grid on two sides), the odd rays, and random rays with ends inside and outside."""
    H, W = occ.shape
    x, y = _free_near(occ, W // 2, H // 2)
    cx, cy = _free_near(occ, 2, 1)
    rng = np.random.default_rng(seed)
    n = 120
    o = np.flatnonzero(occ.ravel() == 0)[rng.integers(0, (occ == 0).sum(), n)]
    rnd = np.stack([o % W, o // W, rng.integers(-20, W + 20, n), rng.integers(-20, H + 20, n)], 1)
    blocked = np.flatnonzero(occ.ravel() != 0)[:2]
    on_obstacle = np.stack([blocked % W, blocked // W, blocked % W + 5, blocked // W], 1).reshape(-1, 4)
    return np.concatenate([st.square_fan(x, y, 40), st.square_fan(cx, cy, 17), odd_rays(W, H, x, y)[0], rnd, on_obstacle]).astype(np.int32)


# ---- twin == C statement ----
@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_c_statement(ref, name):
    occ = _maps()[name]
    H, W = occ.shape
    rays = _rays_for(occ)
    hit = st.cast(occ, rays)
    assert np.array_equal(hit, ref.cast(occ, rays))
    assert (hit >= 0).any() and (hit == st.NO_RETURN).any() and (hit == st.IGNORED).any()
    rng = np.random.default_rng(5)
    L0 = rng.integers(-12, 13, (H, W)).astype(np.int32)                # some of it outside the clamp
    for L in (None, L0):
        for h in (hit, np.where(hit >= 0, st.NO_RETURN, hit)):         # the cast's, and every beam a no-return
            want = st.update(L, rays, h, W, H, **P)
            got = ref.update(L, rays, h, W, H, **P)
            for a, b, k in zip(got, want, ("Lout", "occ_est", "known")):
                assert a.dtype == b.dtype and np.array_equal(a, b), (name, k)
    assert want[1].max() <= 1 and want[2].max() <= 1


# ---- the walk ----
def _touches_at_a_corner_only(ax, ay, bx, by, x, y):
    """The closed unit square of cell (x, y) meets the line through the centres of a and b in a corner and nowhere else: in
    doubled coordinates one corner has cross product 0 and the other three lie strictly on one side."""
    ux, uy = 2 * (bx - ax), 2 * (by - ay)
    s = [ux * (py - 2 * ay) - uy * (px - 2 * ax) for px in (2 * x - 1, 2 * x + 1) for py in (2 * y - 1, 2 * y + 1)]
    return s.count(0) == 1 and (all(v >= 0 for v in s) or all(v <= 0 for v in s))


def test_walk_is_the_supercover_in_order(ref):
    """Over every ray of 40 random origins, to every cell of the grid and of a margin of three cells around it: as a set the
    unbounded walk equals the brute-force supercover; its order is columns ascending, then rows away from a; the C statement
    walks the same sequence.  With the end outside the grid the walk is that sequence cut at its first cell outside, a subset
    of the supercover clipped to the grid, and every cell it leaves out comes after that cut in the sequence: a cell the
    segment only touches at a corner after it has left the grid."""
    W, H = 17, 13
    rng = np.random.default_rng(11)
    cut = 0
    for _ in range(40):
        ax, ay = int(rng.integers(0, W)), int(rng.integers(0, H))
        for bx in range(-3, W + 3):
            for by in range(-3, H + 3):
                inside = 0 <= bx < W and 0 <= by < H
                cells = st.walk((ax, ay, bx, by), W, H)
                assert cells == ref.walk((ax, ay, bx, by), W, H)
                seq = list(st.walk_unbounded(ax, ay, bx, by))
                brute = st.supercover_bruteforce(ax, ay, bx, by)
                assert len(set(seq)) == len(seq) and set(seq) == brute
                # order: the major coordinate never steps back, inside a column the minor one moves away from a
                xmajor = abs(bx - ax) >= abs(by - ay)
                maj = [abs((x - ax) if xmajor else (y - ay)) for x, y in seq]
                mnr = [abs((y - ay) if xmajor else (x - ax)) for x, y in seq]
                assert all(maj[k + 1] == maj[k] and mnr[k + 1] == mnr[k] + 1 or maj[k + 1] == maj[k] + 1 for k in range(len(seq) - 1))
                assert seq[0] == (ax, ay) and seq[-1] == (bx, by)
                if inside:
                    assert [y * W + x for x, y in seq] == cells
                else:
                    first_out = next(k for k, (x, y) in enumerate(seq) if not (0 <= x < W and 0 <= y < H))
                    assert cells == [y * W + x for x, y in seq[:first_out]]
                    clipped = {y * W + x for x, y in brute if 0 <= x < W and 0 <= y < H}
                    assert set(cells) <= clipped
                    behind = {y * W + x for x, y in seq[first_out + 1:] if 0 <= x < W and 0 <= y < H}
                    assert clipped - set(cells) == behind              # nothing is left out but what lies behind the cut
                    for c in behind:                                   # and that is a corner touch: the square meets the
                        x, y = c % W, c // W                           # segment in exactly one point, a corner of the square
                        assert _touches_at_a_corner_only(ax, ay, bx, by, x, y)
                    cut += len(behind)
    assert cut > 0                                                     # the corner case does occur


def test_corner_rule_and_its_order():
    """From (4,4) towards (6,6): the ray passes the corner between (5,4) and (4,5) and either blocks it.  With both occupied
    the hit is (4,5): it is the second row of column 0, and column 0 comes before column 1, which holds (5,4)."""
    ray = [(4, 4, 6, 6)]
    assert st.walk(ray[0], 9, 9) == [4 * 9 + 4, 5 * 9 + 4, 4 * 9 + 5, 5 * 9 + 5, 6 * 9 + 5, 5 * 9 + 6, 6 * 9 + 6]
    assert st.cast(vt.corner_map([]), ray)[0] == st.NO_RETURN
    assert st.cast(vt.corner_map([(5, 4)]), ray)[0] == 4 * 9 + 5
    assert st.cast(vt.corner_map([(4, 5)]), ray)[0] == 5 * 9 + 4
    assert st.cast(vt.corner_map([(5, 4), (4, 5)]), ray)[0] == 5 * 9 + 4


# ---- consequences ----
@pytest.mark.parametrize("name", ["salt0.05", "blocks", "door"])
def test_no_return_is_clear(name):
    occ = _maps()[name]
    H, W = occ.shape
    rng = np.random.default_rng(7)
    free = np.flatnonzero(occ.ravel() == 0)
    a = free[rng.integers(0, len(free), 300)]
    b = rng.integers(0, W * H, 300)
    rays = np.stack([a % W, a // W, b % W, b // W], 1)
    hit = st.cast(occ, rays)
    clear = [vt.clear(occ, *r) for r in rays.tolist()]
    assert [h == st.NO_RETURN for h in hit.tolist()] == [bool(c) for c in clear]
    assert any(clear) and not all(clear)
    for r in rays[:40].tolist():
        assert bool(vt.clear_bruteforce(occ, *r)) == bool(vt.clear(occ, *r))


@pytest.mark.parametrize("cx,cy", [(20, 20), (3, 2)])
def test_fan_covers_its_square(cx, cy):
    W = H = 41
    rays = st.square_fan(cx, cy, 13)
    assert rays.shape == (104, 4) and len({tuple(r) for r in rays.tolist()}) == 104
    assert (np.abs(rays[:, 2:] - rays[:, :2]).max(1) == 13).all()
    hit = st.cast(np.zeros((H, W), np.uint8), rays)
    assert (hit == st.NO_RETURN).all()
    miss, hitmap = st.marks(rays, hit, W, H)
    want = np.zeros((H, W), bool)
    want[max(cy - 13, 0):cy + 14, max(cx - 13, 0):cx + 14] = True
    assert np.array_equal(miss, want) and not hitmap.any()


@pytest.mark.parametrize("name", ["salt0.05", "blocks", "door"])
def test_cast_then_update_is_sound(name):
    occ = _maps()[name]
    H, W = occ.shape
    rays = _rays_for(occ, seed=3)
    hit = st.cast(occ, rays)
    miss, hitmap = st.marks(rays, hit, W, H)
    assert (occ[miss] == 0).all() and (occ[hitmap] != 0).all() and miss.any() and hitmap.any()
    L, occ_est, known = st.update(None, rays, hit, W, H, **st.LOOP_PARAMS)
    assert st.sound(occ, occ_est, known)
    assert np.array_equal(known != 0, miss | hitmap) and np.array_equal(occ_est != 0, hitmap)


# ---- the update rules ----
RULE_RAYS = [(0, 0, 7, 0), (0, 0, 5, 0), (0, 0, 7, 0), (1, 0, 3, 0)]
RULE_HIT = [-1, 3, 3, -2]       # beam 0 misses cell 3, beams 1 and 2 hit it, beam 3 is ignored


def test_hit_wins_and_one_update_per_cell():
    L, occ_est, known = st.update(None, RULE_RAYS, RULE_HIT, 8, 1, **P)
    assert L.tolist() == [[-3, -3, -3, 5, -3, -3, -3, -3]]
    assert occ_est.tolist() == [[0, 0, 0, 1, 0, 0, 0, 0]] and known.all()
    # the order of the beams does not matter
    assert np.array_equal(st.update(None, RULE_RAYS[::-1], RULE_HIT[::-1], 8, 1, **P)[0], L)
    # two calls count twice
    assert st.update(L, RULE_RAYS[:1], [-1], 8, 1, **dict(P, l_clamp=100))[0].tolist() == [[-6, -6, -6, 2, -6, -6, -6, -6]]


def test_clamping_and_a_map_outside_the_clamp(ref):
    L0 = np.array([[100, -100, 7, 7, -8, 0, 2**31 - 1, -2**31]], np.int32)
    L, occ_est, known = st.update(L0, RULE_RAYS, RULE_HIT, 8, 1, **P)
    assert L.tolist() == [[8, -8, 4, 8, -8, -3, 8, -8]]
    assert occ_est.tolist() == [[1, 0, 0, 1, 0, 0, 1, 0]] and known.tolist() == [[1, 1, 0, 1, 1, 1, 1, 1]]
    got = ref.update(L0, RULE_RAYS, RULE_HIT, 8, 1, **P)
    assert np.array_equal(got[0], L) and np.array_equal(got[1], occ_est) and np.array_equal(got[2], known)
    # the largest parameters: the sum is taken in 64 bits
    big = dict(l_hit=2**31 - 1, l_miss=2**31 - 1, l_clamp=2**30, t_occ=2**31 - 1, t_free=2**31 - 1)
    a, b = st.update(L0, RULE_RAYS, RULE_HIT, 8, 1, **big), ref.update(L0, RULE_RAYS, RULE_HIT, 8, 1, **big)
    assert a[0].tolist() == [[-2**30, -2**30, -2**30, 2**30, -2**30, -2**30, 0, -2**30]]
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not a[1].any() and not a[2].any()


def test_fresh_map_in_place_and_no_beams(ref):
    occ = _maps()["blocks"]
    H, W = occ.shape
    rays = _rays_for(occ)
    hit = st.cast(occ, rays)
    fresh = ref.update(None, rays, hit, W, H, **P)
    zeros = ref.update(np.zeros((H, W), np.int32), rays, hit, W, H, **P)
    assert all(np.array_equal(a, b) for a, b in zip(fresh, zeros))     # L = NULL is a map of zeros
    again = st.update(fresh[0], rays, hit, W, H, **P)
    inpl = ref.update(fresh[0], rays, hit, W, H, in_place=True, **P)
    assert all(np.array_equal(a, b) for a, b in zip(again, inpl))      # in place
    # N = 0: the stored map -> masks, clamped
    stored = np.arange(-10, 10, dtype=np.int32).reshape(2, 10)
    for twin_or_c in (st.update, ref.update):
        L, occ_est, known = twin_or_c(stored, np.zeros((0, 4), np.int32), np.zeros(0, np.int32), 10, 2, **P)
        assert np.array_equal(L, np.clip(stored, -8, 8))
        assert np.array_equal(occ_est, (stored >= 5).astype(np.uint8)) and np.array_equal(known, ((stored >= 5) | (stored <= -3)).astype(np.uint8))


# ---- edge cases ----
def test_ignored_beams_and_ends_outside(ref):
    occ = vt.blocks()
    H, W = occ.shape
    x, y = _free_near(occ, W // 2, H // 2)
    rays, ignored = odd_rays(W, H, x, y)
    hit = st.cast(occ, rays)
    assert np.array_equal(hit, ref.cast(occ, rays))
    assert hit[0] == st.NO_RETURN                                      # length 0 on a free cell
    assert (hit[ignored] == st.IGNORED).all() and (np.delete(hit, ignored) != st.IGNORED).all()
    bx, by = np.flatnonzero(occ.ravel() != 0)[0] % W, np.flatnonzero(occ.ravel() != 0)[0] // W
    assert st.cast(occ, [(bx, by, bx, by), (bx, by, x, y)]).tolist() == [st.IGNORED, st.IGNORED]    # the sensor on an obstacle
    # an ignored beam changes nothing: not by its ray, not by hit = -2
    base = st.update(None, rays, hit, W, H, **P)
    live = np.delete(np.arange(len(rays)), ignored)
    assert all(np.array_equal(a, b) for a, b in zip(base, st.update(None, rays[live], hit[live], W, H, **P)))
    forced = np.where(np.arange(len(rays)) % 2 == 0, st.IGNORED, hit)
    keep = forced != st.IGNORED
    assert all(np.array_equal(a, b) for a, b in zip(st.update(None, rays, forced, W, H, **P), st.update(None, rays[keep], forced[keep], W, H, **P)))
    # on a free grid an end outside misses the cells up to the edge and nothing else
    miss, hitmap = st.marks(rays, np.where(hit == st.IGNORED, hit, st.NO_RETURN), W, H)
    assert miss[y, :x + 1].all() and miss[y, x:].all() and miss[:y + 1, x].all() and miss[y:, x].all() and not hitmap.any()


def test_a_hit_cell_off_the_walk(ref):
    ray, h = [(0, 0, 7, 0)], [8 + 5]
    for f in (st.update, ref.update):
        L = f(None, ray, h, 8, 2, **P)[0]
        assert L.tolist() == [[-3] * 8, [0, 0, 0, 0, 0, 5, 0, 0]]
    # a hit on the walk stops the misses there; the cells behind it stay untouched
    assert st.update(None, ray, [6], 8, 1, **P)[0].tolist() == [[-3, -3, -3, -3, -3, -3, 5, 0]]
    # a hit at the origin: no miss at all
    assert st.update(None, ray, [0], 8, 1, **P)[0].tolist() == [[5, 0, 0, 0, 0, 0, 0, 0]]
    # the device form's rule for a hit out of range, which the twin and the C statement share: the beam is ignored
    for bad in (-3, 16):
        assert not st.update(None, ray, [bad], 8, 2, **P)[0].any() and not ref.update(None, ray, [bad], 8, 2, **P)[0].any()


# ---- recorded figures ----
def test_door_map_figures():
    occ = vt.door_map()
    H, W = occ.shape
    rays = st.square_fan(20, 31, 60)
    hit = st.cast(occ, rays)
    miss, hitmap = st.marks(rays, hit, W, H)
    assert (len(rays), int((hit >= 0).sum()), int((hit == st.NO_RETURN).sum())) == (480, 130, 350)
    assert (int(miss.sum()), int(hitmap.sum())) == (3255, 61)
    assert int(hitmap[:, 48].sum()) == 61 == int((occ[:, 48] != 0).sum())                           # every wall cell of column 48
    assert int(miss[:, 49:].sum()) == 180                                                           # seen through the door


# ---- the exploration loop ----
@pytest.mark.parametrize("name,iterations", [("blocks96x80", 208), ("rooms96x80", 100)])
def test_exploration_ends_with_the_component_known(oracle, fields, name, iterations):
    occ = vt.loop_maps()[name]
    start = ft.loop_start(occ)
    goals, known, L = st.explore_loop_scan(occ, start, ft.twin_step(oracle, fields))
    comp = ft.true_component(occ, start)
    assert len(set(goals)) == len(goals)
    assert (known[comp] != 0).all() and comp.ravel()[goals].all()
    assert np.abs(L).max() <= st.LOOP_PARAMS["l_clamp"] and (L[occ != 0] >= 0).all() and (L[occ == 0] <= 0).all()
    assert len(goals) == iterations


# ---- programs of their own under the sanitizers ----
SAN = ["-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _clean(r, last):
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(last) and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr


def test_check_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "scan_ref_check")
    subprocess.check_call(["cc", "-std=c11"] + SAN + ["-o", exe, CHECK, st.SRC])
    _clean(subprocess.run([exe], capture_output=True, text=True, timeout=300), "scan_ref OK")


def test_device_walker_on_the_host_equals_the_c_statement(tmp_path):
    obj, exe = str(tmp_path / "scan_ref.o"), str(tmp_path / "scan_walk_check")
    subprocess.check_call(["cc", "-std=c11"] + SAN + ["-c", "-o", obj, st.SRC])
    subprocess.check_call(["c++", "-std=c++17"] + SAN + ["-I", CSRC, "-o", exe, WALK_CHECK, obj])
    _clean(subprocess.run([exe], capture_output=True, text=True, timeout=300), "scan_walk OK")
