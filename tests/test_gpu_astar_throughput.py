"""GPU parity of the throughput build of the two-wavefront A* kernel with MORE QUERIES THAN SLOTS against the CPU oracle:
status, cost, length, path and the number of nodes every search expanded.

Every case runs 256 queries through FOUR slots (SC_ASTAR_DUAL=4, SC_ASTAR_LATENCY=0), so a slot serves 64 searches one
after the other: the queue order (longest predicted search first), wavefront 1's lazy hand-over and the reuse of a slot's
g array, bitmap and rings -- whose g bytes are stored non-temporally in this build and never cleared -- are all exercised.
Every case creates its own Context after the environment is set (the library reads it when a context first runs A*)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = {"SC_ASTAR_LATENCY": "0", "SC_ASTAR_DUAL": "4"}
GRIDS = {"40x28": (40, 28, 0.1, 1), "64x64": (64, 64, 0.25, 2), "97x61": (97, 61, 0.33, 3)}


def _context(monkeypatch, env):
    import torch
    import sea_current_amd as sc
    assert torch.cuda.is_available()
    for k in ("SC_ASTAR_LATENCY", "SC_ASTAR_DUAL", "SC_ASTAR_CAP", "SC_ASTAR_SLOT_GB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return sc.Context(0)


def _octile(s, g, W):
    dx, dy = np.abs(s % W - g % W), np.abs(s // W - g // W)
    return 10 * np.maximum(dx, dy) + 4 * np.minimum(dx, dy)


def _walled_grid(W, H, p, seed):
    """The suite's salt grid with one free cell walled in by its eight neighbours (traversable, unreachable)."""
    from sea_current_amd import synth
    occ = synth.salt_grid(W, H, p, seed=seed)
    cx, cy = W // 2, H // 2
    occ[cy - 1:cy + 2, cx - 1:cx + 2] = 1
    occ[cy, cx] = 0
    return occ, cy * W + cx


@functools.lru_cache(maxsize=None)
def _case(name):
    """(d2, start, goal) of a grid: 256 queries, long and short searches alternating, special ones spread among them."""
    from oracle import oracle
    from sea_current_amd import synth
    oracle.build()
    W, H, p, seed = GRIDS[name]
    occ, cell = _walled_grid(W, H, p, seed)
    d2 = oracle.edt(occ)
    trav = d2 >= 1
    s, g = synth.queries(trav, 232, seed=seed)
    order = np.argsort(-_octile(s, g, W), kind="stable")
    alt = np.empty(232, np.int64)
    alt[0::2], alt[1::2] = order[:116], order[:115:-1]          # longest, shortest, second longest, second shortest, ..
    s, g = s[alt], g[alt]
    rng = np.random.default_rng(seed)
    free = np.flatnonzero(trav.ravel()).astype(np.int32)
    occd = np.flatnonzero(occ.ravel()).astype(np.int32)
    far = free[np.argsort(-_octile(free, np.full_like(free, cell), W))[:8]]
    sp_s = np.concatenate([far[:6], [cell, cell],                              # walled-off goals (the whole component is searched: no path, no scatter), walled-off starts
                           free[[0, 5, -1, len(free) // 2]],                   # start == goal
                           [-1, W * H, occd[0], free[3]],                      # bad end points
                           rng.choice(free, 8)]).astype(np.int32)              # any two free cells (other components included)
    sp_g = np.concatenate([np.full(6, cell), [far[6], far[7]],
                           free[[0, 5, -1, len(free) // 2]],
                           [free[1], free[2], free[4], occd[1]],
                           rng.choice(free, 8)]).astype(np.int32)
    at = np.arange(24) * 9 + 3                                            # among the alternating ones, not at the end
    s = np.insert(s, at, sp_s).astype(np.int32)
    g = np.insert(g, at, sp_g).astype(np.int32)
    assert s.shape[0] == 256
    return d2, s, g


@functools.lru_cache(maxsize=None)
def _reference(name, Lmax):
    from oracle import oracle
    d2, s, g = _case(name)
    return oracle.astar_batch(d2, s, g, Lmax=Lmax, nthreads=8)


def _compare(got, ref):
    for k in ("status", "cost", "len", "expanded"):
        assert np.array_equal(got[k], ref[k]), (k, np.flatnonzero(got[k] != ref[k])[:8])
    Lmax = got["path"].shape[1]
    for q in np.flatnonzero(ref["status"] == 0):
        L = ref["len"][q]
        assert L <= Lmax and np.array_equal(got["path"][q, :L], ref["path"][q, :L]), q


def _run(c, d2, s, g, Lmax):
    import torch
    out = c.astar_batch(torch.from_numpy(d2).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda(), Lmax=Lmax)
    c.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["expanded"] = c.astar_debug_stats(s.shape[0])[0]
    return got


@pytest.mark.parametrize("name", list(GRIDS))
def test_throughput_matches_oracle(monkeypatch, name):
    """Alternating long and short searches, walled-off goals, start == goal and bad end points on four slots; a second call
    on the same context and slots must give the same again."""
    d2, s, g = _case(name)
    ref = _reference(name, 512)
    assert {0, 1, 2} <= set(np.unique(ref["status"]))
    c = _context(monkeypatch, ENV)
    try:
        _compare(_run(c, d2, s, g, 512), ref)
        _compare(_run(c, d2, s, g, 512), ref)
    finally:
        c.close()


@pytest.mark.parametrize("name", list(GRIDS))
def test_throughput_lmax_truncation(monkeypatch, name):
    """Lmax shorter than the long paths: those report SC_Q_TRUNCATED with the length needed, the short ones their path."""
    d2, s, g = _case(name)
    ref = _reference(name, 24)
    assert (ref["status"] == 3).any() and (ref["status"] == 0).any()
    c = _context(monkeypatch, ENV)
    try:
        _compare(_run(c, d2, s, g, 24), ref)
    finally:
        c.close()


def test_throughput_multi_grid_launch(monkeypatch):
    """One launch over three grids (astar_batch_multi): every query against the oracle on its own grid."""
    import torch
    from oracle import oracle
    from sea_current_amd import synth
    oracle.build()
    W = H = 64
    d2s = [oracle.edt(_walled_grid(W, H, p, seed)[0]) for p, seed in ((0.1, 11), (0.25, 12), (0.33, 13))]
    ss, gs, qg = [], [], []
    for k, d2 in enumerate(d2s):
        s, g = synth.queries(d2 >= 1, (86, 85, 85)[k], seed=20 + k)
        ss.append(s); gs.append(g); qg.append(np.full(s.shape[0], k, np.int32))
    s, g, qgrid = np.concatenate(ss), np.concatenate(gs), np.concatenate(qg)
    s[::37] = (H // 2) * W + W // 2                                  # walled-off starts: no path on every grid
    perm = np.random.default_rng(1).permutation(256)                 # the grids' queries interleaved
    s, g, qgrid = s[perm], g[perm], qgrid[perm]
    c = _context(monkeypatch, ENV)
    try:
        out = c.astar_batch_multi(torch.from_numpy(np.stack(d2s)).cuda(), torch.from_numpy(qgrid).cuda(), torch.from_numpy(s).cuda(),
                                  torch.from_numpy(g).cuda(), Lmax=512)
        c.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got["expanded"] = c.astar_debug_stats(256)[0]
    finally:
        c.close()
    for k, d2 in enumerate(d2s):
        sel = np.flatnonzero(qgrid == k)
        ref = oracle.astar_batch(d2, s[sel], g[sel], Lmax=512, nthreads=4)
        _compare({kk: vv[sel] for kk, vv in got.items()}, ref)


def test_throughput_ring_overflow_retry(monkeypatch):
    """Rings of 1024 entries per level on a 5 % map of 256^2: the wide searches overflow and are rerun by the one-wavefront
    retry pass in a slot that earlier searches of the two-wavefront kernel used; every query still equals the oracle."""
    import ctypes as C
    from oracle import oracle
    from sea_current_amd import synth
    oracle.build()
    occ = synth.salt_grid(256, 256, 0.05, seed=5)
    d2 = oracle.edt(occ)
    s, g = synth.queries(d2 >= 1, 256, seed=6)
    ref = oracle.astar_batch(d2, s, g, Lmax=1024, nthreads=8)
    c = _context(monkeypatch, dict(ENV, SC_ASTAR_CAP="1024"))
    try:
        got = _run(c, d2, s, g, 1024)
        buf = (C.c_int32 * 16)()
        c._l.sc_astar_debug_peek(c._h, buf)
        assert buf[1] > 0, "the small rings were expected to overflow in the first launch"
        assert buf[3] == 0
    finally:
        c.close()
    _compare(got, ref)
