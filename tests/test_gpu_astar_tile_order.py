"""GPU parity of the tile-ordered refill of the throughput build of the two-wavefront A* kernel against the CPU oracle:
status, cost, length, path and the number of nodes every search expanded, query by query.

When a level's refill chunk holds more than 64 entries, the throughput build (SC_ASTAR_LATENCY=0) writes it into the LDS
ring grouped by the closed-bitmap tile of its nodes (32 x 16 cells, row and column modulo 8).  The order of pops inside a
level is free, so nothing the oracle pins may move.  The suite's small grids have levels of at most a few dozen entries and
never reach that code; the maps here do, and every case says so with a host count before it runs:

  the CPU model of the step loop (tools/astar_lines_model.py: rings, chunks, steps, same-f appends, pruning tables) gives
  the number of entries every level takes from its HBM ring; its expansion counts equal the oracle's on these queries.

Every case creates its own Context after the environment is set (the library reads it when a context first runs A*)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = {"SC_ASTAR_LATENCY": "0"}
CQ, REFILL = 1024, 512          # the throughput build's LDS ring and refill chunk


def _context(monkeypatch, env):
    import torch
    import sea_current_amd as sc
    assert torch.cuda.is_available()
    for k in ("SC_ASTAR_LATENCY", "SC_ASTAR_DUAL", "SC_ASTAR_CAP", "SC_ASTAR_SLOT_GB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return sc.Context(0)


def _model():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "astar_lines_model.py")
    spec = importlib.util.spec_from_file_location("astar_lines_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


LEVEL_F = {}     # (case, query) -> f of every level, beside the sizes _case() returns


def level_sizes(name, q, mv, W, H, s, g, expanded):
    """Entries every level of the search s -> g takes from its HBM ring, in rising f (model)."""
    r = _model().simulate(mv, W, H, s, g, order="bin")
    assert r["expanded"] == expanded          # the model expands the oracle's E
    LEVEL_F[(name, q)] = r["level_f"]
    return np.array(r["levels"])


def _corner_queries(d2, n, seed, box=40):
    """n queries from the top-left to the bottom-right corner region of the largest free component."""
    from sea_current_amd import synth
    H, W = d2.shape
    comp = synth.largest_component(d2 >= 1)
    ys, xs = np.nonzero(comp)
    a = np.flatnonzero((xs < box) & (ys < box))
    b = np.flatnonzero((xs >= W - box) & (ys >= H - box))
    rng = np.random.default_rng(seed)
    ia, ib = rng.choice(a, n), rng.choice(b, n)
    return (ys[ia] * W + xs[ia]).astype(np.int32), (ys[ib] * W + xs[ib]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(d2, start, goal, reference, level sizes of the probed queries) of a map; 64 queries each."""
    from oracle import oracle
    from sea_current_amd import synth
    oracle.build()
    if name in ("salt20", "ragged", "long"):
        # 320 x 192 at 20 % salt; `ragged` cuts 5 columns and 3 rows off: W no multiple of 32, H none of 16, 10 tiles wide;
        # `long` is twice as wide: twice the levels per search, so every HBM ring is used four to six times
        W, H = {"salt20": (320, 192), "ragged": (315, 189), "long": (640, 192)}[name]
        d2 = oracle.edt(np.ascontiguousarray(synth.salt_grid(32 * ((W + 31) // 32), 192, 0.20, seed=7)[:H, :W]))
        s, g = _corner_queries(d2, 64, seed=8)
        probe = (0, 63)
    else:
        # 512 x 320 at 8 % salt: query 0 runs edge to edge, its widest level is larger than the LDS ring
        W, H = 512, 320
        d2 = oracle.edt(synth.salt_grid(W, H, 0.08, seed=9))
        s, g = synth.queries(d2 >= 1, 64, seed=10)
        comp = synth.largest_component(d2 >= 1)
        assert comp[H // 2, 1] and comp[H // 3, W - 2]
        s[0], g[0] = (H // 2) * W + 1, (H // 3) * W + W - 2
        probe = (0,)
    mv = oracle.moves(d2).ravel().tolist()
    ref = oracle.astar_batch(d2, s, g, Lmax=1024, nthreads=8)
    assert (ref["status"] == 0).all()
    return d2, s, g, ref, {q: level_sizes(name, q, mv, W, H, int(s[q]), int(g[q]), int(ref["expanded"][q])) for q in probe}


def _compare(got, ref):
    for k in ("status", "cost", "len", "expanded"):
        assert np.array_equal(got[k], ref[k]), (k, np.flatnonzero(got[k] != ref[k])[:8])
    Lmax = got["path"].shape[1]
    for q in np.flatnonzero(ref["status"] == 0):
        L = ref["len"][q]
        assert L <= Lmax and np.array_equal(got["path"][q, :L], ref["path"][q, :L]), q


def _run(monkeypatch, env, d2, s, g, Lmax=1024):
    import ctypes as C
    import torch
    c = _context(monkeypatch, env)
    try:
        out = c.astar_batch(torch.from_numpy(d2).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda(), Lmax=Lmax)
        c.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got["expanded"] = c.astar_debug_stats(s.shape[0])[0]
        buf = (C.c_int32 * 16)()
        c._l.sc_astar_debug_peek(c._h, buf)
        got["overflowed"] = int(buf[1])
    finally:
        c.close()
    return got


@pytest.mark.parametrize("name", ["salt20", "ragged"])
def test_levels_of_one_binned_chunk(monkeypatch, name):
    """Levels of 65 .. 512 entries: one binned chunk per level (the model: 49 to 64 such levels in the two queries it runs, the
    largest 285 to 323 entries).  `ragged`: tiles cut by the right and lower border, and tiles 8 apart (columns 0 and 8, 1 and 9) in
    one bin."""
    d2, s, g, ref, levels = _case(name)
    assert d2.shape[1] > 8 * 32
    if name == "ragged":
        assert d2.shape[1] % 32 and d2.shape[0] % 16
    for q, lv in levels.items():
        assert ((lv > 64) & (lv <= REFILL)).sum() >= 32, (q, lv.max())      # a binned chunk for every HBM ring at least
    got = _run(monkeypatch, ENV, d2, s, g)
    assert got["overflowed"] == 0
    _compare(got, ref)


def test_level_larger_than_the_lds_ring(monkeypatch):
    """A level of more than CQ entries: several chunks, the first ones full, and more entries than the LDS ring holds."""
    d2, s, g, ref, levels = _case("wide")
    assert levels[0].max() > CQ, levels[0].max()
    got = _run(monkeypatch, ENV, d2, s, g)
    assert got["overflowed"] == 0
    _compare(got, ref)


def _binned_chunks_across_ring_end(level_f, level_n, cap):
    """Chunks of more than 64 entries whose positions in their HBM ring of `cap` entries pass the ring's end, counted up
    to the first level that overflows such a ring (the search then ends and is run again by the retry pass)."""
    wraps, total = 0, {}
    for f, n in zip(level_f, level_n):
        if n > cap:
            break
        t0 = total.get(f & 31, 0)                      # the ring's position when the level's first entry arrives
        total[f & 31] = t0 + n
        for c0 in range(t0, t0 + n, REFILL):
            c1 = min(c0 + REFILL, t0 + n)
            if c1 - c0 > 64 and c0 // cap != (c1 - 1) // cap:
                wraps += 1
    return wraps


@pytest.mark.parametrize("name", ["salt20", "long"])
def test_hbm_rings_of_1024_entries(monkeypatch, name):
    """HBM rings of 1024 entries (SC_ASTAR_CAP=1024).  A ring serves every 32nd level and its positions run on, so a binned
    chunk straddles the ring's end when the entries the ring has taken pass a multiple of 1024 inside a level of more than
    64.  By the model the searches of the 320 x 192 map use a ring two or three times and stay below 1024 entries per ring:
    that case runs the small rings without a wrap.  The searches of `long` wrap, which the model must confirm.  Queries
    whose rings overflow would go through the retry pass; the results equal the oracle's either way."""
    d2, s, g, ref, levels = _case(name)
    for q, lv in levels.items():
        wraps = _binned_chunks_across_ring_end(LEVEL_F[(name, q)], lv.tolist(), 1024)
        if name == "long":
            assert wraps >= 1, (q, wraps)              # the model: 15 for query 0; query 63 overflows after its first
    _compare(_run(monkeypatch, dict(ENV, SC_ASTAR_CAP="1024"), d2, s, g), ref)


def test_more_queries_than_slots(monkeypatch):
    """64 searches through four slots: wavefront 1's lazy hand-over, and a slot's rings, bitmap and spare LDS words reused."""
    d2, s, g, ref, _ = _case("salt20")
    got = _run(monkeypatch, dict(ENV, SC_ASTAR_DUAL="4"), d2, s, g)
    assert got["overflowed"] == 0
    _compare(got, ref)
