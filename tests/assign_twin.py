"""NumPy twin of sc_assign_batch and sc_field_cost_matrix: the procedure of include/sea_current_hip.h verbatim (the eager form:
every delta is applied to u, v and minv in the pass that finds it), exact integers throughout.  The certificate proves a result
optimal without a reference.  Checker only: the library never imports it."""
import numpy as np

MAX_DIM = 1024
BIG = 1 << 42
INF = 2**31 - 1          # SC_FIELD_INF: forbidden
OK, BAD = 0, 1
SEED_COST_MAX = 1 << 24
_NONE = -1
_PINF = np.iinfo(np.int64).max


def padded(cost):
    """a[r][c]: the cost, SC_ASSIGN_BIG where forbidden (int64)."""
    a = np.asarray(cost).astype(np.int64)
    return np.where(a == INF, BIG, a)


def assign_one(cost):
    """One problem, cost int32 [R][C] -> dict(col_of [R], row_of [C], u int64 [R], v int64 [C], info int64 [4])."""
    cost = np.asarray(cost)
    R, C = cost.shape
    assert 1 <= R <= MAX_DIM and 1 <= C <= MAX_DIM
    out = dict(col_of=np.full(R, -1, np.int32), row_of=np.full(C, -1, np.int32), u=np.zeros(R, np.int64), v=np.zeros(C, np.int64),
               info=np.zeros(4, np.int64))
    if (cost < 0).any():
        out["info"][3] = BAD
        return out
    swap = R > C
    a = padded(cost.T if swap else cost)
    n, m = a.shape
    u, v, p = np.zeros(n, np.int64), np.zeros(m, np.int64), np.full(m, _NONE, np.int64)
    steps = 0
    for i in range(n):
        minv, way, used = np.full(m, _PINF, np.int64), np.full(m, _NONE, np.int64), np.zeros(m, bool)
        i0, j0 = i, _NONE
        while True:
            steps += 1
            free = ~used
            cur = a[i0] - u[i0] - v
            better = free & (cur < minv)
            minv[better] = cur[better]
            way[better] = j0
            j1 = int(np.argmin(np.where(free, minv, _PINF)))   # argmin returns the lowest index among equals
            delta = minv[j1]
            u[i] += delta
            u[p[used]] += delta
            v[used] -= delta
            minv[free] -= delta
            used[j1] = True
            j0 = j1
            if p[j0] == _NONE:
                break
            i0 = p[j0]
        while True:
            j1 = way[j0]
            p[j0] = i if j1 == _NONE else p[j1]
            j0 = j1
            if j0 == _NONE:
                break
    line_of = p.astype(np.int32)                                # every line is paired (n <= m); posts may be free
    posts = np.flatnonzero(line_of >= 0)
    real = a[line_of[posts], posts] != BIG
    post_pair = np.full(m, -1, np.int32)
    post_pair[posts[real]] = line_of[posts[real]]
    line_pair = np.full(n, -1, np.int32)
    line_pair[line_of[posts[real]]] = posts[real]
    total = int(a[line_of[posts[real]], posts[real]].sum())
    if swap:
        out.update(col_of=post_pair, row_of=line_pair, u=v, v=u)
    else:
        out.update(col_of=line_pair, row_of=post_pair, u=u, v=v)
    out["info"][:] = (int(real.sum()), total, steps, OK)
    return out


def assign(cost):
    """cost int32 [B][R][C] (or [R][C]: B = 1) -> the five arrays with a leading B."""
    cost = np.asarray(cost)
    if cost.ndim == 2:
        cost = cost[None]
    outs = [assign_one(c) for c in cost]
    return {k: np.stack([o[k] for o in outs]) for k in ("col_of", "row_of", "u", "v", "info")} if outs else None


def certificate(cost, out):
    """Asserts, in exact integers, that `out` (one problem) is a matching of the most pairs and, among those, the smallest sum."""
    cost = np.asarray(cost)
    R, C = cost.shape
    col_of, row_of = np.asarray(out["col_of"]).astype(np.int64), np.asarray(out["row_of"]).astype(np.int64)
    u, v = [int(x) for x in out["u"]], [int(x) for x in out["v"]]
    matched, total, steps, status = (int(x) for x in out["info"])
    assert status == OK and 0 <= steps <= min(R, C) * (min(R, C) + 1) // 2
    a = padded(cost)
    # a matching over real edges, col_of and row_of inverse to each other
    rows = np.flatnonzero(col_of >= 0)
    assert len(rows) == matched == int((row_of >= 0).sum())
    assert np.array_equal(row_of[col_of[rows]], rows) and len(set(col_of[rows].tolist())) == matched
    assert (a[rows, col_of[rows]] != BIG).all() and int(a[rows, col_of[rows]].sum()) == total
    # 1. dual feasibility (object arrays: Python integers, no overflow whatever the duals)
    U, V = np.array(u, dtype=object)[:, None], np.array(v, dtype=object)[None, :]
    assert ((U + V) <= a.astype(object)).all()
    # 2. the longer side's duals are <= 0, and 0 on unpaired posts.  A post paired over a forbidden edge reads -1 like an
    #    unpaired one: of the posts that read -1, at most min(R, C) - matched carry a dual
    n = min(R, C)
    long_duals, long_pair = (v, row_of) if R <= C else (u, col_of)
    assert all(x <= 0 for x in long_duals)
    assert sum(1 for x, q in zip(long_duals, long_pair) if q < 0 and x != 0) <= n - matched
    # 3. strong duality on the padded problem
    assert sum(u) + sum(v) == total + BIG * (n - matched)


def field_cost_matrix(g, cells, col_cost=None):
    """cost[r][f] = g[f][cell[r]] (+ col_cost[f]), int64 sum clamped to INT32_MAX - 1; SC_FIELD_INF stays; a cell out of range
    makes its row SC_FIELD_INF."""
    g = np.asarray(g)
    F = g.shape[0]
    flat = g.reshape(F, -1)
    cells = np.asarray(cells).astype(np.int64)
    inside = (cells >= 0) & (cells < flat.shape[1])
    val = flat[:, np.where(inside, cells, 0)].T.astype(np.int64)      # [R][F]
    add = 0 if col_cost is None else np.asarray(col_cost).astype(np.int64)[None, :]
    out = np.where(val == INF, INF, np.minimum(val + add, INF - 1))
    out[~inside] = INF
    return out.astype(np.int32)


def brute_force(cost):
    """(most pairs, smallest sum among those) over all matchings on real edges; small shapes only."""
    cost = np.asarray(cost)
    R, C = cost.shape
    best = {0: (0, 0)}                       # set of used columns -> (pairs, -sum) of the best matching of the rows so far
    for r in range(R):
        nxt = dict(best)                     # row r unpaired
        for mask, (k, s) in best.items():
            for c in range(C):
                if not (mask >> c) & 1 and cost[r, c] != INF:
                    cand = (k + 1, s - int(cost[r, c]))
                    if cand > nxt.get(mask | (1 << c), (-1, 0)):
                        nxt[mask | (1 << c)] = cand
        best = nxt
    k, s = max(best.values())
    return k, -s


def random_cost(rng, R, C, kind, forbidden=0.0):
    """The cost kinds of the tests: 'tie' 0..3, 'small' 0..999, 'octile' 10a + 14b, 'full' 0..INT32_MAX-1."""
    if kind == "tie":
        c = rng.integers(0, 4, (R, C))
    elif kind == "small":
        c = rng.integers(0, 1000, (R, C))
    elif kind == "octile":
        c = 10 * rng.integers(0, 200, (R, C)) + 14 * rng.integers(0, 200, (R, C))
    else:
        c = rng.integers(0, INF, (R, C))
    c = c.astype(np.int32)
    if forbidden > 0:
        c[rng.random((R, C)) < forbidden] = INF
    return c
