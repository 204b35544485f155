/* match_wide_ref.c -- the C statement of wide-window scan matching (sc_scan_match_wide_batch), straight from the definition in
 * include/sea_current_hip.h: `best` by a plain dense search over the whole window, `stats` by the stated procedure (pooled
 * maps as window minima, levels, one dive per rotation and level).  Checker only: the library never links it. */
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>

#define MWX_MAX_REACH 16384
#define MWX_MAX_DIM 8192
#define MWX_IGNORED (-1)
#define MWX_OVERFLOW (-2)
#define MWX_MAX_TOP 5

static int mwx_absent(int32_t p) { return p < -MWX_MAX_REACH || p > MWX_MAX_REACH; }
static int mwx_centre_ok(int32_t c) { return c >= -MWX_MAX_REACH && c <= MWX_MAX_DIM + MWX_MAX_REACH; }

static int32_t mwx_cost(const int32_t* d2, const uint8_t* known, int W, int H, int x, int y, int32_t d2_cap, int32_t unk) {
    if (x < 0 || x >= W || y < 0 || y >= H) return unk;
    size_t c = (size_t)y * W + x;
    if (known && known[c] == 0) return unk;
    return d2[c] < d2_cap ? d2[c] : d2_cap;
}

typedef struct {
    const int32_t *d2, *pts;
    const uint8_t* known;
    int W, H, N, wx, wy, cx, cy;
    int32_t d2_cap, unk;
    uint16_t* P[MWX_MAX_TOP + 1]; /* P[j]: [H + m + 1][W + m + 1] over x in -m .. W, y in -m .. H, m = 4^j */
} mwx_scan;

typedef struct { int r, dx0, dy0; int64_t B; } mwx_node;

static int mwx_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

/* P_m as a window minimum, rows first: tmp[y][x] = min over i < m of cost(x + i, y) for y in -m .. H + m - 1 */
static uint16_t* mwx_pool(const int32_t* d2, const uint8_t* known, int W, int H, int32_t d2_cap, int32_t unk, int m) {
    const int Wm = W + m + 1, Hm = H + m + 1, Ht = H + 2 * m;
    uint16_t* tmp = malloc((size_t)Ht * Wm * 2);
    uint16_t* out = malloc((size_t)Hm * Wm * 2);
    if (!tmp || !out) {
        free(tmp), free(out);
        return NULL;
    }
    for (int y = -m; y < H + m; ++y)
        for (int x = -m; x <= W; ++x) {
            int32_t v = unk;
            if (y >= 0 && y < H) {
                v = 32767;
                for (int i = 0; i < m; ++i) {
                    const int32_t c = mwx_cost(d2, known, W, H, x + i, y, d2_cap, unk);
                    if (c < v) v = c;
                }
            }
            tmp[(size_t)(y + m) * Wm + (x + m)] = (uint16_t)v;
        }
    for (int y = -m; y <= H; ++y) { /* then columns: the minimum over the m rows from y on, a row at a time */
        uint16_t* o = out + (size_t)(y + m) * Wm;
        for (int x = 0; x < Wm; ++x) o[x] = 65535;
        for (int j = 0; j < m; ++j) {
            const uint16_t* t = tmp + (size_t)(y + j + m) * Wm;
            for (int x = 0; x < Wm; ++x)
                if (t[x] < o[x]) o[x] = t[x];
        }
    }
    free(tmp);
    return out;
}

/* the bound of a node of size m = 4^j; for j = 0 the score */
static int64_t mwx_bound(const mwx_scan* s, int j, int r, int dx0, int dy0) {
    const int m = 1 << (2 * j), Wm = s->W + m + 1;
    const int32_t* p = s->pts + (size_t)r * s->N * 2;
    int64_t sum = 0; /* at most 32767 * 65536 < 2^31 */
    for (int k = 0; k < s->N; ++k) {
        if (mwx_absent(p[2 * k]) || mwx_absent(p[2 * k + 1])) continue;
        const int x = mwx_clamp(s->cx + dx0 + p[2 * k], -m, s->W), y = mwx_clamp(s->cy + dy0 + p[2 * k + 1], -m, s->H);
        sum += s->P[j][(size_t)(y + m) * Wm + (x + m)];
    }
    return sum;
}

/* (B, dy0, dx0) of a before that of b */
static int mwx_before(const mwx_node* a, const mwx_node* b) {
    if (a->B != b->B) return a->B < b->B;
    if (a->dy0 != b->dy0) return a->dy0 < b->dy0;
    return a->dx0 < b->dx0;
}

/* the children of size 4^j of node p, bounded, into out (room for 16); their number */
static int mwx_children(const mwx_scan* s, const mwx_node* p, int j, mwx_node* out) {
    const int q = 1 << (2 * j);
    int n = 0;
    for (int b = 0; b < 4; ++b)
        for (int a = 0; a < 4; ++a) {
            const int dx0 = p->dx0 + a * q, dy0 = p->dy0 + b * q;
            if (dx0 > s->wx || dy0 > s->wy) continue;
            out[n].r = p->r, out[n].dx0 = dx0, out[n].dy0 = dy0;
            out[n].B = mwx_bound(s, j, p->r, dx0, dy0);
            ++n;
        }
    return n;
}

/* the procedure of one live scan with a present point: stats, and whether it overflowed.  -1: out of memory. */
static int mwx_procedure(const mwx_scan* s, int R, int top, int max_nodes, int32_t* stats) {
    mwx_node* cur = malloc((size_t)max_nodes * sizeof(mwx_node));
    mwx_node* next = malloc((size_t)max_nodes * sizeof(mwx_node));
    if (!cur || !next) {
        free(cur), free(next);
        return -1;
    }
    int64_t U = mwx_bound(s, 0, 0, 0, 0);
    for (int r = 1; r < R; ++r) {
        const int64_t v = mwx_bound(s, 0, r, 0, 0);
        if (v < U) U = v;
    }
    const int m_top = 1 << (2 * top);
    int n = 0, over = 0;
    int64_t n_dive = 0;
    for (int r = 0; r < R; ++r)
        for (int dy0 = -s->wy; dy0 <= s->wy; dy0 += m_top)
            for (int dx0 = -s->wx; dx0 <= s->wx; dx0 += m_top) cur[n].r = r, cur[n].dx0 = dx0, cur[n].dy0 = dy0, ++n;
    for (int j = top; j >= 0; --j) {
        for (int i = 0; i < n; ++i) cur[i].B = mwx_bound(s, j, cur[i].r, cur[i].dx0, cur[i].dy0);
        stats[j] = n;
        if (j == 0) break;
        int64_t Unew = U;
        for (int r = 0; r < R; ++r) {
            const mwx_node* b = NULL;
            for (int i = 0; i < n; ++i)
                if (cur[i].r == r && (!b || mwx_before(&cur[i], b))) b = &cur[i];
            if (!b || b->B > U) continue; /* U of the start of this level */
            mwx_node at = *b, kids[16];
            for (int jj = j - 1; jj >= 0; --jj) {
                const int nk = mwx_children(s, &at, jj, kids);
                n_dive += nk;
                int k = 0;
                for (int i = 1; i < nk; ++i)
                    if (mwx_before(&kids[i], &kids[k])) k = i;
                at = kids[k];
            }
            if (at.B < Unew) Unew = at.B;
        }
        U = Unew;
        int64_t nn = 0;
        const int q = 1 << (2 * (j - 1));
        for (int i = 0; i < n && !over; ++i) {
            if (cur[i].B > U) continue;
            for (int b = 0; b < 4; ++b)
                for (int a = 0; a < 4; ++a) {
                    const int dx0 = cur[i].dx0 + a * q, dy0 = cur[i].dy0 + b * q;
                    if (dx0 > s->wx || dy0 > s->wy) continue;
                    if (nn == max_nodes) {
                        over = 1;
                        continue;
                    }
                    next[nn].r = cur[i].r, next[nn].dx0 = dx0, next[nn].dy0 = dy0, ++nn;
                }
        }
        if (over) break;
        mwx_node* t = cur;
        cur = next, next = t, n = (int)nn;
    }
    stats[6] = (int32_t)n_dive, stats[7] = (int32_t)U;
    free(cur), free(next);
    return over;
}

/* 0; 1 for arguments outside the contract; 2 out of memory.  stats may be NULL: then only the dense search runs (a scan
 * that would overflow is not detected). */
int mwx_match(const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre, int S, int R, int N, int W, int H, int wx,
              int wy, int32_t d2_cap, int32_t unk, int top, int max_nodes, int32_t* best, int32_t* stats) {
    if (!d2 || !pts || !centre || !best || S < 0 || R < 1 || R > 256 || N < 1 || N > 65536 || W < 1 || W > MWX_MAX_DIM || H < 1 ||
        H > MWX_MAX_DIM || wx < 0 || wx > 2048 || wy < 0 || wy > 2048 || d2_cap < 1 || d2_cap > 32767 || unk < 0 || unk > d2_cap ||
        top < 0 || top > MWX_MAX_TOP || max_nodes < 64 || max_nodes > (1 << 22) || (int64_t)S * max_nodes > (1 << 26) || (int64_t)R * (2 * wx + 1) * (2 * wy + 1) > INT32_MAX || stats == best)
        return 1;
    const int m_top = 1 << (2 * top);
    if ((int64_t)R * ((2 * wx) / m_top + 1) * ((2 * wy) / m_top + 1) > max_nodes) return 1;
    mwx_scan sc = {d2, NULL, known, W, H, N, wx, wy, 0, 0, d2_cap, unk, {0}};
    int status = 0;
    if (stats)
        for (int j = 0; j <= top && !status; ++j)
            if (!(sc.P[j] = mwx_pool(d2, known, W, H, d2_cap, unk, 1 << (2 * j)))) status = 2;
    for (int s = 0; s < S && !status; ++s) {
        int32_t* b = best + (size_t)s * 6;
        const int cx = centre[2 * s], cy = centre[2 * s + 1];
        b[0] = b[1] = b[2] = b[3] = b[4] = b[5] = 0;
        if (stats)
            for (int i = 0; i < 8; ++i) stats[(size_t)s * 8 + i] = 0;
        if (!mwx_centre_ok(cx) || !mwx_centre_ok(cy)) {
            b[0] = MWX_IGNORED;
            continue;
        }
        const int32_t* ps = pts + (size_t)s * R * N * 2;
        int any = 0;
        for (size_t k = 0; k < (size_t)R * N && !any; ++k) any = !mwx_absent(ps[2 * k]) && !mwx_absent(ps[2 * k + 1]);
        if (!any) {
            b[5] = (int32_t)((int64_t)R * (2 * wx + 1) * (2 * wy + 1));
            continue;
        }
        if (stats) {
            sc.pts = ps, sc.cx = cx, sc.cy = cy;
            const int over = mwx_procedure(&sc, R, top, max_nodes, stats + (size_t)s * 8);
            if (over < 0) status = 2;
            if (over) {
                b[0] = MWX_OVERFLOW;
                continue;
            }
        }
        /* the dense search, as in match_ref.c */
        int have = 0;
        int64_t bs = 0, bd = 0, ties = 0;
        int br = 0, bdy = 0, bdx = 0;
        for (int r = 0; r < R; ++r) {
            const int32_t* p = ps + (size_t)r * N * 2;
            for (int dy = -wy; dy <= wy; ++dy)
                for (int dx = -wx; dx <= wx; ++dx) {
                    int64_t sum = 0;
                    for (int k = 0; k < N; ++k) {
                        if (mwx_absent(p[2 * k]) || mwx_absent(p[2 * k + 1])) continue;
                        sum += mwx_cost(d2, known, W, H, cx + dx + p[2 * k], cy + dy + p[2 * k + 1], d2_cap, unk);
                    }
                    const int64_t d = (int64_t)dx * dx + (int64_t)dy * dy;
                    if (have && sum == bs) ++ties;
                    if (!have || sum < bs || (sum == bs && d < bd)) {
                        if (!have || sum < bs) ties = 1;
                        have = 1, bs = sum, bd = d, br = r, bdy = dy, bdx = dx;
                    }
                }
        }
        int np = 0;
        const int32_t* p = ps + (size_t)br * N * 2;
        for (int k = 0; k < N; ++k) np += !mwx_absent(p[2 * k]) && !mwx_absent(p[2 * k + 1]);
        b[0] = br, b[1] = bdx, b[2] = bdy, b[3] = (int32_t)bs, b[4] = np, b[5] = (int32_t)ties;
    }
    for (int j = 0; j <= MWX_MAX_TOP; ++j) free(sc.P[j]);
    return status;
}
