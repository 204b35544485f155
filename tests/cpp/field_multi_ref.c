/* field_multi_ref.c -- CPU twin of sc_cost_field_multi_batch / sc_field_paths_multi_batch (tests only), written from the
 * definition in include/sea_current_hip.h, one field at a time.
 *
 * Graph: 8 moves, T(c) <=> d2[c] >= max(r2, 1), no corner cutting, no move off the grid; the move n -> c in direction d
 * costs w_d + min(pen[c], cap), w_d = 10 / 14 (pen NULL: w_d).
 * Field: a multi-source bucket-queue Dijkstra.  The valid seeds are sorted by cost and enter the queue when the sweep
 * reaches their cost (a seed whose cell is already cheaper never enters: it is dominated).
 * Terminal: the smallest valid seed index s with seed[s] == c and seed_cost[s] == g[c].  Owner: by the walk -- follow the
 * parent rule (smallest d with a legal move n -> c, legality from d2, and g[n] + w_d + pen(c) == g[c]) to the first
 * terminal cell.  Read-out: the same walk, written out.
 * A field's seeds are seed[0 .. n_seed-1] of the pointers passed; s0 is added to every index reported (the position of
 * the field's first seed in the call's array). */
#include <stdint.h>
#include <stdlib.h>

#define FM_INF INT32_MAX
#define FM_SEED_COST_MAX (1 << 24)
static const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1};
static const int DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
static const int WC[8] = {10, 10, 10, 10, 14, 14, 14, 14};
enum { NB = 512 }; /* circular buckets: more than the largest edge weight 14 + 255 */

static int trav(const int32_t* d2, int c, int32_t thr) { return d2[c] >= thr; }
static int32_t pcap(const uint8_t* pen, int c, int cap) { return !pen ? 0 : (pen[c] < cap ? pen[c] : cap); }

static int legal(const int32_t* d2, int W, int H, int32_t thr, int x, int y, int d) {
    const int nx = x + DX[d], ny = y + DY[d];
    if (nx < 0 || ny < 0 || nx >= W || ny >= H) return 0;
    if (!trav(d2, y * W + x, thr) || !trav(d2, ny * W + nx, thr)) return 0;
    if (d >= 4 && (!trav(d2, y * W + nx, thr) || !trav(d2, ny * W + x, thr))) return 0;
    return 1;
}

static int seed_valid(const int32_t* d2, int64_t n, int32_t thr, const int32_t* seed, const int32_t* seed_cost, int s) {
    const int32_t c = seed[s], sc = seed_cost ? seed_cost[s] : 0;
    return c >= 0 && c < n && sc >= 0 && sc <= FM_SEED_COST_MAX && trav(d2, c, thr);
}

typedef struct { int32_t cost; int idx; } sref;
static int sref_cmp(const void* a, const void* b) {
    const sref *x = (const sref*)a, *y = (const sref*)b;
    return x->cost != y->cost ? (x->cost < y->cost ? -1 : 1) : (x->idx < y->idx ? -1 : (x->idx > y->idx));
}

/* the parent of a finite cell c by the parent rule, -1 if it has none */
static int parent_of(const int32_t* d2, const uint8_t* pen, int cap, int W, int H, int32_t thr, const int32_t* g, int c) {
    const int cx = c % W, cy = c / W;
    for (int d = 0; d < 8; ++d) {
        const int px = cx - DX[d], py = cy - DY[d];
        if (px < 0 || py < 0 || px >= W || py >= H) continue;
        if (!legal(d2, W, H, thr, px, py, d)) continue;
        const int p = py * W + px;
        if (g[p] != FM_INF && (int64_t)g[p] + WC[d] + pcap(pen, c, cap) == g[c]) return p;
    }
    return -1;
}

/* term[c] = the smallest valid s with seed[s] == c and seed_cost[s] == g[c], else -1 */
static void terminals(const int32_t* d2, int64_t n, int32_t thr, const int32_t* g, const int32_t* seed, const int32_t* seed_cost, int n_seed,
                      int32_t* term) {
    for (int64_t i = 0; i < n; ++i) term[i] = -1;
    for (int s = n_seed - 1; s >= 0; --s)
        if (seed_valid(d2, n, thr, seed, seed_cost, s) && g[seed[s]] == (seed_cost ? seed_cost[s] : 0)) term[seed[s]] = s;
}

/* g int32 [H][W], owner int32 [H][W] or NULL; returns 0 (SC_Q_OK) or 2 (SC_Q_BAD_ENDPOINT: no valid seed, g all INF) */
int fm_cost_field(const int32_t* d2, const uint8_t* pen, int cap, int W, int H, int32_t r2, const int32_t* seed, const int32_t* seed_cost,
                  int n_seed, int s0, int32_t* g, int32_t* owner) {
    const int64_t n = (int64_t)W * H;
    const int32_t thr = r2 > 1 ? r2 : 1;
    for (int64_t i = 0; i < n; ++i) g[i] = FM_INF;
    if (owner)
        for (int64_t i = 0; i < n; ++i) owner[i] = -1;
    sref* sv = (sref*)malloc((size_t)(n_seed > 0 ? n_seed : 1) * sizeof(sref));
    int nv = 0;
    for (int s = 0; s < n_seed; ++s)
        if (seed_valid(d2, n, thr, seed, seed_cost, s)) { sv[nv].cost = seed_cost ? seed_cost[s] : 0; sv[nv].idx = s; ++nv; }
    if (nv == 0) { free(sv); return 2; }
    qsort(sv, (size_t)nv, sizeof(sref), sref_cmp);
    int* bk[NB];
    size_t cnt[NB], cp[NB];
    for (int b = 0; b < NB; ++b) { cp[b] = 64; cnt[b] = 0; bk[b] = (int*)malloc(cp[b] * sizeof(int)); }
    size_t pending = 0;
    int next = 0;
    int64_t cur = sv[0].cost;
    while (pending || next < nv) {
        if (!pending && sv[next].cost > cur) cur = sv[next].cost;
        const int b = (int)(cur % NB);
        for (; next < nv && sv[next].cost == cur; ++next) {
            const int c = seed[sv[next].idx];
            if (g[c] > cur) {
                g[c] = (int32_t)cur;
                if (cnt[b] == cp[b]) { cp[b] *= 2; bk[b] = (int*)realloc(bk[b], cp[b] * sizeof(int)); }
                bk[b][cnt[b]++] = c;
                ++pending;
            }
        }
        while (cnt[b]) {
            const int c = bk[b][--cnt[b]];
            --pending;
            if (g[c] != cur) continue; /* stale */
            const int x = c % W, y = c / W;
            for (int d = 0; d < 8; ++d) {
                if (!legal(d2, W, H, thr, x, y, d)) continue;
                const int u = (y + DY[d]) * W + x + DX[d];
                const int64_t ng = cur + WC[d] + pcap(pen, u, cap);
                if (ng < g[u]) {
                    g[u] = (int32_t)ng;
                    const int nb = (int)(ng % NB);
                    if (cnt[nb] == cp[nb]) { cp[nb] *= 2; bk[nb] = (int*)realloc(bk[nb], cp[nb] * sizeof(int)); }
                    bk[nb][cnt[nb]++] = u;
                    ++pending;
                }
            }
        }
        ++cur;
    }
    for (int b = 0; b < NB; ++b) free(bk[b]);
    free(sv);
    if (owner) {
        /* the walk from every cell; the cells of a walk share its end, so each is walked once */
        int32_t* term = (int32_t*)malloc((size_t)n * sizeof(int32_t));
        int* chain = (int*)malloc((size_t)n * sizeof(int));
        terminals(d2, n, thr, g, seed, seed_cost, n_seed, term);
        for (int64_t i = 0; i < n; ++i)
            if (term[i] >= 0) owner[i] = term[i] + s0;
        for (int64_t i = 0; i < n; ++i) {
            if (g[i] == FM_INF || owner[i] >= 0) continue;
            int64_t len = 0;
            int c = (int)i;
            while (c >= 0 && owner[c] < 0) {
                chain[len++] = c;
                c = parent_of(d2, pen, cap, W, H, thr, g, c);
            }
            const int32_t o = c >= 0 ? owner[c] : -1; /* c < 0 cannot happen on a field */
            for (int64_t k = 0; k < len; ++k) owner[chain[k]] = o;
        }
        free(term);
        free(chain);
    }
    return 0;
}

/* Q read-outs on one field with sc_field_paths_multi_batch's conventions */
void fm_field_paths(const int32_t* d2, const uint8_t* pen, int cap, int W, int H, int32_t r2, const int32_t* g, const int32_t* seed,
                    const int32_t* seed_cost, int n_seed, int s0, const int32_t* target, int Q, int Lmax, int to_seed, int32_t* path,
                    int32_t* len, int32_t* cost, int32_t* status, int32_t* which) {
    const int64_t n = (int64_t)W * H;
    const int32_t thr = r2 > 1 ? r2 : 1;
    int32_t* term = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    terminals(d2, n, thr, g, seed, seed_cost, n_seed, term);
    for (int q = 0; q < Q; ++q) {
        int32_t* P = path + (size_t)q * Lmax;
        const int t = target[q];
        len[q] = 0;
        cost[q] = -1;
        which[q] = -1;
        if (t < 0 || t >= n || !trav(d2, t, thr)) { status[q] = 2; continue; }
        if (g[t] == FM_INF) { status[q] = 1; continue; }
        int64_t L = 1;
        int c = t;
        if (Lmax > 0) P[0] = c;
        while (c >= 0 && term[c] < 0) {
            c = parent_of(d2, pen, cap, W, H, thr, g, c);
            if (c < 0) break;
            if (L < Lmax) P[L] = c;
            ++L;
        }
        if (c < 0) { status[q] = 1; continue; } /* cannot happen on a field */
        len[q] = (int32_t)L;
        cost[q] = g[t];
        which[q] = term[c] + s0;
        if (L > Lmax) { status[q] = 3; continue; }
        if (!to_seed)
            for (int64_t i = 0; i < L / 2; ++i) {
                const int32_t v = P[i];
                P[i] = P[L - 1 - i];
                P[L - 1 - i] = v;
            }
        status[q] = 0;
    }
    free(term);
}
