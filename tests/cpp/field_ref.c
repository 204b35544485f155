/* field_ref.c -- CPU twin of sc_cost_field_batch / sc_field_paths_batch (tests only).
 *
 * Field: a bucket-queue Dijkstra from the root over the A* graph (8 moves, costs 10 / 14, T(c) <=> d2[c] >= max(r2, 1),
 * no corner cutting, no move off the grid).  Read-out: the oracle's parent rule from the target, with the legality of
 * every move decided from d2, not from g, so that it checks the kernel's g-only rule. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define FR_INF INT32_MAX
static const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1};
static const int DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
static const int WC[8] = {10, 10, 10, 10, 14, 14, 14, 14};

static int trav(const int32_t* d2, int c, int32_t thr) { return d2[c] >= thr; }

/* move from (x, y) in direction d is legal */
static int legal(const int32_t* d2, int W, int H, int32_t thr, int x, int y, int d) {
    const int nx = x + DX[d], ny = y + DY[d];
    if (nx < 0 || ny < 0 || nx >= W || ny >= H) return 0;
    if (!trav(d2, y * W + x, thr) || !trav(d2, ny * W + nx, thr)) return 0;
    if (d >= 4 && (!trav(d2, y * W + nx, thr) || !trav(d2, ny * W + x, thr))) return 0;
    return 1;
}

/* g int32 [H][W]; returns 0 (SC_Q_OK) or 2 (SC_Q_BAD_ENDPOINT, g all INF) */
int fr_cost_field(const int32_t* d2, int W, int H, int32_t r2, int root, int32_t* g) {
    const size_t n = (size_t)W * H;
    const int32_t thr = r2 > 1 ? r2 : 1;
    for (size_t i = 0; i < n; ++i) g[i] = FR_INF;
    if (root < 0 || (size_t)root >= n || !trav(d2, root, thr)) return 2;
    /* circular bucket queue over costs mod 16 (every edge weighs <= 14); each bucket a growable stack */
    enum { NB = 16 };
    int* bk[NB];
    size_t cnt[NB], cap[NB];
    for (int b = 0; b < NB; ++b) { cap[b] = 64; cnt[b] = 0; bk[b] = (int*)malloc(cap[b] * sizeof(int)); }
    g[root] = 0;
    bk[0][cnt[0]++] = root;
    size_t pending = 1;
    for (int64_t cur = 0; pending; ++cur) {
        const int b = (int)(cur % NB);
        while (cnt[b]) {
            const int c = bk[b][--cnt[b]];
            --pending;
            if (g[c] != cur) continue; /* stale */
            const int x = c % W, y = c / W;
            for (int d = 0; d < 8; ++d) {
                if (!legal(d2, W, H, thr, x, y, d)) continue;
                const int u = (y + DY[d]) * W + x + DX[d];
                const int32_t ng = (int32_t)cur + WC[d];
                if (ng < g[u]) {
                    g[u] = ng;
                    const int nb = ng % NB;
                    if (cnt[nb] == cap[nb]) { cap[nb] *= 2; bk[nb] = (int*)realloc(bk[nb], cap[nb] * sizeof(int)); }
                    bk[nb][cnt[nb]++] = u;
                    ++pending;
                }
            }
        }
    }
    for (int b = 0; b < NB; ++b) free(bk[b]);
    return 0;
}

/* one read-out with sc_astar_batch's conventions; path: Lmax cells; returns the status */
int fr_field_path(const int32_t* d2, int W, int H, int32_t r2, const int32_t* g, int root, int target, int Lmax, int to_root,
                  int32_t* path, int32_t* len, int32_t* cost) {
    const int64_t n = (int64_t)W * H;
    const int32_t thr = r2 > 1 ? r2 : 1;
    *len = 0;
    *cost = -1;
    if (root < 0 || root >= n || target < 0 || target >= n || !trav(d2, root, thr) || !trav(d2, target, thr)) return 2;
    if (g[target] == FR_INF) return 1;
    int64_t L = 1;
    int c = target;
    if (Lmax > 0) path[0] = c;
    while (c != root) {
        const int cx = c % W, cy = c / W;
        int d = 0;
        for (; d < 8; ++d) {
            const int px = cx - DX[d], py = cy - DY[d];
            if (px < 0 || py < 0 || px >= W || py >= H) continue;
            if (!legal(d2, W, H, thr, px, py, d)) continue;
            const int p = py * W + px;
            if (g[p] != FR_INF && g[p] + WC[d] == g[c]) break;
        }
        if (d == 8) return 1; /* cannot happen on a field */
        c = (cy - DY[d]) * W + cx - DX[d];
        if (L < Lmax) path[L] = c;
        ++L;
    }
    *len = (int32_t)L;
    *cost = g[target];
    if (L > Lmax) return 3;
    if (!to_root)
        for (int64_t i = 0; i < L / 2; ++i) {
            const int32_t t = path[i];
            path[i] = path[L - 1 - i];
            path[L - 1 - i] = t;
        }
    return 0;
}

/* batch form: Q queries on one field */
void fr_field_paths(const int32_t* d2, int W, int H, int32_t r2, const int32_t* g, int root, const int32_t* target, int Q, int Lmax,
                    int to_root, int32_t* path, int32_t* len, int32_t* cost, int32_t* status) {
    for (int q = 0; q < Q; ++q)
        status[q] = fr_field_path(d2, W, H, r2, g, root, target[q], Lmax, to_root, path + (size_t)q * Lmax, len + q, cost + q);
}
