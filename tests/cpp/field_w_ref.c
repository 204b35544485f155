/* field_w_ref.c -- CPU twin of sc_cost_field_weighted_batch / sc_field_paths_weighted_batch (tests only).
 *
 * Field: a binary-heap Dijkstra from the root over the weighted field graph: 8 moves, T(c) <=> d2[c] >= max(r2, 1), no
 * corner cutting, no move off the grid; the move n -> c in direction d costs w_d + min(pen[c], cap), w_d = 10 / 14.
 * Read-out: the parent rule from the target (smallest d with a legal move n -> c and g[n] + w_d + min(pen[c], cap) ==
 * g[c]), with the legality of every move decided from d2, not from g, so that it checks the kernel's g-only rule. */
#include <stdint.h>
#include <stdlib.h>

#define FW_INF INT32_MAX
static const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1};
static const int DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
static const int WC[8] = {10, 10, 10, 10, 14, 14, 14, 14};

static int trav(const int32_t* d2, int c, int32_t thr) { return d2[c] >= thr; }
static int32_t pcap(const uint8_t* pen, int c, int cap) { return pen[c] < cap ? pen[c] : cap; }

/* move from (x, y) in direction d is legal */
static int legal(const int32_t* d2, int W, int H, int32_t thr, int x, int y, int d) {
    const int nx = x + DX[d], ny = y + DY[d];
    if (nx < 0 || ny < 0 || nx >= W || ny >= H) return 0;
    if (!trav(d2, y * W + x, thr) || !trav(d2, ny * W + nx, thr)) return 0;
    if (d >= 4 && (!trav(d2, y * W + nx, thr) || !trav(d2, ny * W + x, thr))) return 0;
    return 1;
}

typedef struct { int64_t key; int cell; } hent;
typedef struct { hent* a; size_t n, cap; } heap;

static void heap_push(heap* h, int64_t key, int cell) {
    if (h->n == h->cap) { h->cap *= 2; h->a = (hent*)realloc(h->a, h->cap * sizeof(hent)); }
    size_t i = h->n++;
    while (i > 0) {
        const size_t p = (i - 1) / 2;
        if (h->a[p].key <= key) break;
        h->a[i] = h->a[p];
        i = p;
    }
    h->a[i].key = key;
    h->a[i].cell = cell;
}

static hent heap_pop(heap* h) {
    const hent top = h->a[0], last = h->a[--h->n];
    size_t i = 0;
    for (;;) {
        size_t c = 2 * i + 1;
        if (c >= h->n) break;
        if (c + 1 < h->n && h->a[c + 1].key < h->a[c].key) ++c;
        if (last.key <= h->a[c].key) break;
        h->a[i] = h->a[c];
        i = c;
    }
    if (h->n) h->a[i] = last;
    return top;
}

/* g int32 [H][W]; returns 0 (SC_Q_OK) or 2 (SC_Q_BAD_ENDPOINT, g all INF) */
int fw_cost_field(const int32_t* d2, const uint8_t* pen, int cap, int W, int H, int32_t r2, int root, int32_t* g) {
    const size_t n = (size_t)W * H;
    const int32_t thr = r2 > 1 ? r2 : 1;
    for (size_t i = 0; i < n; ++i) g[i] = FW_INF;
    if (root < 0 || (size_t)root >= n || !trav(d2, root, thr)) return 2;
    heap h;
    h.cap = 1024; h.n = 0; h.a = (hent*)malloc(h.cap * sizeof(hent));
    g[root] = 0;
    heap_push(&h, 0, root);
    while (h.n) {
        const hent e = heap_pop(&h);
        if (e.key != g[e.cell]) continue; /* stale */
        const int x = e.cell % W, y = e.cell / W;
        for (int d = 0; d < 8; ++d) {
            if (!legal(d2, W, H, thr, x, y, d)) continue;
            const int u = (y + DY[d]) * W + x + DX[d];
            const int64_t ng = e.key + WC[d] + pcap(pen, u, cap);
            if (ng < g[u]) {
                g[u] = (int32_t)ng;
                heap_push(&h, ng, u);
            }
        }
    }
    free(h.a);
    return 0;
}

/* one read-out with sc_field_paths_batch's conventions; path: Lmax cells; returns the status */
int fw_field_path(const int32_t* d2, const uint8_t* pen, int cap, int W, int H, int32_t r2, const int32_t* g, int root, int target,
                  int Lmax, int to_root, int32_t* path, int32_t* len, int32_t* cost) {
    const int64_t n = (int64_t)W * H;
    const int32_t thr = r2 > 1 ? r2 : 1;
    *len = 0;
    *cost = -1;
    if (root < 0 || root >= n || target < 0 || target >= n || !trav(d2, root, thr) || !trav(d2, target, thr)) return 2;
    if (g[target] == FW_INF) return 1;
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
            if (g[p] != FW_INF && (int64_t)g[p] + WC[d] + pcap(pen, c, cap) == g[c]) break;
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
void fw_field_paths(const int32_t* d2, const uint8_t* pen, int cap, int W, int H, int32_t r2, const int32_t* g, int root,
                    const int32_t* target, int Q, int Lmax, int to_root, int32_t* path, int32_t* len, int32_t* cost, int32_t* status) {
    for (int q = 0; q < Q; ++q)
        status[q] = fw_field_path(d2, pen, cap, W, H, r2, g, root, target[q], Lmax, to_root, path + (size_t)q * Lmax, len + q, cost + q);
}
