/* field_update_ref.c -- the repair of a cost field after a map change, stated in plain C (the CPU statement of
 * sc_cost_field_update_batch; the definition is the header comment of
 * include/sea_current_hip_update.h).
 *
 * Graph: 8 moves dx = {1,-1,0,0,1,-1,1,-1}, dy = {0,0,1,-1,1,1,-1,-1}, costs 10 / 14, T(c) <=> d2[c] >= max(r2, 1), a
 * diagonal needs both side cells traversable, no move leaves the grid; with a costmap the move n -> c costs
 * w_d + min(pen[c], cap).  Primes mark the new map.  g holds the exact field of the old map for `root`.
 *
 * Unsupported set U: the least set such that a cell c with g[c] finite is in U if !T'(c), or if c is not the root and
 * every neighbour n with the move n -> c legal under T', g[n] finite and g[n] + w'(n -> c) == g[c] is in U.  It is grown
 * here from the cells with !T' by a worklist over the number of such neighbours every cell still has.  The cells of U
 * become INF; a binary-heap Dijkstra seeded with every finite cell at or next to a changed or raised cell, and the
 * root, then lowers what can fall.
 *
 * fu_update returns the status of the field (0 = ok, 2 = bad endpoint: the root is out of range or not traversable in
 * the new map, g is all INF), -1 for arguments it refuses or when it runs out of memory.  stats[0] = cells with
 * T != T' or (T && T' and the capped penalties differ), stats[1] = |U|; stats may be NULL.  pen_old and pen_new are
 * both NULL (unweighted) or both given. */
#include <stdint.h>
#include <stdlib.h>

#define INF INT32_MAX

static const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1};
static const int DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};

typedef struct {
    const int32_t* d2;
    const uint8_t* pen;
    int cap, W, H;
    int32_t thr;
} map_t;

static int trav(const map_t* m, int x, int y) { return x >= 0 && y >= 0 && x < m->W && y < m->H && m->d2[y * m->W + x] >= m->thr; }
static int pcap(const map_t* m, int c) { return !m->pen ? 0 : (m->pen[c] < m->cap ? m->pen[c] : m->cap); }

/* the cost of the move from (x, y) in direction d, -1 if it is not legal */
static int move_cost(const map_t* m, int x, int y, int d) {
    const int nx = x + DX[d], ny = y + DY[d];
    if (!trav(m, x, y) || !trav(m, nx, ny)) return -1;
    if (d >= 4 && (!trav(m, nx, y) || !trav(m, x, ny))) return -1;
    return (d < 4 ? 10 : 14) + pcap(m, ny * m->W + nx);
}

/* (x, y) supports its neighbour in direction d: the move is legal under the new map, both values are finite, the edge is tight */
static int supports(const map_t* m, const int32_t* g, int x, int y, int d) {
    const int mc = move_cost(m, x, y, d);
    if (mc < 0) return 0;
    const int c = y * m->W + x, nc = (y + DY[d]) * m->W + x + DX[d];
    return g[c] != INF && g[nc] != INF && (int64_t)g[c] + mc == g[nc];
}

typedef struct { int32_t* key; int32_t* cell; int n; } heap_t;

static void heap_push(heap_t* h, int32_t key, int32_t cell) {
    int i = h->n++;
    while (i > 0 && h->key[(i - 1) / 2] > key) {
        h->key[i] = h->key[(i - 1) / 2];
        h->cell[i] = h->cell[(i - 1) / 2];
        i = (i - 1) / 2;
    }
    h->key[i] = key;
    h->cell[i] = cell;
}

static void heap_pop(heap_t* h, int32_t* key, int32_t* cell) {
    *key = h->key[0];
    *cell = h->cell[0];
    const int32_t k = h->key[--h->n], c = h->cell[h->n];
    int i = 0;
    for (;;) {
        int j = 2 * i + 1;
        if (j >= h->n) break;
        if (j + 1 < h->n && h->key[j + 1] < h->key[j]) ++j;
        if (h->key[j] >= k) break;
        h->key[i] = h->key[j];
        h->cell[i] = h->cell[j];
        i = j;
    }
    if (h->n > 0) { h->key[i] = k; h->cell[i] = c; }
}

int fu_update(const int32_t* d2_old, const uint8_t* pen_old, const int32_t* d2_new, const uint8_t* pen_new, int cap, int W, int H,
              int32_t r2, int root, int32_t* g, int32_t* stats) {
    if (!d2_old || !d2_new || !g || W <= 0 || H <= 0 || (pen_old == NULL) != (pen_new == NULL) || cap < 0 || cap > 255) return -1;
    if ((14ll + (pen_new ? cap : 0)) * ((long long)W * H - 1) > (long long)INT32_MAX - 1) return -1;
    const int n = W * H;
    for (int c = 0; c < n; ++c)
        if (g[c] < 0) return -1;
    const int32_t thr = r2 > 1 ? r2 : 1;
    const map_t m0 = {d2_old, pen_old, cap, W, H, thr}, m1 = {d2_new, pen_new, cap, W, H, thr};
    const int has_root = root >= 0 && root < n;
    const int root_ok = has_root && d2_new[root] >= thr;
    int32_t* count = (int32_t*)calloc((size_t)n, sizeof(int32_t));
    uint8_t* inU = (uint8_t*)calloc((size_t)n, 1);
    uint8_t* dmg = (uint8_t*)calloc((size_t)n, 1);
    int32_t* work = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    if (!count || !inU || !dmg || !work) { free(count); free(inU); free(dmg); free(work); return -1; }
    int changed = 0, nU = 0, nwork = 0;
    for (int c = 0; c < n; ++c) {
        const int t0 = d2_old[c] >= thr, t1 = d2_new[c] >= thr;
        if (t0 != t1 || (t0 && t1 && pcap(&m0, c) != pcap(&m1, c))) { ++changed; dmg[c] = 1; }
    }
    for (int c = 0; c < n; ++c)
        for (int d = 0; d < 8; ++d)
            if (supports(&m1, g, c % W, c / W, d)) ++count[(c / W + DY[d]) * W + c % W + DX[d]];
    for (int c = 0; c < n; ++c) {
        if (g[c] == INF) continue;
        if (d2_new[c] < thr || (count[c] == 0 && !(root_ok && c == root))) { inU[c] = 1; work[nwork++] = c; }
    }
    while (nwork > 0) {
        const int c = work[--nwork];
        ++nU;
        for (int d = 0; d < 8; ++d) {
            if (!supports(&m1, g, c % W, c / W, d)) continue;
            const int nc = (c / W + DY[d]) * W + c % W + DX[d];
            if (--count[nc] == 0 && !inU[nc] && !(root_ok && nc == root)) { inU[nc] = 1; work[nwork++] = nc; }
        }
    }
    if (stats) { stats[0] = changed; stats[1] = nU; }
    for (int c = 0; c < n; ++c)
        if (inU[c]) { g[c] = INF; dmg[c] = 1; }
    free(count); free(work);
    if (!root_ok) {
        for (int c = 0; c < n; ++c) g[c] = INF;
        free(inU); free(dmg);
        return 2;
    }
    g[root] = 0;
    dmg[root] = 1;
    /* Dijkstra with lazy deletion: a push happens only when a value falls; the heap grows on demand */
    int hcap = n + 16;
    heap_t h = {(int32_t*)malloc((size_t)hcap * sizeof(int32_t)), (int32_t*)malloc((size_t)hcap * sizeof(int32_t)), 0};
    if (!h.key || !h.cell) { free(h.key); free(h.cell); free(inU); free(dmg); return -1; }
    for (int c = 0; c < n; ++c) {
        if (g[c] == INF) continue;
        int near = 0;
        for (int dy = -1; dy <= 1 && !near; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int x = c % W + dx, y = c / W + dy;
                if (x >= 0 && y >= 0 && x < W && y < H && dmg[y * W + x]) { near = 1; break; }
            }
        if (near) heap_push(&h, g[c], c);
    }
    int rc = 0;
    while (h.n > 0) {
        int32_t key, c;
        heap_pop(&h, &key, &c);
        if (key > g[c]) continue;
        for (int d = 0; d < 8; ++d) {
            const int mc = move_cost(&m1, c % W, c / W, d);
            if (mc < 0) continue;
            const int nc = (c / W + DY[d]) * W + c % W + DX[d];
            if ((int64_t)key + mc < g[nc]) {
                g[nc] = (int32_t)(key + mc);
                if (h.n == hcap) {
                    hcap *= 2;
                    int32_t* k2 = (int32_t*)realloc(h.key, (size_t)hcap * sizeof(int32_t));
                    if (k2) h.key = k2;
                    int32_t* c2 = (int32_t*)realloc(h.cell, (size_t)hcap * sizeof(int32_t));
                    if (c2) h.cell = c2;
                    if (!k2 || !c2) { rc = -1; h.n = 0; break; }
                }
                heap_push(&h, g[nc], nc);
            }
        }
    }
    free(h.key); free(h.cell); free(inU); free(dmg);
    return rc;
}
