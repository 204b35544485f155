/* car_ref.c -- the C statement of car-like pose planning (include/sea_current_hip_car.h): the arc mask
 * by walking the 2n steps of every arc, the car field as a binary-heap Dijkstra over the 8 W H states (toward: over the edges
 * INTO a state, listed directly, no renaming), and the read-out.  Plain C11, no dependencies; tests/car_twin.py builds it on
 * demand, tests/cpp/car_ref_check.c drives it under the sanitizers. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define CX_INF INT32_MAX
enum { CX_OK = 0, CX_NO_PATH = 1, CX_BAD_ENDPOINT = 2, CX_TRUNCATED = 3 };

static const int HX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
static const int HY[8] = {0, 1, 1, 1, 0, -1, -1, -1};

int cx_args_ok(int W, int H, int arc_n, int arc_cost, int rev_cost) {
    if (W < 1 || H < 1 || arc_n < 1 || arc_n > 4 || arc_cost < 0 || arc_cost > 255 || rev_cost < -1 || rev_cost > 255) return 0;
    const int64_t top = 24ll * arc_n + arc_cost + 2ll * arc_n * (rev_cost > 0 ? rev_cost : 0);
    return top * (8ll * W * H - 1) <= (int64_t)INT32_MAX - 1;
}

typedef struct {
    const int32_t* d2;
    const uint8_t* hm;
    int W, H;
    int32_t thr;
    int n, rev, ca, cr;
} cx_graph;

static int Tc(const cx_graph* g, int x, int y) { return x >= 0 && y >= 0 && x < g->W && y < g->H && g->d2[(size_t)y * g->W + x] >= g->thr; }

static int valid(const cx_graph* g, int x, int y, int k) {
    return Tc(g, x, y) && (!g->hm || ((g->hm[(size_t)y * g->W + x] >> k) & 1));
}

/* A*'s rule for the move (x, y) -> (x + dx, y + dy) */
static int move_ok(const cx_graph* g, int x, int y, int dx, int dy) {
    if (!Tc(g, x, y) || !Tc(g, x + dx, y + dy)) return 0;
    return !(dx && dy) || (Tc(g, x + dx, y) && Tc(g, x, y + dy));
}

/* is A((x, y), k, s) legal?  Its end cell goes to (*ex, *ey); its end heading is (k + s) mod 8. */
static int arc_ok(const cx_graph* g, int x, int y, int k, int s, int* ex, int* ey) {
    const int kn = (k + s + 8) & 7;
    int ok = valid(g, x, y, k);
    for (int i = 0; i < g->n; ++i) {
        ok = ok && move_ok(g, x, y, HX[k], HY[k]) && valid(g, x + HX[k], y + HY[k], k);
        x += HX[k];
        y += HY[k];
    }
    ok = ok && valid(g, x, y, kn);
    for (int j = 0; j < g->n; ++j) {
        ok = ok && move_ok(g, x, y, HX[kn], HY[kn]) && valid(g, x + HX[kn], y + HY[kn], kn);
        x += HX[kn];
        y += HY[kn];
    }
    *ex = x;
    *ey = y;
    return ok;
}

/* The edges of the valid pose (x, y, k) in the order of the definition: out = 1: the heads of the edges out of it, out = 0: the
 * tails of the edges into it.  Slot j (0 .. 5) is edge j + 1; ok[j] says whether it is legal. */
static void edges_of(const cx_graph* g, int x, int y, int k, int out, int* nx, int* ny, int* nk, int* cost, int* ok) {
    const int w = (k & 1) ? 14 : 10, n = g->n, d = out ? 1 : -1;
    /* 1: forward.  out: to c + h; in: from c - h */
    nx[0] = x + d * HX[k]; ny[0] = y + d * HY[k]; nk[0] = k; cost[0] = w;
    ok[0] = valid(g, x, y, k) && valid(g, nx[0], ny[0], k) && move_ok(g, x, y, d * HX[k], d * HY[k]);
    /* 2: reverse.  out: to c - h; in: from c + h */
    nx[1] = x - d * HX[k]; ny[1] = y - d * HY[k]; nk[1] = k; cost[1] = w + g->rev;
    ok[1] = g->rev >= 0 && valid(g, x, y, k) && valid(g, nx[1], ny[1], k) && move_ok(g, x, y, -d * HX[k], -d * HY[k]);
    for (int j = 2; j < 6; ++j) {
        const int s = (j & 1) ? -1 : 1, fwd = j < 4;
        cost[j] = fwd ? g->ca : g->cr;
        if (fwd == out) {   /* the forward arc starts here: driven out of the state, or undone into it */
            nk[j] = (k + s + 8) & 7;
            ok[j] = arc_ok(g, x, y, k, s, &nx[j], &ny[j]);
        } else {            /* the forward arc ends here: it started at heading k - s */
            int ex, ey;
            nk[j] = (k - s + 8) & 7;
            nx[j] = x - n * HX[k] - n * HX[nk[j]];
            ny[j] = y - n * HY[k] - n * HY[nk[j]];
            ok[j] = arc_ok(g, nx[j], ny[j], nk[j], s, &ex, &ey) && ex == x && ey == y;
        }
        if (!fwd && g->rev < 0) ok[j] = 0;
    }
}

/* amask uint16 [H][W].  0: done, 1: bad arguments */
int cx_arc_mask(const int32_t* d2, const uint8_t* hmask, int W, int H, int32_t r2, int arc_n, uint16_t* amask) {
    if (!d2 || !amask || W < 1 || H < 1 || arc_n < 1 || arc_n > 4) return 1;
    const cx_graph g = {d2, hmask, W, H, r2 > 1 ? r2 : 1, arc_n, -1, 0, 0};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            unsigned m = 0;
            int ex, ey;
            if (Tc(&g, x, y))
                for (int k = 0; k < 8; ++k) {
                    if (arc_ok(&g, x, y, k, 1, &ex, &ey)) m |= 1u << (2 * k);
                    if (arc_ok(&g, x, y, k, -1, &ex, &ey)) m |= 1u << (2 * k + 1);
                }
            amask[(size_t)y * W + x] = (uint16_t)m;
        }
    return 0;
}

/* a binary heap of (key, state) with lazy deletion */
typedef struct { int64_t key; int64_t s; } cx_item;
typedef struct { cx_item* a; size_t n, cap; } cx_heap;

static int heap_push(cx_heap* h, int64_t key, int64_t s) {
    if (h->n == h->cap) {
        const size_t nc = h->cap ? 2 * h->cap : 1024;
        cx_item* na = (cx_item*)realloc(h->a, nc * sizeof(cx_item));
        if (!na) return 0;
        h->a = na;
        h->cap = nc;
    }
    size_t i = h->n++;
    while (i > 0) {
        const size_t p = (i - 1) / 2;
        if (h->a[p].key <= key) break;
        h->a[i] = h->a[p];
        i = p;
    }
    h->a[i].key = key;
    h->a[i].s = s;
    return 1;
}

static cx_item heap_pop(cx_heap* h) {
    const cx_item top = h->a[0], last = h->a[--h->n];
    size_t i = 0;
    for (;;) {
        size_t c = 2 * i + 1;
        if (c >= h->n) break;
        if (c + 1 < h->n && h->a[c + 1].key < h->a[c].key) ++c;
        if (h->a[c].key >= last.key) break;
        h->a[i] = h->a[c];
        i = c;
    }
    if (h->n) h->a[i] = last;
    return top;
}

static cx_graph graph_of(const int32_t* d2, const uint8_t* hmask, int W, int H, int32_t r2, int arc_n, int arc_cost, int rev_cost) {
    const cx_graph g = {d2, hmask, W, H, r2 > 1 ? r2 : 1, arc_n, rev_cost, 24 * arc_n + arc_cost,
                        24 * arc_n + arc_cost + 2 * arc_n * (rev_cost > 0 ? rev_cost : 0)};
    return g;
}

/* gp int32 [8][H][W].  Returns the field's status (CX_OK / CX_BAD_ENDPOINT), -1 for bad arguments or no memory. */
int cx_car_field(const int32_t* d2, const uint8_t* hmask, int W, int H, int32_t r2, int arc_n, int arc_cost, int rev_cost, int toward,
                 int root, int rhead, int32_t* gp) {
    if (!d2 || !gp || !cx_args_ok(W, H, arc_n, arc_cost, rev_cost)) return -1;
    const cx_graph g = graph_of(d2, hmask, W, H, r2, arc_n, arc_cost, rev_cost);
    const int64_t n = (int64_t)W * H;
    for (int64_t i = 0; i < 8 * n; ++i) gp[i] = CX_INF;
    if (root < 0 || root >= n || rhead < -1 || rhead > 7) return CX_BAD_ENDPOINT;
    cx_heap h = {0, 0, 0};
    int any = 0;
    for (int k = 0; k < 8; ++k)
        if ((rhead == k || rhead == -1) && valid(&g, root % W, root / W, k)) {
            gp[k * n + root] = 0;
            if (!heap_push(&h, 0, k * n + root)) { free(h.a); return -1; }
            any = 1;
        }
    if (!any) { free(h.a); return CX_BAD_ENDPOINT; }
    while (h.n) {
        const cx_item it = heap_pop(&h);
        if (it.key > gp[it.s]) continue;
        const int k = (int)(it.s / n), c = (int)(it.s % n), x = c % W, y = c / W;
        int nx[6], ny[6], nk[6], ec[6], ok[6];
        edges_of(&g, x, y, k, !toward, nx, ny, nk, ec, ok);
        for (int j = 0; j < 6; ++j) {
            if (!ok[j]) continue;
            const int64_t s2 = nk[j] * n + (int64_t)ny[j] * W + nx[j];
            if (it.key + ec[j] < gp[s2]) {
                gp[s2] = (int32_t)(it.key + ec[j]);
                if (!heap_push(&h, it.key + ec[j], s2)) { free(h.a); return -1; }
            }
        }
    }
    free(h.a);
    return CX_OK;
}

static int abit(const uint16_t* amask, int W, int H, int x, int y, int b) {
    return x >= 0 && y >= 0 && x < W && y < H && ((amask[(size_t)y * W + x] >> b) & 1);
}

/* Q read-outs of one field.  0: done, 1: bad arguments. */
int cx_car_paths(const int32_t* d2, const uint8_t* hmask, const uint16_t* amask, int W, int H, int32_t r2, int arc_n, int arc_cost,
                 int rev_cost, int toward, const int32_t* gp, int root, int rhead, const int32_t* target, const int32_t* thead, int Q,
                 int Lmax, int to_root, int32_t* path, uint8_t* head, int32_t* len, int32_t* cost, int32_t* status) {
    if (!d2 || !amask || !gp || !target || !thead || !path || !head || !len || !cost || !status || Q < 0 || Lmax <= 0 ||
        !cx_args_ok(W, H, arc_n, arc_cost, rev_cost))
        return 1;
    const cx_graph g = graph_of(d2, hmask, W, H, r2, arc_n, arc_cost, rev_cost);
    const int64_t n = (int64_t)W * H;
    const int an = arc_n;
    for (int q = 0; q < Q; ++q) {
        int32_t* P = path + (size_t)q * Lmax;
        uint8_t* Hd = head + (size_t)q * Lmax;
        const int t = target[q], th = thead[q];
        len[q] = 0; cost[q] = -1; status[q] = CX_BAD_ENDPOINT;
        if (root < 0 || root >= n || rhead < -1 || rhead > 7 || t < 0 || t >= n || th < -1 || th > 7) continue;
        int rv = 0;
        for (int k = 0; k < 8; ++k) rv |= (rhead == k || rhead == -1) && valid(&g, root % W, root / W, k);
        if (!rv || !(th >= 0 ? valid(&g, t % W, t / W, th) : Tc(&g, t % W, t / W))) continue;
        int k = th >= 0 ? th : 0;
        int64_t v = th >= 0 ? gp[th * n + t] : CX_INF;
        for (int j = 0; th < 0 && j < 8; ++j)
            if (gp[j * n + t] < v) { v = gp[j * n + t]; k = j; }
        status[q] = CX_NO_PATH;
        if (v >= CX_INF) continue;
        const int32_t total = (int32_t)v;
        int x = t % W, y = t / W, fail = 0;
        int64_t L = 0, steps = 0;
        for (;;) {
            if (L < Lmax) { P[L] = y * W + x; Hd[L] = (uint8_t)k; }
            ++L;
            if (v == 0) break;
            /* the candidates 1 .. 6: in-edges (toward = 0) or out-edges (toward = 1).  Straight moves are judged from d2 and
             * hmask, arcs from amask. */
            int nx[6], ny[6], nk[6], ec[6], ok[6], first[6];
            edges_of(&g, x, y, k, toward, nx, ny, nk, ec, ok);
            for (int j = 2; j < 6; ++j) {
                const int s = (j & 1) ? -1 : 1, fwd = j < 4;
                first[j] = fwd == (toward != 0);    /* the forward arc starts at this state */
                ok[j] = (fwd || rev_cost >= 0) && nx[j] >= 0 && ny[j] >= 0 && nx[j] < W && ny[j] < H &&
                        (first[j] ? abit(amask, W, H, x, y, 2 * k + (s < 0)) : abit(amask, W, H, nx[j], ny[j], 2 * nk[j] + (s < 0)));
            }
            int j = 0;
            for (; j < 6; ++j)
                if (ok[j]) {
                    const int64_t pv = gp[nk[j] * n + (int64_t)ny[j] * W + nx[j]];
                    if (pv < CX_INF && pv + ec[j] == v) break;
                }
            if (j == 6 || ++steps > 8 * n) { fail = 1; break; }
            if (j >= 2) {
                /* the forward arc runs from (ax, ay, ka) to heading kb; its cells p_1 .. p_(2n-1) in walk order */
                const int ax = first[j] ? x : nx[j], ay = first[j] ? y : ny[j], ka = first[j] ? k : nk[j], kb = first[j] ? nk[j] : k;
                for (int m = 1; m < 2 * an; ++m) {
                    const int i = first[j] ? m : 2 * an - m, i1 = i < an ? i : an, i2 = i - i1;
                    const int cx = ax + i1 * HX[ka] + i2 * HX[kb], cy = ay + i1 * HY[ka] + i2 * HY[kb];
                    /* reached by the first leg up to the corner when driven forwards, short of it when driven backwards */
                    const int hd = i < an ? ka : i > an ? kb : (j < 4 ? ka : kb);
                    if (L < Lmax) { P[L] = cy * W + cx; Hd[L] = (uint8_t)hd; }
                    ++L;
                }
            }
            v -= ec[j];
            x = nx[j]; y = ny[j]; k = nk[j];
        }
        if (fail) continue;
        if (L <= Lmax && !to_root)
            for (int64_t i = 0; i < L / 2; ++i) {
                const int32_t a = P[i];
                P[i] = P[L - 1 - i];
                P[L - 1 - i] = a;
                const uint8_t b = Hd[i];
                Hd[i] = Hd[L - 1 - i];
                Hd[L - 1 - i] = b;
            }
        len[q] = (int32_t)L; cost[q] = total; status[q] = L <= Lmax ? CX_OK : CX_TRUNCATED;
    }
    return 0;
}
