/* pose_ref.c -- the C statement of planning in poses (include/sea_current_hip.h): the footprint mask
 * by looping over the covered offsets, the pose field as a binary-heap Dijkstra over the 8 W H states (toward: over the
 * edges INTO a state, i.e. on the transposed graph), and the read-out.  Plain C11, no dependencies; tests/pose_twin.py
 * builds it on demand, tests/cpp/pose_ref_check.c drives it under the sanitizers. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define PX_INF INT32_MAX
enum { PX_OK = 0, PX_NO_PATH = 1, PX_BAD_ENDPOINT = 2, PX_TRUNCATED = 3 };

static const int HX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
static const int HY[8] = {0, 1, 1, 1, 0, -1, -1, -1};

int px_args_ok(int W, int H, int turn_cost, int rev_cost, int readout) {
    if (W < 1 || H < 1 || turn_cost < 0 || turn_cost > 255 || rev_cost < -1 || rev_cost > 255) return 0;
    if (readout && turn_cost == 0) return 0;
    int64_t top = 14 + (rev_cost > 0 ? rev_cost : 0);
    if (turn_cost > top) top = turn_cost;
    return top * (8ll * W * H - 1) <= (int64_t)INT32_MAX - 1;
}

static int covered(int k, int dx, int dy, int front, int back, int left, int right) {
    const int n = HX[k] * HX[k] + HY[k] * HY[k], u = dx * HX[k] + dy * HY[k], v = -dx * HY[k] + dy * HX[k];
    return (u >= 0 ? u * u <= n * front * front : u * u <= n * back * back) && (v >= 0 ? v * v <= n * left * left : v * v <= n * right * right);
}

/* 0: done, 1: bad arguments */
int px_footprint_mask(const int32_t* d2, int W, int H, int32_t r2, int front, int back, int left, int right, uint8_t* out) {
    if (!d2 || !out || W < 1 || H < 1 || front < 0 || front > 32 || back < 0 || back > 32 || left < 0 || left > 32 || right < 0 || right > 32)
        return 1;
    const int32_t thr = r2 > 1 ? r2 : 1;
    int R = front;
    if (back > R) R = back;
    if (left > R) R = left;
    if (right > R) R = right;
    R *= 2;
    const int side = 2 * R + 1;
    int* ox = (int*)malloc(sizeof(int) * side * side);
    int* oy = (int*)malloc(sizeof(int) * side * side);
    if (!ox || !oy) { free(ox); free(oy); return 1; }
    memset(out, 0, (size_t)W * H);
    for (int k = 0; k < 8; ++k) {
        int no = 0;
        for (int dy = -R; dy <= R; ++dy)
            for (int dx = -R; dx <= R; ++dx)
                if (covered(k, dx, dy, front, back, left, right)) { ox[no] = dx; oy[no] = dy; ++no; }
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int ok = 1;
                for (int i = 0; i < no && ok; ++i) {
                    const int nx = x + ox[i], ny = y + oy[i];
                    if (nx < 0 || ny < 0 || nx >= W || ny >= H) continue;
                    if (d2[(size_t)ny * W + nx] < thr) ok = 0;
                }
                if (ok) out[(size_t)y * W + x] |= (uint8_t)(1u << k);
            }
    }
    free(ox);
    free(oy);
    return 0;
}

typedef struct {
    const int32_t* d2;
    const uint8_t* hm;
    int W, H;
    int32_t thr;
    int turn, rev;
} px_graph;

static int Tc(const px_graph* g, int x, int y) { return x >= 0 && y >= 0 && x < g->W && y < g->H && g->d2[(size_t)y * g->W + x] >= g->thr; }

static int valid(const px_graph* g, int x, int y, int k) {
    return Tc(g, x, y) && (!g->hm || ((g->hm[(size_t)y * g->W + x] >> k) & 1));
}

/* A*'s rule for the move (x, y) -> (x + dx, y + dy) */
static int move_ok(const px_graph* g, int x, int y, int dx, int dy) {
    if (!Tc(g, x, y) || !Tc(g, x + dx, y + dy)) return 0;
    return !(dx && dy) || (Tc(g, x + dx, y) && Tc(g, x, y + dy));
}

/* the cost of the legal edge (ax, ay, ak) -> (bx, by, bk), -1 where there is none */
static int edge_cost(const px_graph* g, int ax, int ay, int ak, int bx, int by, int bk) {
    if (!valid(g, ax, ay, ak) || !valid(g, bx, by, bk)) return -1;
    const int w = (ak & 1) ? 14 : 10;
    if (ak == bk) {
        if (bx == ax + HX[ak] && by == ay + HY[ak]) return move_ok(g, ax, ay, HX[ak], HY[ak]) ? w : -1;
        if (bx == ax - HX[ak] && by == ay - HY[ak]) return g->rev >= 0 && move_ok(g, ax, ay, -HX[ak], -HY[ak]) ? w + g->rev : -1;
        return -1;
    }
    if (ax == bx && ay == by && (bk == ((ak + 1) & 7) || bk == ((ak + 7) & 7))) return g->turn;
    return -1;
}

/* a binary heap of (key, state) with lazy deletion */
typedef struct { int64_t key; int64_t s; } px_item;
typedef struct { px_item* a; size_t n, cap; } px_heap;

static int heap_push(px_heap* h, int64_t key, int64_t s) {
    if (h->n == h->cap) {
        const size_t nc = h->cap ? 2 * h->cap : 1024;
        px_item* na = (px_item*)realloc(h->a, nc * sizeof(px_item));
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

static px_item heap_pop(px_heap* h) {
    const px_item top = h->a[0], last = h->a[--h->n];
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

/* gp int32 [8][H][W].  Returns the field's status (PX_OK / PX_BAD_ENDPOINT), -1 for bad arguments or no memory. */
int px_pose_field(const int32_t* d2, const uint8_t* hmask, int W, int H, int32_t r2, int turn_cost, int rev_cost, int toward, int root,
                  int rhead, int32_t* gp) {
    if (!d2 || !gp || !px_args_ok(W, H, turn_cost, rev_cost, 0)) return -1;
    const px_graph g = {d2, hmask, W, H, r2 > 1 ? r2 : 1, turn_cost, rev_cost};
    const int64_t n = (int64_t)W * H;
    for (int64_t i = 0; i < 8 * n; ++i) gp[i] = PX_INF;
    if (root < 0 || root >= n || rhead < -1 || rhead > 7) return PX_BAD_ENDPOINT;
    px_heap h = {0, 0, 0};
    int any = 0;
    for (int k = 0; k < 8; ++k)
        if ((rhead == k || rhead == -1) && valid(&g, root % W, root / W, k)) {
            gp[k * n + root] = 0;
            if (!heap_push(&h, 0, k * n + root)) { free(h.a); return -1; }
            any = 1;
        }
    if (!any) { free(h.a); return PX_BAD_ENDPOINT; }
    while (h.n) {
        const px_item it = heap_pop(&h);
        if (it.key > gp[it.s]) continue;
        const int k = (int)(it.s / n), c = (int)(it.s % n), x = c % W, y = c / W;
        /* the neighbours: the heads of the edges out of (x, y, k), toward: the tails of the edges into it */
        int nx[4], ny[4], nk[4];
        nx[0] = x + HX[k]; ny[0] = y + HY[k]; nk[0] = k;
        nx[1] = x - HX[k]; ny[1] = y - HY[k]; nk[1] = k;
        nx[2] = x; ny[2] = y; nk[2] = (k + 1) & 7;
        nx[3] = x; ny[3] = y; nk[3] = (k + 7) & 7;
        for (int j = 0; j < 4; ++j) {
            if (nx[j] < 0 || ny[j] < 0 || nx[j] >= W || ny[j] >= H) continue;
            const int c2 = toward ? edge_cost(&g, nx[j], ny[j], nk[j], x, y, k) : edge_cost(&g, x, y, k, nx[j], ny[j], nk[j]);
            if (c2 < 0) continue;
            const int64_t s2 = nk[j] * n + (int64_t)ny[j] * W + nx[j];
            if (it.key + c2 < gp[s2]) {
                gp[s2] = (int32_t)(it.key + c2);
                if (!heap_push(&h, it.key + c2, s2)) { free(h.a); return -1; }
            }
        }
    }
    free(h.a);
    return PX_OK;
}

/* Q read-outs of one field.  0: done, 1: bad arguments. */
int px_pose_paths(const int32_t* d2, const uint8_t* hmask, int W, int H, int32_t r2, int turn_cost, int rev_cost, int toward,
                  const int32_t* gp, int root, int rhead, const int32_t* target, const int32_t* thead, int Q, int Lmax, int to_root,
                  int cells_only, int32_t* path, uint8_t* head, int32_t* len, int32_t* cost, int32_t* status) {
    if (!d2 || !gp || !target || !thead || !path || !head || !len || !cost || !status || Q < 0 || Lmax <= 0 ||
        !px_args_ok(W, H, turn_cost, rev_cost, 1))
        return 1;
    const px_graph g = {d2, hmask, W, H, r2 > 1 ? r2 : 1, turn_cost, rev_cost};
    const int64_t n = (int64_t)W * H;
    const int sgn = toward ? -1 : 1;   /* the transposed graph is the graph with every heading vector negated */
    for (int q = 0; q < Q; ++q) {
        int32_t* P = path + (size_t)q * Lmax;
        uint8_t* Hd = head + (size_t)q * Lmax;
        const int t = target[q], th = thead[q];
        len[q] = 0; cost[q] = -1; status[q] = PX_BAD_ENDPOINT;
        if (root < 0 || root >= n || rhead < -1 || rhead > 7 || t < 0 || t >= n || th < -1 || th > 7) continue;
        int rv = 0;
        for (int k = 0; k < 8; ++k) rv |= (rhead == k || rhead == -1) && valid(&g, root % W, root / W, k);
        if (!rv || !(th >= 0 ? valid(&g, t % W, t / W, th) : Tc(&g, t % W, t / W))) continue;
        int k = th >= 0 ? th : 0;
        int64_t v = th >= 0 ? gp[th * n + t] : PX_INF;
        for (int j = 0; th < 0 && j < 8; ++j)
            if (gp[j * n + t] < v) { v = gp[j * n + t]; k = j; }
        status[q] = PX_NO_PATH;
        if (v >= PX_INF) continue;
        const int32_t total = (int32_t)v;
        int x = t % W, y = t / W, fail = 0;
        int64_t L = 0, steps = 0;
        int last = -1;
        for (;;) {
            const int c = y * W + x;
            if (cells_only && c == last) {
                if (!to_root && L - 1 < Lmax) Hd[L - 1] = (uint8_t)k;
            } else {
                if (L < Lmax) { P[L] = c; Hd[L] = (uint8_t)k; }
                ++L;
                last = c;
            }
            if (v == 0) break;
            /* the candidates: forward predecessor, reverse predecessor, the turn from k - 1, the turn from k + 1 */
            const int w = (k & 1) ? 14 : 10;
            int px[4], py[4], pk[4], ec[4], ok[4];
            px[0] = x - sgn * HX[k]; py[0] = y - sgn * HY[k]; pk[0] = k; ec[0] = w;
            px[1] = x + sgn * HX[k]; py[1] = y + sgn * HY[k]; pk[1] = k; ec[1] = w + rev_cost;
            px[2] = x; py[2] = y; pk[2] = (k + 7) & 7; ec[2] = turn_cost;
            px[3] = x; py[3] = y; pk[3] = (k + 1) & 7; ec[3] = turn_cost;
            ok[0] = valid(&g, px[0], py[0], k) && move_ok(&g, px[0], py[0], x - px[0], y - py[0]);
            ok[1] = rev_cost >= 0 && valid(&g, px[1], py[1], k) && move_ok(&g, px[1], py[1], x - px[1], y - py[1]);
            ok[2] = valid(&g, x, y, pk[2]);
            ok[3] = valid(&g, x, y, pk[3]);
            int j = 0;
            for (; j < 4; ++j)
                if (ok[j]) {
                    const int64_t pv = gp[pk[j] * n + (int64_t)py[j] * W + px[j]];
                    if (pv < PX_INF && pv + ec[j] == v) break;
                }
            if (j == 4 || ++steps > 8 * n) { fail = 1; break; }
            v -= ec[j];
            x = px[j]; y = py[j]; k = pk[j];
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
        len[q] = (int32_t)L; cost[q] = total; status[q] = L <= Lmax ? PX_OK : PX_TRUNCATED;
    }
    return 0;
}
