/* waypoints_ref.c -- CPU twin of sc_path_waypoints_batch (test infrastructure), a plain C restatement of the definition
 * in include/sea_current_hip.h / DESIGN.md section 9.  Built by the tests with `cc -O2 -shared` and loaded with ctypes.
 *
 *   wr_visible(d2, W, H, r2, a, b)        Visible(a, b): 1 / 0
 *   wr_path_waypoints_batch(...)          same arguments and outputs as sc_path_waypoints_batch (host pointers)
 */
#include <stdint.h>
#include <stdlib.h>

enum { Q_OK = 0, Q_TRUNCATED = 3, Q_BAD_PATH = 5 };

static int64_t floor_div(int64_t n, int64_t d) { /* d > 0 */
    return n >= 0 ? n / d : -((-n + d - 1) / d);
}
static int64_t ceil_div(int64_t n, int64_t d) { return -floor_div(-n, d); }

static int traversable(const int32_t* d2, int c, int32_t thr) { return d2[c] >= thr; }

/* Columns (or rows) of the segment's major axis.  In doubled coordinates the centre of cell c is (2cx, 2cy) and its square
 * is [2cx-1, 2cx+1] x [2cy-1, 2cy+1].  Within the slab of major coordinate u the segment spans the major interval
 * [max(2u-1, 2ua), min(2u+1, 2ub)] (ua <= ub); over it the minor coordinate runs between its values at both ends, and a
 * square of that slab meets the segment iff its minor interval meets that range. */
static int visible_thr(const int32_t* d2, int W, int H, int32_t thr, int a, int b) {
    int ax = a % W, ay = a / W, bx = b % W, by = b / W;
    if (ax == bx && ay == by) return traversable(d2, a, thr);
    int xmajor = abs(bx - ax) >= abs(by - ay);
    /* (u, v) = (major, minor) coordinates, ordered so that ua < ub */
    int64_t ua = xmajor ? ax : ay, va = xmajor ? ay : ax, ub = xmajor ? bx : by, vb = xmajor ? by : bx;
    if (ua > ub) { int64_t t = ua; ua = ub; ub = t; t = va; va = vb; vb = t; }
    const int64_t du = ub - ua, dv = vb - va;
    for (int64_t u = ua; u <= ub; ++u) {
        const int64_t s0 = (2 * u - 1 > 2 * ua ? 2 * u - 1 : 2 * ua) - 2 * ua;   /* doubled major offsets from a */
        const int64_t s1 = (2 * u + 1 < 2 * ub ? 2 * u + 1 : 2 * ub) - 2 * ua;
        /* doubled minor coordinate at offset s: 2 va + s dv / du; the range is [lo, hi] = the two ends, ordered */
        const int64_t n0 = 2 * va * du + s0 * dv, n1 = 2 * va * du + s1 * dv;   /* times du */
        const int64_t lo = n0 < n1 ? n0 : n1, hi = n0 < n1 ? n1 : n0;
        /* rows v with 2v + 1 >= lo / du and 2v - 1 <= hi / du */
        const int64_t vlo = ceil_div(lo - du, 2 * du), vhi = floor_div(hi + du, 2 * du);
        for (int64_t v = vlo; v <= vhi; ++v) {
            const int64_t x = xmajor ? u : v, y = xmajor ? v : u;
            if (x < 0 || y < 0 || x >= W || y >= H) return 0;
            if (!traversable(d2, (int)(y * W + x), thr)) return 0;
        }
    }
    return 1;
}

int wr_visible(const int32_t* d2, int W, int H, int32_t r2_clear, int a, int b) {
    return visible_thr(d2, W, H, r2_clear > 1 ? r2_clear : 1, a, b);
}

/* 1 = same direction, -1 = reverse direction, 0 = not collinear (or a degenerate triple) */
static int collinear(int W, int a, int b, int w) {
    const int64_t ux = b % W - a % W, uy = b / W - a / W, vx = w % W - b % W, vy = w / W - b / W;
    if (ux * vy - uy * vx != 0) return 0;
    const int64_t dot = ux * vx + uy * vy;
    return dot > 0 ? 1 : dot < 0 ? -1 : 0;
}

static int one_path(const int32_t* d2, int W, int H, int32_t thr, const int32_t* p, int L, int Lmax, int32_t* stack, int* n_out) {
    const int cells = W * H;
    if (L < 1 || L > Lmax) return Q_BAD_PATH;
    for (int i = 0; i < L; ++i)
        if (p[i] < 0 || p[i] >= cells) return Q_BAD_PATH;
    if (L == 1 && !traversable(d2, p[0], thr)) return Q_BAD_PATH;
    for (int i = 0; i + 1 < L; ++i) {
        const int ddx = abs(p[i + 1] % W - p[i] % W), ddy = abs(p[i + 1] / W - p[i] / W);
        if ((ddx > ddy ? ddx : ddy) != 1 || !visible_thr(d2, W, H, thr, p[i], p[i + 1])) return Q_BAD_PATH;
    }
    int n = 0, a = 0;
    stack[n++] = p[0];
    while (a < L - 1) {
        int j = a + 1;
        while (j + 1 < L && visible_thr(d2, W, H, thr, p[a], p[j + 1])) ++j;
        if (n >= 2)
            while (j > a + 1 && collinear(W, stack[n - 2], p[a], p[j]) < 0) --j;
        while (n >= 2 && collinear(W, stack[n - 2], stack[n - 1], p[j]) > 0) --n;
        stack[n++] = p[j];
        a = j;
    }
    *n_out = n;
    return Q_OK;
}

int wr_path_waypoints_batch(const int32_t* d2, int W, int H, int32_t r2_clear, const int32_t* path, const int32_t* len,
                            const int32_t* astar_status, int Q, int Lmax, int Wmax, int32_t* wp, int32_t* n_wp, int32_t* status) {
    const int32_t thr = r2_clear > 1 ? r2_clear : 1;
    int32_t* stack = (int32_t*)malloc(sizeof(int32_t) * (size_t)Lmax);
    if (!stack) return 1;
    for (int q = 0; q < Q; ++q) {
        if (astar_status && astar_status[q] != Q_OK) { n_wp[q] = 0; status[q] = astar_status[q]; continue; }
        int n = 0;
        const int st = one_path(d2, W, H, thr, path + (size_t)q * Lmax, len[q], Lmax, stack, &n);
        if (st != Q_OK) { n_wp[q] = 0; status[q] = st; continue; }
        for (int i = 0; i < n && i < Wmax; ++i) wp[(size_t)q * Wmax + i] = stack[i];
        n_wp[q] = n;
        status[q] = n <= Wmax ? Q_OK : Q_TRUNCATED;
    }
    free(stack);
    return 0;
}
