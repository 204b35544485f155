// views_ref.c -- the C statement of line-of-sight sensing (sc_known_from_views, sc_view_gain_batch), single-threaded, straight
// from the definition in include/sea_current_hip.h: one ray per (view, cell of the view's clipped box), every ray walked from
// scratch.  Test infrastructure: tests/views_twin.py builds it, tests/cpp/views_ref_check.c runs it under the sanitizers.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

// Clear(a, b): every cell whose closed unit square meets the closed segment between the centres of a and b has occ == 0.
// Column i (0 .. D) of the major axis, doubled coordinates relative to a: the segment spans t in [max(2i-1, 0), min(2i+1, 2D)]
// and rises t * m / (2D) on the minor axis; it meets rows ceil((tlo m - D) / 2D) .. floor((thi m + D) / 2D).  a and b inside
// the grid; every cell visited lies in their bounding box.
int vx_clear(const uint8_t* occ, int W, int H, int ax, int ay, int bx, int by) {
    (void)H;
    const int64_t dx = (int64_t)bx - ax, dy = (int64_t)by - ay;
    if (dx == 0 && dy == 0) return occ[(size_t)ay * W + ax] == 0;
    const int xmajor = llabs(dx) >= llabs(dy);
    const int64_t D = xmajor ? llabs(dx) : llabs(dy), m = xmajor ? llabs(dy) : llabs(dx);
    const int smaj = (xmajor ? dx : dy) < 0 ? -1 : 1, smin = (xmajor ? dy : dx) < 0 ? -1 : 1;
    for (int64_t i = 0; i <= D; ++i) {
        const int64_t tlo = 2 * i - 1 > 0 ? 2 * i - 1 : 0, thi = 2 * i + 1 < 2 * D ? 2 * i + 1 : 2 * D;
        const int64_t nlo = tlo * m - D, nhi = thi * m + D;
        const int64_t rlo = nlo <= 0 ? 0 : (nlo + 2 * D - 1) / (2 * D), rhi = nhi / (2 * D);
        for (int64_t r = rlo; r <= rhi; ++r) {
            const int64_t x = xmajor ? ax + smaj * i : ax + smin * r, y = xmajor ? ay + smin * r : ay + smaj * i;
            if (occ[(size_t)y * W + x] != 0) return 0;
        }
    }
    return 1;
}

static int64_t isqrt64(int64_t v) {
    int64_t r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

typedef void (*vx_visit)(void* user, size_t cell);

// calls visit for every cell view (cx, cy, r2) sees; nothing for an ignored view or a centre on an occupied cell
static void vx_each_seen(const uint8_t* occ, int W, int H, int64_t cx, int64_t cy, int64_t r2, vx_visit visit, void* user) {
    if (r2 < 0 || cx < 0 || cy < 0 || cx >= W || cy >= H) return;
    if (occ[(size_t)cy * W + cx] != 0) return;
    const int64_t r = isqrt64(r2);
    const int64_t x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < W - 1 ? cx + r : W - 1;
    const int64_t y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < H - 1 ? cy + r : H - 1;
    for (int64_t y = y0; y <= y1; ++y)
        for (int64_t x = x0; x <= x1; ++x)
            if ((x - cx) * (x - cx) + (y - cy) * (y - cy) <= r2 && vx_clear(occ, W, H, (int)cx, (int)cy, (int)x, (int)y))
                visit(user, (size_t)y * W + x);
}

static void mark(void* user, size_t cell) { ((uint8_t*)user)[cell] = 1; }

// known = base != 0 | vis | surf, occ_seen = known ? occ : 0 (may be NULL).  base may be NULL or known itself.  0, or 1 when
// the vis scratch cannot be allocated.
int vx_known_from_views(const uint8_t* base, const uint8_t* occ, const int32_t* views, int R, int W, int H, uint8_t* known,
                        uint8_t* occ_seen) {
    const size_t n = (size_t)W * H;
    uint8_t* vis = (uint8_t*)calloc(n, 1);
    if (!vis) return 1;
    for (int v = 0; v < R; ++v) vx_each_seen(occ, W, H, views[3 * v], views[3 * v + 1], views[3 * v + 2], mark, vis);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t c = (size_t)y * W + x;
            int k = (base && base[c] != 0) || vis[c];
            if (!k && occ[c] != 0)
                k = (x > 0 && vis[c - 1]) || (x + 1 < W && vis[c + 1]) || (y > 0 && vis[c - W]) || (y + 1 < H && vis[c + W]);
            known[c] = k ? 1 : 0;
            if (occ_seen) occ_seen[c] = k ? occ[c] : 0;
        }
    free(vis);
    return 0;
}

struct count_unknown {
    const uint8_t* known;
    int32_t n;
};

static void count(void* user, size_t cell) {
    struct count_unknown* cu = (struct count_unknown*)user;
    cu->n += cu->known[cell] == 0;
}

// gain[i] = the cells with known == 0 that view i alone sees
void vx_view_gain(const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H, int32_t* gain) {
    for (int i = 0; i < N; ++i) {
        struct count_unknown cu = {known, 0};
        vx_each_seen(occ, W, H, views[3 * i], views[3 * i + 1], views[3 * i + 2], count, &cu);
        gain[i] = cu.n;
    }
}
