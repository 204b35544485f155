// sectors_ref.c -- the C statement of sensors with a field of view (sc_known_from_sectors, sc_sector_gain_batch,
// sc_view_gain_headings_batch, sc_views_from_cells), single-threaded, straight from the definitions in
// include/sea_current_hip.h: int64 throughout, one ray per (view, cell of the view's clipped box), the bin of an offset found by
// trying every bin.  Clear(a, b) is views_ref.c's vx_clear: the two files are compiled together.  Test infrastructure:
// tests/sectors_twin.py builds it, tests/cpp/sectors_ref_check.c runs it under the sanitizers.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

int vx_clear(const uint8_t* occ, int W, int H, int ax, int ay, int bx, int by);

static int64_t cross(int64_t px, int64_t py, int64_t qx, int64_t qy) { return px * qy - py * qx; }
static int64_t dot(int64_t px, int64_t py, int64_t qx, int64_t qy) { return px * qx + py * qy; }
static int comp_ok(int64_t v) { return v >= -32767 && v <= 32767; }

// In(d; a, b): 1 / 0, or -1 when the pair (a, b) makes an ignored view
int sx_in(int64_t dx, int64_t dy, int64_t ax, int64_t ay, int64_t bx, int64_t by) {
    const int full = ax == 0 && ay == 0 && bx == 0 && by == 0;
    if (!full) {
        if (!comp_ok(ax) || !comp_ok(ay) || !comp_ok(bx) || !comp_ok(by)) return -1;
        if ((ax == 0 && ay == 0) != (bx == 0 && by == 0)) return -1;
        if (cross(ax, ay, bx, by) == 0 && dot(ax, ay, bx, by) > 0) return -1;
    }
    if (dx == 0 && dy == 0) return 1;
    if (full) return 1;
    const int64_t s = cross(ax, ay, bx, by);
    if (s > 0) return cross(ax, ay, dx, dy) >= 0 && cross(dx, dy, bx, by) > 0;
    if (s < 0) return !(cross(bx, by, dx, dy) >= 0 && cross(dx, dy, ax, ay) > 0);
    return cross(ax, ay, dx, dy) > 0 || (cross(ax, ay, dx, dy) == 0 && dot(ax, ay, dx, dy) > 0);
}

// the heading table's rules: 1 valid, 0 not
int sx_dirs_valid(const int32_t* dirs, int B) {
    if (!dirs || B < 3 || B > 64) return 0;
    for (int i = 0; i < 2 * B; ++i)
        if (!comp_ok(dirs[i])) return 0;
    int leaves = 0;
    for (int b = 0; b < B; ++b) {
        const int n = (b + 1) % B;
        if (cross(dirs[2 * b], dirs[2 * b + 1], dirs[2 * n], dirs[2 * n + 1]) <= 0) return 0;
        const int up = dirs[2 * b + 1] > 0 || (dirs[2 * b + 1] == 0 && dirs[2 * b] > 0);
        const int nup = dirs[2 * n + 1] > 0 || (dirs[2 * n + 1] == 0 && dirs[2 * n] > 0);
        leaves += up && !nup;
    }
    return leaves == 1;
}

// the bins that hold offset d != 0, as a count; *bin receives the first (-1: none).  A valid table gives exactly one.
int sx_bins_of(const int32_t* dirs, int B, int64_t dx, int64_t dy, int* bin) {
    int n = 0;
    *bin = -1;
    if (dx == 0 && dy == 0) return 0;
    for (int b = 0; b < B; ++b) {
        const int nx = (b + 1) % B;
        if (sx_in(dx, dy, dirs[2 * b], dirs[2 * b + 1], dirs[2 * nx], dirs[2 * nx + 1]) == 1) {
            if (n == 0) *bin = b;
            ++n;
        }
    }
    return n;
}

static int64_t isqrt64(int64_t v) {
    int64_t r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

typedef void (*sx_visit)(void* user, size_t cell, int64_t dx, int64_t dy);

// calls visit for every cell sector row s = (cx, cy, r2, ax, ay, bx, by) sees
static void sx_each_seen(const uint8_t* occ, int W, int H, const int32_t* s, sx_visit visit, void* user) {
    const int64_t cx = s[0], cy = s[1], r2 = s[2];
    if (sx_in(0, 0, s[3], s[4], s[5], s[6]) < 0) return;
    if (r2 < 0 || cx < 0 || cy < 0 || cx >= W || cy >= H) return;
    if (occ[(size_t)cy * W + cx] != 0) return;
    const int64_t r = isqrt64(r2);
    const int64_t x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < W - 1 ? cx + r : W - 1;
    const int64_t y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < H - 1 ? cy + r : H - 1;
    for (int64_t y = y0; y <= y1; ++y)
        for (int64_t x = x0; x <= x1; ++x)
            if ((x - cx) * (x - cx) + (y - cy) * (y - cy) <= r2 && sx_in(x - cx, y - cy, s[3], s[4], s[5], s[6]) == 1 &&
                vx_clear(occ, W, H, (int)cx, (int)cy, (int)x, (int)y))
                visit(user, (size_t)y * W + x, x - cx, y - cy);
}

static void mark(void* user, size_t cell, int64_t dx, int64_t dy) {
    (void)dx; (void)dy;
    ((uint8_t*)user)[cell] = 1;
}

// known = base != 0 | vis | surf, occ_seen = known ? occ : 0 (may be NULL).  base may be NULL or known itself.  0, or 1 when
// the vis scratch cannot be allocated.
int sx_known_from_sectors(const uint8_t* base, const uint8_t* occ, const int32_t* sviews, int R, int W, int H, uint8_t* known,
                          uint8_t* occ_seen) {
    const size_t n = (size_t)W * H;
    uint8_t* vis = (uint8_t*)calloc(n, 1);
    if (!vis) return 1;
    for (int v = 0; v < R; ++v) sx_each_seen(occ, W, H, sviews + 7 * (size_t)v, mark, vis);
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
    const int32_t* dirs;
    int B;
    int32_t n, c0;
    int32_t* hist;
};

static void count(void* user, size_t cell, int64_t dx, int64_t dy) {
    (void)dx; (void)dy;
    struct count_unknown* cu = (struct count_unknown*)user;
    cu->n += cu->known[cell] == 0;
}

// gain[i] = the cells with known == 0 that sector row i alone sees
void sx_sector_gain(const uint8_t* occ, const uint8_t* known, const int32_t* sviews, int N, int W, int H, int32_t* gain) {
    for (int i = 0; i < N; ++i) {
        struct count_unknown cu = {known, NULL, 0, 0, 0, NULL};
        sx_each_seen(occ, W, H, sviews + 7 * (size_t)i, count, &cu);
        gain[i] = cu.n;
    }
}

static void count_bin(void* user, size_t cell, int64_t dx, int64_t dy) {
    struct count_unknown* cu = (struct count_unknown*)user;
    if (cu->known[cell] != 0) return;
    if (dx == 0 && dy == 0) { cu->c0 = 1; return; }
    int bin;
    sx_bins_of(cu->dirs, cu->B, dx, dy, &bin);
    if (bin >= 0) cu->hist[bin] += 1;
}

// hist, gainh int32 [N][B] (each may be NULL), best int32 [N][2].  0; 1 for an invalid table or span; 2 without memory.
int sx_view_gain_headings(const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H, const int32_t* dirs, int B,
                          int span, int32_t* hist, int32_t* gainh, int32_t* best) {
    if (!sx_dirs_valid(dirs, B) || span < 1 || span > B) return 1;
    int32_t* row = (int32_t*)malloc((size_t)B * 4);
    if (!row) return 2;
    for (int i = 0; i < N; ++i) {
        const int32_t s[7] = {views[3 * (size_t)i], views[3 * (size_t)i + 1], views[3 * (size_t)i + 2], 0, 0, 0, 0};
        struct count_unknown cu = {known, dirs, B, 0, 0, row};
        memset(row, 0, (size_t)B * 4);
        sx_each_seen(occ, W, H, s, count_bin, &cu);
        int32_t bg = -1, bh = 0;
        for (int h = 0; h < B; ++h) {
            int32_t g = cu.c0;
            for (int j = 0; j < span; ++j) g += row[(h + j) % B];
            if (gainh) gainh[(size_t)i * B + h] = g;
            if (g > bg) { bg = g; bh = h; }
        }
        if (hist) memcpy(hist + (size_t)i * B, row, (size_t)B * 4);
        best[2 * (size_t)i] = bg;
        best[2 * (size_t)i + 1] = bh;
    }
    free(row);
    return 0;
}

void sx_views_from_cells(const int32_t* cell, int N, int W, int H, int32_t r2, int32_t* views) {
    for (int i = 0; i < N; ++i) {
        const int64_t c = cell[i];
        const int ok = c >= 0 && c < (int64_t)W * H;
        views[3 * (size_t)i] = ok ? (int32_t)(c % W) : 0;
        views[3 * (size_t)i + 1] = ok ? (int32_t)(c / W) : 0;
        views[3 * (size_t)i + 2] = ok ? r2 : -1;
    }
}
