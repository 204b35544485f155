/* Stand-alone driver of the C reference of line-of-sight sensing (views_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -std=c11 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -o views_ref_check views_ref_check.c views_ref.c
 * Every array is allocated at its exact size, so a read or write outside the grid is caught.  The small cases: the corner
 * rule; the door map (96 x 64, a wall in column 48 with a door in rows 30 .. 32, the sensor at (20, 31) with r2 = 3600) and
 * its counts; i.i.d. obstacles on 130 x 70 with views that stick out of the grid, stand on obstacles, have a negative radius
 * and the largest radius, checked against the defining properties (vis inside the discs and free, surface cells occupied
 * with a seen neighbour, known = base | vis | surf, occ_seen); a 1 x 200 and a 200 x 1 line; R = 0; base in place; occ_seen
 * NULL; the gain identity with the true map.  Prints one line per case and "views_ref OK"; exit code 1 on the first failed
 * check. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int vx_clear(const uint8_t* occ, int W, int H, int ax, int ay, int bx, int by);
int vx_known_from_views(const uint8_t* base, const uint8_t* occ, const int32_t* views, int R, int W, int H, uint8_t* known,
                        uint8_t* occ_seen);
void vx_view_gain(const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H, int32_t* gain);

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

static int in_a_disc(const int32_t* views, int R, int W, int H, int x, int y) {
    for (int v = 0; v < R; ++v) {
        const int64_t cx = views[3 * v], cy = views[3 * v + 1], r2 = views[3 * v + 2];
        if (r2 < 0 || cx < 0 || cy < 0 || cx >= W || cy >= H) continue;
        if ((x - cx) * (x - cx) + (y - cy) * (y - cy) <= r2) return 1;
    }
    return 0;
}

/* the defining properties of one call, and the gain identity view by view */
static int check_case(const char* name, const uint8_t* occ, const uint8_t* base, const int32_t* views, int R, int W, int H) {
    const size_t n = (size_t)W * H;
    uint8_t* known = (uint8_t*)malloc(n);
    uint8_t* seen = (uint8_t*)malloc(n);
    uint8_t* vis = (uint8_t*)malloc(n);
    uint8_t* lean = (uint8_t*)malloc(n);
    uint8_t* zero = (uint8_t*)calloc(n, 1);
    CHECK(known && seen && vis && lean && zero);
    CHECK(vx_known_from_views(base, occ, views, R, W, H, known, seen) == 0);
    CHECK(vx_known_from_views(base, occ, views, R, W, H, lean, NULL) == 0 && memcmp(lean, known, n) == 0);   /* occ_seen NULL */
    /* vis by the definition, ray by ray */
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int s = 0;
            for (int v = 0; v < R && !s; ++v) {
                const int64_t cx = views[3 * v], cy = views[3 * v + 1], r2 = views[3 * v + 2];
                if (r2 < 0 || cx < 0 || cy < 0 || cx >= W || cy >= H) continue;
                s = (x - cx) * (x - cx) + (y - cy) * (y - cy) <= r2 && vx_clear(occ, W, H, (int)cx, (int)cy, x, y);
            }
            vis[(size_t)y * W + x] = (uint8_t)s;
        }
    int n_vis = 0, n_surf = 0, n_known = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t c = (size_t)y * W + x;
            const int b = base && base[c] != 0;
            const int nb = (x > 0 && vis[c - 1]) || (x + 1 < W && vis[c + 1]) || (y > 0 && vis[c - W]) || (y + 1 < H && vis[c + W]);
            const int surf = occ[c] != 0 && nb;
            if (vis[c]) CHECK(occ[c] == 0 && in_a_disc(views, R, W, H, x, y));
            CHECK(known[c] == (b || vis[c] || surf) && known[c] <= 1);
            CHECK(seen[c] == (known[c] ? occ[c] : 0));
            if (known[c] && !b)                                          /* known \ base lies in the discs dilated by one step */
                CHECK(in_a_disc(views, R, W, H, x, y) || (x > 0 && in_a_disc(views, R, W, H, x - 1, y)) ||
                      (x + 1 < W && in_a_disc(views, R, W, H, x + 1, y)) || (y > 0 && in_a_disc(views, R, W, H, x, y - 1)) ||
                      (y + 1 < H && in_a_disc(views, R, W, H, x, y + 1)));
            n_vis += vis[c]; n_surf += surf; n_known += known[c];
        }
    /* base in place */
    if (base) {
        memcpy(lean, base, n);
        CHECK(vx_known_from_views(lean, occ, views, R, W, H, lean, NULL) == 0 && memcmp(lean, known, n) == 0);
    }
    /* the gain identity with the true map: gain[i] = the free cells view i newly marks */
    int32_t* gain = (int32_t*)malloc((size_t)(R > 0 ? R : 1) * 4);
    CHECK(gain);
    const uint8_t* before = base ? base : zero;
    vx_view_gain(occ, before, views, R, W, H, gain);
    long total = 0;
    for (int v = 0; v < R; ++v) {
        CHECK(vx_known_from_views(before, occ, views + 3 * v, 1, W, H, lean, NULL) == 0);
        int fresh = 0;
        for (size_t c = 0; c < n; ++c) fresh += lean[c] && !before[c] && occ[c] == 0;
        CHECK(gain[v] == fresh);
        total += gain[v];
    }
    printf("%-10s %4d x %-4d %2d views: %6d seen, %5d surface, %6d known, gains add up to %ld\n", name, W, H, R, n_vis, n_surf, n_known, total);
    free(known); free(seen); free(vis); free(lean); free(zero); free(gain);
    return 0;
}

int main(void) {
    /* the corner rule: (5,5) from (4,4) needs both (5,4) and (4,5) */
    {
        uint8_t* occ = (uint8_t*)calloc(81, 1);
        CHECK(occ && vx_clear(occ, 9, 9, 4, 4, 5, 5));
        occ[4 * 9 + 5] = 1;
        CHECK(!vx_clear(occ, 9, 9, 4, 4, 5, 5));
        occ[4 * 9 + 5] = 0; occ[5 * 9 + 4] = 1;
        CHECK(!vx_clear(occ, 9, 9, 4, 4, 5, 5) && vx_clear(occ, 9, 9, 4, 4, 5, 4) && vx_clear(occ, 9, 9, 4, 4, 4, 4));
        CHECK(!vx_clear(occ, 9, 9, 4, 4, 4, 5) && !vx_clear(occ, 9, 9, 4, 5, 4, 5));   /* the target itself, a point on an obstacle */
        free(occ);
    }
    /* the door map and its counts */
    {
        enum { W = 96, H = 64 };
        uint8_t* occ = (uint8_t*)calloc((size_t)W * H, 1);
        uint8_t* known = (uint8_t*)malloc((size_t)W * H);
        CHECK(occ && known);
        for (int y = 0; y < H; ++y) occ[y * W + 48] = (y >= 30 && y <= 32) ? 0 : 1;
        const int32_t view[3] = {20, 31, 3600};
        CHECK(vx_known_from_views(NULL, occ, view, 1, W, H, known, NULL) == 0);
        int n_known = 0, wall = 0, beyond = 0;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                n_known += known[y * W + x];
                wall += x == 48 && known[y * W + x];
                beyond += x >= 49 && known[y * W + x];
            }
        CHECK(n_known == 3276 && wall == 64 && beyond == 140);
        int32_t gain = -1;
        memset(known, 0, (size_t)W * H);
        vx_view_gain(occ, known, view, 1, W, H, &gain);
        CHECK(gain == 3215);
        CHECK(check_case("door", occ, NULL, view, 1, W, H) == 0);
        free(occ); free(known);
    }
    /* i.i.d. obstacles on 130 x 70 with every kind of view */
    for (int round = 0; round < 2; ++round) {
        enum { W = 130, H = 70 };
        const double p = round ? 0.2 : 0.05;
        uint8_t* occ = (uint8_t*)malloc((size_t)W * H);
        uint8_t* base = (uint8_t*)malloc((size_t)W * H);
        CHECK(occ && base);
        for (int c = 0; c < W * H; ++c) { occ[c] = rnd() < p ? (uint8_t)(1 + (int)(rnd() * 200)) : 0; base[c] = rnd() < 0.1 ? 7 : 0; }
        occ[35 * W + 30] = 0; occ[0] = 0; occ[69 * W + 129] = 0; occ[35 * W + 65] = 1;
        const int32_t views[] = {30, 35, 400,  65, 35, 400 /* on an obstacle */,  0, 0, 100,  129, 69, 81,  -1, 10, 400,  130, 10, 400,
                                 10, -1, 400,  10, 70, 400,  40, 40, -1,  30, 35, 0,  30, 35, 2147483647};
        CHECK(check_case(round ? "salt0.2" : "salt0.05", occ, NULL, views, 10, W, H) == 0);
        CHECK(check_case("with base", occ, base, views, 10, W, H) == 0);
        CHECK(check_case("largest r2", occ, base, views + 30, 1, W, H) == 0);
        CHECK(check_case("R = 0", occ, base, views, 0, W, H) == 0);
        free(occ); free(base);
    }
    /* lines */
    {
        uint8_t* occ = (uint8_t*)calloc(200, 1);
        CHECK(occ);
        occ[80] = occ[150] = 1;
        const int32_t row[] = {50, 0, 10000, 120, 0, 25}, col[] = {0, 50, 10000, 0, 120, 25};
        CHECK(check_case("1 x 200", occ, NULL, row, 2, 200, 1) == 0);
        CHECK(check_case("200 x 1", occ, NULL, col, 2, 1, 200) == 0);
        uint8_t known[200];
        CHECK(vx_known_from_views(NULL, occ, row, 1, 200, 1, known, NULL) == 0);
        for (int x = 0; x < 200; ++x) CHECK(known[x] == (x <= 80));      /* the wall cell is surface, nothing behind it */
        free(occ);
    }
    printf("views_ref OK\n");
    return 0;
}
