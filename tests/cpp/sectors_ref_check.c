/* Stand-alone driver of the C statement of sensors with a field of view (sectors_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -std=c11 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -o sectors_ref_check sectors_ref_check.c \
 *      sectors_ref.c views_ref.c -lm
 * Every array is allocated at its exact size, so a read or write outside it is caught.  The cases: the four predicate cases
 * and every ignored kind; tables of 3, 8, 16 and 64 directions at three phases are valid, their bins partition every offset
 * within 45 cells, and the union of `span` consecutive bins is In(.; u_h, u_{h+span}) for every h and span (the half turn and
 * the reflex case included); reversed, doubled, swapped and repeated tables are refused; on i.i.d. obstacles 130 x 70 and on
 * a 1 x 200 line: a row with a = b = 0 equals the full view, hist + c0 sums to the full gain, gainh[h] equals the sector
 * gain of (u_h, u_{h+span}) and the full gain at span = B, best is the first maximum; rows from cells.  Prints one line per
 * case and "sectors_ref OK"; exit code 1 on the first failed check. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int vx_known_from_views(const uint8_t* base, const uint8_t* occ, const int32_t* views, int R, int W, int H, uint8_t* known,
                        uint8_t* occ_seen);
void vx_view_gain(const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H, int32_t* gain);
int sx_in(int64_t dx, int64_t dy, int64_t ax, int64_t ay, int64_t bx, int64_t by);
int sx_dirs_valid(const int32_t* dirs, int B);
int sx_bins_of(const int32_t* dirs, int B, int64_t dx, int64_t dy, int* bin);
int sx_known_from_sectors(const uint8_t* base, const uint8_t* occ, const int32_t* sviews, int R, int W, int H, uint8_t* known,
                          uint8_t* occ_seen);
void sx_sector_gain(const uint8_t* occ, const uint8_t* known, const int32_t* sviews, int N, int W, int H, int32_t* gain);
int sx_view_gain_headings(const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H, const int32_t* dirs, int B,
                          int span, int32_t* hist, int32_t* gainh, int32_t* best);
void sx_views_from_cells(const int32_t* cell, int N, int W, int H, int32_t r2, int32_t* views);

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

static void table(int B, double phase, int32_t* dirs) {
    const double pi = 3.14159265358979323846;
    for (int b = 0; b < B; ++b) {
        dirs[2 * b] = (int32_t)lround(32767.0 * cos(2 * pi * (b + phase) / B));
        dirs[2 * b + 1] = (int32_t)lround(32767.0 * sin(2 * pi * (b + phase) / B));
    }
}

static int check_table(int B, double phase) {
    int32_t* dirs = (int32_t*)malloc((size_t)B * 8);
    int32_t* bad = (int32_t*)malloc((size_t)B * 16);
    CHECK(dirs && bad);
    table(B, phase, dirs);
    CHECK(sx_dirs_valid(dirs, B));
    for (int dy = -45; dy <= 45; ++dy)
        for (int dx = -45; dx <= 45; ++dx) {
            int bin;
            const int n = sx_bins_of(dirs, B, dx, dy, &bin);
            if (dx == 0 && dy == 0) { CHECK(n == 0 && bin == -1); continue; }
            CHECK(n == 1 && bin >= 0 && bin < B);
            for (int span = 1; span < B; ++span) {   /* the union of span consecutive bins from h holds d iff In(d; u_h, u_{h+span}) */
                for (int h = 0; h < B; ++h) {
                    const int e = (h + span) % B;
                    const int in_union = (bin - h + B) % B < span;
                    CHECK(sx_in(dx, dy, dirs[2 * h], dirs[2 * h + 1], dirs[2 * e], dirs[2 * e + 1]) == in_union);
                }
            }
        }
    /* refused: reversed, doubled (two turns), two entries swapped, a repeated direction, too few, too many, out of range */
    for (int b = 0; b < B; ++b) { bad[2 * b] = dirs[2 * (B - 1 - b)]; bad[2 * b + 1] = dirs[2 * (B - 1 - b) + 1]; }
    CHECK(!sx_dirs_valid(bad, B));
    if (2 * B <= 64) {   /* the table twice over: every step counter-clockwise, two turns */
        for (int b = 0; b < 2 * B; ++b) { bad[2 * b] = dirs[2 * (b % B)]; bad[2 * b + 1] = dirs[2 * (b % B) + 1]; }
        CHECK(!sx_dirs_valid(bad, 2 * B));
    }
    if (B % 2 && B >= 5) {   /* every second direction of an odd table: B distinct entries, every step counter-clockwise, two turns */
        for (int b = 0; b < B; ++b) { bad[2 * b] = dirs[2 * ((2 * b) % B)]; bad[2 * b + 1] = dirs[2 * ((2 * b) % B) + 1]; }
        CHECK(!sx_dirs_valid(bad, B));
    }
    memcpy(bad, dirs, (size_t)B * 8);
    bad[0] = dirs[2]; bad[1] = dirs[3]; bad[2] = dirs[0]; bad[3] = dirs[1];
    CHECK(!sx_dirs_valid(bad, B));
    memcpy(bad, dirs, (size_t)B * 8);
    bad[2] = dirs[0]; bad[3] = dirs[1];
    CHECK(!sx_dirs_valid(bad, B));
    memcpy(bad, dirs, (size_t)B * 8);
    bad[0] = 32768; bad[1] = 0;
    CHECK(!sx_dirs_valid(bad, B) && !sx_dirs_valid(dirs, 2) && !sx_dirs_valid(NULL, B));
    printf("table B = %2d phase %.3f: valid, bins partition +-45, unions of bins are sectors\n", B, phase);
    free(dirs); free(bad);
    return 0;
}

static int check_map(const char* name, const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H, int B, double phase) {
    const size_t n = (size_t)W * H;
    int32_t* dirs = (int32_t*)malloc((size_t)B * 8);
    int32_t* hist = (int32_t*)malloc((size_t)N * B * 4);
    int32_t* gainh = (int32_t*)malloc((size_t)N * B * 4);
    int32_t* best = (int32_t*)malloc((size_t)N * 8);
    int32_t* best2 = (int32_t*)malloc((size_t)N * 8);
    int32_t* full = (int32_t*)malloc((size_t)N * 4);
    int32_t* sg = (int32_t*)malloc((size_t)N * 4);
    int32_t* sv = (int32_t*)malloc((size_t)N * 28);
    uint8_t* k1 = (uint8_t*)malloc(n);
    uint8_t* k2 = (uint8_t*)malloc(n);
    uint8_t* s1 = (uint8_t*)malloc(n);
    uint8_t* s2 = (uint8_t*)malloc(n);
    CHECK(dirs && hist && gainh && best && best2 && full && sg && sv && k1 && k2 && s1 && s2);
    table(B, phase, dirs);
    vx_view_gain(occ, known, views, N, W, H, full);
    /* (c): rows with a = b = 0 are the full views */
    for (int i = 0; i < N; ++i) { memcpy(sv + 7 * i, views + 3 * i, 12); memset(sv + 7 * i + 3, 0, 16); }
    CHECK(sx_known_from_sectors(known, occ, sv, N, W, H, k1, s1) == 0 && vx_known_from_views(known, occ, views, N, W, H, k2, s2) == 0);
    CHECK(memcmp(k1, k2, n) == 0 && memcmp(s1, s2, n) == 0);
    CHECK(sx_known_from_sectors(known, occ, sv, N, W, H, k1, NULL) == 0 && memcmp(k1, k2, n) == 0);
    sx_sector_gain(occ, known, sv, N, W, H, sg);
    CHECK(memcmp(sg, full, (size_t)N * 4) == 0);
    long total = 0;
    const int spans[4] = {1, B / 2, B - 1, B};
    for (int k = 0; k < 4; ++k) {
        const int span = spans[k];
        CHECK(sx_view_gain_headings(occ, known, views, N, W, H, dirs, B, span, hist, gainh, best) == 0);
        CHECK(sx_view_gain_headings(occ, known, views, N, W, H, dirs, B, span, NULL, NULL, best2) == 0 && memcmp(best, best2, (size_t)N * 8) == 0);
        for (int i = 0; i < N; ++i) {
            long sum = 0;
            for (int b = 0; b < B; ++b) sum += hist[i * B + b];
            CHECK(sum == full[i] || sum + 1 == full[i]);                    /* (a), c0 being 0 or 1 */
            int first = 0;
            for (int h = 0; h < B; ++h) {
                if (gainh[i * B + h] > gainh[i * B + first]) first = h;
                if (span == B) CHECK(gainh[i * B + h] == full[i]);
            }
            CHECK(best[2 * i] == gainh[i * B + first] && best[2 * i + 1] == first);
            total += best[2 * i];
        }
        if (span == B) continue;
        for (int h = 0; h < B; ++h) {                                        /* (b) */
            const int e = (h + span) % B;
            for (int i = 0; i < N; ++i) {
                memcpy(sv + 7 * i, views + 3 * i, 12);
                sv[7 * i + 3] = dirs[2 * h]; sv[7 * i + 4] = dirs[2 * h + 1]; sv[7 * i + 5] = dirs[2 * e]; sv[7 * i + 6] = dirs[2 * e + 1];
            }
            sx_sector_gain(occ, known, sv, N, W, H, sg);
            for (int i = 0; i < N; ++i) CHECK(sg[i] == gainh[i * B + h]);
        }
    }
    CHECK(sx_view_gain_headings(occ, known, views, N, W, H, dirs, B, 0, hist, gainh, best) == 1);
    CHECK(sx_view_gain_headings(occ, known, views, N, W, H, dirs, B, B + 1, hist, gainh, best) == 1);
    printf("%-10s %4d x %-4d %2d views, B = %2d: the three identities hold, best gains add up to %ld\n", name, W, H, N, B, total);
    free(dirs); free(hist); free(gainh); free(best); free(best2); free(full); free(sg); free(sv); free(k1); free(k2); free(s1); free(s2);
    return 0;
}

int main(void) {
    /* the predicate: along a (in), along b (out), opposite to a; the four cases; the ignored kinds */
    CHECK(sx_in(3, 0, 1, 0, 0, 1) == 1 && sx_in(0, 3, 1, 0, 0, 1) == 0 && sx_in(-3, 0, 1, 0, 0, 1) == 0 && sx_in(2, 2, 1, 0, 0, 1) == 1);      /* s > 0 */
    CHECK(sx_in(0, 3, 0, 1, 1, 0) == 1 && sx_in(3, 0, 0, 1, 1, 0) == 0 && sx_in(0, -3, 0, 1, 1, 0) == 1 && sx_in(2, 2, 0, 1, 1, 0) == 0);      /* s < 0 */
    CHECK(sx_in(3, 0, 1, 0, -1, 0) == 1 && sx_in(-3, 0, 1, 0, -1, 0) == 0 && sx_in(0, 3, 1, 0, -1, 0) == 1 && sx_in(0, -3, 1, 0, -1, 0) == 0);  /* half a turn */
    CHECK(sx_in(-5, -7, 0, 0, 0, 0) == 1 && sx_in(0, 0, 1, 0, 0, 1) == 1 && sx_in(0, 0, 0, 1, 1, 0) == 1);                                     /* full circle; the centre */
    CHECK(sx_in(1, 0, 1, 0, 2, 0) == -1 && sx_in(1, 0, 3, 3, 3, 3) == -1 && sx_in(0, 0, 1, 0, 0, 0) == -1 && sx_in(0, 0, 0, 0, 0, 1) == -1);
    CHECK(sx_in(0, 0, 32768, 0, 0, 1) == -1 && sx_in(0, 0, 1, 0, 0, -32768) == -1 && sx_in(1, 1, 32767, -32767, -32767, 32767) == 1);
    const int Bs[4] = {3, 8, 16, 64};
    const double phases[3] = {0.0, 0.5, 0.123};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 3; ++j) CHECK(check_table(Bs[i], phases[j]) == 0);
    CHECK(check_table(5, 0.123) == 0 && check_table(13, 0.5) == 0);
    /* i.i.d. obstacles on 130 x 70 */
    {
        enum { W = 130, H = 70 };
        uint8_t* occ = (uint8_t*)malloc((size_t)W * H);
        uint8_t* known = (uint8_t*)malloc((size_t)W * H);
        CHECK(occ && known);
        for (int c = 0; c < W * H; ++c) { occ[c] = rnd() < 0.05 ? (uint8_t)(1 + (int)(rnd() * 200)) : 0; known[c] = rnd() < 0.1 ? 7 : 0; }
        occ[35 * W + 30] = 0; occ[0] = 0; occ[69 * W + 129] = 0; occ[35 * W + 65] = 1; known[0] = 0; known[35 * W + 30] = 1;
        const int32_t views[] = {30, 35, 400,  65, 35, 400 /* on an obstacle */,  0, 0, 100,  129, 69, 81,  -1, 10, 400,  40, 40, -1,  30, 35, 0};
        CHECK(check_map("salt0.05", occ, known, views, 7, W, H, 3, 0.123) == 0);
        CHECK(check_map("salt0.05", occ, known, views, 7, W, H, 8, 0.0) == 0);
        CHECK(check_map("salt0.05", occ, known, views, 7, W, H, 64, 0.5) == 0);
        free(occ); free(known);
    }
    /* lines */
    {
        uint8_t* occ = (uint8_t*)calloc(200, 1);
        uint8_t* known = (uint8_t*)calloc(200, 1);
        CHECK(occ && known);
        occ[80] = occ[150] = 1;
        const int32_t row[] = {50, 0, 10000, 120, 0, 25}, col[] = {0, 50, 10000, 0, 120, 25};
        CHECK(check_map("1 x 200", occ, known, row, 2, 200, 1, 8, 0.0) == 0);
        CHECK(check_map("200 x 1", occ, known, col, 2, 1, 200, 16, 0.123) == 0);
        free(occ); free(known);
    }
    /* rows from cells */
    {
        const int32_t cell[5] = {0, 129, 130 * 70 - 1, -1, 130 * 70};
        int32_t v[15];
        sx_views_from_cells(cell, 5, 130, 70, 100, v);
        const int32_t want[15] = {0, 0, 100, 129, 0, 100, 129, 69, 100, 0, 0, -1, 0, 0, -1};
        CHECK(memcmp(v, want, sizeof want) == 0);
        sx_views_from_cells(cell, 0, 130, 70, 100, NULL);
    }
    printf("sectors_ref OK\n");
    return 0;
}
