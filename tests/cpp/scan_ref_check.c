/* Stand-alone driver of the C statement of the range-scan calls (scan_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -std=c11 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -o scan_ref_check scan_ref_check.c scan_ref.c
 * Every array is allocated at its exact size, so a read or write outside the grid is caught.  The cases: the corner rule and
 * its order; the door map (96 x 64, a wall in column 48 with a door in rows 30 .. 32) with the fan of half-side 60 from
 * (20, 31) and its counts; fan coverage on a free 41 x 41 grid from the centre and from (3, 2); i.i.d. obstacles on 130 x 70
 * with fans that stick out of the grid on every side, every ignored kind of beam, and soundness of cast -> update; hit wins,
 * one update per cell, clamping, a map outside the clamp, L NULL, in place, N = 0; a 1 x 200 and a 200 x 1 line; rays at the
 * reach limit with INT32 ends.  Prints one line per case and "scan_ref OK"; exit code 1 on the first failed check. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int sx_ray_ok(const int32_t* ray, int W, int H);
int sx_walk(const int32_t* ray, int W, int H, int32_t* cells, int cap);
void sx_cast(const uint8_t* occ, const int32_t* rays, int N, int W, int H, int32_t* hit);
int sx_update(const int32_t* L, const int32_t* rays, const int32_t* hit, int N, int W, int H, int32_t l_hit, int32_t l_miss,
              int32_t l_clamp, int32_t t_occ, int32_t t_free, int32_t* Lout, uint8_t* occ_est, uint8_t* known);

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

/* the 8 r rays from (cx, cy) to the perimeter of the square of half-side r; exact size */
static int32_t* square_fan(int cx, int cy, int r) {
    int32_t* rays = (int32_t*)malloc((size_t)8 * r * 16);
    if (!rays) return NULL;
    int k = 0;
    for (int t = -r; t < r; ++t, ++k) { rays[4 * k + 2] = cx + t; rays[4 * k + 3] = cy - r; }
    for (int t = -r; t < r; ++t, ++k) { rays[4 * k + 2] = cx + r; rays[4 * k + 3] = cy + t; }
    for (int t = -r; t < r; ++t, ++k) { rays[4 * k + 2] = cx - t; rays[4 * k + 3] = cy + r; }
    for (int t = -r; t < r; ++t, ++k) { rays[4 * k + 2] = cx - r; rays[4 * k + 3] = cy - t; }
    for (k = 0; k < 8 * r; ++k) { rays[4 * k] = cx; rays[4 * k + 1] = cy; }
    return rays;
}

/* cast N rays on occ, update a fresh map with (2, 1, 8, 2, 1): soundness, and the outputs against L */
static int cast_update_case(const char* name, const uint8_t* occ, const int32_t* rays, int N, int W, int H) {
    const size_t n = (size_t)W * H;
    int32_t* hit = (int32_t*)malloc((size_t)(N > 0 ? N : 1) * 4);
    int32_t* L = (int32_t*)malloc(n * 4);
    int32_t* L2 = (int32_t*)malloc(n * 4);
    uint8_t* est = (uint8_t*)malloc(n);
    uint8_t* known = (uint8_t*)malloc(n);
    CHECK(hit && L && L2 && est && known);
    sx_cast(occ, rays, N, W, H, hit);
    int hits = 0, none = 0, ign = 0;
    for (int k = 0; k < N; ++k) {
        CHECK(hit[k] >= -2 && hit[k] < (int64_t)n);
        if (hit[k] >= 0) CHECK(occ[hit[k]] != 0);
        if (hit[k] == -2) CHECK(!sx_ray_ok(rays + 4 * k, W, H) || occ[(size_t)rays[4 * k + 1] * W + rays[4 * k]] != 0);
        hits += hit[k] >= 0; none += hit[k] == -1; ign += hit[k] == -2;
    }
    CHECK(sx_update(NULL, rays, hit, N, W, H, 2, 1, 8, 2, 1, L, est, known) == 0);
    int missed = 0, struck = 0;
    for (size_t c = 0; c < n; ++c) {
        CHECK(L[c] == 0 || L[c] == 2 || L[c] == -1);
        if (L[c] == 2) CHECK(occ[c] != 0);                                /* soundness: a hit cell is occupied */
        if (L[c] == -1) CHECK(occ[c] == 0);                               /*            a missed cell is free  */
        CHECK(est[c] == (L[c] >= 2) && known[c] == (L[c] != 0));
        missed += L[c] == -1; struck += L[c] == 2;
    }
    /* the same scan again, in place, optional outputs NULL: one more update per touched cell */
    memcpy(L2, L, n * 4);
    CHECK(sx_update(L2, rays, hit, N, W, H, 2, 1, 8, 2, 1, L2, NULL, NULL) == 0);
    for (size_t c = 0; c < n; ++c) CHECK(L2[c] == 2 * L[c]);
    /* N = 0: the stored map -> masks, clamped */
    CHECK(sx_update(L2, NULL, NULL, 0, W, H, 2, 1, 1, 2, 1, L, est, known) == 0);
    for (size_t c = 0; c < n; ++c) CHECK(L[c] == (L2[c] > 1 ? 1 : L2[c] < -1 ? -1 : L2[c]) && est[c] == 0 && known[c] == (L[c] == -1));
    printf("%-10s %4d x %-4d %5d beams: %5d hits, %5d no-returns, %4d ignored, %6d cells missed, %5d hit\n", name, W, H, N, hits, none, ign,
           missed, struck);
    free(hit); free(L); free(L2); free(est); free(known);
    return 0;
}

int main(void) {
    /* the corner rule and its order: from (4,4) towards (6,6) the walk is (4,4) (4,5) | (5,4) (5,5) (5,6) | (6,5) (6,6) */
    {
        uint8_t* occ = (uint8_t*)calloc(81, 1);
        int32_t cells[16], hit = 7;
        const int32_t ray[4] = {4, 4, 6, 6};
        CHECK(occ && sx_walk(ray, 9, 9, cells, 16) == 7);
        const int32_t want[7] = {4 * 9 + 4, 5 * 9 + 4, 4 * 9 + 5, 5 * 9 + 5, 6 * 9 + 5, 5 * 9 + 6, 6 * 9 + 6};
        CHECK(memcmp(cells, want, sizeof want) == 0);
        sx_cast(occ, ray, 1, 9, 9, &hit);
        CHECK(hit == -1);
        occ[4 * 9 + 5] = 1; sx_cast(occ, ray, 1, 9, 9, &hit); CHECK(hit == 4 * 9 + 5);                      /* (5,4) */
        occ[5 * 9 + 4] = 1; sx_cast(occ, ray, 1, 9, 9, &hit); CHECK(hit == 5 * 9 + 4);                      /* both: (4,5) comes first */
        occ[4 * 9 + 5] = 0; sx_cast(occ, ray, 1, 9, 9, &hit); CHECK(hit == 5 * 9 + 4);                      /* (4,5) */
        occ[4 * 9 + 4] = 1; sx_cast(occ, ray, 1, 9, 9, &hit); CHECK(hit == -2);                             /* the sensor on an obstacle */
        free(occ);
    }
    /* the door map and its counts */
    {
        enum { W = 96, H = 64, N = 480 };
        uint8_t* occ = (uint8_t*)calloc((size_t)W * H, 1);
        int32_t* rays = square_fan(20, 31, 60);
        int32_t* hit = (int32_t*)malloc(N * 4);
        int32_t* L = (int32_t*)malloc((size_t)W * H * 4);
        CHECK(occ && rays && hit && L);
        for (int y = 0; y < H; ++y) occ[y * W + 48] = (y >= 30 && y <= 32) ? 0 : 1;
        sx_cast(occ, rays, N, W, H, hit);
        CHECK(sx_update(NULL, rays, hit, N, W, H, 2, 1, 8, 2, 1, L, NULL, NULL) == 0);
        int hits = 0, none = 0, missed = 0, struck = 0, wall = 0, beyond = 0;
        for (int k = 0; k < N; ++k) { hits += hit[k] >= 0; none += hit[k] == -1; }
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int32_t l = L[y * W + x];
                missed += l == -1; struck += l == 2; wall += x == 48 && l == 2; beyond += x >= 49 && l == -1;
            }
        CHECK(hits == 130 && none == 350 && missed == 3255 && struck == 61 && wall == 61 && beyond == 180);
        CHECK(cast_update_case("door", occ, rays, N, W, H) == 0);
        free(occ); free(rays); free(hit); free(L);
    }
    /* fan coverage on a free grid: exactly the square, clipped */
    for (int round = 0; round < 2; ++round) {
        enum { W = 41, H = 41, R = 13 };
        const int cx = round ? 3 : 20, cy = round ? 2 : 20;
        int32_t* rays = square_fan(cx, cy, R);
        int32_t* hit = (int32_t*)malloc(8 * R * 4);
        int32_t* L = (int32_t*)malloc((size_t)W * H * 4);
        CHECK(rays && hit && L);
        for (int k = 0; k < 8 * R; ++k) hit[k] = -1;
        CHECK(sx_update(NULL, rays, hit, 8 * R, W, H, 2, 1, 8, 2, 1, L, NULL, NULL) == 0);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) CHECK(L[y * W + x] == ((abs(x - cx) <= R && abs(y - cy) <= R) ? -1 : 0));
        printf("fan        from (%d, %d): covers its square\n", cx, cy);
        free(rays); free(hit); free(L);
    }
    /* i.i.d. obstacles on 130 x 70: fans sticking out on every side, every ignored kind */
    for (int round = 0; round < 2; ++round) {
        enum { W = 130, H = 70 };
        const double p = round ? 0.2 : 0.05;
        uint8_t* occ = (uint8_t*)malloc((size_t)W * H);
        CHECK(occ);
        for (int c = 0; c < W * H; ++c) occ[c] = rnd() < p ? (uint8_t)(1 + (int)(rnd() * 200)) : 0;
        occ[35 * W + 30] = 0; occ[0] = 0; occ[69 * W + 129] = 0; occ[35 * W + 65] = 1;
        const int centres[][3] = {{30, 35, 40}, {0, 0, 25}, {129, 69, 25}, {129, 0, 90}, {0, 69, 90}, {65, 35, 20} /* on an obstacle */};
        for (int i = 0; i < 6; ++i) {
            int32_t* rays = square_fan(centres[i][0], centres[i][1], centres[i][2]);
            CHECK(rays && cast_update_case(round ? "salt0.2" : "salt0.05", occ, rays, 8 * centres[i][2], W, H) == 0);
            free(rays);
        }
        const int32_t odd[] = {-1, 10, 5, 10,  130, 10, 5, 10,  10, -1, 10, 5,  10, 70, 10, 5,  30, 35, 30 + 16385, 35,  30, 35, 30, 35 - 16385,
                               30, 35, 30 + 16384, 35 + 16384,  30, 35, 30, 35,  30, 35, INT32_MAX, INT32_MIN,  INT32_MIN, INT32_MAX, 3, 3};
        CHECK(cast_update_case("odd rays", occ, odd, 10, W, H) == 0);
        int32_t hit[10];
        sx_cast(occ, odd, 10, W, H, hit);
        for (int k = 0; k < 10; ++k) CHECK((hit[k] == -2) == (k != 6 && k != 7));
        free(occ);
    }
    /* the update rules on 8 x 1 */
    {
        const int32_t rays[] = {0, 0, 7, 0,  0, 0, 5, 0,  0, 0, 7, 0,  1, 0, 3, 0};
        const int32_t hit[] = {-1, 3, 3, -2};                              /* beam 0 misses cell 3, beams 1 and 2 hit it; beam 3 is ignored */
        const int32_t L0[8] = {100, -100, 7, 7, -8, 0, INT32_MAX, INT32_MIN};
        int32_t L[8];
        uint8_t est[8], known[8];
        CHECK(sx_update(NULL, rays, hit, 4, 8, 1, 5, 3, 8, 5, 3, L, est, known) == 0);
        const int32_t w0[8] = {-3, -3, -3, 5, -3, -3, -3, -3};
        CHECK(memcmp(L, w0, sizeof w0) == 0);                              /* hit wins; one update however many beams cross */
        for (int c = 0; c < 8; ++c) CHECK(est[c] == (c == 3) && known[c] == 1);
        CHECK(sx_update(L0, rays, hit, 4, 8, 1, 5, 3, 8, 5, 3, L, est, known) == 0);
        const int32_t w1[8] = {8, -8, 4, 8, -8, -3, 8, -8};
        CHECK(memcmp(L, w1, sizeof w1) == 0);                              /* clamping at both ends, a map outside the clamp */
        const int32_t off[] = {0, 0, 7, 0};
        const int32_t h6 = 6, far = 5;                                     /* a hit cell on the walk; on 8 x 2, one that is not */
        CHECK(sx_update(NULL, off, &h6, 1, 8, 1, 5, 3, 8, 5, 3, L, NULL, NULL) == 0);
        const int32_t w2[8] = {-3, -3, -3, -3, -3, -3, 5, 0};
        CHECK(memcmp(L, w2, sizeof w2) == 0);
        int32_t L2[16];
        const int32_t h13 = 8 + far;
        CHECK(sx_update(NULL, off, &h13, 1, 8, 2, 5, 3, 8, 5, 3, L2, NULL, NULL) == 0);
        for (int c = 0; c < 16; ++c) CHECK(L2[c] == (c < 8 ? -3 : c == 13 ? 5 : 0));
        const int32_t bad[] = {-3, 16};                                    /* a hit value out of range: the beam is ignored */
        for (int k = 0; k < 2; ++k) {
            CHECK(sx_update(NULL, off, bad + k, 1, 8, 2, 5, 3, 8, 5, 3, L2, NULL, NULL) == 0);
            for (int c = 0; c < 16; ++c) CHECK(L2[c] == 0);
        }
        printf("rules      hit wins, one update per cell, clamps, hit off the walk\n");
    }
    /* lines */
    {
        uint8_t* occ = (uint8_t*)calloc(200, 1);
        CHECK(occ);
        occ[80] = occ[150] = 1;
        const int32_t row[] = {50, 0, 199, 0,  50, 0, -40, 0,  120, 0, 400, 0,  120, 0, 120, 7}, col[] = {0, 50, 0, 199,  0, 50, 0, -40,  0, 120, 0, 400,  0, 120, -7, 120};
        int32_t hit[4];
        sx_cast(occ, row, 4, 200, 1, hit);
        CHECK(hit[0] == 80 && hit[1] == -1 && hit[2] == 150 && hit[3] == -1);
        sx_cast(occ, col, 4, 1, 200, hit);
        CHECK(hit[0] == 80 && hit[1] == -1 && hit[2] == 150 && hit[3] == -1);
        CHECK(cast_update_case("1 x 200", occ, row, 4, 200, 1) == 0);
        CHECK(cast_update_case("200 x 1", occ, col, 4, 1, 200) == 0);
        free(occ);
    }
    printf("scan_ref OK\n");
    return 0;
}
