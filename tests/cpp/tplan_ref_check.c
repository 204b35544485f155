/* Stand-alone driver of the CPU reference of the space-time re-planning (tplan_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -std=c11 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o tplan_ref_check \
 *      tests/cpp/tplan_ref_check.c tests/cpp/tplan_ref.c -lm
 * The corridor with a pocket by hand (the robot steps in, waits and arrives at layer 17; without the pocket there is no path),
 * then seeded random grids and fleets at widths around a word: every path is a legal move sequence from start to goal that
 * starts at t_start, steps only onto cells unreserved at their layer, stays at a goal that is never reserved again, has len = arrive - t_start + 1, and its knots are the
 * centres; statuses other than OK leave NaN rows; sequential robots find their predecessors' rows reserved.  Prints one line
 * per case and "tplan_ref OK"; exit code 1 on the first failed check. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void tp_moves(const int32_t* d2, int W, int H, int32_t r2_clear, uint8_t* moves);
void tp_fleet_replan(const double* knots, int32_t* tstatus, int P, int K, const double* radius, const int32_t* select, double pad, int W, int H,
                     float x_min, float y_min, float res_x, float res_y, uint32_t* res, const int32_t* d2, int32_t r2_clear, const int32_t* start,
                     const int32_t* goal, const int32_t* t_start, int B, int hold, int32_t* path, int32_t* len, int32_t* arrive, int32_t* status,
                     double* knots_out, uint32_t* reach, const double* r_new, int sequential);

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

static int resbit(const uint32_t* res, int W, int H, int t, int c) {
    const int Wq = (W + 31) / 32;
    return (int)(res[((size_t)t * H + c / W) * Wq + (c % W >> 5)] >> (c % W & 31) & 1u);
}

static int corridor(int pocket) {
    enum { W = 11, H = 4, L = 24 };
    int32_t d2[W * H] = {0};
    for (int x = 0; x < W; ++x) d2[2 * W + x] = 1;
    if (pocket) d2[3] = d2[W + 3] = 1;
    double knots[L][2];
    for (int k = 0; k < L; ++k) { knots[k][0] = (k < W ? W - 1 - k : 0) + 0.5; knots[k][1] = 2.5; }
    const double radius = 0.3, pad = 0.3 + sqrt(2.0) / 2 * (1 + ldexp(1.0, -20));
    const int32_t start = 2 * W, goal = 2 * W + W - 1;
    int32_t path[L], len, arrive, status;
    double ko[L][2];
    static uint32_t res[L * H], reach[L * H];
    memset(res, 0, sizeof res);
    tp_fleet_replan(&knots[0][0], NULL, 1, L - 1, &radius, NULL, pad, W, H, 0.f, 0.f, 1.f, 1.f, res, d2, 0, &start, &goal, NULL, 1, 1, path, &len,
                    &arrive, &status, &ko[0][0], reach, NULL, 0);
    if (!pocket) {
        CHECK(status == 1 && arrive == -1 && len == 0 && isnan(ko[0][0]) && isnan(ko[L - 1][1]));
        printf("corridor, head-on: no path\n");
        return 0;
    }
    CHECK(status == 0 && arrive == 17 && len == 18);
    CHECK(path[3] == 2 * W + 3 && path[4] == W + 3 && path[5] == 3 && path[8] == 3 && path[9] == W + 3 && path[10] == 2 * W + 3 && path[17] == goal);
    CHECK(ko[4][0] == 3.5 && ko[4][1] == 1.5 && ko[23][0] == 10.5 && ko[23][1] == 2.5);
    printf("corridor with a pocket: arrive %d, waits at cell 3 from layer 5 to 8\n", arrive);
    return 0;
}

static int fleet(int W, int H, int L, int P, int B, int hold, int sequential) {
    const int Wq = (W + 31) / 32, K = L - 1;
    const float x_min = -1.f, y_min = 2.f, rx = 0.05f, ry = 0.07f;
    int32_t* d2 = malloc(sizeof(int32_t) * W * H);
    for (int i = 0; i < W * H; ++i) d2[i] = rnd() >= 0.12;
    uint8_t* mv = malloc((size_t)W * H);
    tp_moves(d2, W, H, 0, mv);
    double* knots = malloc(sizeof(double) * P * L * 2);
    double* radius = malloc(sizeof(double) * P);
    int32_t* tstatus = calloc(P, sizeof(int32_t));
    for (int p = 0; p < P; ++p) {
        double x = x_min + rnd() * W * rx, y = y_min + rnd() * H * ry;
        radius[p] = 0.02;
        for (int k = 0; k < L; ++k) {
            x += (rnd() * 2 - 1) * rx;
            y += (rnd() * 2 - 1) * ry;
            const int gone = rnd() < 0.05;
            knots[((size_t)p * L + k) * 2] = gone ? NAN : x;
            knots[((size_t)p * L + k) * 2 + 1] = gone ? NAN : y;
        }
    }
    if (P > 2) { radius[1] = -1.0; tstatus[2] = 1; }
    int32_t *start = malloc(4 * B), *goal = malloc(4 * B), *t_start = malloc(4 * B), *path = malloc(sizeof(int32_t) * B * L), *len = malloc(4 * B),
            *arrive = malloc(4 * B), *status = malloc(4 * B);
    double* r_new = malloc(sizeof(double) * B);
    for (int b = 0; b < B; ++b) {
        start[b] = (int)(rnd() * (W * H + 2)) - 1;
        goal[b] = (int)(rnd() * W * H);
        t_start[b] = (int)(rnd() * (L + 2)) - 1;
        r_new[b] = 0.02;
    }
    double* ko = malloc(sizeof(double) * B * L * 2);
    uint32_t* res = calloc((size_t)L * H * Wq, 4);
    uint32_t* reach = malloc((size_t)(sequential ? 1 : B) * L * H * Wq * 4);
    const double pad = 0.02 + sqrt((double)rx * rx + (double)ry * ry) / 2;
    tp_fleet_replan(knots, tstatus, P, K, radius, NULL, pad, W, H, x_min, y_min, rx, ry, res, d2, 0, start, goal, t_start, B, hold, path, len,
                    arrive, status, ko, reach, r_new, sequential);
    if (P > 2) CHECK(tstatus[0] == 0 && tstatus[1] == 2 && tstatus[2] == 1);
    int n_ok = 0, n_wait = 0, count[4] = {0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
        CHECK(status[b] >= 0 && status[b] <= 3);
        count[status[b]]++;
        const double* row = ko + (size_t)b * L * 2;
        if (status[b] != 0) {
            CHECK(len[b] == 0 && arrive[b] == -1);
            for (int t = 0; t < 2 * L; ++t) CHECK(isnan(row[t]));
            continue;
        }
        ++n_ok;
        const int32_t* p = path + (size_t)b * L;
        CHECK(len[b] == arrive[b] - t_start[b] + 1 && len[b] >= 1 && p[0] == start[b] && p[len[b] - 1] == goal[b]);
        for (int i = 0; i < len[b]; ++i) {
            const int t = t_start[b] + i;
            CHECK(p[i] >= 0 && p[i] < W * H && d2[p[i]] >= 1);
            if (!sequential) CHECK(!resbit(res, W, H, t, p[i]));
            CHECK(row[2 * t] == (double)(x_min + ((float)(p[i] % W) + 0.5f) * rx) && row[2 * t + 1] == (double)(y_min + ((float)(p[i] / W) + 0.5f) * ry));
            if (i == 0) continue;
            const int dx = p[i] % W - p[i - 1] % W, dy = p[i] / W - p[i - 1] / W;
            if (dx == 0 && dy == 0) { ++n_wait; continue; }
            int legal = 0;
            static const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1}, DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
            for (int d = 0; d < 8; ++d) legal |= DX[d] == dx && DY[d] == dy && (mv[p[i - 1]] >> d & 1);
            CHECK(legal);
        }
        for (int t = 0; t < t_start[b]; ++t) CHECK(isnan(row[2 * t]));
        for (int t = arrive[b] + 1; t < L; ++t) {
            if (!hold) CHECK(isnan(row[2 * t]));
            else if (!sequential) CHECK(!resbit(res, W, H, t, goal[b]));   /* it stays: the goal is never reserved again */
        }
    }
    /* with sequential every OK robot's own cells are reserved afterwards */
    if (sequential)
        for (int b = 0; b < B; ++b)
            for (int i = 0; status[b] == 0 && i < len[b]; ++i) CHECK(resbit(res, W, H, t_start[b] + i, path[(size_t)b * L + i]));
    printf("fleet %d x %d, L %d, P %d, B %d, hold %d, sequential %d: ok %d, no path %d, bad endpoint %d, start blocked %d, waits %d\n", W, H, L, P, B,
           hold, sequential, n_ok, count[1], count[2], count[3], n_wait);
    free(d2); free(mv); free(knots); free(radius); free(tstatus); free(start); free(goal); free(t_start); free(path); free(len); free(arrive);
    free(status); free(r_new); free(ko); free(res); free(reach);
    return 0;
}

int main(void) {
    if (corridor(0) || corridor(1)) return 1;
    static const int cfg[][7] = {{1, 1, 2, 1, 4, 1, 0}, {31, 9, 30, 3, 12, 1, 0}, {32, 9, 30, 3, 12, 0, 0}, {33, 20, 60, 5, 16, 1, 1},
                                 {70, 45, 100, 12, 24, 1, 0}, {65, 33, 80, 8, 20, 0, 1}};
    for (unsigned i = 0; i < sizeof cfg / sizeof cfg[0]; ++i)
        if (fleet(cfg[i][0], cfg[i][1], cfg[i][2], cfg[i][3], cfg[i][4], cfg[i][5], cfg[i][6])) return 1;
    printf("tplan_ref OK\n");
    return 0;
}
