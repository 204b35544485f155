/* Stand-alone driver of the C statement of coordinated exploration goals by gain (explore_gain_ref.c) for sanitizer runs on
 * the host:
 *   cc -g -O1 -std=c11 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -o explore_gain_ref_check \
 *      explore_gain_ref_check.c explore_gain_ref.c sectors_ref.c views_ref.c -lm
 * Every array is allocated at its exact size, so a read or write outside it is caught.  The cases, on i.i.d. obstacles with a
 * known disc in the middle: full circle and tables of 3, 8 and 64 directions; R > N and N > R; dead candidates of both kinds
 * and two candidates on one cell; every optional output NULL; known_out aliasing known; rounds = 0 and N = 0; refused
 * arguments.  Checked: the gains of the picks add up to the free cells newly known, gains only fall, picks are pairwise
 * different robots and candidates, a dead candidate is never picked, the outputs do not depend on which optional arrays are
 * given; and the centres of a labelled strip.  Prints one line per case and "explore_gain_ref OK"; exit code 1 on the first
 * failed check. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int ex_explore_gain(const uint8_t* occ, const uint8_t* known, const int32_t* g, int R, const int32_t* cand, int N, int W, int H, int32_t r2,
                    const int32_t* dirs, int B, int span, int32_t wg, int32_t wc, int32_t min_gain, int rounds, int32_t* goal, int32_t* gcost,
                    int32_t* ggain, int32_t* head, int32_t* cand_of, int32_t* pick, int32_t* npick, int32_t* gain0, int32_t* gain_end,
                    uint8_t* known_out);
void ex_frontier_centres(const int32_t* slot, const int32_t* csize, const int64_t* csum, int W, int H, int Cmax, int32_t* centre);

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

static void table(int B, int32_t* dirs) {
    const double pi = 3.14159265358979323846;
    for (int b = 0; b < B; ++b) {
        dirs[2 * b] = (int32_t)lround(32767.0 * cos(2 * pi * b / B));
        dirs[2 * b + 1] = (int32_t)lround(32767.0 * sin(2 * pi * b / B));
    }
}

/* Manhattan fields: 10 per step from the robot's cell, the obstacles and the unknown cells unreachable */
static void fields(const uint8_t* occ, const uint8_t* known, int W, int H, const int32_t* robot, int R, int32_t* g) {
    for (int r = 0; r < R; ++r)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t c = (size_t)y * W + x;
                g[(size_t)r * W * H + c] = (occ[c] || !known[c]) ? INT32_MAX : 10 * (abs(x - robot[r] % W) + abs(y - robot[r] / W));
            }
}

static int check_case(const char* name, int W, int H, int R, int N, int32_t r2, int B, int span, int32_t wg, int32_t min_gain) {
    const size_t cells = (size_t)W * H;
    uint8_t* occ = (uint8_t*)malloc(cells);
    uint8_t* known = (uint8_t*)malloc(cells);
    uint8_t* kout = (uint8_t*)malloc(cells);
    uint8_t* kalias = (uint8_t*)malloc(cells);
    int32_t* g = (int32_t*)malloc((size_t)R * cells * 4);
    int32_t* robot = (int32_t*)malloc((size_t)R * 4);
    int32_t* cand = (int32_t*)malloc((size_t)N * 4);
    int32_t* out = (int32_t*)malloc((size_t)R * 6 * 4);   /* goal, gcost, ggain, head, cand_of, pick */
    int32_t* out2 = (int32_t*)malloc((size_t)R * 2 * 4);
    int32_t* gain0 = (int32_t*)malloc((size_t)N * 4);
    int32_t* gain_end = (int32_t*)malloc((size_t)N * 4);
    int32_t* dirs = B ? (int32_t*)malloc((size_t)B * 8) : NULL;
    int32_t npick = -7, npick2 = -7;
    CHECK(occ && known && kout && kalias && g && robot && cand && out && out2 && gain0 && gain_end && (dirs || !B));
    if (B) table(B, dirs);
    for (size_t c = 0; c < cells; ++c) {
        const long x = (long)(c % W) - W / 2, y = (long)(c / W) - H / 2;
        known[c] = x * x + y * y <= 100;
        occ[c] = known[c] && rnd() < 0.1;   /* the observed map: unknown cells read 0 */
    }
    occ[(size_t)(H / 2) * W + W / 2] = 0;
    for (int r = 0; r < R; ++r) robot[r] = (int32_t)((H / 2) * W + W / 2 + (r % 5) - 2);
    fields(occ, known, W, H, robot, R, g);
    for (int n = 0; n < N; ++n) {   /* on the rim of the known disc, where there is something to see */
        const double a = 6.283185307179586 * n / N;
        cand[n] = (int32_t)((H / 2 + (int)lround(9 * sin(a))) * W + W / 2 + (int)lround(9 * cos(a)));
    }
    if (N >= 5) {
        cand[1] = cand[0];
        cand[2] = -1;
        cand[3] = (int32_t)cells;
        for (size_t c = 0; c < cells; ++c)
            if (occ[c]) { cand[4] = (int32_t)c; break; }
    }
    const int32_t* d = dirs;
    CHECK(ex_explore_gain(occ, known, g, R, cand, N, W, H, r2, d, B, span, wg, 1, min_gain, R, out, out + R, out + 2 * R, out + 3 * R,
                          out + 4 * R, out + 5 * R, &npick, gain0, gain_end, kout) == 0);
    /* the optional outputs left out, known_out aliasing known: the mandatory outputs stay */
    memcpy(kalias, known, cells);
    CHECK(ex_explore_gain(occ, kalias, g, R, cand, N, W, H, r2, d, B, span, wg, 1, min_gain, R, out2, out2 + R, NULL, NULL, NULL, NULL, &npick2,
                          NULL, NULL, kalias) == 0);
    CHECK(npick2 == npick && memcmp(out, out2, (size_t)R * 8) == 0 && memcmp(kout, kalias, cells) == 0);
    CHECK(ex_explore_gain(occ, known, g, R, cand, N, W, H, r2, d, B, span, wg, 1, min_gain, R, out2, out2 + R, NULL, NULL, NULL, NULL, &npick2,
                          NULL, NULL, NULL) == 0);
    CHECK(npick2 == npick && memcmp(out, out2, (size_t)R * 8) == 0);
    long sum = 0, fresh = 0;
    int picks = 0;
    for (int r = 0; r < R; ++r) {
        const int32_t n = out[4 * R + r];
        if (out[r] < 0) { CHECK(n == -1 && out[R + r] == -1 && out[2 * R + r] == 0 && out[3 * R + r] == -1 && out[5 * R + r] == -1); continue; }
        ++picks;
        CHECK(n >= 0 && n < N && cand[n] == out[r] && cand[n] >= 0 && (size_t)cand[n] < cells && !occ[cand[n]]);
        CHECK(out[R + r] == g[(size_t)r * cells + cand[n]] && out[2 * R + r] >= min_gain && out[5 * R + r] >= 0 && out[5 * R + r] < npick);
        CHECK(B ? (out[3 * R + r] >= 0 && out[3 * R + r] < B) : out[3 * R + r] == -1);
        for (int q = 0; q < r; ++q) CHECK(out[4 * R + q] != n && (out[q] < 0 || out[5 * R + q] != out[5 * R + r]));
        sum += out[2 * R + r];
    }
    CHECK(picks == npick && npick <= (R < N ? R : N));
    for (size_t c = 0; c < cells; ++c) fresh += !occ[c] && kout[c] && !known[c];
    CHECK(sum == fresh);
    for (int n = 0; n < N; ++n) CHECK(gain_end[n] <= gain0[n] && gain_end[n] >= 0);
    if (N >= 5) CHECK(gain0[2] == 0 && gain0[3] == 0 && gain0[4] == 0 && gain0[1] == gain0[0]);
    /* rounds = 0 and N = 0 pick nothing and leave known as it is */
    CHECK(ex_explore_gain(occ, known, g, R, cand, N, W, H, r2, d, B, span, wg, 1, min_gain, 0, out2, out2 + R, NULL, NULL, NULL, NULL, &npick2,
                          NULL, NULL, kalias) == 0);
    CHECK(npick2 == 0 && memcmp(kalias, known, cells) == 0);
    CHECK(ex_explore_gain(occ, known, g, R, NULL, 0, W, H, r2, d, B, span, wg, 1, min_gain, R, out2, out2 + R, NULL, NULL, NULL, NULL, &npick2,
                          NULL, NULL, kalias) == 0);
    CHECK(npick2 == 0 && out2[0] == -1 && out2[R] == -1 && memcmp(kalias, known, cells) == 0);
    /* refused arguments */
    CHECK(ex_explore_gain(occ, known, g, R, cand, N, W, H, -1, d, B, span, wg, 1, min_gain, R, out2, out2 + R, NULL, NULL, NULL, NULL, &npick2,
                          NULL, NULL, NULL) == 1);
    CHECK(ex_explore_gain(occ, known, g, R, cand, N, W, H, r2, d, B, span, (1 << 20) + 1, 1, min_gain, R, out2, out2 + R, NULL, NULL, NULL, NULL,
                          &npick2, NULL, NULL, NULL) == 1);
    if (B)
        CHECK(ex_explore_gain(occ, known, g, R, cand, N, W, H, r2, d, B, B, wg, 1, min_gain, R, out2, out2 + R, NULL, NULL, NULL, NULL, &npick2,
                              NULL, NULL, NULL) == 1);
    CHECK(ex_explore_gain(occ, known, g, R, cand, N, W, H, r2, d, B, span, wg, 1, min_gain, R, out2, out2 + R, NULL, NULL, NULL, NULL, &npick2,
                          NULL, NULL, occ) == 1);
    printf("%-10s %3d x %-3d R = %2d N = %2d r2 = %3d B = %2d span = %2d: %d picks, their gains add up to %ld = the free cells newly known\n",
           name, W, H, R, N, (int)r2, B, span, (int)npick, sum);
    free(occ); free(known); free(kout); free(kalias); free(g); free(robot); free(cand); free(out); free(out2); free(gain0); free(gain_end);
    free(dirs);
    return 0;
}

static int check_centres(void) {
    /* 9 x 3: cluster 0 is the top row (its centre the middle cell), cluster 1 two cells with a tie (the smaller cell wins),
     * row 2 of the list is empty */
    enum { W = 9, H = 3, C = 3 };
    int32_t* slot = (int32_t*)malloc(W * H * 4);
    int32_t* csize = (int32_t*)calloc(C, 4);
    int64_t* csum = (int64_t*)calloc(2 * C, 8);
    int32_t* centre = (int32_t*)malloc(C * 4);
    CHECK(slot && csize && csum && centre);
    for (int c = 0; c < W * H; ++c) slot[c] = c < W ? 0 : -1;
    slot[2 * W + 3] = slot[2 * W + 4] = 1;
    for (int c = 0; c < W * H; ++c)
        if (slot[c] >= 0) {
            csize[slot[c]] += 1;
            csum[2 * slot[c]] += c % W;
            csum[2 * slot[c] + 1] += c / W;
        }
    ex_frontier_centres(slot, csize, csum, W, H, C, centre);
    CHECK(centre[0] == 4 && centre[1] == 2 * W + 3 && centre[2] == -1);
    printf("centres    9 x 3: the middle of a row, the smaller cell of a tie, -1 for an empty row\n");
    free(slot); free(csize); free(csum); free(centre);
    return 0;
}

int main(void) {
    if (check_case("circle", 65, 63, 3, 9, 36, 0, 0, 2, 1)) return 1;
    if (check_case("circle", 40, 30, 7, 5, 49, 0, 0, 1, 0)) return 1;
    if (check_case("circle", 40, 30, 2, 12, 16, 0, 0, 0, 3)) return 1;
    if (check_case("table", 65, 63, 3, 9, 36, 3, 1, 2, 1)) return 1;
    if (check_case("table", 40, 30, 9, 7, 49, 8, 4, 1, 1)) return 1;
    if (check_case("table", 40, 30, 2, 12, 25, 8, 7, 3, 0)) return 1;
    if (check_case("table", 50, 41, 3, 8, 36, 64, 32, 2, 1)) return 1;
    if (check_centres()) return 1;
    printf("explore_gain_ref OK\n");
    return 0;
}
