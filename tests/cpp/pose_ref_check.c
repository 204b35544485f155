/* pose_ref_check.c -- drives the C statement of planning in poses (pose_ref.c) alone, as a program of its own, so that it can
 * run under AddressSanitizer and UBSan: masks of every kind of body on grids of odd shapes, fields with and without a mask,
 * from and toward the root, with every bad-root kind, read-outs in both orders with a small Lmax, and the hand values of the
 * header.  Prints "pose_ref OK" and returns 0 when every check holds. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int px_args_ok(int W, int H, int turn_cost, int rev_cost, int readout);
int px_footprint_mask(const int32_t* d2, int W, int H, int32_t r2, int front, int back, int left, int right, uint8_t* out);
int px_pose_field(const int32_t* d2, const uint8_t* hmask, int W, int H, int32_t r2, int turn_cost, int rev_cost, int toward, int root,
                  int rhead, int32_t* gp);
int px_pose_paths(const int32_t* d2, const uint8_t* hmask, int W, int H, int32_t r2, int turn_cost, int rev_cost, int toward,
                  const int32_t* gp, int root, int rhead, const int32_t* target, const int32_t* thead, int Q, int Lmax, int to_root,
                  int cells_only, int32_t* path, uint8_t* head, int32_t* len, int32_t* cost, int32_t* status);

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAILED line %d: %s\n", __LINE__, #c);             \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static uint32_t rnd_state = 12345u;
static uint32_t rnd(void) {
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

static void one_grid(int W, int H, int pct) {
    const int n = W * H, Q = 24, Lmax = 20;
    int32_t* d2 = (int32_t*)malloc(sizeof(int32_t) * n);
    uint8_t* hm = (uint8_t*)malloc(n);
    int32_t* gp = (int32_t*)malloc(sizeof(int32_t) * 8 * n);
    int32_t* path = (int32_t*)malloc(sizeof(int32_t) * Q * Lmax);
    uint8_t* head = (uint8_t*)malloc(Q * Lmax);
    int32_t target[24], thead[24], len[24], cost[24], status[24];
    for (int i = 0; i < n; ++i) d2[i] = (int)(rnd() % 100) < pct ? 0 : 1 + (int)(rnd() % 5);
    const int exts[5][4] = {{0, 0, 0, 0}, {3, 3, 1, 1}, {5, 0, 2, 1}, {32, 32, 32, 32}, {0, 1, 32, 0}};
    for (int e = 0; e < 5; ++e)
        for (int r2 = 0; r2 <= 2; r2 += 2) CHECK(px_footprint_mask(d2, W, H, r2, exts[e][0], exts[e][1], exts[e][2], exts[e][3], hm) == 0);
    CHECK(px_footprint_mask(d2, W, H, 0, 0, 0, 0, 0, hm) == 0);
    for (int i = 0; i < n; ++i) CHECK(hm[i] == (d2[i] >= 1 ? 0xFF : 0));
    CHECK(px_footprint_mask(d2, W, H, 0, 2, 1, 1, 0, hm) == 0);
    CHECK(px_footprint_mask(d2, W, H, 0, 33, 0, 0, 0, hm) == 1);
    for (int q = 0; q < Q; ++q) {
        target[q] = (int)(rnd() % (uint32_t)(n + 2)) - 1;
        thead[q] = (int)(rnd() % 11) - 2;
    }
    const int roots[4] = {-1, n, (int)(rnd() % (uint32_t)n), (int)(rnd() % (uint32_t)n)};
    for (int r = 0; r < 4; ++r)
        for (int rh = -2; rh <= 8; rh += 2)
            for (int toward = 0; toward < 2; ++toward)
                for (int rev = -1; rev <= 7; rev += 4) {
                    const uint8_t* m = (rh & 2) ? hm : NULL;
                    const int st = px_pose_field(d2, m, W, H, 0, 3, rev, toward, roots[r], rh, gp);
                    CHECK(st == 0 || st == 2);
                    if (st == 2)
                        for (int i = 0; i < 8 * n; ++i) CHECK(gp[i] == INT32_MAX);
                    for (int o = 0; o < 4; ++o) {
                        CHECK(px_pose_paths(d2, m, W, H, 0, 3, rev, toward, gp, roots[r], rh, target, thead, Q, Lmax, o & 1, o >> 1, path, head, len,
                                            cost, status) == 0);
                        for (int q = 0; q < Q; ++q) {
                            CHECK(status[q] >= 0 && status[q] <= 3);
                            CHECK((status[q] == 0 || status[q] == 3) ? (len[q] >= 1 && cost[q] >= 0) : (len[q] == 0 && cost[q] == -1));
                            if (st == 2) CHECK(status[q] == 2);
                        }
                    }
                }
    free(d2); free(hm); free(gp); free(path); free(head);
}

int main(void) {
    /* the hand values of the header: an open 9 x 9 grid, root (4, 4) heading 0, turn_cost 5 */
    int32_t d2[81], gp[8 * 81];
    for (int i = 0; i < 81; ++i) d2[i] = 1;
    CHECK(px_pose_field(d2, NULL, 9, 9, 0, 5, -1, 0, 4 * 9 + 4, 0, gp) == 0);
    CHECK(gp[0 * 81 + 4 * 9 + 6] == 20 && gp[2 * 81 + 6 * 9 + 4] == 30 && gp[4 * 81 + 4 * 9 + 4] == 20);
    CHECK(gp[1 * 81 + 6 * 9 + 6] == 33 && gp[0 * 81 + 6 * 9 + 6] == 38 && gp[0 * 81 + 4 * 9 + 2] == 60);
    CHECK(px_pose_field(d2, NULL, 9, 9, 0, 5, 3, 0, 4 * 9 + 4, 0, gp) == 0 && gp[0 * 81 + 4 * 9 + 2] == 26);
    CHECK(px_args_ok(9, 9, 0, -1, 0) && !px_args_ok(9, 9, 0, -1, 1) && !px_args_ok(9, 9, 256, 0, 0) && !px_args_ok(9, 9, 1, -2, 0));
    CHECK(px_args_ok(1024, 1024, 1, 242, 0) && !px_args_ok(1024, 1024, 1, 243, 0) && !px_args_ok(8192, 8192, 1, -1, 0));
    CHECK(px_pose_field(d2, NULL, 9, 9, 0, 256, 0, 0, 0, 0, gp) == -1);
    one_grid(33, 31, 10);
    one_grid(1, 70, 3);
    one_grid(70, 1, 3);
    one_grid(20, 20, 45);
    if (fails) {
        printf("pose_ref: %d checks failed\n", fails);
        return 1;
    }
    printf("pose_ref OK\n");
    return 0;
}
