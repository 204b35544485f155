/* car_ref_check.c -- drives the C statement of car-like pose planning (car_ref.c) alone, as a program of its own, so that it
 * can run under AddressSanitizer and UBSan: arc masks with and without a footprint mask on grids of odd shapes, fields from and
 * toward the root for every arc_n, with every bad-root kind, read-outs in both orders with a small Lmax and with a wrong
 * (all-ones) arc mask, and the anchor values of DESIGN.md section 32.  Prints "car_ref OK" and returns 0 when every check
 * holds. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int cx_args_ok(int W, int H, int arc_n, int arc_cost, int rev_cost);
int cx_arc_mask(const int32_t* d2, const uint8_t* hmask, int W, int H, int32_t r2, int arc_n, uint16_t* amask);
int cx_car_field(const int32_t* d2, const uint8_t* hmask, int W, int H, int32_t r2, int arc_n, int arc_cost, int rev_cost, int toward,
                 int root, int rhead, int32_t* gp);
int cx_car_paths(const int32_t* d2, const uint8_t* hmask, const uint16_t* amask, int W, int H, int32_t r2, int arc_n, int arc_cost,
                 int rev_cost, int toward, const int32_t* gp, int root, int rhead, const int32_t* target, const int32_t* thead, int Q,
                 int Lmax, int to_root, int32_t* path, uint8_t* head, int32_t* len, int32_t* cost, int32_t* status);

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAILED line %d: %s\n", __LINE__, #c);             \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static uint32_t rnd_state = 54321u;
static uint32_t rnd(void) {
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

static void one_grid(int W, int H, int pct) {
    const int n = W * H, Q = 24, Lmax = 20;
    int32_t* d2 = (int32_t*)malloc(sizeof(int32_t) * n);
    uint8_t* hm = (uint8_t*)malloc(n);
    uint16_t* am = (uint16_t*)malloc(sizeof(uint16_t) * n);
    uint16_t* ones = (uint16_t*)malloc(sizeof(uint16_t) * n);
    int32_t* gp = (int32_t*)malloc(sizeof(int32_t) * 8 * n);
    int32_t* path = (int32_t*)malloc(sizeof(int32_t) * Q * Lmax);
    uint8_t* head = (uint8_t*)malloc(Q * Lmax);
    int32_t target[24], thead[24], len[24], cost[24], status[24];
    for (int i = 0; i < n; ++i) {
        d2[i] = (int)(rnd() % 100) < pct ? 0 : 1 + (int)(rnd() % 5);
        hm[i] = (uint8_t)(rnd() | rnd());   /* most headings fit */
        ones[i] = 0xFFFF;
    }
    for (int q = 0; q < Q; ++q) {
        target[q] = (int)(rnd() % (uint32_t)(n + 2)) - 1;
        thead[q] = (int)(rnd() % 11) - 2;
    }
    const int roots[4] = {-1, n, (int)(rnd() % (uint32_t)n), (int)(rnd() % (uint32_t)n)};
    for (int an = 1; an <= 4; ++an)
        for (int r = 0; r < 4; ++r)
            for (int rh = -2; rh <= 8; rh += 2)
                for (int toward = 0; toward < 2; ++toward)
                    for (int rev = -1; rev <= 7; rev += 4) {
                        const uint8_t* m = (rh & 2) ? hm : NULL;
                        CHECK(cx_arc_mask(d2, m, W, H, 0, an, am) == 0);
                        for (int i = 0; i < n; ++i) CHECK(d2[i] >= 1 || am[i] == 0);
                        const int st = cx_car_field(d2, m, W, H, 0, an, 3, rev, toward, roots[r], rh, gp);
                        CHECK(st == 0 || st == 2);
                        if (st == 2)
                            for (int i = 0; i < 8 * n; ++i) CHECK(gp[i] == INT32_MAX);
                        for (int o = 0; o < 4; ++o) {
                            const uint16_t* a = (o >> 1) ? ones : am;   /* the wrong mask only has to return */
                            CHECK(cx_car_paths(d2, m, a, W, H, 0, an, 3, rev, toward, gp, roots[r], rh, target, thead, Q, Lmax, o & 1, path,
                                               head, len, cost, status) == 0);
                            for (int q = 0; q < Q; ++q) {
                                CHECK(status[q] >= 0 && status[q] <= 3);
                                CHECK((status[q] == 0 || status[q] == 3) ? (len[q] >= 1 && cost[q] >= 0) : (len[q] == 0 && cost[q] == -1));
                                if (st == 2) CHECK(status[q] == 2);
                            }
                        }
                    }
    CHECK(cx_arc_mask(d2, NULL, W, H, 0, 0, am) == 1 && cx_arc_mask(d2, NULL, W, H, 0, 5, am) == 1);
    free(d2); free(hm); free(am); free(ones); free(gp); free(path); free(head);
}

int main(void) {
    /* anchor values: an open 64 x 64 grid, root (32, 32) heading 0, arc_cost 0 */
    enum { S = 64, N = S * S };
    int32_t* d2 = (int32_t*)malloc(sizeof(int32_t) * N);
    int32_t* gp = (int32_t*)malloc(sizeof(int32_t) * 8 * N);
    for (int i = 0; i < N; ++i) d2[i] = 1;
    const int root = 32 * S + 32;
    int inf = 0;
    CHECK(cx_car_field(d2, NULL, S, S, 0, 1, 0, -1, 0, root, 0, gp) == 0);
    CHECK(gp[0 * N + 32 * S + 37] == 50 && gp[4 * N + root] == 220 && gp[0 * N + 33 * S + 32] == 202);
    for (int i = 0; i < 8 * N; ++i) inf += gp[i] == INT32_MAX;
    CHECK(inf == 1340);
    CHECK(cx_car_field(d2, NULL, S, S, 0, 2, 0, -1, 0, root, 0, gp) == 0);
    CHECK(gp[4 * N + root] == 440 && gp[0 * N + 33 * S + 32] == 394);
    inf = 0;
    for (int i = 0; i < 8 * N; ++i) inf += gp[i] == INT32_MAX;
    CHECK(inf == 2800);
    CHECK(cx_car_field(d2, NULL, S, S, 0, 1, 0, 10, 0, root, 0, gp) == 0);
    CHECK(gp[4 * N + root] == 156 && gp[0 * N + 32 * S + 31] == 20 && gp[0 * N + 33 * S + 32] == 102);
    CHECK(cx_car_field(d2, NULL, S, S, 0, 2, 0, 10, 0, root, 0, gp) == 0);
    CHECK(gp[4 * N + root] == 312 && gp[0 * N + 33 * S + 32] == 170);
    /* the argument and overflow rules */
    CHECK(cx_args_ok(9, 9, 1, 0, -1) && cx_args_ok(9, 9, 4, 255, 255) && !cx_args_ok(9, 9, 0, 0, 0) && !cx_args_ok(9, 9, 5, 0, 0));
    CHECK(!cx_args_ok(9, 9, 1, -1, 0) && !cx_args_ok(9, 9, 1, 256, 0) && !cx_args_ok(9, 9, 1, 0, -2) && !cx_args_ok(9, 9, 1, 0, 256));
    CHECK(cx_args_ok(1024, 1024, 1, 232, 0) && !cx_args_ok(1024, 1024, 1, 233, 0) && cx_args_ok(1024, 1024, 1, 232, -1));
    CHECK(cx_args_ok(1024, 1024, 1, 30, 101) && !cx_args_ok(1024, 1024, 1, 31, 101) && !cx_args_ok(8192, 8192, 1, 0, -1));
    CHECK(cx_car_field(d2, NULL, S, S, 0, 5, 0, 0, 0, 0, 0, gp) == -1);
    free(d2);
    free(gp);
    one_grid(33, 31, 10);
    one_grid(1, 70, 3);
    one_grid(70, 1, 3);
    one_grid(20, 20, 45);
    if (fails) {
        printf("car_ref: %d checks failed\n", fails);
        return 1;
    }
    printf("car_ref OK\n");
    return 0;
}
