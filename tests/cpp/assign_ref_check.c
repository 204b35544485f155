// assign_ref_check.c -- stand-alone check of tests/cpp/assign_ref.c, built with -fsanitize=address,undefined by
// tests/test_assign_ref.py (a program of its own: nothing loaded into Python is sanitised).  It runs the reference on the hand
// cases of the definition, on random shapes of every cost kind and forbidden fraction, and on i * j at 256 x 256 (which attains
// the step bound), and checks each result with the certificate of include/sea_current_hip.h in exact integers.
// Exit code 0 and "assign_ref OK" = all passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define BIG (1ll << 42)
#define INF INT32_MAX

void assign_ref(const int32_t* cost, int B, int R, int C, int32_t* col_of, int32_t* row_of, int64_t* u, int64_t* v, int64_t* info,
                int64_t* max_raw);
void field_cost_matrix_ref(const int32_t* g, int F, int W, int H, const int32_t* cell, int R, const int32_t* col_cost, int32_t* cost);

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); exit(1); }         \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd(void) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static int64_t pad(int32_t c) { return c == INF ? BIG : c; }

struct result { int32_t *col_of, *row_of; int64_t *u, *v, info[4]; };

static struct result solve(const int32_t* cost, int R, int C, int64_t* max_raw) {
    struct result o;
    o.col_of = malloc(sizeof(int32_t) * R); o.row_of = malloc(sizeof(int32_t) * C);
    o.u = malloc(sizeof(int64_t) * R); o.v = malloc(sizeof(int64_t) * C);
    assign_ref(cost, 1, R, C, o.col_of, o.row_of, o.u, o.v, o.info, max_raw);
    return o;
}

static void drop(struct result* o) { free(o->col_of); free(o->row_of); free(o->u); free(o->v); }

static void certificate(const int32_t* cost, int R, int C, const struct result* o) {
    const int n = R < C ? R : C;
    int64_t matched = 0, total = 0, su = 0, sv = 0, loose = 0;
    CHECK(o->info[3] == 0 && o->info[2] <= (int64_t)n * (n + 1) / 2);
    for (int r = 0; r < R; ++r) {
        su += o->u[r];
        if (o->col_of[r] < 0) continue;
        CHECK(o->col_of[r] < C && o->row_of[o->col_of[r]] == r && cost[(size_t)r * C + o->col_of[r]] != INF);
        ++matched;
        total += cost[(size_t)r * C + o->col_of[r]];
    }
    for (int c = 0; c < C; ++c) {
        sv += o->v[c];
        if (o->row_of[c] >= 0) CHECK(o->row_of[c] < R && o->col_of[o->row_of[c]] == c);
    }
    CHECK(matched == o->info[0] && total == o->info[1]);
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < C; ++c) CHECK(o->u[r] + o->v[c] <= pad(cost[(size_t)r * C + c]));
    if (R <= C) {
        for (int c = 0; c < C; ++c) { CHECK(o->v[c] <= 0); loose += o->row_of[c] < 0 && o->v[c] != 0; }
    } else {
        for (int r = 0; r < R; ++r) { CHECK(o->u[r] <= 0); loose += o->col_of[r] < 0 && o->u[r] != 0; }
    }
    CHECK(loose <= n - matched);
    CHECK(su + sv == total + BIG * (n - matched));
}

static void fill(int32_t* cost, int R, int C, int kind, int forbidden_pct) {
    for (long k = 0; k < (long)R * C; ++k) {
        int32_t c;
        if (kind == 0) c = (int32_t)(rnd() % 4);
        else if (kind == 1) c = (int32_t)(rnd() % 1000);
        else if (kind == 2) c = (int32_t)(10 * (rnd() % 200) + 14 * (rnd() % 200));
        else c = (int32_t)(rnd() % INF);
        if ((int)(rnd() % 100) < forbidden_pct) c = INF;
        cost[k] = c;
    }
}

int main(void) {
    // the unique optimum
    const int32_t hand[9] = {4, 1, 3, 2, 0, 5, 3, 2, 2};
    struct result o = solve(hand, 3, 3, NULL);
    CHECK(o.col_of[0] == 1 && o.col_of[1] == 0 && o.col_of[2] == 2 && o.info[0] == 3 && o.info[1] == 5);
    certificate(hand, 3, 3, &o);
    drop(&o);
    // random shapes, every kind and forbidden fraction; a forbidden row and column; the transpose
    static const int shapes[][2] = {{1, 1}, {1, 5}, {5, 1}, {6, 7}, {7, 6}, {17, 64}, {64, 17}, {65, 65}, {100, 130}, {130, 100}};
    static const int pct[] = {0, 10, 50, 90, 100};
    int64_t max_raw = 0;
    for (unsigned s = 0; s < sizeof(shapes) / sizeof(shapes[0]); ++s)
        for (int kind = 0; kind < 4; ++kind)
            for (int f = 0; f < 5; ++f) {
                const int R = shapes[s][0], C = shapes[s][1];
                int32_t *cost = malloc(sizeof(int32_t) * R * C), *t = malloc(sizeof(int32_t) * R * C);
                fill(cost, R, C, kind, pct[f]);
                if (f == 1) for (int c = 0; c < C; ++c) cost[(size_t)(R / 2) * C + c] = INF;
                if (f == 2) for (int r = 0; r < R; ++r) cost[(size_t)r * C + C / 2] = INF;
                o = solve(cost, R, C, &max_raw);
                certificate(cost, R, C, &o);
                if (f == 4) CHECK(o.info[0] == 0 && o.info[1] == 0);
                for (int r = 0; r < R; ++r)
                    for (int c = 0; c < C; ++c) t[(size_t)c * R + r] = cost[(size_t)r * C + c];
                struct result ot = solve(t, C, R, NULL);
                certificate(t, C, R, &ot);
                if (R != C) {   // the same lines and posts, so the same run; a square matrix and its transpose may differ under ties
                    CHECK(!memcmp(o.col_of, ot.row_of, sizeof(int32_t) * R) && !memcmp(o.row_of, ot.col_of, sizeof(int32_t) * C));
                    CHECK(!memcmp(o.u, ot.v, sizeof(int64_t) * R) && !memcmp(o.v, ot.u, sizeof(int64_t) * C) && !memcmp(o.info, ot.info, 32));
                }
                drop(&o); drop(&ot); free(cost); free(t);
            }
    CHECK(max_raw < (1ll << 53));   // the key (minv << 10) | j of the library's reduction fits 64 bits
    // a negative entry: that problem alone is bad
    int32_t three[3 * 6];
    fill(three, 3, 6, 1, 0);
    three[6 + 4] = -5;
    int32_t co[9], ro[6];
    int64_t u[9], v[6], info[12];
    assign_ref(three, 3, 3, 2, co, ro, u, v, info, NULL);
    CHECK(info[3] == 0 && info[7] == 1 && info[11] == 0 && info[4] == 0 && info[5] == 0 && info[6] == 0);
    CHECK(co[3] == -1 && co[4] == -1 && co[5] == -1 && ro[2] == -1 && ro[3] == -1 && u[3] == 0 && v[2] == 0);
    // i * j attains the step bound
    {
        const int n = 256;
        int32_t* cost = malloc(sizeof(int32_t) * n * n);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) cost[(size_t)i * n + j] = i * j;
        o = solve(cost, n, n, &max_raw);
        certificate(cost, n, n, &o);
        CHECK(o.info[2] == (int64_t)n * (n + 1) / 2);
        drop(&o); free(cost);
    }
    // the matrix taken from fields
    {
        int32_t g[2 * 12], cell[5] = {0, 11, -1, 12, 5}, cc[2] = {7, 1 << 24}, m[10];
        for (int k = 0; k < 24; ++k) g[k] = k;
        g[23] = INF;
        g[12 + 5] = INF - 10;
        field_cost_matrix_ref(g, 2, 4, 3, cell, 5, NULL, m);
        CHECK(m[0] == 0 && m[1] == 12 && m[2] == 11 && m[3] == INF && m[4] == INF && m[5] == INF && m[6] == INF && m[7] == INF &&
              m[8] == 5 && m[9] == INF - 10);
        field_cost_matrix_ref(g, 2, 4, 3, cell, 5, cc, m);
        CHECK(m[0] == 7 && m[1] == 12 + (1 << 24) && m[2] == 18 && m[3] == INF && m[8] == 12 && m[9] == INF - 1);
    }
    printf("largest lazy key value 2^%.1f\n", max_raw > 0 ? __builtin_log2((double)max_raw) : 0.0);
    printf("assign_ref OK\n");
    return 0;
}
