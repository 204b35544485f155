/* Stand-alone driver of the CPU twin (field_multi_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o field_multi_ref_check field_multi_ref_check.c field_multi_ref.c
 * Small maps -- i.i.d. obstacles at p = 0.2 on 96 x 80 (unweighted and with a random costmap), the serpentine corridor on
 * 64 x 64, a 1 x 200 and a 200 x 1 line, the plug map (130 x 3, a seed whose only free neighbour is in the next tile), the
 * mirror map (33 x 17, two seeds, 17 tied cells), duplicate / dominated / exactly tied seeds, invalid and empty seed lists
 * -- are run through fm_cost_field and fm_field_paths and the defining properties checked: g is a fixed point of the
 * relaxation with the seeds as sources, the owner is >= 0 exactly where g is finite, a terminal seed owns its cell, every
 * read-out ends at seed[which], which == owner[target], its cost is g[target] and its steps add up to cost -
 * seed_cost[which].  Prints one line per map and "field_multi_ref OK"; exit code 1 on the first failed check. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int fm_cost_field(const int32_t* d2, const uint8_t* pen, int cap, int W, int H, int32_t r2, const int32_t* seed, const int32_t* seed_cost,
                  int n_seed, int s0, int32_t* g, int32_t* owner);
void fm_field_paths(const int32_t* d2, const uint8_t* pen, int cap, int W, int H, int32_t r2, const int32_t* g, const int32_t* seed,
                    const int32_t* seed_cost, int n_seed, int s0, const int32_t* target, int Q, int Lmax, int to_seed, int32_t* path,
                    int32_t* len, int32_t* cost, int32_t* status, int32_t* which);

#define INF INT32_MAX
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

static const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1};
static const int DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};

static int pc(const uint8_t* pen, int cap, int c) { return !pen ? 0 : (pen[c] < cap ? pen[c] : cap); }

/* the cost of the move a -> b, -1 if it is not one legal move */
static int move_cost(const int32_t* d2, const uint8_t* pen, int cap, int W, int H, int a, int b) {
    const int ax = a % W, ay = a / W, bx = b % W, by = b / W, dx = bx - ax, dy = by - ay;
    (void)H;
    if (dx < -1 || dx > 1 || dy < -1 || dy > 1 || (dx == 0 && dy == 0)) return -1;
    if (d2[a] < 1 || d2[b] < 1) return -1;
    if (dx && dy && (d2[ay * W + bx] < 1 || d2[by * W + ax] < 1)) return -1;
    return (dx && dy ? 14 : 10) + pc(pen, cap, b);
}

static int check_map(const char* name, const int32_t* d2, const uint8_t* pen, int cap, int W, int H, const int32_t* seed, const int32_t* cost,
                     int n_seed, int expect_status) {
    const int n = W * H;
    enum { Q = 96, LMAX = 40 };
    int32_t* g = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    int32_t* owner = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    int32_t* g2 = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    int32_t* path = (int32_t*)malloc((size_t)Q * LMAX * sizeof(int32_t));
    int32_t tg[Q], len[Q], cst[Q], st[Q], wh[Q];
    CHECK(g && owner && g2 && path);
    CHECK(fm_cost_field(d2, pen, cap, W, H, 0, seed, cost, n_seed, 0, g, owner) == expect_status);
    CHECK(fm_cost_field(d2, pen, cap, W, H, 0, seed, cost, n_seed, 0, g2, NULL) == expect_status);
    long long fin = 0;
    for (int c = 0; c < n; ++c) {
        CHECK(g[c] == g2[c]);
        CHECK((owner[c] >= 0) == (g[c] != INF) && owner[c] < n_seed && owner[c] >= -1);
        if (g[c] == INF) continue;
        ++fin;
        CHECK(d2[c] >= 1);
        /* no move lowers a value; the value is a seed's cost or comes over a move */
        int64_t best = INF;
        for (int s = 0; s < n_seed; ++s)
            if (seed[s] == c && (!cost || (cost[s] >= 0 && cost[s] <= (1 << 24))) && (cost ? cost[s] : 0) < best) best = cost ? cost[s] : 0;
        for (int d = 0; d < 8; ++d) {
            const int px = c % W - DX[d], py = c / W - DY[d];
            if (px < 0 || py < 0 || px >= W || py >= H) continue;
            const int p = py * W + px, mc = move_cost(d2, pen, cap, W, H, p, c);
            if (mc >= 0 && g[p] != INF && (int64_t)g[p] + mc < best) best = (int64_t)g[p] + mc;
        }
        CHECK(best == g[c]);
    }
    for (int s = 0; s < n_seed; ++s) {
        const int c = seed[s];
        if (c < 0 || c >= n || g[c] == INF || (cost ? cost[s] : 0) != g[c]) continue;
        CHECK(owner[c] <= s && seed[owner[c]] == c && (cost ? cost[owner[c]] : 0) == g[c]);
    }
    for (int q = 0; q < Q; ++q) tg[q] = (int32_t)(rnd() * (n + 4)) - 2;
    for (int to_seed = 0; to_seed < 2; ++to_seed) {
        fm_field_paths(d2, pen, cap, W, H, 0, g, seed, cost, n_seed, 0, tg, Q, LMAX, to_seed, path, len, cst, st, wh);
        for (int q = 0; q < Q; ++q) {
            const int t = tg[q];
            if (t < 0 || t >= n || d2[t] < 1) { CHECK(st[q] == 2 && wh[q] == -1 && len[q] == 0 && cst[q] == -1); continue; }
            if (g[t] == INF) { CHECK(st[q] == 1 && wh[q] == -1 && len[q] == 0 && cst[q] == -1); continue; }
            CHECK((st[q] == 0 || st[q] == 3) && wh[q] == owner[t] && cst[q] == g[t] && len[q] >= 1 && (st[q] == 3) == (len[q] > LMAX));
            if (st[q] != 0) continue;
            const int32_t* P = path + (size_t)q * LMAX;
            const int first = to_seed ? P[len[q] - 1] : P[0], last = to_seed ? P[0] : P[len[q] - 1];
            CHECK(first == seed[wh[q]] && last == t);
            int64_t sum = cost ? cost[wh[q]] : 0;
            for (int i = 1; i < len[q]; ++i) {
                const int mc = to_seed ? move_cost(d2, pen, cap, W, H, P[len[q] - i], P[len[q] - 1 - i]) : move_cost(d2, pen, cap, W, H, P[i - 1], P[i]);
                CHECK(mc >= 0);
                sum += mc;
            }
            CHECK(sum == cst[q]);
        }
    }
    printf("%s %dx%d: %d seeds, %lld finite cells\n", name, W, H, n_seed, fin);
    free(g); free(owner); free(g2); free(path);
    return 0;
}

int main(void) {
    {   /* i.i.d. obstacles, 5 seeds, without and with costs, unweighted and with a random costmap */
        enum { W = 96, H = 80 };
        static int32_t d2[W * H];
        static uint8_t pen[W * H];
        int32_t seed[5], cost[5];
        for (int i = 0; i < W * H; ++i) { d2[i] = rnd() < 0.2 ? 0 : 1; pen[i] = (uint8_t)(rnd() * 256); }
        for (int s = 0; s < 5; ++s) {
            do seed[s] = (int32_t)(rnd() * W * H); while (d2[seed[s]] < 1);
            cost[s] = (int32_t)(rnd() * 400);
        }
        if (check_map("salt20", d2, NULL, 0, W, H, seed, NULL, 5, 0)) return 1;
        if (check_map("salt20_costs", d2, NULL, 0, W, H, seed, cost, 5, 0)) return 1;
        if (check_map("salt20_pen", d2, pen, 255, W, H, seed, cost, 5, 0)) return 1;
        if (check_map("salt20_pen_cap40", d2, pen, 40, W, H, seed, cost, 5, 0)) return 1;
    }
    {   /* walls of two rows every four rows, open at alternating ends */
        enum { N = 64 };
        static int32_t d2[N * N];
        int k = 0;
        for (int i = 0; i < N * N; ++i) d2[i] = 1;
        for (int y = 2; y < N - 1; y += 4, ++k)
            for (int yy = y; yy < y + 2 && yy < N; ++yy)
                for (int x = 0; x < N; ++x)
                    if (k % 2 == 0 ? x < N - 2 : x >= 2) d2[yy * N + x] = 0;
        const int32_t seed[2] = {0, N * N - 1}, cost[2] = {5000, 0};
        if (check_map("serpentine", d2, NULL, 0, N, N, seed, cost, 2, 0)) return 1;
    }
    {   /* lines */
        static int32_t d2[200];
        for (int i = 0; i < 200; ++i) d2[i] = rnd() < 0.1 ? 0 : 1;
        d2[3] = d2[150] = 1;
        const int32_t seed[2] = {3, 150}, cost[2] = {17, 0};
        if (check_map("row", d2, NULL, 0, 200, 1, seed, cost, 2, 0)) return 1;
        if (check_map("column", d2, NULL, 0, 1, 200, seed, cost, 2, 0)) return 1;
    }
    {   /* the plug map */
        enum { W = 130, H = 3 };
        static int32_t d2[W * H];
        for (int i = 0; i < W * H; ++i) d2[i] = 1;
        d2[0 * W + 62] = d2[0 * W + 63] = d2[1 * W + 62] = d2[2 * W + 62] = d2[2 * W + 63] = 0;
        const int32_t seed[1] = {1 * W + 63};
        if (check_map("plug", d2, NULL, 0, W, H, seed, NULL, 1, 0)) return 1;
    }
    {   /* the mirror map; duplicates, a dominated seed, an exact tie; invalid and empty lists */
        enum { W = 33, H = 17 };
        static int32_t d2[W * H];
        for (int i = 0; i < W * H; ++i) d2[i] = 1;
        const int32_t a = 8 * W + 4, b = 8 * W + 28;
        const int32_t mirror[2] = {a, b};
        if (check_map("mirror", d2, NULL, 0, W, H, mirror, NULL, 2, 0)) return 1;
        const int32_t dup[3] = {a, b, a}, dupc[3] = {7, 0, 7};
        if (check_map("duplicates", d2, NULL, 0, W, H, dup, dupc, 3, 0)) return 1;
        const int32_t domc[2] = {0, 300}, tiec[2] = {0, 240};
        if (check_map("dominated", d2, NULL, 0, W, H, mirror, domc, 2, 0)) return 1;
        if (check_map("exact_tie", d2, NULL, 0, W, H, mirror, tiec, 2, 0)) return 1;
        const int32_t bad[3] = {-1, W * H, 5}, badc[3] = {0, 0, (1 << 24) + 1};
        if (check_map("invalid", d2, NULL, 0, W, H, bad, badc, 3, 2)) return 1;
        if (check_map("empty", d2, NULL, 0, W, H, bad, NULL, 0, 2)) return 1;
    }
    printf("field_multi_ref OK\n");
    return 0;
}
