/* Stand-alone driver of the C statement of the field repair (field_update_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o field_update_ref_check field_update_ref_check.c field_update_ref.c
 * A fresh field is the repair of an all-INF field from an all-blocked map (the root becomes free: the field appears).
 * Maps: i.i.d. obstacles at p = 0.2 on 96 x 80 (unweighted and with a random costmap, cap 255 and 40), the serpentine
 * corridor on 64 x 64, a 1 x 200 and a 200 x 1 line.  Per map a chain of frames, each fed the previous repair: random
 * cells flipped (and penalties redrawn), the root blocked, the root freed, no change.  Checked per frame: the repair equals
 * the fresh field of the new map cell for cell and in status, it is a fixed point of the relaxation, stats[0] is the
 * number of changed cells counted here, stats[1] lies between the cells that turned INF or rose and the finite cells of
 * the old field, no change gives stats 0 0, a blocked root gives |U| = every finite cell.  Then the argument errors.
 * Prints one line per map and "field_update_ref OK"; exit code 1 on the first failed check. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int fu_update(const int32_t* d2_old, const uint8_t* pen_old, const int32_t* d2_new, const uint8_t* pen_new, int cap, int W, int H,
              int32_t r2, int root, int32_t* g, int32_t* stats);

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

static int move_cost(const int32_t* d2, const uint8_t* pen, int cap, int W, int a, int b) {
    const int ax = a % W, ay = a / W, bx = b % W, by = b / W, dx = bx - ax, dy = by - ay;
    if (d2[a] < 1 || d2[b] < 1) return -1;
    if (dx && dy && (d2[ay * W + bx] < 1 || d2[by * W + ax] < 1)) return -1;
    return (dx && dy ? 14 : 10) + pc(pen, cap, b);
}

/* g is the field of (d2, pen) for root: 0 at the root, elsewhere the cheapest move in; INF where nothing comes in */
static int fixed_point(const int32_t* d2, const uint8_t* pen, int cap, int W, int H, int root, const int32_t* g) {
    for (int c = 0; c < W * H; ++c) {
        int64_t best = INF;
        if (c == root && d2[c] >= 1) best = 0;
        for (int d = 0; d < 8 && d2[c] >= 1; ++d) {
            const int px = c % W - DX[d], py = c / W - DY[d];
            if (px < 0 || py < 0 || px >= W || py >= H) continue;
            const int p = py * W + px, mc = move_cost(d2, pen, cap, W, p, c);
            if (mc >= 0 && g[p] != INF && (int64_t)g[p] + mc < best) best = (int64_t)g[p] + mc;
        }
        CHECK(best == g[c]);
    }
    return 0;
}

static int check_chain(const char* name, int32_t* d2, uint8_t* pen, int cap, int W, int H, int root, int frames) {
    const int n = W * H;
    int32_t* zero = (int32_t*)calloc((size_t)n, sizeof(int32_t));
    int32_t* d2n = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    int32_t* g = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    int32_t* gold = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    int32_t* fresh = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    uint8_t* penn = pen ? (uint8_t*)malloc((size_t)n) : NULL;
    int32_t st[2];
    long long sumU = 0;
    CHECK(zero && d2n && g && gold && fresh && (!pen || penn));
    for (int c = 0; c < n; ++c) g[c] = INF;
    CHECK(fu_update(zero, pen, d2, pen, cap, W, H, 0, root, g, st) == 0 && st[1] == 0);
    if (fixed_point(d2, pen, cap, W, H, root, g)) return 1;
    for (int k = 0; k < frames; ++k) {
        memcpy(d2n, d2, (size_t)n * sizeof(int32_t));
        if (pen) memcpy(penn, pen, (size_t)n);
        const int kind = k % 5;   /* 0, 1: random flips; 2: the root blocked; 3: the root freed; 4: no change */
        if (kind < 2) {
            for (int j = 0; j < 1 + n / 200; ++j) {
                const int c = (int)(rnd() * n);
                if (c != root) d2n[c] = d2n[c] >= 1 ? 0 : 1;
                if (pen) penn[(int)(rnd() * n)] = (uint8_t)(rnd() * 256);
            }
        } else if (kind == 2) d2n[root] = 0;
        else if (kind == 3) d2n[root] = 1;
        int changed = 0, fin_old = 0, rose = 0;
        for (int c = 0; c < n; ++c) {
            const int t0 = d2[c] >= 1, t1 = d2n[c] >= 1;
            changed += t0 != t1 || (t0 && t1 && pc(pen, cap, c) != pc(penn, cap, c));
            fin_old += g[c] != INF;
        }
        memcpy(gold, g, (size_t)n * sizeof(int32_t));
        const int status = fu_update(d2, pen, d2n, penn, cap, W, H, 0, root, g, st);
        for (int c = 0; c < n; ++c) fresh[c] = INF;
        int32_t st2[2];
        const int status2 = fu_update(zero, penn, d2n, penn, cap, W, H, 0, root, fresh, st2);
        CHECK(status == status2 && status == (d2n[root] >= 1 ? 0 : 2));
        for (int c = 0; c < n; ++c) {
            CHECK(g[c] == fresh[c]);
            rose += gold[c] != INF && g[c] > gold[c];
        }
        if (fixed_point(d2n, penn, cap, W, H, root, g)) return 1;
        CHECK(st[0] == changed && st[1] >= rose && st[1] <= fin_old);
        if (kind == 4) CHECK(st[0] == 0 && st[1] == 0);
        if (status == 2) CHECK(st[1] == fin_old);
        sumU += st[1];
        memcpy(d2, d2n, (size_t)n * sizeof(int32_t));
        if (pen) memcpy(pen, penn, (size_t)n);
    }
    printf("%s %dx%d: %d frames, %lld cells raised in all\n", name, W, H, frames, sumU);
    free(zero); free(d2n); free(g); free(gold); free(fresh); free(penn);
    return 0;
}

int main(void) {
    {
        enum { W = 96, H = 80 };
        static int32_t d2[W * H], d2b[W * H];
        static uint8_t pen[W * H];
        for (int i = 0; i < W * H; ++i) { d2[i] = rnd() < 0.2 ? 0 : 1; pen[i] = (uint8_t)(rnd() * 256); }
        int root;
        do root = (int)(rnd() * W * H); while (d2[root] < 1);
        memcpy(d2b, d2, sizeof d2);
        if (check_chain("salt20", d2b, NULL, 0, W, H, root, 15)) return 1;
        memcpy(d2b, d2, sizeof d2);
        if (check_chain("salt20_pen", d2b, pen, 255, W, H, root, 15)) return 1;
        memcpy(d2b, d2, sizeof d2);
        if (check_chain("salt20_pen_cap40", d2b, pen, 40, W, H, root, 10)) return 1;
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
        if (check_chain("serpentine", d2, NULL, 0, N, N, 0, 10)) return 1;
    }
    {   /* lines */
        static int32_t d2[200];
        for (int i = 0; i < 200; ++i) d2[i] = rnd() < 0.1 ? 0 : 1;
        d2[3] = 1;
        if (check_chain("row", d2, NULL, 0, 200, 1, 3, 10)) return 1;
        if (check_chain("column", d2, NULL, 0, 1, 200, 3, 10)) return 1;
    }
    {   /* argument errors */
        int32_t d2[4] = {1, 1, 1, 1}, g[4] = {0, 10, 10, 14}, neg[4] = {0, -1, 10, 14};
        uint8_t pen[4] = {0};
        CHECK(fu_update(NULL, NULL, d2, NULL, 0, 2, 2, 0, 0, g, NULL) == -1);
        CHECK(fu_update(d2, NULL, NULL, NULL, 0, 2, 2, 0, 0, g, NULL) == -1);
        CHECK(fu_update(d2, NULL, d2, NULL, 0, 2, 2, 0, 0, NULL, NULL) == -1);
        CHECK(fu_update(d2, NULL, d2, NULL, 0, 0, 2, 0, 0, g, NULL) == -1);
        CHECK(fu_update(d2, pen, d2, NULL, 0, 2, 2, 0, 0, g, NULL) == -1);
        CHECK(fu_update(d2, pen, d2, pen, 256, 2, 2, 0, 0, g, NULL) == -1);
        CHECK(fu_update(d2, NULL, d2, NULL, 0, 2, 2, 0, 0, neg, NULL) == -1);
        CHECK(fu_update(d2, NULL, d2, NULL, 0, 2, 2, 0, 0, g, NULL) == 0 && g[3] == 14);
        CHECK(fu_update(d2, NULL, d2, NULL, 0, 2, 2, 0, 4, g, NULL) == 2 && g[0] == INF);
    }
    printf("field_update_ref OK\n");
    return 0;
}
