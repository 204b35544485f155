/* Stand-alone driver of the CPU twin (components_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o components_ref_check components_ref_check.c components_ref.c
 * Three maps -- i.i.d. obstacles at p = 0.41 on 97 x 61, the serpentine corridor of the field tests on 64 x 64, a 1 x 200
 * line, plus an all-blocked grid -- are labelled and the defining properties checked: a label is negative exactly on the
 * blocked cells, label[label[c]] == label[c] <= c, orthogonal traversable neighbours share a label, the sizes sit at the
 * representatives and add up to the traversable cells, ncomp counts them, largest has the largest size with ties to the
 * smaller index.  Then cr_reachable on queries that include out-of-range cells and grids.  Prints one line per map and
 * "components_ref OK"; exit code 1 on the first failed check. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int cr_components(const int32_t* d2, int W, int H, int32_t r2_clear, int32_t* label, int32_t* size, int32_t* ncomp, int32_t* largest);
void cr_reachable(const int32_t* label, int G, const int32_t* qgrid, int W, int H, const int32_t* start, const int32_t* goal, int Q,
                  int32_t* status);

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

static int check_map(const char* name, const int32_t* d2, int W, int H, int32_t r2) {
    const int32_t thr = r2 > 1 ? r2 : 1;
    const int n = W * H;
    int32_t* label = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    int32_t* size = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    int32_t ncomp = -7, largest = -7;
    CHECK(label && size);
    CHECK(cr_components(d2, W, H, r2, label, size, &ncomp, &largest) == 0);
    long long trav = 0, cells = 0;
    int32_t roots = 0, best = -1, best_size = 0;
    for (int c = 0; c < n; ++c) {
        const int32_t l = label[c];
        CHECK((l >= 0) == (d2[c] >= thr));
        if (l < 0) { CHECK(size[c] == 0); continue; }
        ++trav;
        CHECK(l <= c && label[l] == l);
        if (c % W + 1 < W && label[c + 1] >= 0) CHECK(label[c + 1] == l);
        if (c + W < n && label[c + W] >= 0) CHECK(label[c + W] == l);
        if (l == c) {
            ++roots;
            CHECK(size[c] >= 1);
            if (size[c] > best_size) { best_size = size[c]; best = c; }
        } else CHECK(size[c] == 0);
        cells += size[c];
    }
    CHECK(cells == trav && roots == ncomp && best == largest);
    /* without the optional outputs */
    int32_t* label2 = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    CHECK(label2 && cr_components(d2, W, H, r2, label2, NULL, NULL, NULL) == 0);
    for (int c = 0; c < n; ++c) CHECK(label2[c] == label[c]);
    /* reachability: the cells around the grid's ends and beyond them, on grids -1 .. 1 of one */
    enum { Q = 64 };
    int32_t s[Q], g[Q], qg[Q], st[Q];
    for (int q = 0; q < Q; ++q) {
        s[q] = (int32_t)(rnd() * (n + 4)) - 2;
        g[q] = q % 5 == 0 ? s[q] : (int32_t)(rnd() * (n + 4)) - 2;
        qg[q] = q % 9 == 8 ? (q % 2 ? 1 : -1) : 0;
    }
    cr_reachable(label, 1, qg, W, H, s, g, Q, st);
    for (int q = 0; q < Q; ++q) {
        const int in = qg[q] == 0 && s[q] >= 0 && s[q] < n && g[q] >= 0 && g[q] < n && label[s[q]] >= 0 && label[g[q]] >= 0;
        CHECK(st[q] == (in ? (label[s[q]] == label[g[q]] ? 0 : 1) : 2));
    }
    cr_reachable(label, 1, NULL, W, H, s, g, Q, st);
    for (int q = 0; q < Q; ++q) CHECK(st[q] >= 0 && st[q] <= 2);
    printf("%s %dx%d: %d traversable cells, %d components, largest %d (%d cells)\n", name, W, H, (int)trav, ncomp, largest, best_size);
    free(label); free(size); free(label2);
    return 0;
}

int main(void) {
    {   /* i.i.d. obstacles */
        enum { W = 97, H = 61 };
        static int32_t d2[W * H];
        for (int i = 0; i < W * H; ++i) d2[i] = rnd() < 0.41 ? 0 : 1 + (int32_t)(rnd() * 5);
        if (check_map("salt41", d2, W, H, 0)) return 1;
        if (check_map("salt41_r2_3", d2, W, H, 3)) return 1;
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
        if (check_map("serpentine", d2, N, N, 0)) return 1;
    }
    {   /* a line, and a grid without a traversable cell */
        static int32_t d2[200];
        for (int i = 0; i < 200; ++i) d2[i] = rnd() < 0.1 ? 0 : 1;
        if (check_map("row", d2, 200, 1, 0)) return 1;
        if (check_map("column", d2, 1, 200, 0)) return 1;
        for (int i = 0; i < 200; ++i) d2[i] = 0;
        if (check_map("blocked", d2, 20, 10, 0)) return 1;
    }
    printf("components_ref OK\n");
    return 0;
}
