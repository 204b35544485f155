/* Stand-alone driver of the C reference of the exploration frontiers (frontier_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -std=c11 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -o frontier_ref_check frontier_ref_check.c frontier_ref.c
 * Known masks from disc lists (discs that stick out of the grid, a negative radius, the largest radius) over i.i.d. obstacles
 * on 130 x 70, a 1 x 200 line, an all-known and an all-unknown grid are labelled and the defining properties checked: a label
 * is negative exactly off the frontier, label[label[c]] == label[c] <= c, frontier cells that touch (diagonals included) share
 * a label, the listed rows ascend by representative and agree with a recount (size, box, sums, slot), ncl counts both kinds,
 * the Cmax cut keeps the first rows, the optional outputs may be NULL.  Then the cost matrix against a recount, with a field
 * on a grid that does not exist.  Prints one line per map and "frontier_ref OK"; exit code 1 on the first failed check. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void fx_known_from_discs(const uint8_t* base, const int32_t* discs, int R, int W, int H, uint8_t* known);
void fx_d2_known(const int32_t* d2, const uint8_t* known, int64_t cells, int32_t* d2k);
int fx_frontier(const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size, int Cmax, int32_t* label,
                int32_t* slot, int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox, int64_t* csum);
void fx_cost_matrix(const int32_t* g, int F, const int32_t* fgrid, const int32_t* slot, const int32_t* csize, int G, int W, int H, int Cmax,
                    int32_t gain, int32_t size_cap, int32_t* cost, int32_t* cell);

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

static int is_fr(const int32_t* d2, const uint8_t* known, int W, int H, int32_t thr, int x, int y) {
    const int c = y * W + x;
    if (!known[c] || d2[c] < thr) return 0;
    return (x > 0 && !known[c - 1]) || (x + 1 < W && !known[c + 1]) || (y > 0 && !known[c - W]) || (y + 1 < H && !known[c + W]);
}

static int check_map(const char* name, const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2, int min_size, int Cmax) {
    const int32_t thr = r2 > 1 ? r2 : 1;
    const int n = W * H;
    int32_t* label = (int32_t*)malloc((size_t)n * 4);
    int32_t* slot = (int32_t*)malloc((size_t)n * 4);
    int32_t* rep = (int32_t*)malloc((size_t)Cmax * 4);
    int32_t* csize = (int32_t*)malloc((size_t)Cmax * 4);
    int32_t* cbox = (int32_t*)malloc((size_t)Cmax * 16);
    int64_t* csum = (int64_t*)malloc((size_t)Cmax * 16);
    int32_t ncl[2] = {-7, -7};
    CHECK(label && slot && rep && csize && cbox && csum);
    CHECK(fx_frontier(d2, known, W, H, r2, min_size, Cmax, label, slot, ncl, rep, csize, cbox, csum) == 0);
    int cells = 0, roots = 0, big = 0;
    for (int c = 0; c < n; ++c) {
        const int x = c % W, y = c / W;
        const int32_t l = label[c];
        CHECK((l >= 0) == is_fr(d2, known, W, H, thr, x, y));
        if (l < 0) { CHECK(slot[c] == -1); continue; }
        ++cells;
        CHECK(l <= c && label[l] == l);
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = x + dx, yy = y + dy;
                if (xx < 0 || yy < 0 || xx >= W || yy >= H) continue;
                if (label[yy * W + xx] >= 0) CHECK(label[yy * W + xx] == l);
            }
        if (l == c) {
            int size = 0;
            for (int q = c; q < n; ++q) size += label[q] == c;
            ++roots;
            big += size >= min_size;
        }
    }
    CHECK(ncl[0] == big && ncl[1] == roots);
    const int L = big < Cmax ? big : Cmax;
    for (int k = 0; k < Cmax; ++k) {
        if (k >= L) {
            CHECK(rep[k] == -1 && csize[k] == 0 && !cbox[4 * k] && !cbox[4 * k + 1] && !cbox[4 * k + 2] && !cbox[4 * k + 3] && !csum[2 * k] &&
                  !csum[2 * k + 1]);
            continue;
        }
        CHECK(rep[k] >= 0 && rep[k] < n && label[rep[k]] == rep[k] && (k == 0 || rep[k] > rep[k - 1]));
        int size = 0, x0 = W, y0 = H, x1 = -1, y1 = -1;
        int64_t sx = 0, sy = 0;
        for (int c = 0; c < n; ++c) {
            if (label[c] != rep[k]) { CHECK(slot[c] != k); continue; }
            const int x = c % W, y = c / W;
            CHECK(slot[c] == k);
            ++size; sx += x; sy += y;
            if (x < x0) x0 = x;
            if (x > x1) x1 = x;
            if (y < y0) y0 = y;
            if (y > y1) y1 = y;
        }
        CHECK(size == csize[k] && size >= min_size && cbox[4 * k] == x0 && cbox[4 * k + 1] == y0 && cbox[4 * k + 2] == x1 && cbox[4 * k + 3] == y1 &&
              csum[2 * k] == sx && csum[2 * k + 1] == sy);
    }
    /* without the optional outputs, and cut to two columns */
    int32_t ncl2[2], rep2[2], csize2[2];
    CHECK(fx_frontier(d2, known, W, H, r2, min_size, 2, NULL, NULL, ncl2, rep2, csize2, NULL, NULL) == 0);
    CHECK(ncl2[0] == ncl[0] && ncl2[1] == ncl[1]);
    for (int k = 0; k < 2 && k < Cmax; ++k) CHECK(rep2[k] == rep[k] && csize2[k] == csize[k]);
    /* the matrix: three fields, the last on a grid that does not exist */
    enum { F = 3 };
    int32_t* g = (int32_t*)malloc((size_t)F * n * 4);
    int32_t* cost = (int32_t*)malloc((size_t)F * Cmax * 4);
    int32_t* cell = (int32_t*)malloc((size_t)F * Cmax * 4);
    const int32_t fgrid[F] = {0, 0, 1};
    CHECK(g && cost && cell);
    for (int i = 0; i < F * n; ++i) g[i] = rnd() < 0.2 ? INT32_MAX : (int32_t)(rnd() * 40);
    const int32_t gain = 3, cap = 4;
    fx_cost_matrix(g, F, fgrid, slot, csize, 1, W, H, Cmax, gain, cap, cost, cell);
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < Cmax; ++k) {
            int32_t m = INT32_MAX, at = -1;
            for (int c = 0; c < n && f < 2; ++c)
                if (slot[c] == k && g[f * n + c] < m) { m = g[f * n + c]; at = c; }
            CHECK(cell[f * Cmax + k] == at);
            CHECK(cost[f * Cmax + k] == (at < 0 ? INT32_MAX : m + gain * (cap - (csize[k] < cap ? csize[k] : cap))));
        }
    fx_cost_matrix(g, 2, NULL, slot, csize, 1, W, H, Cmax, 0, 0, cost, cell);
    for (int i = 0; i < 2 * Cmax; ++i) CHECK(cell[i] < 0 ? cost[i] == INT32_MAX : cost[i] == g[(i / Cmax) * n + cell[i]]);
    printf("%s %dx%d: %d frontier cells, %d clusters, %d listed (min_size %d, Cmax %d)\n", name, W, H, cells, ncl[1], ncl[0], min_size, Cmax);
    free(label); free(slot); free(rep); free(csize); free(cbox); free(csum); free(g); free(cost); free(cell);
    return 0;
}

int main(void) {
    {   /* i.i.d. obstacles, three discs, one of them over the border; the ignored and the all-covering disc */
        enum { W = 130, H = 70 };
        static int32_t d2[W * H], d2k[W * H];
        static uint8_t known[W * H], again[W * H];
        const int32_t discs[] = {30, 35, 400, 65, 35, 400, 125, 60, 400, 10, 10, -1};
        for (int i = 0; i < W * H; ++i) d2[i] = rnd() < 0.2 ? 0 : 1 + (int32_t)(rnd() * 5);
        fx_known_from_discs(NULL, discs, 4, W, H, known);
        CHECK(known[35 * W + 30] == 1 && known[35 * W + 10] == 1 && known[35 * W + 9] == 0 && known[10 * W + 10] == 0 && known[69 * W + 129] == 1);
        fx_known_from_discs(known, discs, 0, W, H, again);          /* R == 0 copies */
        CHECK(memcmp(known, again, sizeof known) == 0);
        fx_known_from_discs(again, discs, 2, W, H, again);          /* base may alias known */
        CHECK(memcmp(known, again, sizeof known) == 0);
        fx_d2_known(d2, known, W * H, d2k);
        for (int i = 0; i < W * H; ++i) CHECK(d2k[i] == (known[i] ? d2[i] : 0));
        if (check_map("salt20", d2, known, W, H, 0, 1, 128)) return 1;
        if (check_map("salt20_on_d2k", d2k, known, W, H, 0, 1, 128)) return 1;
        if (check_map("salt20_r2_3_min3_cmax8", d2, known, W, H, 3, 3, 8)) return 1;
        const int32_t all[] = {0, 0, INT32_MAX};
        fx_known_from_discs(NULL, all, 1, W, H, known);
        for (int i = 0; i < W * H; ++i) CHECK(known[i] == 1);
        if (check_map("all_known", d2, known, W, H, 0, 1, 16)) return 1;
        memset(known, 0, sizeof known);
        if (check_map("all_unknown", d2, known, W, H, 0, 1, 16)) return 1;
    }
    {   /* a line in both directions */
        static int32_t d2[200];
        static uint8_t known[200];
        const int32_t row[] = {50, 0, 100, 120, 0, 25}, col[] = {0, 50, 100, 0, 120, 25};
        for (int i = 0; i < 200; ++i) d2[i] = rnd() < 0.1 ? 0 : 1;
        fx_known_from_discs(NULL, row, 2, 200, 1, known);
        if (check_map("row", d2, known, 200, 1, 0, 1, 8)) return 1;
        fx_known_from_discs(NULL, col, 2, 1, 200, known);
        if (check_map("column", d2, known, 1, 200, 0, 1, 8)) return 1;
    }
    {   /* known on and below the diagonal: every link of the frontier is diagonal */
        enum { N = 90 };
        static int32_t d2[N * N];
        static uint8_t known[N * N];
        for (int i = 0; i < N * N; ++i) { d2[i] = 1; known[i] = (uint8_t)(i % N <= i / N); }
        if (check_map("diagonal", d2, known, N, N, 0, 1, 4)) return 1;
    }
    printf("frontier_ref OK\n");
    return 0;
}
