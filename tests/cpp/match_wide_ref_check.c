/* Stand-alone driver of the C statement of wide-window scan matching (match_wide_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -std=c11 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -o match_wide_ref_check \
 *      match_wide_ref_check.c match_wide_ref.c
 * Every array is allocated at its exact size, so a read or write outside one is caught.  The cases: an L-shaped map whose
 * points are taken from the walls themselves, searched with every top 0 .. 3 from priors all over a +-21 x +-13 window (the
 * pruned procedure runs beside the dense search; the true pose is the unique best and the stats obey their invariants); a
 * window smaller than one node; a prior outside the grid; top 5 with a +-2048 x 0 window on a 1 x 200 grid; an ignored scan
 * between two live ones and all points absent; the overflow pair on a grid nobody knows; argument errors.  Prints one line
 * per case and "match_wide_ref OK"; exit code 1 on the first failed check. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int mwx_match(const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre, int S, int R, int N, int W, int H, int wx,
              int wy, int32_t d2_cap, int32_t unk, int top, int max_nodes, int32_t* best, int32_t* stats);

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

/* squared distance to the nearest obstacle by brute force; INT32_MAX without one */
static int32_t* edt(const uint8_t* occ, int W, int H) {
    int32_t* d2 = (int32_t*)malloc((size_t)W * H * 4);
    if (!d2) return NULL;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int64_t m = INT32_MAX;
            for (int v = 0; v < H; ++v)
                for (int u = 0; u < W; ++u)
                    if (occ[v * W + u]) {
                        int64_t d = (int64_t)(u - x) * (u - x) + (int64_t)(v - y) * (v - y);
                        if (d < m) m = d;
                    }
            d2[y * W + x] = (int32_t)m;
        }
    return d2;
}

static int eq6(const int32_t* b, int r, int dx, int dy, int sc, int np, int nt) {
    return b[0] == r && b[1] == dx && b[2] == dy && b[3] == sc && b[4] == np && b[5] == nt;
}

int main(void) {
    enum { W = 37, H = 23 };
    uint8_t* occ = (uint8_t*)calloc((size_t)W * H, 1);
    CHECK(occ);
    for (int x = 5; x < 30; ++x) occ[4 * W + x] = 1;
    for (int y = 4; y < 20; ++y) occ[y * W + 30] = 1;
    occ[15 * W + 9] = 1;
    int32_t* d2 = edt(occ, W, H);
    CHECK(d2);
    int n_occ = 0;
    for (int c = 0; c < W * H; ++c) n_occ += occ[c];
    const int ax = 12, ay = 11, N = n_occ + 2;
    int32_t* pts = (int32_t*)malloc((size_t)N * 8);
    CHECK(pts);
    int k = 0;
    for (int c = 0; c < W * H; ++c)
        if (occ[c]) { pts[2 * k] = c % W - ax; pts[2 * k + 1] = c / W - ay; ++k; }
    pts[2 * k] = INT32_MIN, pts[2 * k + 1] = INT32_MIN, ++k;
    pts[2 * k] = 16385, pts[2 * k + 1] = 0, ++k;
    CHECK(k == N);
    int32_t best[6], best2[6], stats[8];

    /* every top from priors over the window, the prior outside the grid included */
    {
        const int wx = 21, wy = 13, all = (2 * wx + 1) * (2 * wy + 1);
        for (int top = 0; top <= 3; ++top)
            for (int ey = -wy; ey <= wy; ey += 3)
                for (int ex = -wx; ex <= wx; ex += 4) {
                    const int32_t centre[2] = {ax + ex, ay + ey};
                    CHECK(mwx_match(d2, NULL, pts, centre, 1, 1, N, W, H, wx, wy, 64, 1, top, 4096, best, stats) == 0);
                    CHECK(eq6(best, 0, -ex, -ey, 0, n_occ, 1));
                    CHECK(mwx_match(d2, NULL, pts, centre, 1, 1, N, W, H, wx, wy, 64, 1, top, 4096, best2, NULL) == 0);
                    CHECK(memcmp(best, best2, sizeof best) == 0);
                    CHECK(stats[7] >= 0 && (top > 0 || stats[7] >= best[3]));
                    CHECK(stats[0] >= 1 && stats[0] <= all && (top > 0 || (stats[0] == all && stats[6] == 0)));
                    for (int j = top + 1; j < 6; ++j) CHECK(stats[j] == 0);
                }
        printf("L map %dx%d: recovered with top 0 .. 3\n", W, H);
    }

    /* a window smaller than one node */
    {
        const int32_t centre[2] = {ax + 2, ay - 3};
        CHECK(mwx_match(d2, NULL, pts, centre, 1, 1, N, W, H, 3, 3, 64, 1, 1, 64, best, stats) == 0);
        CHECK(eq6(best, 0, -2, 3, 0, n_occ, 1) && stats[1] == 4 && stats[0] >= 1 && stats[0] <= 49);
        CHECK(mwx_match(d2, NULL, pts, centre, 1, 1, N, W, H, 3, 3, 64, 1, 3, 64, best, stats) == 0);
        CHECK(eq6(best, 0, -2, 3, 0, n_occ, 1) && stats[3] == 1 && stats[2] == 1 && stats[1] == 4);
        printf("windows smaller than a node: ok\n");
    }

    /* top 5 on a line */
    {
        enum { LW = 200 };
        uint8_t line[LW] = {0};
        line[80] = line[150] = 1;
        int32_t* l2 = edt(line, LW, 1);
        CHECK(l2);
        const int32_t p[6] = {-20, 0, 50, 0, 3, 0}, centre[2] = {100 + 1500, 0};
        CHECK(mwx_match(l2, NULL, p, centre, 1, 1, 3, LW, 1, 2048, 0, 64, 64, 5, 4096, best, stats) == 0);
        CHECK(best[0] == 0 && best[1] == -1500 && best[2] == 0 && best[4] == 3 && stats[5] == 5);
        CHECK(mwx_match(l2, NULL, p, centre, 1, 1, 3, LW, 1, 2048, 0, 64, 64, 5, 4096, best2, NULL) == 0);
        CHECK(memcmp(best, best2, sizeof best) == 0);
        free(l2);
        printf("top 5, +-2048 x 0 on 1 x 200: ok\n");
    }

    /* an ignored scan between two live ones; all points absent */
    {
        enum { S = 3, R = 2, M = 5 };
        int32_t* p3 = (int32_t*)malloc((size_t)S * R * M * 8);
        int32_t b3[S * 6], s3[S * 8];
        CHECK(p3);
        for (int i = 0; i < S * R * M * 2; ++i) p3[i] = INT32_MIN;
        p3[2 * R * M * 2] = 1, p3[2 * R * M * 2 + 1] = 2;   /* scan 2, rotation 0, point 0 */
        const int32_t centre[6] = {-16384, 8192 + 16384, 8192 + 16385, 0, 3, 3};
        CHECK(mwx_match(d2, NULL, p3, centre, S, R, M, W, H, 9, 6, 64, 1, 1, 1024, b3, s3) == 0);
        CHECK(eq6(b3, 0, 0, 0, 0, 0, R * 19 * 13) && eq6(b3 + 6, -1, 0, 0, 0, 0, 0) && b3[12] == 1 && b3[15] == 0);
        for (int i = 0; i < 16; ++i) CHECK(s3[i] == 0);
        CHECK(s3[17] > 0);
        free(p3);
        printf("ignored, absent: ok\n");
    }

    /* overflow: a grid nobody knows, every candidate ties */
    {
        uint8_t* known = (uint8_t*)calloc((size_t)W * H, 1);
        CHECK(known);
        const int32_t centre[2] = {ax, ay};
        CHECK(mwx_match(d2, known, pts, centre, 1, 1, 8, W, H, 20, 20, 64, 1, 2, 1024, best, stats) == 0);
        CHECK(eq6(best, -2, 0, 0, 0, 0, 0) && stats[2] == 9 && stats[1] == 121 && stats[0] == 0 && stats[7] == 8);
        CHECK(mwx_match(d2, known, pts, centre, 1, 1, 8, W, H, 20, 20, 64, 1, 2, 2048, best, stats) == 0);
        CHECK(eq6(best, 0, 0, 0, 8, 8, 1681) && stats[0] == 1681);
        free(known);
        printf("overflow at 1024 nodes, 1681 ties at 2048: ok\n");
    }

    /* argument errors */
    {
        const int32_t centre[2] = {ax, ay};
        CHECK(mwx_match(NULL, NULL, pts, centre, 1, 1, N, W, H, 5, 5, 64, 1, 1, 64, best, NULL) == 1);
        CHECK(mwx_match(d2, NULL, pts, centre, 1, 1, N, W, H, 2049, 5, 64, 1, 1, 64, best, NULL) == 1);
        CHECK(mwx_match(d2, NULL, pts, centre, 1, 1, N, W, H, 5, 5, 64, 1, 6, 64, best, NULL) == 1);
        CHECK(mwx_match(d2, NULL, pts, centre, 1, 1, N, W, H, 5, 5, 64, 1, 1, 63, best, NULL) == 1);
        CHECK(mwx_match(d2, NULL, pts, centre, 1, 1, N, W, H, 5, 5, 64, 1, 1, (1 << 22) + 1, best, NULL) == 1);
        CHECK(mwx_match(d2, NULL, pts, centre, 17, 1, N, W, H, 5, 5, 64, 1, 1, 1 << 22, best, NULL) == 1);
        CHECK(mwx_match(d2, NULL, pts, centre, 1, 1, N, W, H, 20, 20, 64, 1, 0, 1024, best, NULL) == 1);   /* 1681 top nodes */
        CHECK(mwx_match(d2, NULL, pts, centre, 1, 1, N, W, H, 5, 5, 64, 1, 1, 64, best, best) == 1);
        CHECK(mwx_match(d2, NULL, pts, centre, 0, 1, N, W, H, 5, 5, 64, 1, 1, 64, best, NULL) == 0);
    }
    free(occ);
    free(d2);
    free(pts);
    printf("match_wide_ref OK\n");
    return 0;
}
