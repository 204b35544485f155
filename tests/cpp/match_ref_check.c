/* Stand-alone driver of the C statement of scan matching (match_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -std=c11 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -o match_ref_check match_ref_check.c match_ref.c
 * Every array is allocated at its exact size, so a read or write outside one is caught.  The cases: a two-wall map whose
 * points are taken from the walls themselves (the true pose scores 0 and is the unique best from every offset of the
 * window, the window partly outside the grid included); all points absent; an ignored scan between two live ones, with and
 * without the volume; every absent kind (INT32_MIN, INT32_MAX, one past the reach) and a centre at each end of its range;
 * known NULL against all ones and against all zeros; the tie order (equal displacement, two rotations); the int32 bound
 * (65536 points of cost 32767); a grid without obstacles; argument errors.  Prints one line per case and "match_ref OK"; exit
 * code 1 on the first failed check. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int mx_match(const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre, int S, int R, int N, int W, int H, int wx,
             int wy, int32_t d2_cap, int32_t unk, int32_t* best, int32_t* score);

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
    for (int x = 5; x < 30; ++x) occ[4 * W + x] = 1;          /* a wall along y = 4 */
    for (int y = 4; y < 20; ++y) occ[y * W + 30] = 1;         /* and one along x = 30: an L, no translation keeps it */
    occ[15 * W + 9] = 1;
    int32_t* d2 = edt(occ, W, H);
    CHECK(d2);
    int n_occ = 0;
    for (int c = 0; c < W * H; ++c) n_occ += occ[c];

    /* the points: every obstacle cell as an offset from the true pose (12, 11), plus one absent point of each kind */
    const int ax = 12, ay = 11, N = n_occ + 3;
    int32_t* pts = (int32_t*)malloc((size_t)N * 8);
    CHECK(pts);
    int k = 0;
    for (int c = 0; c < W * H; ++c)
        if (occ[c]) { pts[2 * k] = c % W - ax; pts[2 * k + 1] = c / W - ay; ++k; }
    pts[2 * k] = INT32_MIN, pts[2 * k + 1] = INT32_MIN, ++k;
    pts[2 * k] = 0, pts[2 * k + 1] = INT32_MAX, ++k;
    pts[2 * k] = 16385, pts[2 * k + 1] = 0, ++k;
    CHECK(k == N);
    const int wx = 6, wy = 4, ndx = 2 * wx + 1, ndy = 2 * wy + 1;
    int32_t* score = (int32_t*)malloc((size_t)ndx * ndy * 4);
    int32_t best[6], best2[6];
    CHECK(score);
    for (int ey = -wy; ey <= wy; ++ey)
        for (int ex = -wx; ex <= wx; ++ex) {
            const int32_t centre[2] = {ax + ex, ay + ey};
            CHECK(mx_match(d2, NULL, pts, centre, 1, 1, N, W, H, wx, wy, 64, 1, best, score) == 0);
            CHECK(eq6(best, 0, -ex, -ey, 0, n_occ, 1));
            CHECK(score[(wy - ey) * ndx + (wx - ex)] == 0);
            CHECK(mx_match(d2, NULL, pts, centre, 1, 1, N, W, H, wx, wy, 64, 1, best2, NULL) == 0);
            CHECK(memcmp(best, best2, sizeof best) == 0);
        }
    printf("L map %dx%d: %d points recovered from all %d offsets\n", W, H, n_occ, ndx * ndy);

    /* the window partly outside the grid: the true pose near a corner */
    {
        const int bx = 1, by = 1;
        for (int i = 0; i < n_occ; ++i) { pts[2 * i] += ax - bx; pts[2 * i + 1] += ay - by; }
        const int32_t centre[2] = {bx - 3, by - 2};   /* the prior itself lies outside the grid */
        CHECK(mx_match(d2, NULL, pts, centre, 1, 1, N, W, H, wx, wy, 64, 1, best, score) == 0);
        CHECK(eq6(best, 0, 3, 2, 0, n_occ, 1));
        for (int i = 0; i < n_occ; ++i) { pts[2 * i] -= ax - bx; pts[2 * i + 1] -= ay - by; }
        printf("prior outside the grid: recovered\n");
    }

    /* known: NULL == all ones; all zeros costs unk per present point everywhere */
    {
        uint8_t* known = (uint8_t*)malloc((size_t)W * H);
        int32_t* score2 = (int32_t*)malloc((size_t)ndx * ndy * 4);
        CHECK(known && score2);
        const int32_t centre[2] = {ax + 2, ay - 1};
        memset(known, 1, (size_t)W * H);
        CHECK(mx_match(d2, NULL, pts, centre, 1, 1, N, W, H, wx, wy, 9, 9, best, score) == 0);
        CHECK(mx_match(d2, known, pts, centre, 1, 1, N, W, H, wx, wy, 9, 9, best2, score2) == 0);
        CHECK(memcmp(best, best2, sizeof best) == 0 && memcmp(score, score2, (size_t)ndx * ndy * 4) == 0);
        memset(known, 0, (size_t)W * H);
        CHECK(mx_match(d2, known, pts, centre, 1, 1, N, W, H, wx, wy, 9, 2, best, score) == 0);
        CHECK(eq6(best, 0, 0, 0, 2 * n_occ, n_occ, ndx * ndy));
        CHECK(mx_match(d2, known, pts, centre, 1, 1, N, W, H, wx, wy, 9, 0, best, score) == 0);
        CHECK(eq6(best, 0, 0, 0, 0, n_occ, ndx * ndy));
        free(known);
        free(score2);
        printf("known NULL, ones, zeros: ok\n");
    }

    /* an ignored scan between two live ones; every end of the centre's range; all points absent */
    {
        enum { S = 3, R = 2, M = 5 };
        int32_t* p3 = (int32_t*)malloc((size_t)S * R * M * 8);
        int32_t* vol = (int32_t*)malloc((size_t)S * R * ndx * ndy * 4);
        int32_t b3[S * 6], b3n[S * 6];
        CHECK(p3 && vol);
        for (int i = 0; i < S * R * M * 2; ++i) p3[i] = INT32_MIN;
        int32_t centre[6] = {-16384, 8192 + 16384, 8192 + 16385, 0, 3, 3};
        memset(vol, 0x55, (size_t)S * R * ndx * ndy * 4);
        CHECK(mx_match(d2, NULL, p3, centre, S, R, M, W, H, wx, wy, 64, 1, b3, vol) == 0);
        CHECK(mx_match(d2, NULL, p3, centre, S, R, M, W, H, wx, wy, 64, 1, b3n, NULL) == 0);
        CHECK(memcmp(b3, b3n, sizeof b3) == 0);
        CHECK(eq6(b3, 0, 0, 0, 0, 0, R * ndx * ndy) && eq6(b3 + 6, -1, 0, 0, 0, 0, 0) && eq6(b3 + 12, 0, 0, 0, 0, 0, R * ndx * ndy));
        for (int i = 0; i < S * R * ndx * ndy; ++i) CHECK(vol[i] == 0);
        centre[2] = 0, centre[3] = -16385;
        CHECK(mx_match(d2, NULL, p3, centre, S, R, M, W, H, wx, wy, 64, 1, b3, vol) == 0 && b3[6] == -1);
        /* a centre at the end of its range with a point at the end of its reach: the sums stay in int32 */
        p3[0] = 16384, p3[1] = -16384;
        CHECK(mx_match(d2, NULL, p3, centre, 1, R, M, W, H, wx, wy, 64, 7, b3, vol) == 0);
        CHECK(eq6(b3, 1, 0, 0, 0, 0, ndx * ndy));   /* rotation 1 has no point and scores 0; rotation 0 pays unk */
        free(p3);
        free(vol);
        printf("ignored, absent, range ends: ok\n");
    }

    /* tie order on a single obstacle: one point at offset 0 matches it from (+1, 0) and (0, +1) away at equal
     * displacement -> the smaller dy wins, then the smaller dx; two equal rotations -> the earlier */
    {
        enum { TW = 9, TH = 9 };
        uint8_t o2[TW * TH] = {0};
        o2[4 * TW + 3] = 1, o2[3 * TW + 4] = 1, o2[4 * TW + 5] = 1, o2[5 * TW + 4] = 1;   /* a plus without its centre */
        int32_t* t2 = edt(o2, TW, TH);
        CHECK(t2);
        const int32_t p[4] = {0, 0, 0, 0}, centre[2] = {4, 4};
        int32_t sc[2 * 9];
        CHECK(mx_match(t2, NULL, p, centre, 1, 2, 1, TW, TH, 1, 1, 64, 1, best, sc) == 0);
        CHECK(eq6(best, 0, 0, -1, 0, 1, 8));   /* (dy, dx) = (-1, 0) before (0, -1), (0, 1), (1, 0); rotation 0 before 1 */
        CHECK(sc[4] == 1 && sc[1] == 0 && sc[3] == 0 && sc[5] == 0 && sc[7] == 0 && sc[0] == 1);
        free(t2);
        printf("tie order: ok\n");
    }

    /* the int32 bound: 65536 points on an 8 x 8 grid without obstacles, cap 32767, window 0 */
    {
        enum { BW = 8, BN = 65536 };
        int32_t* inf = (int32_t*)malloc((size_t)BW * BW * 4);
        int32_t* p = (int32_t*)calloc((size_t)BN * 2, 4);
        CHECK(inf && p);
        for (int i = 0; i < BW * BW; ++i) inf[i] = INT32_MAX;
        for (int i = 0; i < BN; ++i) { p[2 * i] = i % BW - 3; p[2 * i + 1] = (i / BW) % BW - 3; }
        const int32_t centre[2] = {3, 3};
        int32_t one;
        CHECK(mx_match(inf, NULL, p, centre, 1, 1, BN, BW, BW, 0, 0, 32767, 0, best, &one) == 0);
        CHECK(eq6(best, 0, 0, 0, 2147418112, BN, 1) && one == 2147418112);
        free(inf);
        free(p);
        printf("int32 bound: 2147418112\n");
    }

    /* argument errors */
    {
        const int32_t centre[2] = {ax, ay};
        CHECK(mx_match(NULL, NULL, pts, centre, 1, 1, N, W, H, wx, wy, 64, 1, best, NULL) == 1);
        CHECK(mx_match(d2, NULL, pts, centre, 1, 0, N, W, H, wx, wy, 64, 1, best, NULL) == 1);
        CHECK(mx_match(d2, NULL, pts, centre, 1, 1, 0, W, H, wx, wy, 64, 1, best, NULL) == 1);
        CHECK(mx_match(d2, NULL, pts, centre, 1, 1, N, W, H, 65, wy, 64, 1, best, NULL) == 1);
        CHECK(mx_match(d2, NULL, pts, centre, 1, 1, N, W, H, wx, wy, 32768, 1, best, NULL) == 1);
        CHECK(mx_match(d2, NULL, pts, centre, 1, 1, N, W, H, wx, wy, 64, 65, best, NULL) == 1);
        CHECK(mx_match(d2, NULL, pts, centre, 1, 1, N, W, H, wx, wy, 64, 1, best, best) == 1);
        CHECK(mx_match(d2, NULL, pts, centre, 0, 1, N, W, H, wx, wy, 64, 1, best, NULL) == 0);
    }
    free(occ);
    free(d2);
    free(pts);
    free(score);
    printf("match_ref OK\n");
    return 0;
}
