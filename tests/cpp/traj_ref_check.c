/* Stand-alone driver of the CPU reference (traj_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -std=c11 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o traj_ref_check \
 *      tests/cpp/traj_ref_check.c tests/cpp/traj_ref.c -lm
 * The head-on hand case (first_t 3.5, min_sep 0), then seeded random fleets with skipped paths, paths outside the contract,
 * one-sample paths, every flag combination and groups: the matrix is symmetric with an empty diagonal, n_conf is the
 * population of a row, first_with / min_with point at partners whose own results are at least as early / close, paths
 * that are not OK read "none" and appear in no row, and a second call with every optional output NULL but one gives the
 * same values.  Prints one line per fleet and "traj_ref OK"; exit code 1 on the first failed check. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void tr_knots(const double* time, const float* pts, const int32_t* offsets, const int32_t* length, const int32_t* status, int P,
              const double* t0, const int32_t* flags, double T0, double dt_c, int K, double* knots, int32_t* tstatus);
void tr_conflicts(const double* knots, int32_t* tstatus, int P, int K, double T0, double dt_c, const double* radius,
                  const int32_t* group, double sep_cap, double* first_t, int32_t* first_with, double* min_sep, int32_t* min_with,
                  int32_t* n_conf, uint32_t* conflict);

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

static int head_on(void) {
    double time[18], knots[2 * 17 * 2], first_t[2], min_sep[2], radius[2] = {0.5, 0.5};
    float pts[36];
    int32_t offsets[3] = {0, 9, 18}, length[2] = {9, 9}, ts[2], fw[2], mw[2], nc[2];
    uint32_t bits[2];
    for (int i = 0; i < 9; ++i) {
        time[i] = time[9 + i] = i;
        pts[2 * i] = (float)i; pts[2 * i + 1] = 0.f;
        pts[18 + 2 * i] = (float)(8 - i); pts[18 + 2 * i + 1] = 0.f;
    }
    tr_knots(time, pts, offsets, length, NULL, 2, NULL, NULL, 0.0, 0.5, 16, knots, ts);
    tr_conflicts(knots, ts, 2, 16, 0.0, 0.5, radius, NULL, INFINITY, first_t, fw, min_sep, mw, nc, bits);
    CHECK(ts[0] == 0 && ts[1] == 0);
    CHECK(first_t[0] == 3.5 && first_t[1] == 3.5 && min_sep[0] == 0.0 && min_sep[1] == 0.0);
    CHECK(fw[0] == 1 && fw[1] == 0 && mw[0] == 1 && mw[1] == 0 && nc[0] == 1 && nc[1] == 1 && bits[0] == 2u && bits[1] == 1u);
    printf("head-on: first_t %.17g, min_sep %.17g\n", first_t[0], min_sep[0]);
    return 0;
}

static int fleet(int P, int K, double dt_c, double sep_cap) {
    const int nw = (P + 31) / 32;
    int32_t* offsets = (int32_t*)malloc((size_t)(P + 1) * sizeof(int32_t));
    int32_t* length = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* status = (int32_t*)calloc((size_t)P, sizeof(int32_t));
    int32_t* flags = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* group = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    double* t0 = (double*)malloc((size_t)P * sizeof(double));
    double* radius = (double*)malloc((size_t)P * sizeof(double));
    CHECK(offsets && length && status && flags && group && t0 && radius);
    offsets[0] = 0;
    for (int p = 0; p < P; ++p) {
        length[p] = p % 11 == 0 ? 1 : 2 + (int)(rnd() * 30);
        offsets[p + 1] = offsets[p] + length[p];
        flags[p] = p % 4;
        group[p] = (int)(rnd() * 7) - 2;
        t0[p] = rnd() * 20 - 2;
        radius[p] = 0.3 + rnd();
    }
    const int M = offsets[P];
    double* time = (double*)malloc((size_t)M * sizeof(double));
    float* pts = (float*)malloc((size_t)M * 2 * sizeof(float));
    CHECK(time && pts);
    for (int p = 0; p < P; ++p) {
        double t = rnd() * 2, x = rnd() * 30, y = rnd() * 30, h = rnd() * 6.283185307179586;
        for (int i = 0; i < length[p]; ++i) {
            const double dt = rnd() < 0.05 ? 0.0 : 0.1 + rnd();
            time[offsets[p] + i] = t;
            pts[2 * (offsets[p] + i)] = (float)x;
            pts[2 * (offsets[p] + i) + 1] = (float)y;
            t += dt; h += (rnd() - 0.5) * 0.3;
            x += cos(h) * dt * 1.5; y += sin(h) * dt * 1.5;
        }
    }
    if (P >= 8) {
        status[2] = 4;                                 /* skipped */
        length[3] = 0;                                 /* skipped */
        pts[2 * offsets[4]] = NAN;                     /* bad */
        radius[5] = -1.0;                              /* bad */
        if (length[6] >= 2) time[offsets[6] + 1] = time[offsets[6]] - 1.0;   /* bad */
    }
    double* knots = (double*)malloc((size_t)P * (K + 1) * 2 * sizeof(double));
    int32_t* ts = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* ts2 = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    double* first_t = (double*)malloc((size_t)P * sizeof(double));
    double* min_sep = (double*)malloc((size_t)P * sizeof(double));
    double* first2 = (double*)malloc((size_t)P * sizeof(double));
    int32_t* fw = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* mw = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* nc = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    uint32_t* bits = (uint32_t*)malloc((size_t)P * nw * sizeof(uint32_t));
    CHECK(knots && ts && ts2 && first_t && min_sep && first2 && fw && mw && nc && bits);
    tr_knots(time, pts, offsets, length, status, P, t0, flags, -1.0, dt_c, K, knots, ts);
    memcpy(ts2, ts, (size_t)P * sizeof(int32_t));
    tr_conflicts(knots, ts, P, K, -1.0, dt_c, radius, group, sep_cap, first_t, fw, min_sep, mw, nc, bits);
    tr_conflicts(knots, ts2, P, K, -1.0, dt_c, radius, group, sep_cap, first2, NULL, NULL, NULL, NULL, NULL);
    int pairs = 0, okp = 0;
    for (int p = 0; p < P; ++p) {
        CHECK(ts[p] == ts2[p] && (first_t[p] == first2[p]));
        int pop = 0;
        for (int q = 0; q < P; ++q) {
            const int b = (bits[(size_t)p * nw + (q >> 5)] >> (q & 31)) & 1, bt = (bits[(size_t)q * nw + (p >> 5)] >> (p & 31)) & 1;
            CHECK(b == bt);
            if (b) CHECK(p != q && ts[p] == 0 && ts[q] == 0 && !(group[p] == group[q] && group[p] >= 0));
            pop += b;
        }
        for (int q = P; q < nw * 32; ++q) CHECK(!((bits[(size_t)p * nw + (q >> 5)] >> (q & 31)) & 1));
        CHECK(pop == nc[p]);
        pairs += pop;
        if (ts[p] != 0) {
            CHECK(isinf(first_t[p]) && isinf(min_sep[p]) && fw[p] == -1 && mw[p] == -1 && nc[p] == 0);
            for (int k = 0; k < 2 * (K + 1); ++k) if (ts[p] != 2 || isnan(radius[p]) || radius[p] >= 0) CHECK(isnan(knots[(size_t)p * (K + 1) * 2 + k]));
            continue;
        }
        ++okp;
        CHECK((nc[p] > 0) == (fw[p] >= 0) && (nc[p] > 0) == (first_t[p] < INFINITY));
        if (fw[p] >= 0) CHECK(first_t[fw[p]] <= first_t[p] && ((bits[(size_t)p * nw + (fw[p] >> 5)] >> (fw[p] & 31)) & 1));
        if (mw[p] >= 0) CHECK(min_sep[p] < sep_cap && min_sep[mw[p]] <= min_sep[p]);
        else CHECK(isinf(min_sep[p]));
        if (nc[p] > 0 && sep_cap == INFINITY) CHECK(min_sep[p] < radius[p] + 1.3 + 1e-9);
    }
    if (P >= 8) CHECK(ts[2] == 1 && ts[3] == 1 && ts[4] == 2 && ts[5] == 2 && (length[6] < 2 || ts[6] == 2));
    printf("fleet P %d K %d dt_c %g sep_cap %g: %d paths OK, %d conflicting pairs\n", P, K, dt_c, sep_cap, okp, pairs / 2);
    free(offsets); free(length); free(status); free(flags); free(group); free(t0); free(radius); free(time); free(pts);
    free(knots); free(ts); free(ts2); free(first_t); free(min_sep); free(first2); free(fw); free(mw); free(nc); free(bits);
    return 0;
}

int main(void) {
    if (head_on()) return 1;
    if (fleet(1, 1, 0.5, INFINITY)) return 1;
    if (fleet(2, 1, 40.0, INFINITY)) return 1;
    if (fleet(33, 17, 1.0, INFINITY)) return 1;
    if (fleet(97, 160, 0.25, INFINITY)) return 1;
    if (fleet(97, 160, 0.25, 2.0)) return 1;
    printf("traj_ref OK\n");
    return 0;
}
