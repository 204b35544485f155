/* Stand-alone driver of the CPU reference of the delay schedules (traj_sched_ref.c) for sanitizer runs on the host:
 *   cc -g -O1 -std=c11 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o traj_sched_ref_check \
 *      tests/cpp/traj_sched_ref_check.c tests/cpp/traj_sched_ref.c tests/cpp/traj_ref.c -lm
 * The right-angle crossing by hand (the second path gets slot 3), then seeded random fleets with skipped paths, paths outside
 * the contract, every flag combination and groups, K extended so that every path rests where the shifts end: table[p][q] is
 * the bit reversal of table[q][p], the diagonal and the bits from 2D-1 up are 0, the r = 0 bit is tr_conflicts' matrix, the
 * table is the same with and without the box skip, every slot obeys the greedy rule (its window bit is clear and every lower
 * one set), counts add up, a random order and pinned paths are honoured, and tr_conflicts on the shifted knots reports no
 * conflict among the scheduled paths.  Prints one line per fleet and "traj_sched_ref OK"; exit code 1 on the first failed
 * check. */
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
void ts_shift_table(const double* knots, int32_t* tstatus, int P, int K, const double* radius, const int32_t* group, int D, int stride,
                    int skip, uint64_t* table, int64_t* stats);
void ts_schedule(const uint64_t* table, const int32_t* tstatus, int P, int D, const int32_t* order, const int32_t* jmax, int32_t* slot,
                 int32_t* counts);
void ts_shift_knots(const double* knots, int P, int K, const int32_t* slot, int stride, double* out);

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

/* (0,0) -> (8,0) and (4,-4) -> (4,4) in 8 s each, radius 0.5, both absent after their runs, dt_c 0.5.  With the second path
 * delta seconds behind, the two are delta / sqrt(2) apart at their closest: they meet iff |delta| < sqrt(2) s, i.e. for relative
 * shifts of -2 .. 2 ticks (bits 5 .. 9 of both entries), and the second path's first free slot is 3. */
static int crossing(void) {
    double time[18], knots[2 * 31 * 2], out[2 * 31 * 2], radius[2] = {0.5, 0.5};
    float pts[36];
    int32_t offsets[3] = {0, 9, 18}, length[2] = {9, 9}, flags[2] = {0, 0}, ts[2], slot[2], counts[4];
    uint64_t table[4];
    for (int i = 0; i < 9; ++i) {
        time[i] = time[9 + i] = i;
        pts[2 * i] = (float)i; pts[2 * i + 1] = 0.f;
        pts[18 + 2 * i] = 4.f; pts[18 + 2 * i + 1] = (float)(i - 4);
    }
    tr_knots(time, pts, offsets, length, NULL, 2, NULL, flags, 0.0, 0.5, 30, knots, ts);
    ts_shift_table(knots, ts, 2, 30, radius, NULL, 8, 1, 1, table, NULL);
    ts_schedule(table, ts, 2, 8, NULL, NULL, slot, counts);
    ts_shift_knots(knots, 2, 30, slot, 1, out);
    printf("crossing: table[1][0] = 0x%llx, slots %d %d\n", (unsigned long long)table[2], slot[0], slot[1]);
    CHECK(table[0] == 0 && table[3] == 0 && table[2] == 0x3e0ull && table[1] == 0x3e0ull);
    CHECK(slot[0] == 0 && slot[1] == 3 && counts[0] == 1 && counts[1] == 1 && counts[2] == 0 && counts[3] == 0);
    CHECK(out[2 * 31 + 0] == 4.0 && out[2 * 31 + 2 * 3 + 1] == -4.0 && out[2 * 31 + 2 * 4 + 1] == -3.5);
    return 0;
}

static uint64_t reverse_bits(uint64_t w, int nb) {
    uint64_t m = 0;
    for (int b = 0; b < nb; ++b)
        if ((w >> b) & 1) m |= (uint64_t)1 << (nb - 1 - b);
    return m;
}

static int fleet(int P, int K0, double dt_c, int D, int stride) {
    const int K = K0 + (D - 1) * stride, nw = (P + 31) / 32, nb = 2 * D - 1;
    int32_t* offsets = (int32_t*)malloc((size_t)(P + 1) * sizeof(int32_t));
    int32_t* length = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* status = (int32_t*)calloc((size_t)P, sizeof(int32_t));
    int32_t* flags = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* group = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* order = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* jmax = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    double* t0 = (double*)malloc((size_t)P * sizeof(double));
    double* radius = (double*)malloc((size_t)P * sizeof(double));
    CHECK(offsets && length && status && flags && group && order && jmax && t0 && radius);
    offsets[0] = 0;
    const double span = K0 * dt_c;   /* every path ends before T0 + span */
    for (int p = 0; p < P; ++p) {
        length[p] = p % 11 == 0 ? 1 : 2 + (int)(rnd() * 30);
        offsets[p + 1] = offsets[p] + length[p];
        flags[p] = p % 4;
        group[p] = (int)(rnd() * 7) - 2;
        t0[p] = rnd() * span * 0.3;
        radius[p] = 0.3 + rnd();
        order[p] = (int)(rnd() * (P + 2)) - 1;          /* repeats, omissions, -1 and P */
        jmax[p] = p % 7 == 3 ? -1 : (int)(rnd() * (D + 2));
    }
    const int M = offsets[P];
    double* time = (double*)malloc((size_t)M * sizeof(double));
    float* pts = (float*)malloc((size_t)M * 2 * sizeof(float));
    CHECK(time && pts);
    for (int p = 0; p < P; ++p) {
        const double step = span * 0.6 / 32;
        double t = rnd() * step, x = rnd() * 20, y = rnd() * 20, h = rnd() * 6.283185307179586;
        for (int i = 0; i < length[p]; ++i) {
            const double dt = rnd() < 0.05 ? 0.0 : step * (0.1 + 0.9 * rnd());
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
    }
    const size_t kn = (size_t)P * (K + 1) * 2;
    double* knots = (double*)malloc(kn * sizeof(double));
    double* moved = (double*)malloc(kn * sizeof(double));
    int32_t* ts = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* ts2 = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* slot = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* slot2 = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    int32_t* nc = (int32_t*)malloc((size_t)P * sizeof(int32_t));
    uint32_t* bits = (uint32_t*)malloc((size_t)P * nw * sizeof(uint32_t));
    uint64_t* table = (uint64_t*)malloc((size_t)P * P * sizeof(uint64_t));
    uint64_t* dense = (uint64_t*)malloc((size_t)P * P * sizeof(uint64_t));
    CHECK(knots && moved && ts && ts2 && slot && slot2 && nc && bits && table && dense);
    int32_t counts[4], counts2[4];
    int64_t stats[2];
    tr_knots(time, pts, offsets, length, status, P, t0, flags, -1.0, dt_c, K, knots, ts);
    memcpy(ts2, ts, (size_t)P * sizeof(int32_t));
    ts_shift_table(knots, ts, P, K, radius, group, D, stride, 1, table, stats);
    ts_shift_table(knots, ts2, P, K, radius, group, D, stride, 0, dense, NULL);
    CHECK(memcmp(table, dense, (size_t)P * P * sizeof(uint64_t)) == 0 && memcmp(ts, ts2, (size_t)P * sizeof(int32_t)) == 0);
    if (P >= 8) CHECK(ts[2] == 1 && ts[3] == 1 && ts[4] == 2 && ts[5] == 2);
    tr_conflicts(knots, ts2, P, K, -1.0, dt_c, radius, group, INFINITY, NULL, NULL, NULL, NULL, nc, bits);
    for (int p = 0; p < P; ++p)
        for (int q = 0; q < P; ++q) {
            const uint64_t w = table[(size_t)p * P + q];
            CHECK(w == reverse_bits(table[(size_t)q * P + p], nb) && (nb == 64 || (w >> nb) == 0));
            if (p == q || ts[p] != 0 || ts[q] != 0 || (group[p] >= 0 && group[p] == group[q])) CHECK(w == 0);
            CHECK(((w >> (D - 1)) & 1) == ((bits[(size_t)p * nw + (q >> 5)] >> (q & 31)) & 1));
        }
    /* the natural order, then a random order with repeats, omissions, pins and per-path limits */
    for (int round = 0; round < 2; ++round) {
        const int32_t *ord = round ? order : NULL, *jm = round ? jmax : NULL;
        int32_t* s = round ? slot2 : slot;
        int32_t* c = round ? counts2 : counts;
        ts_schedule(table, ts, P, D, ord, jm, s, c);
        CHECK(c[0] + c[1] + c[2] + c[3] == P);
        char* placed = (char*)calloc((size_t)P, 1);
        CHECK(placed);
        for (int i = 0; i < P; ++i) {
            const int p = ord ? ord[i] : i;
            if (p < 0 || p >= P || placed[p] == 2) continue;
            const int lim = jm ? jm[p] : D - 1;
            if (ts[p] != 0) CHECK(s[p] == -2);
            else if (lim < 0) CHECK(s[p] == 0);
            else {
                const int top = lim < D - 1 ? lim : D - 1;
                CHECK(s[p] >= -1 && s[p] <= top);
                for (int j = 0; j <= (s[p] >= 0 ? s[p] : top); ++j) {
                    int blocked = 0;
                    for (int q = 0; q < P; ++q)
                        if (placed[q] == 2 && s[q] >= 0 && ((table[(size_t)p * P + q] >> (j - s[q] + D - 1)) & 1)) blocked = 1;
                    CHECK(blocked == (j != s[p]));
                }
            }
            placed[p] = 2;
        }
        for (int p = 0; p < P; ++p)
            if (!placed[p]) CHECK(s[p] == -3);
        free(placed);
    }
    ts_shift_knots(knots, P, K, slot, stride, moved);
    memcpy(ts2, ts, (size_t)P * sizeof(int32_t));
    tr_conflicts(moved, ts2, P, K, -1.0, dt_c, radius, group, INFINITY, NULL, NULL, NULL, NULL, nc, NULL);
    int left = 0;
    for (int p = 0; p < P; ++p) {
        left += nc[p];
        for (int k = 0; k <= K; ++k) {
            const double* o = moved + ((size_t)p * (K + 1) + k) * 2;
            if (slot[p] < 0) { CHECK(isnan(o[0]) && isnan(o[1])); continue; }
            const int src = k - slot[p] * stride > 0 ? k - slot[p] * stride : 0;
            CHECK(memcmp(o, knots + ((size_t)p * (K + 1) + src) * 2, 16) == 0);
        }
    }
    CHECK(left == 0);
    printf("fleet P %d K %d D %d stride %d: %lld pairs compared, %lld dropped by the box, slots %d / %d / %d / %d, random order %d / %d / %d / %d\n",
           P, K, D, stride, (long long)stats[0], (long long)stats[1], counts[0], counts[1], counts[2], counts[3], counts2[0], counts2[1],
           counts2[2], counts2[3]);
    free(offsets); free(length); free(status); free(flags); free(group); free(order); free(jmax); free(t0); free(radius); free(time);
    free(pts); free(knots); free(moved); free(ts); free(ts2); free(slot); free(slot2); free(nc); free(bits); free(table); free(dense);
    return 0;
}

int main(void) {
    if (crossing()) return 1;
    if (fleet(1, 1, 0.5, 1, 1)) return 1;
    if (fleet(2, 4, 10.0, 2, 3)) return 1;
    if (fleet(33, 40, 1.0, 8, 1)) return 1;
    if (fleet(97, 160, 0.25, 8, 4)) return 1;
    if (fleet(60, 120, 0.25, 32, 2)) return 1;
    printf("traj_sched_ref OK\n");
    return 0;
}
