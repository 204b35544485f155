/* Single-threaded C statement of the delay schedules (sc_traj_shift_table_batch, sc_traj_schedule_batch,
 * sc_traj_shift_knots_batch; the definition is in include/sea_current_hip.h): the shift-conflict table, the priority greedy
 * and the shifted knots, from the knots traj_ref.c's tr_knots writes.  The predicate is tr_conflicts' m2 < R*R, product by
 * product; compile with -ffp-contract=off.  tests/test_traj_sched_ref.py compares it with the NumPy twin bit for bit. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define TS_OK 0
#define TS_BAD 2
#define TS_BOX_SLACK 0x1p-48

static double clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

static const double* knot(const double* row, int k, int s) { return row + 2 * (size_t)(k - s > 0 ? k - s : 0); }

/* does lo, shifted by sl ticks, meet hi, shifted by sh ticks, on some interval? */
static int pair_conf(const double* lo, const double* hi, int K, int sl, int sh, double RR) {
    double d0x = hi[0] - lo[0], d0y = hi[1] - lo[1];
    for (int k = 0; k < K; ++k) {
        const double *a = knot(lo, k + 1, sl), *b = knot(hi, k + 1, sh);
        const double d1x = b[0] - a[0], d1y = b[1] - a[1];
        const double ex = d1x - d0x, ey = d1y - d0y;
        const double aa = ex * ex + ey * ey;
        const double bb = d0x * ex + d0y * ey;
        const double lam = aa > 0.0 ? clamp01(-bb / aa) : 0.0;
        const double px = d0x + lam * ex, py = d0y + lam * ey;
        const double m2 = px * px + py * py;
        if (m2 < RR) return 1;
        d0x = d1x;
        d0y = d1y;
    }
    return 0;
}

static void box_of(const double* row, int K, double* b) {
    b[0] = b[2] = INFINITY;
    b[1] = b[3] = -INFINITY;
    for (int k = 0; k <= K; ++k) {
        const double x = row[2 * (size_t)k], y = row[2 * (size_t)k + 1];
        if (!(x == x && y == y)) continue;
        if (x < b[0]) b[0] = x;
        if (x > b[1]) b[1] = x;
        if (y < b[2]) b[2] = y;
        if (y > b[3]) b[3] = y;
    }
}

static double gap2(const double* a, const double* b) {
    const double lx = a[0] > b[0] ? a[0] : b[0], hx = a[1] < b[1] ? a[1] : b[1];
    const double ly = a[2] > b[2] ? a[2] : b[2], hy = a[3] < b[3] ? a[3] : b[3];
    const double wx = (a[1] > b[1] ? a[1] : b[1]) - (a[0] < b[0] ? a[0] : b[0]);
    const double wy = (a[3] > b[3] ? a[3] : b[3]) - (a[2] < b[2] ? a[2] : b[2]);
    double gx = (lx - hx) - TS_BOX_SLACK * wx, gy = (ly - hy) - TS_BOX_SLACK * wy;
    gx = gx > 0.0 ? gx : 0.0;
    gy = gy > 0.0 ? gy : 0.0;
    return gx * gx + gy * gy;
}

/* table uint64 [P][P]; skip != 0 drops the pairs whose boxes are too far apart (the same table either way); stats (may be NULL)
 * int64 [2]: pairs compared, pairs the box test drops */
void ts_shift_table(const double* knots, int32_t* tstatus, int P, int K, const double* radius, const int32_t* group, int D, int stride,
                    int skip, uint64_t* table, int64_t* stats) {
    const int nb = 2 * D - 1;
    int64_t compared = 0, skipped = 0;
    for (int p = 0; p < P; ++p)
        if (tstatus[p] == TS_OK && !(isfinite(radius[p]) && radius[p] >= 0.0)) tstatus[p] = TS_BAD;
    for (size_t i = 0; i < (size_t)P * P; ++i) table[i] = 0;
    for (int lo = 0; lo + 1 < P; ++lo) {
        if (tstatus[lo] != TS_OK) continue;
        const double* klo = knots + (size_t)lo * (K + 1) * 2;
        double blo[4];
        box_of(klo, K, blo);
        for (int hi = lo + 1; hi < P; ++hi) {
            if (tstatus[hi] != TS_OK || (group && group[lo] >= 0 && group[lo] == group[hi])) continue;
            const double* khi = knots + (size_t)hi * (K + 1) * 2;
            const double R = radius[lo] + radius[hi];
            const double RR = R * R;
            double bhi[4];
            box_of(khi, K, bhi);
            ++compared;
            if (!(gap2(blo, bhi) < RR)) {
                ++skipped;
                if (skip) continue;
            }
            uint64_t w = 0, m = 0;
            for (int b = 0; b < nb; ++b) {
                const int r = b - (D - 1);
                if (pair_conf(klo, khi, K, (r > 0 ? r : 0) * stride, (r < 0 ? -r : 0) * stride, RR)) {
                    w |= (uint64_t)1 << b;
                    m |= (uint64_t)1 << (nb - 1 - b);
                }
            }
            table[(size_t)lo * P + hi] = w;
            table[(size_t)hi * P + lo] = m;
        }
    }
    if (stats) { stats[0] = compared; stats[1] = skipped; }
}

void ts_schedule(const uint64_t* table, const int32_t* tstatus, int P, int D, const int32_t* order, const int32_t* jmax, int32_t* slot,
                 int32_t* counts) {
    const uint64_t mask = ((uint64_t)1 << D) - 1;
    for (int p = 0; p < P; ++p) slot[p] = -3;
    for (int i = 0; i < P; ++i) {
        const int p = order ? order[i] : i;
        if (p < 0 || p >= P || slot[p] != -3) continue;
        const int jm = jmax ? jmax[p] : D - 1;
        if (tstatus[p] != TS_OK) { slot[p] = -2; continue; }
        if (jm < 0) { slot[p] = 0; continue; }
        uint64_t busy = 0;
        for (int q = 0; q < P; ++q)
            if (slot[q] >= 0) busy |= (table[(size_t)p * P + q] >> (D - 1 - slot[q])) & mask;
        int s = -1;
        for (int j = 0; j <= (jm < D - 1 ? jm : D - 1); ++j)
            if (!((busy >> j) & 1)) { s = j; break; }
        slot[p] = s;
    }
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int p = 0; p < P; ++p) ++counts[slot[p] == 0 ? 0 : (slot[p] > 0 ? 1 : (slot[p] == -1 ? 2 : 3))];
}

void ts_shift_knots(const double* knots, int P, int K, const int32_t* slot, int stride, double* out) {
    for (int p = 0; p < P; ++p) {
        const double* row = knots + (size_t)p * (K + 1) * 2;
        double* o = out + (size_t)p * (K + 1) * 2;
        for (int k = 0; k <= K; ++k) {
            if (slot[p] < 0) { o[2 * k] = o[2 * k + 1] = NAN; continue; }
            const long long src = (long long)k - (long long)slot[p] * stride;
            o[2 * k] = row[2 * (size_t)(src > 0 ? src : 0)];
            o[2 * k + 1] = row[2 * (size_t)(src > 0 ? src : 0) + 1];
        }
    }
}
