/* CPU reference of the timed-path conflicts (sc_traj_knots_batch, sc_traj_conflicts_batch): the definition of
 * include/sea_current_hip.h in plain C, fp64, one pair and one interval at a time.  Build with -ffp-contract=off.
 * tests/test_traj_ref.py compares it bit for bit with the NumPy twin (tests/traj_twin.py); tests/cpp/traj_ref_check.c
 * drives it under the sanitizers; tools/traj_conflicts_time.py times it (single-threaded) beside the GPU. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

enum { TR_OK = 0, TR_SKIPPED = 1, TR_BAD = 2 };

static double clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

/* knots fp64 [P][K+1][2], tstatus int32 [P] */
void tr_knots(const double* time, const float* pts, const int32_t* offsets, const int32_t* length, const int32_t* status, int P,
              const double* t0, const int32_t* flags, double T0, double dt_c, int K, double* knots, int32_t* tstatus) {
    for (int p = 0; p < P; ++p) {
        double* out = knots + (size_t)p * (K + 1) * 2;
        const int n = length[p];
        int st = TR_OK;
        if ((status && status[p] != 0) || n < 1) st = TR_SKIPPED;
        const double* t = time + (st == TR_OK ? offsets[p] : 0);
        const float* xy = pts + (st == TR_OK ? 2 * (size_t)offsets[p] : 0);
        const double d = t0 ? t0[p] : 0.0;
        if (st == TR_OK) {
            if (!isfinite(d)) st = TR_BAD;
            for (int i = 0; i < n; ++i) {
                if (!isfinite(t[i]) || !isfinite(xy[2 * i]) || !isfinite(xy[2 * i + 1])) st = TR_BAD;
                if (i + 1 < n && t[i + 1] < t[i]) st = TR_BAD;
            }
        }
        tstatus[p] = st;
        if (st != TR_OK) {
            for (int k = 0; k < 2 * (K + 1); ++k) out[k] = NAN;
            continue;
        }
        const int fl = flags ? flags[p] : 3;
        for (int k = 0; k <= K; ++k) {
            const double tau = T0 + (double)k * dt_c;
            const double u = tau - d;
            double x, y;
            if (u < t[0]) {
                x = (fl & 1) ? (double)xy[0] : NAN;
                y = (fl & 1) ? (double)xy[1] : NAN;
            } else if (u > t[n - 1]) {
                x = (fl & 2) ? (double)xy[2 * (n - 1)] : NAN;
                y = (fl & 2) ? (double)xy[2 * (n - 1) + 1] : NAN;
            } else if (n == 1) {
                x = (double)xy[0];
                y = (double)xy[1];
            } else {
                int lo = 0, hi = n; /* the number of time[i] <= u */
                while (lo < hi) {
                    const int m = (lo + hi) >> 1;
                    if (t[m] <= u) lo = m + 1; else hi = m;
                }
                int j = lo - 1;
                if (j < 0) j = 0;
                if (j > n - 2) j = n - 2;
                const double den = t[j + 1] - t[j];
                const double f = den > 0.0 ? (u - t[j]) / den : 0.0;
                const double ax = (double)xy[2 * j], ay = (double)xy[2 * j + 1];
                const double bx = (double)xy[2 * j + 2], by = (double)xy[2 * j + 3];
                x = ax + f * (bx - ax);
                y = ay + f * (by - ay);
            }
            out[2 * k] = x;
            out[2 * k + 1] = y;
        }
    }
}

/* Every output may be NULL but tstatus (in: what tr_knots gave; out: TR_BAD also where the radius is outside the contract).
 * conflict uint32 [P][ceil(P/32)]. */
void tr_conflicts(const double* knots, int32_t* tstatus, int P, int K, double T0, double dt_c, const double* radius,
                  const int32_t* group, double sep_cap, double* first_t, int32_t* first_with, double* min_sep, int32_t* min_with,
                  int32_t* n_conf, uint32_t* conflict) {
    const int nw = (P + 31) / 32;
    for (int p = 0; p < P; ++p)
        if (tstatus[p] == TR_OK && !(isfinite(radius[p]) && radius[p] >= 0.0)) tstatus[p] = TR_BAD;
    if (conflict)
        for (size_t i = 0; i < (size_t)P * nw; ++i) conflict[i] = 0u;
    for (int p = 0; p < P; ++p) {
        double bf = INFINITY, bs = INFINITY;
        int bfw = -1, bsw = -1, nc = 0;
        for (int q = 0; q < P && tstatus[p] == TR_OK; ++q) {
            if (q == p || tstatus[q] != TR_OK) continue;
            if (group && group[p] == group[q] && group[p] >= 0) continue;
            const int lo = p < q ? p : q, hi = p < q ? q : p;
            const double* kl = knots + (size_t)lo * (K + 1) * 2;
            const double* kh = knots + (size_t)hi * (K + 1) * 2;
            const double R = radius[lo] + radius[hi];
            const double RR = R * R;
            double first = INFINITY, sep2 = INFINITY;
            for (int k = 0; k < K; ++k) {
                if (isnan(kl[2 * k]) || isnan(kh[2 * k]) || isnan(kl[2 * k + 2]) || isnan(kh[2 * k + 2])) continue;
                const double d0x = kh[2 * k] - kl[2 * k], d0y = kh[2 * k + 1] - kl[2 * k + 1];
                const double d1x = kh[2 * k + 2] - kl[2 * k + 2], d1y = kh[2 * k + 3] - kl[2 * k + 3];
                const double ex = d1x - d0x, ey = d1y - d0y;
                const double a = ex * ex + ey * ey;
                const double b = d0x * ex + d0y * ey;
                const double c = d0x * d0x + d0y * d0y;
                const double lam = a > 0.0 ? clampd(-b / a, 0.0, 1.0) : 0.0;
                const double px = d0x + lam * ex, py = d0y + lam * ey;
                const double m2 = px * px + py * py;
                if (m2 < sep2) sep2 = m2;
                if (m2 < RR) {
                    double lc = 0.0;
                    if (!(c < RR)) {
                        double disc = b * b - a * (c - RR);
                        disc = disc > 0.0 ? disc : 0.0;
                        lc = clampd((-b - sqrt(disc)) / a, 0.0, lam);
                    }
                    const double tau = T0 + (double)k * dt_c;
                    const double t = tau + lc * dt_c;
                    if (t < first) first = t;
                }
            }
            if (first < INFINITY) {
                ++nc;
                if (conflict) conflict[(size_t)p * nw + (q >> 5)] |= 1u << (q & 31);
            }
            if (first < bf) { bf = first; bfw = q; }
            if (sep2 < bs) { bs = sep2; bsw = q; }
        }
        const double ms = sqrt(bs);
        const int rep = ms < sep_cap;
        if (first_t) first_t[p] = bf;
        if (first_with) first_with[p] = bfw;
        if (min_sep) min_sep[p] = rep ? ms : INFINITY;
        if (min_with) min_with[p] = rep ? bsw : -1;
        if (n_conf) n_conf[p] = nc;
    }
}
