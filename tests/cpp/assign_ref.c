// assign_ref.c -- single-threaded C restatement of sc_assign_batch and sc_field_cost_matrix (the definition is in
// include/sea_current_hip.h): the shortest-augmenting-path Hungarian method on the padded int64 matrix, every delta applied in the
// pass that finds it, ties towards the lowest post.  Checker and yardstick only; the library never links it.
#include <stdint.h>
#include <stdlib.h>

#define AR_MAX_DIM 1024
#define AR_BIG (1ll << 42)
#define AR_INF INT32_MAX
#define AR_NONE (-1)

// one problem; a is read as lines x posts through (sl, sp): a[i][j] = cost[i * sl + j * sp].  max_raw (may be NULL): the
// largest cur + (sum of the deltas of the line so far) met, the value the library's lazy form keeps per post.
static void ar_solve(const int32_t* cost, int n, int m, long sl, long sp, int64_t* u, int64_t* v, int32_t* p, int64_t* steps,
                     int64_t* max_raw) {
    int64_t minv[AR_MAX_DIM];
    int32_t way[AR_MAX_DIM];
    unsigned char used[AR_MAX_DIM];
    for (int i = 0; i < n; ++i) u[i] = 0;
    for (int j = 0; j < m; ++j) { v[j] = 0; p[j] = AR_NONE; }
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < m; ++j) { minv[j] = INT64_MAX; way[j] = AR_NONE; used[j] = 0; }
        int i0 = i, j0 = AR_NONE;
        int64_t dsum = 0;
        for (;;) {
            ++*steps;
            const int32_t* row = cost + (long)i0 * sl;
            const int64_t u0 = u[i0];
            int j1 = AR_NONE;
            int64_t delta = INT64_MAX;
            for (int j = 0; j < m; ++j) {
                if (used[j]) continue;
                const int32_t c = row[(long)j * sp];
                const int64_t cur = (c == AR_INF ? AR_BIG : (int64_t)c) - u0 - v[j];
                if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
                if (max_raw && cur + dsum > *max_raw) *max_raw = cur + dsum;
                if (minv[j] < delta) { delta = minv[j]; j1 = j; }   // strict: the lowest j among equals
            }
            u[i] += delta;
            for (int j = 0; j < m; ++j) {
                if (used[j]) { u[p[j]] += delta; v[j] -= delta; }
                else minv[j] -= delta;
            }
            dsum += delta;
            used[j1] = 1;
            j0 = j1;
            if (p[j0] == AR_NONE) break;
            i0 = p[j0];
        }
        do {
            const int j1 = way[j0];
            p[j0] = j1 == AR_NONE ? i : p[j1];
            j0 = j1;
        } while (j0 != AR_NONE);
    }
}

void assign_ref(const int32_t* cost, int B, int R, int C, int32_t* col_of, int32_t* row_of, int64_t* u, int64_t* v, int64_t* info,
                int64_t* max_raw) {
    const int swap = R > C, n = swap ? C : R, m = swap ? R : C;
    int32_t p[AR_MAX_DIM];
    for (int b = 0; b < B; ++b) {
        const int32_t* a = cost + (size_t)b * R * C;
        int32_t *co = col_of + (size_t)b * R, *ro = row_of + (size_t)b * C;
        int64_t *ub = u + (size_t)b * R, *vb = v + (size_t)b * C, *ib = info + (size_t)b * 4;
        int bad = 0;
        for (long k = 0; k < (long)R * C; ++k) bad |= a[k] < 0;
        for (int r = 0; r < R; ++r) { co[r] = -1; ub[r] = 0; }
        for (int c = 0; c < C; ++c) { ro[c] = -1; vb[c] = 0; }
        ib[0] = ib[1] = ib[2] = 0;
        ib[3] = bad;
        if (bad) continue;
        // lines get their duals in ul, posts in vp: rows / columns, or columns / rows when swapped
        int64_t *ul = swap ? vb : ub, *vp = swap ? ub : vb;
        int32_t *line_pair = swap ? ro : co, *post_pair = swap ? co : ro;
        const long sl = swap ? 1 : C, sp = swap ? C : 1;
        ar_solve(a, n, m, sl, sp, ul, vp, p, &ib[2], max_raw);
        for (int j = 0; j < m; ++j) {
            if (p[j] == AR_NONE) continue;
            const int32_t c = a[(long)p[j] * sl + (long)j * sp];
            if (c == AR_INF) continue;
            post_pair[j] = p[j];
            line_pair[p[j]] = j;
            ++ib[0];
            ib[1] += c;
        }
    }
}

void field_cost_matrix_ref(const int32_t* g, int F, int W, int H, const int32_t* cell, int R, const int32_t* col_cost, int32_t* cost) {
    const long cells = (long)W * H;
    for (int r = 0; r < R; ++r)
        for (int f = 0; f < F; ++f) {
            int32_t out = AR_INF;
            if (cell[r] >= 0 && cell[r] < cells) {
                const int32_t gv = g[(size_t)f * cells + cell[r]];
                if (gv != AR_INF) {
                    const int64_t s = (int64_t)gv + (col_cost ? col_cost[f] : 0);
                    out = s > AR_INF - 1 ? AR_INF - 1 : (int32_t)s;
                }
            }
            cost[(size_t)r * F + f] = out;
        }
}
