// explore_gain_ref.c -- the C statement of coordinated exploration goals by gain (sc_explore_gain_batch, sc_frontier_centres),
// straight from the definitions in include/sea_current_hip.h, on top of views_ref.c and sectors_ref.c: every round recomputes
// every gain with their gain functions and applies the pick with their known-space functions.  Nothing is updated by
// differences here: the library's delta pass has to equal this.  Link with views_ref.c and sectors_ref.c.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define EX_INF INT32_MAX
#define EX_MAX_R 1024
#define EX_MAX_N 65536

int vx_known_from_views(const uint8_t* base, const uint8_t* occ, const int32_t* views, int R, int W, int H, uint8_t* known, uint8_t* occ_seen);
void vx_view_gain(const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H, int32_t* gain);
int sx_dirs_valid(const int32_t* dirs, int B);
int sx_known_from_sectors(const uint8_t* base, const uint8_t* occ, const int32_t* sviews, int R, int W, int H, uint8_t* known,
                          uint8_t* occ_seen);
int sx_view_gain_headings(const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H, const int32_t* dirs, int B,
                          int span, int32_t* hist, int32_t* gainh, int32_t* best);
void sx_views_from_cells(const int32_t* cell, int N, int W, int H, int32_t r2, int32_t* views);

// gain[n], heading[n] of every candidate against kw; 0, or the status of the headings statement
static int ex_gains(const uint8_t* occ, const uint8_t* kw, const int32_t* views, int N, int W, int H, const int32_t* dirs, int B, int span,
                    int32_t* best, int32_t* gain, int32_t* heading) {
    if (!dirs) {
        vx_view_gain(occ, kw, views, N, W, H, gain);
        for (int n = 0; n < N; ++n) heading[n] = -1;
        return 0;
    }
    const int st = sx_view_gain_headings(occ, kw, views, N, W, H, dirs, B, span, NULL, NULL, best);
    for (int n = 0; st == 0 && n < N; ++n) {
        gain[n] = best[2 * (size_t)n];
        heading[n] = best[2 * (size_t)n + 1];
    }
    return st;
}

// Every output may be NULL except goal, gcost and npick; known_out may be known.  0; 1 for arguments the definition refuses
// (a g value below 0 included); 2 without memory.
int ex_explore_gain(const uint8_t* occ, const uint8_t* known, const int32_t* g, int R, const int32_t* cand, int N, int W, int H, int32_t r2,
                    const int32_t* dirs, int B, int span, int32_t wg, int32_t wc, int32_t min_gain, int rounds, int32_t* goal, int32_t* gcost,
                    int32_t* ggain, int32_t* head, int32_t* cand_of, int32_t* pick, int32_t* npick, int32_t* gain0, int32_t* gain_end,
                    uint8_t* known_out) {
    if (!occ || !known || !g || !goal || !gcost || !npick || (!cand && N > 0) || known_out == occ) return 1;
    if (W < 1 || W > 8192 || H < 1 || H > 8192 || R < 1 || R > EX_MAX_R || N < 0 || N > EX_MAX_N || (int64_t)R * N > ((int64_t)1 << 26)) return 1;
    if (r2 < 0 || wg < 0 || wg > (1 << 20) || wc < 0 || wc > (1 << 20) || min_gain < 0 || rounds < 0 || rounds > EX_MAX_R) return 1;
    if (dirs && (!sx_dirs_valid(dirs, B) || span < 1 || span >= B)) return 1;
    const size_t cells = (size_t)W * H;
    for (size_t k = 0; k < (size_t)R * cells; ++k)
        if (g[k] < 0) return 1;
    for (int r = 0; r < R; ++r) {
        goal[r] = gcost[r] = -1;
        if (ggain) ggain[r] = 0;
        if (head) head[r] = -1;
        if (cand_of) cand_of[r] = -1;
        if (pick) pick[r] = -1;
    }
    npick[0] = 0;
    uint8_t* kw = known_out ? known_out : (uint8_t*)malloc(cells);
    int32_t* views = (int32_t*)malloc((size_t)(N ? N : 1) * 12);
    int32_t* best = (int32_t*)malloc((size_t)(N ? N : 1) * 8);
    int32_t* gain = (int32_t*)malloc((size_t)(N ? N : 1) * 4);
    int32_t* heading = (int32_t*)malloc((size_t)(N ? N : 1) * 4);
    uint8_t* taken = (uint8_t*)calloc((size_t)(N ? N : 1), 1);
    uint8_t* assigned = (uint8_t*)calloc((size_t)R, 1);
    int st = (kw && views && best && gain && heading && taken && assigned) ? 0 : 2;
    if (st == 0 && kw != known) memcpy(kw, known, cells);
    if (st == 0 && N > 0) {
        sx_views_from_cells(cand, N, W, H, r2, views);
        st = ex_gains(occ, kw, views, N, W, H, dirs, B, span, best, gain, heading) ? 2 : 0;
        if (st == 0 && gain0) memcpy(gain0, gain, (size_t)N * 4);
        int T = rounds < R ? rounds : R;
        if (N < T) T = N;
        for (int t = 0; st == 0 && t < T; ++t) {
            int br = -1, bn = -1;
            int64_t bs = 0;
            for (int r = 0; r < R; ++r) {
                if (assigned[r]) continue;
                for (int n = 0; n < N; ++n) {
                    const int64_t c = cand[n];
                    if (taken[n] || c < 0 || c >= (int64_t)cells || occ[c] != 0) continue;   // taken or dead
                    const int32_t cost = g[(size_t)r * cells + c];
                    if (cost == EX_INF || gain[n] < min_gain) continue;
                    const int64_t s = (int64_t)wg * gain[n] - (int64_t)wc * cost;
                    if (br < 0 || s > bs) { br = r; bn = n; bs = s; }   // ascending r, then n: the first of equals stays
                }
            }
            if (br < 0) break;
            goal[br] = cand[bn];
            gcost[br] = g[(size_t)br * cells + cand[bn]];
            if (ggain) ggain[br] = gain[bn];
            if (head) head[br] = heading[bn];
            if (cand_of) cand_of[br] = bn;
            if (pick) pick[br] = t;
            assigned[br] = 1;
            taken[bn] = 1;
            npick[0] = t + 1;
            if (!dirs) {
                st = vx_known_from_views(kw, occ, views + 3 * (size_t)bn, 1, W, H, kw, NULL) ? 2 : 0;
            } else {
                const int h = heading[bn], h1 = (h + span) % B;
                const int32_t row[7] = {views[3 * (size_t)bn], views[3 * (size_t)bn + 1], views[3 * (size_t)bn + 2], dirs[2 * h], dirs[2 * h + 1],
                                        dirs[2 * h1], dirs[2 * h1 + 1]};
                st = sx_known_from_sectors(kw, occ, row, 1, W, H, kw, NULL) ? 2 : 0;
            }
            if (st == 0) st = ex_gains(occ, kw, views, N, W, H, dirs, B, span, best, gain, heading) ? 2 : 0;
        }
        if (st == 0 && gain_end) memcpy(gain_end, gain, (size_t)N * 4);
    }
    if (kw != known_out) free(kw);
    free(views); free(best); free(gain); free(heading); free(taken); free(assigned);
    return st;
}

// one grid: centre[k] = the cell with slot == k that minimises |csize x - sumx| + |csize y - sumy| (the first in index order
// among equals), -1 for a row without cells
void ex_frontier_centres(const int32_t* slot, const int32_t* csize, const int64_t* csum, int W, int H, int Cmax, int32_t* centre) {
    for (int k = 0; k < Cmax; ++k) {
        int64_t bk = -1;
        centre[k] = -1;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                if (slot[(size_t)y * W + x] != k) continue;
                const int64_t ex = (int64_t)csize[k] * x - csum[2 * k], ey = (int64_t)csize[k] * y - csum[2 * k + 1];
                const int64_t key = (ex < 0 ? -ex : ex) + (ey < 0 ? -ey : ey);
                if (bk < 0 || key < bk) { bk = key; centre[k] = (int32_t)(y * W + x); }
            }
    }
}
