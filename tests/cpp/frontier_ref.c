/* Single-threaded C statement of the exploration frontiers (include/sea_current_hip.h, "exploration frontiers"): the known
 * mask of a disc list, d2 restricted to it, the frontier cells with their 8-connected clusters (one flood fill per cluster,
 * started in index order, so a cluster's first cell is its representative and the clusters come out in listing order), and
 * the robots x clusters cost matrix by a plain loop.  Checker and timing reference only: the library never sees it.
 *   cc -O2 -std=c11 -fPIC -shared -o libfrontier_ref.so frontier_ref.c */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define FX_INF INT32_MAX

void fx_known_from_discs(const uint8_t* base, const int32_t* discs, int R, int W, int H, uint8_t* known) {
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t c = (size_t)y * W + x;
            int k = base && base[c] != 0;
            for (int r = 0; r < R && !k; ++r) {
                const int64_t dx = (int64_t)x - discs[3 * r], dy = (int64_t)y - discs[3 * r + 1], r2 = discs[3 * r + 2];
                k = r2 >= 0 && dx * dx + dy * dy <= r2;
            }
            known[c] = (uint8_t)k;
        }
}

void fx_d2_known(const int32_t* d2, const uint8_t* known, int64_t cells, int32_t* d2k) {
    for (int64_t c = 0; c < cells; ++c) d2k[c] = known[c] ? d2[c] : 0;
}

static int fx_is_frontier(const int32_t* d2, const uint8_t* known, int W, int H, int32_t thr, int x, int y) {
    const size_t c = (size_t)y * W + x;
    if (!known[c] || d2[c] < thr) return 0;
    return (x > 0 && !known[c - 1]) || (x + 1 < W && !known[c + 1]) || (y > 0 && !known[c - W]) || (y + 1 < H && !known[c + W]);
}

/* One grid.  label, slot, cbox and csum may be NULL.  Returns 0, or 1 when memory ran out. */
int fx_frontier(const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size, int Cmax, int32_t* label,
                int32_t* slot, int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox, int64_t* csum) {
    const int32_t thr = r2_clear > 1 ? r2_clear : 1;
    const size_t n = (size_t)W * H;
    int32_t* lab = (int32_t*)malloc(n * sizeof(int32_t));
    int32_t* stack = (int32_t*)malloc(n * sizeof(int32_t));
    int32_t* col = (int32_t*)malloc(n * sizeof(int32_t));   /* the column of the cluster whose representative the cell is */
    if (!lab || !stack || !col) { free(lab); free(stack); free(col); return 1; }
    for (size_t c = 0; c < n; ++c) lab[c] = -2;              /* -2: not looked at yet */
    for (int k = 0; k < Cmax; ++k) {
        rep[k] = -1;
        csize[k] = 0;
        if (cbox) memset(cbox + 4 * k, 0, 4 * sizeof(int32_t));
        if (csum) csum[2 * k] = csum[2 * k + 1] = 0;
    }
    int32_t listed = 0, all = 0;
    for (int y0 = 0; y0 < H; ++y0)
        for (int x0 = 0; x0 < W; ++x0) {
            const int32_t r = y0 * W + x0;
            if (lab[r] != -2) continue;
            if (!fx_is_frontier(d2, known, W, H, thr, x0, y0)) { lab[r] = -1; continue; }
            /* a new cluster: r is its smallest cell, everything before it in index order is labelled */
            int32_t top = 0, size = 0, bx0 = x0, by0 = y0, bx1 = x0, by1 = y0;
            int64_t sx = 0, sy = 0;
            stack[top++] = r;
            lab[r] = r;
            while (top) {
                const int32_t c = stack[--top];
                const int x = c % W, y = c / W;
                ++size; sx += x; sy += y;
                if (x < bx0) bx0 = x;
                if (x > bx1) bx1 = x;
                if (y < by0) by0 = y;
                if (y > by1) by1 = y;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int xx = x + dx, yy = y + dy;
                        if ((!dx && !dy) || xx < 0 || yy < 0 || xx >= W || yy >= H) continue;
                        const int32_t q = yy * W + xx;
                        if (lab[q] != -2) continue;
                        if (fx_is_frontier(d2, known, W, H, thr, xx, yy)) { lab[q] = r; stack[top++] = q; }
                        else lab[q] = -1;
                    }
            }
            ++all;
            col[r] = -1;
            if (size >= min_size) {
                if (listed < Cmax) {
                    const int32_t k = listed;
                    col[r] = k;
                    rep[k] = r;
                    csize[k] = size;
                    if (cbox) { cbox[4 * k] = bx0; cbox[4 * k + 1] = by0; cbox[4 * k + 2] = bx1; cbox[4 * k + 3] = by1; }
                    if (csum) { csum[2 * k] = sx; csum[2 * k + 1] = sy; }
                }
                ++listed;
            }
        }
    ncl[0] = listed;
    ncl[1] = all;
    for (size_t c = 0; c < n; ++c) {
        if (label) label[c] = lab[c];
        if (slot) slot[c] = lab[c] >= 0 ? col[lab[c]] : -1;
    }
    free(lab); free(stack); free(col);
    return 0;
}

/* cost, cell [F][Cmax]; slot [G][H][W], csize [G][Cmax]; fgrid NULL: every field on grid 0 */
void fx_cost_matrix(const int32_t* g, int F, const int32_t* fgrid, const int32_t* slot, const int32_t* csize, int G, int W, int H, int Cmax,
                    int32_t gain, int32_t size_cap, int32_t* cost, int32_t* cell) {
    const size_t n = (size_t)W * H;
    for (int f = 0; f < F; ++f) {
        int32_t* co = cost + (size_t)f * Cmax;
        int32_t* ce = cell + (size_t)f * Cmax;
        for (int k = 0; k < Cmax; ++k) { co[k] = FX_INF; ce[k] = -1; }
        const int gi = fgrid ? fgrid[f] : 0;
        if (gi < 0 || gi >= G) continue;
        for (size_t c = 0; c < n; ++c) {            /* ascending c: the first cell to attain the minimum stays */
            const int32_t k = slot[(size_t)gi * n + c], v = g[(size_t)f * n + c];
            if (k < 0 || k >= Cmax || v < 0 || v == FX_INF) continue;
            if (v < co[k]) { co[k] = v; ce[k] = (int32_t)c; }
        }
        for (int k = 0; k < Cmax; ++k) {
            if (ce[k] < 0) continue;
            const int64_t s = csize[(size_t)gi * Cmax + k];
            const int64_t v = (int64_t)co[k] + (int64_t)gain * ((int64_t)size_cap - (s < size_cap ? s : size_cap));
            co[k] = (int32_t)(v < (int64_t)INT32_MAX - 1 ? v : (int64_t)INT32_MAX - 1);
        }
    }
}
