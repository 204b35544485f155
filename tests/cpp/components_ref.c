/* CPU twin of sc_components_batch and sc_reachable_batch (include/sea_current_hip.h): plain C, one breadth-first search per
 * component.  T(c) <=> d2[c] >= max(r2_clear, 1); components are 4-connected; label[c] = the smallest linear index of c's
 * component, -1 where c is not traversable.  Cells are scanned in index order, so the cell a search starts from is its
 * component's minimum. */
#include <stdint.h>
#include <stdlib.h>

/* One grid.  size (may be NULL): the cell count at every representative, 0 elsewhere.  *ncomp, *largest (may be NULL): the
 * number of components and the representative of the largest one, ties to the smaller index, -1 when there is none.
 * Returns 0, or -1 when the queue cannot be allocated. */
int cr_components(const int32_t* d2, int W, int H, int32_t r2_clear, int32_t* label, int32_t* size, int32_t* ncomp, int32_t* largest) {
    const int32_t thr = r2_clear > 1 ? r2_clear : 1;
    const size_t n = (size_t)W * (size_t)H;
    int32_t* queue = (int32_t*)malloc((n ? n : 1) * sizeof(int32_t));
    if (!queue) return -1;
    for (size_t i = 0; i < n; ++i) {
        label[i] = -1;
        if (size) size[i] = 0;
    }
    int32_t count = 0, best = -1, best_size = 0;
    for (size_t r = 0; r < n; ++r) {
        if (d2[r] < thr || label[r] >= 0) continue;
        size_t head = 0, tail = 0;
        label[r] = (int32_t)r;
        queue[tail++] = (int32_t)r;
        while (head < tail) {
            const int32_t c = queue[head++];
            const int x = c % W, y = c / W;
            const int32_t nb[4] = {x + 1 < W ? c + 1 : -1, x > 0 ? c - 1 : -1, y + 1 < H ? c + W : -1, y > 0 ? c - W : -1};
            for (int k = 0; k < 4; ++k) {
                const int32_t u = nb[k];
                if (u < 0 || d2[u] < thr || label[u] >= 0) continue;
                label[u] = (int32_t)r;
                queue[tail++] = u;
            }
        }
        ++count;
        if (size) size[r] = (int32_t)tail;
        if ((int32_t)tail > best_size) {   /* strictly larger: a tie keeps the smaller index */
            best_size = (int32_t)tail;
            best = (int32_t)r;
        }
    }
    if (ncomp) *ncomp = count;
    if (largest) *largest = best;
    free(queue);
    return 0;
}

/* status[q]: 2 (SC_Q_BAD_ENDPOINT) for an endpoint or a grid out of range or a negative label, 1 (SC_Q_NO_PATH) for labels that
 * differ, else 0 (SC_Q_OK).  label is [G][H][W]; qgrid may be NULL when G == 1. */
void cr_reachable(const int32_t* label, int G, const int32_t* qgrid, int W, int H, const int32_t* start, const int32_t* goal, int Q,
                  int32_t* status) {
    const int64_t n = (int64_t)W * H;
    for (int q = 0; q < Q; ++q) {
        const int gi = qgrid ? qgrid[q] : 0;
        const int32_t s = start[q], t = goal[q];
        if (gi < 0 || gi >= G || s < 0 || t < 0 || s >= n || t >= n) {
            status[q] = 2;
            continue;
        }
        const int32_t ls = label[(size_t)gi * (size_t)n + (size_t)s], lt = label[(size_t)gi * (size_t)n + (size_t)t];
        status[q] = (ls < 0 || lt < 0) ? 2 : (ls == lt ? 0 : 1);
    }
}
