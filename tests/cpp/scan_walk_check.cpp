/* The walker the kernels of scan.hip run (sea-current_amd/csrc/ray_walk.h: rw_ray_ok, rw_walk, rw_each), compiled for the host
 * and compared with the C statement (scan_ref.c: one division per column, 64-bit) ray by ray, in cells and in order:
 *   c++ -g -O1 -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -I../../sea-current_amd/csrc \
 *       -o scan_walk_check scan_walk_check.cpp scan_ref.o
 * Random rays on random grids (ends inside, outside beyond every side and corner, far outside, at the reach limit and past it,
 * origins outside), then the longest rays the contract allows on the largest grid.  Prints the number of rays compared and
 * "scan_walk OK"; exit code 1 on the first difference. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ray_walk.h"

extern "C" int sx_walk(const int32_t* ray, int W, int H, int32_t* cells, int cap);

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 20;
}
static int uni(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }

static std::vector<int32_t> ref_cells(3 * (2 * SC_SCAN_MAX_REACH + 2));
static long n_rays = 0, n_cells = 0, n_ignored = 0, n_clipped = 0;

static int compare(int W, int H, int ax, int ay, int bx, int by) {
    const int32_t ray[4] = {ax, ay, bx, by};
    const int n = sx_walk(ray, W, H, ref_cells.data(), (int)ref_cells.size());
    const bool ok = rw_ray_ok(ax, ay, bx, by, W, H);
    ++n_rays;
    if (ok != (n >= 0)) { printf("FAIL ignored: %d x %d ray %d %d %d %d\n", W, H, ax, ay, bx, by); return 1; }
    if (!ok) { ++n_ignored; return 0; }
    int k = 0;
    bool same = true;
    rw_each(ax, ay, bx, by, W, H, [&](int c) {
        same = same && k < n && ref_cells[k] == c;
        ++k;
        return true;
    });
    if (!same || k != n) { printf("FAIL walk: %d x %d ray %d %d %d %d (%d cells, the statement has %d)\n", W, H, ax, ay, bx, by, k, n); return 1; }
    n_cells += n;
    n_clipped += bx < 0 || by < 0 || bx >= W || by >= H;
    return 0;
}

int main() {
    for (int it = 0; it < 120000; ++it) {
        const int W = uni(1, it % 3 ? 48 : 300), H = uni(1, it % 5 ? 48 : 300);
        const int ax = uni(it % 50 ? 0 : -2, it % 50 ? W - 1 : W + 1), ay = uni(it % 50 ? 0 : -2, it % 50 ? H - 1 : H + 1);
        int bx, by;
        switch (it % 4) {
            case 0: bx = uni(0, W - 1); by = uni(0, H - 1); break;                      /* inside */
            case 1: bx = uni(-W - 3, 2 * W + 3); by = uni(-H - 3, 2 * H + 3); break;    /* beyond any side or corner */
            case 2: bx = ax + uni(-3, 3) * uni(0, 40); by = ay + uni(-3, 3) * uni(0, 40); break;   /* axes, diagonals, slopes 1/2, 1/3 */
            default: bx = ax + uni(-SC_SCAN_MAX_REACH - 1, SC_SCAN_MAX_REACH + 1); by = ay + uni(-400, 400); break;
        }
        if (compare(W, H, ax, ay, bx, by)) return 1;
    }
    /* the reach limit on the largest grid: the products of the walk at their largest */
    const int M = SC_MAX_DIM, R = SC_SCAN_MAX_REACH;
    const int far[][4] = {{0, 0, R, R}, {0, 0, R, R - 1}, {0, 0, R - 1, R}, {M - 1, M - 1, M - 1 - R, M - 1 - R + 1}, {0, M - 1, R, M - 1 - R},
                          {M - 1, 0, M - 1 - R, R - 1}, {100, 200, 100 + R, 200 + 1}, {100, 200, 100 + 1, 200 + R}, {0, 0, R + 1, 0},
                          {0, 0, 0, -R - 1}, {0, 0, INT32_MAX, INT32_MAX}, {M - 1, M - 1, INT32_MIN, INT32_MIN}, {5, 5, INT32_MIN, 5}};
    for (const auto& f : far)
        if (compare(M, M, f[0], f[1], f[2], f[3])) return 1;
    printf("%ld rays (%ld ignored, %ld with the end outside the grid), %ld cells\nscan_walk OK\n", n_rays, n_ignored, n_clipped, n_cells);
    return 0;
}
