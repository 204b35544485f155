// scan_ref.c -- the C statement of the range-scan calls (sc_scan_cast_batch, sc_logodds_update), single-threaded, straight from
// the definition in include/sea_current_hip.h: every ray walked from scratch with one division per column, 64-bit throughout.
// Test infrastructure: tests/scan_twin.py builds it, tests/cpp/scan_ref_check.c runs it under the sanitizers.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define SX_NO_RETURN (-1)
#define SX_IGNORED (-2)
#define SX_MAX_REACH 16384

// a ray that is not ignored: a inside the grid, |bx - ax| and |by - ay| <= SX_MAX_REACH
int sx_ray_ok(const int32_t* ray, int W, int H) {
    const int64_t ax = ray[0], ay = ray[1], dx = (int64_t)ray[2] - ax, dy = (int64_t)ray[3] - ay;
    return ax >= 0 && ay >= 0 && ax < W && ay < H && llabs(dx) <= SX_MAX_REACH && llabs(dy) <= SX_MAX_REACH;
}

// visit returns 0 to end the walk
typedef int (*sx_visit)(void* user, int32_t cell);

// Walk(a, b) of a ray that is not ignored, in sequence order: column i (0 .. D) of the major axis, doubled coordinates relative
// to a: the segment spans t in [max(2i-1, 0), min(2i+1, 2D)] and rises t * m / (2D) on the minor axis; it meets rows
// ceil((tlo m - D) / 2D) .. floor((thi m + D) / 2D), counted away from a.  The walk ends before its first cell outside the grid.
static void sx_each(const int32_t* ray, int W, int H, sx_visit visit, void* user) {
    const int64_t ax = ray[0], ay = ray[1], dx = (int64_t)ray[2] - ax, dy = (int64_t)ray[3] - ay;
    const int xmajor = llabs(dx) >= llabs(dy);
    const int64_t D = xmajor ? llabs(dx) : llabs(dy), m = xmajor ? llabs(dy) : llabs(dx);
    const int smaj = (xmajor ? dx : dy) < 0 ? -1 : 1, smin = (xmajor ? dy : dx) < 0 ? -1 : 1;
    for (int64_t i = 0; i <= D; ++i) {
        int64_t rlo = 0, rhi = 0;
        if (D > 0) {
            const int64_t tlo = 2 * i - 1 > 0 ? 2 * i - 1 : 0, thi = 2 * i + 1 < 2 * D ? 2 * i + 1 : 2 * D;
            const int64_t nlo = tlo * m - D, nhi = thi * m + D;
            rlo = nlo <= 0 ? 0 : (nlo + 2 * D - 1) / (2 * D);
            rhi = nhi / (2 * D);
        }
        for (int64_t r = rlo; r <= rhi; ++r) {
            const int64_t x = xmajor ? ax + smaj * i : ax + smin * r, y = xmajor ? ay + smin * r : ay + smaj * i;
            if (x < 0 || y < 0 || x >= W || y >= H) return;
            if (!visit(user, (int32_t)(y * W + x))) return;
        }
    }
}

struct sx_list {
    int32_t* cells;
    int cap, n;
};

static int sx_collect(void* user, int32_t cell) {
    struct sx_list* l = (struct sx_list*)user;
    if (l->n < l->cap) l->cells[l->n] = cell;
    ++l->n;
    return 1;
}

// the cells of Walk(a, b) in sequence order into cells[0 .. cap); returns their number (which may exceed cap), -1 for an
// ignored ray
int sx_walk(const int32_t* ray, int W, int H, int32_t* cells, int cap) {
    if (!sx_ray_ok(ray, W, H)) return -1;
    struct sx_list l = {cells, cap, 0};
    sx_each(ray, W, H, sx_collect, &l);
    return l.n;
}

struct sx_first {
    const uint8_t* occ;
    int32_t hit;
};

static int sx_first_occupied(void* user, int32_t cell) {
    struct sx_first* f = (struct sx_first*)user;
    if (f->occ[cell] == 0) return 1;
    f->hit = cell;
    return 0;
}

void sx_cast(const uint8_t* occ, const int32_t* rays, int N, int W, int H, int32_t* hit) {
    for (int k = 0; k < N; ++k) {
        const int32_t* ray = rays + 4 * (size_t)k;
        if (!sx_ray_ok(ray, W, H) || occ[(size_t)ray[1] * W + ray[0]] != 0) { hit[k] = SX_IGNORED; continue; }
        struct sx_first f = {occ, SX_NO_RETURN};
        sx_each(ray, W, H, sx_first_occupied, &f);
        hit[k] = f.hit;
    }
}

struct sx_miss {
    uint8_t* miss;
    int32_t hit;
};

static int sx_mark_miss(void* user, int32_t cell) {
    struct sx_miss* s = (struct sx_miss*)user;
    if (cell == s->hit) return 0;
    s->miss[cell] = 1;
    return 1;
}

static int sx_count(void* user, int32_t cell) {
    int64_t* s = (int64_t*)user;
    if (cell == (int32_t)s[1]) return 0;
    ++s[0];
    return 1;
}

// the cells the beams of an update miss, counted beam by beam (a cell crossed by two beams counts twice): the byte stores
// the mark kernel of the library issues (tools/scan_time.py)
int64_t sx_miss_steps(const int32_t* rays, const int32_t* hit, int N, int W, int H) {
    int64_t s[2] = {0, 0};
    for (int k = 0; k < N; ++k) {
        const int32_t* ray = rays + 4 * (size_t)k;
        if (!sx_ray_ok(ray, W, H) || hit[k] < SX_NO_RETURN || (int64_t)hit[k] >= (int64_t)W * H) continue;
        s[1] = hit[k];
        sx_each(ray, W, H, sx_count, s);
    }
    return s[0];
}

// Lout = clamp(L + (hit ? l_hit : missed ? -l_miss : 0)); occ_est, known may be NULL; L may be NULL or Lout.  A beam with a hit
// below -1 or >= W * H is ignored (the device form's rule).  0, or 1 when the flag maps cannot be allocated.
int sx_update(const int32_t* L, const int32_t* rays, const int32_t* hit, int N, int W, int H, int32_t l_hit, int32_t l_miss,
              int32_t l_clamp, int32_t t_occ, int32_t t_free, int32_t* Lout, uint8_t* occ_est, uint8_t* known) {
    const size_t n = (size_t)W * H;
    uint8_t* miss = (uint8_t*)calloc(n, 1);
    uint8_t* hitmap = (uint8_t*)calloc(n, 1);
    if (!miss || !hitmap) { free(miss); free(hitmap); return 1; }
    for (int k = 0; k < N; ++k) {
        const int32_t* ray = rays + 4 * (size_t)k;
        if (!sx_ray_ok(ray, W, H) || hit[k] < SX_NO_RETURN || (int64_t)hit[k] >= (int64_t)n) continue;
        if (hit[k] >= 0) hitmap[hit[k]] = 1;
        struct sx_miss s = {miss, hit[k]};
        sx_each(ray, W, H, sx_mark_miss, &s);
    }
    for (size_t c = 0; c < n; ++c) {
        int64_t l = L ? L[c] : 0;
        l += hitmap[c] ? (int64_t)l_hit : miss[c] ? -(int64_t)l_miss : 0;
        if (l > l_clamp) l = l_clamp;
        if (l < -(int64_t)l_clamp) l = -(int64_t)l_clamp;
        Lout[c] = (int32_t)l;
        if (occ_est) occ_est[c] = l >= t_occ;
        if (known) known[c] = l >= t_occ || l <= -(int64_t)t_free;
    }
    free(miss); free(hitmap);
    return 0;
}
