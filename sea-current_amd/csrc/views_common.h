// views_common.h -- the ray walker of line-of-sight sensing, shared by views.hip (discs: DESIGN.md section 23) and sectors.hip
// (sectors and gain per heading: section 27): the supercover walk of a ray over occ bytes, a view's clipped box, a thread's
// target in a 16 x 16 tile of it, and the host helpers that size a launch.  The text is views.hip's, moved, not changed.
#pragma once
#include "sc_internal.h"

namespace {

constexpr int VW_TILE = 16;       // tile edge of a workgroup; a wavefront takes an 8 x 8 quarter
constexpr int VW_COLS = 4;        // columns whose loads are in flight together
constexpr int VW_SLOTS = 2048;    // workgroups per view at most (tiles are strided over them)

// The supercover of the segment from a (cell index ca, always free) to a target, column by column of the major axis.
// Column i, doubled coordinates relative to a: t in [max(2i-1, 0), min(2i+1, 2D)], rows
//   rhi(i) = min(floor(((2i+1) m + D) / 2D), m),   rlo(i) = ceil(((2i-1) m - D) / 2D) for i >= 1, 0 for i = 0.
// With n(i) = (2i+1) m + D = q(i) * 2D + rem(i):  rhi(i) = min(q(i), m), and (2i-1) m - D = n(i-1) - 2D gives
// rlo(i) = q(i-1) - (rem(i-1) == 0).  n(i+1) = n(i) + 2m with 2m <= 2D: q grows by at most one per column.  rhi - rlo <= 2.
struct vw_ray {
    int ca, D, m, twoD, sM, sm;
    int i, q, rem, rlo;   // column i: q, rem of n(i); rlo of column i
    __device__ void init(int W, int ax, int ay, int bx, int by) {
        const int dx = bx - ax, dy = by - ay;
        const bool xmajor = abs(dx) >= abs(dy);
        D = xmajor ? abs(dx) : abs(dy);
        m = xmajor ? abs(dy) : abs(dx);
        const int smaj = (xmajor ? dx : dy) < 0 ? -1 : 1, smin = (xmajor ? dy : dx) < 0 ? -1 : 1;
        sM = xmajor ? smaj : smaj * W;
        sm = xmajor ? smin * W : smin;
        twoD = 2 * D;
        ca = ay * W + ax;
        i = 0;
        // n(0) = m + D < 2D unless m == D (then q = 1, rem = 0); D == 0: one column, row 0
        q = (D > 0 && m == D) ? 1 : 0;
        rem = (D > 0 && m == D) ? 0 : m + D;
        rlo = 0;
    }
    __device__ bool finished() const { return i > D; }
    // VW_COLS columns, every load issued before any test.  Columns past D and unused rows repeat the centre cell, which is
    // free.  Every cell lies in the bounding box of the two endpoints, hence in the grid; the index guard only keeps a broken
    // invariant from reading outside occ.
    __device__ bool step(const uint8_t* __restrict__ occ, int cells) {
        uint32_t v[VW_COLS][3];
#pragma unroll
        for (int c = 0; c < VW_COLS; ++c) {
            const bool live = i <= D;
            const int rhi = min(q, m);
            const int base = ca + i * sM;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int idx = (live && rlo + r <= rhi) ? base + (rlo + r) * sm : ca;
                v[c][r] = (unsigned)idx < (unsigned)cells ? occ[idx] : 1u;
            }
            // to column i + 1
            rlo = q - (rem == 0 ? 1 : 0);
            rem += 2 * m;
            if (rem >= twoD && twoD > 0) { rem -= twoD; ++q; }
            ++i;
        }
        unsigned any = 0;
#pragma unroll
        for (int c = 0; c < VW_COLS; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) any |= v[c][r];
        return any == 0;
    }
};

struct vw_box {
    int cx, cy, x0, y0, tx, ntiles;   // ntiles == 0: the view sees nothing
    long long r2;
};

// floor(sqrt(v)) for 0 <= v < 2^31, exact: the float estimate is corrected in integers
__device__ __forceinline__ int vw_isqrt(long long v) {
    long long r = (long long)sqrtf((float)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return (int)r;
}

// the clipped box of view v; uniform across the workgroup
__device__ __forceinline__ vw_box vw_view_box(const uint8_t* __restrict__ occ, const int32_t* __restrict__ views, int v, int W, int H) {
    vw_box b;
    b.cx = views[3 * v];
    b.cy = views[3 * v + 1];
    b.r2 = views[3 * v + 2];
    b.x0 = b.y0 = b.tx = b.ntiles = 0;
    if (b.r2 < 0 || b.cx < 0 || b.cy < 0 || b.cx >= W || b.cy >= H) return b;   // ignored
    if (occ[b.cy * W + b.cx] != 0) return b;                                      // stands on an occupied cell
    const int r = vw_isqrt(b.r2);                                                 // <= 46340
    b.x0 = max(b.cx - r, 0);
    b.y0 = max(b.cy - r, 0);
    const int x1 = (int)min((long long)b.cx + r, (long long)W - 1), y1 = (int)min((long long)b.cy + r, (long long)H - 1);
    b.tx = (x1 - b.x0) / VW_TILE + 1;
    b.ntiles = b.tx * ((y1 - b.y0) / VW_TILE + 1);
    return b;
}

// this thread's target in tile t of the box: wave w of the workgroup is the 8 x 8 quarter (w & 1, w >> 1); -1 when the
// target lies outside the grid or the disc
__device__ __forceinline__ int vw_target(const vw_box& b, int t, int W, int H, int& x, int& y) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    x = b.x0 + (t % b.tx) * VW_TILE + (wv & 1) * 8 + (lane & 7);
    y = b.y0 + (t / b.tx) * VW_TILE + (wv >> 1) * 8 + (lane >> 3);
    if (x >= W || y >= H) return -1;
    const long long dx = x - b.cx, dy = y - b.cy;
    return dx * dx + dy * dy <= b.r2 ? y * W + x : -1;
}

__device__ __forceinline__ bool vw_clear(const uint8_t* __restrict__ occ, int W, int cells, const vw_box& b, int x, int y) {
    vw_ray ray;
    ray.init(W, b.cx, b.cy, x, y);
    bool ok = true;
    while (ok && !ray.finished()) ok = ray.step(occ, cells);
    return ok;
}

}  // namespace

static bool vw_dims_ok(int W, int H) { return W >= 1 && W <= SC_MAX_DIM && H >= 1 && H <= SC_MAX_DIM; }

// tile slots of a launch: the tiles of a box that covers the grid, VW_SLOTS at most
static unsigned vw_slots(int W, int H, int cap) {
    const long long t = (long long)((W + VW_TILE - 1) / VW_TILE) * ((H + VW_TILE - 1) / VW_TILE);
    return (unsigned)(t < cap ? t : cap);
}

// vw_combine_kernel (views.hip) on the context's stream: known = base | vis | surf, occ_seen = known ? occ : 0
int sc_launch_view_combine(sc_ctx* ctx, const uint8_t* base, const uint8_t* occ, const uint8_t* vis, int W, int H, uint8_t* known,
                           uint8_t* occ_seen);
