// sectors_common.h -- the sector predicate of sensors with a field of view, shared by sectors.hip and
// explore_gain.hip (coordinated goals by gain: section 29): the case of In(.; a, b), the predicate, a sector row's box, the
// tile skip, the heading table as a kernel argument, the cone test of the bin search and the table's rules on the host.  The
// text is sectors.hip's, moved, not changed.
#pragma once
#include "views_common.h"

namespace {

enum { VS_IGNORED = -1, VS_FULL = 0, VS_CONVEX = 1, VS_REFLEX = 2, VS_HALF = 3 };

struct vs_sector {
    int ax, ay, bx, by, kind;
};

__host__ __device__ __forceinline__ bool vs_comp_ok(int v) { return v >= -32767 && v <= 32767; }

// the case of In(.; a, b) a pair of directions takes
__host__ __device__ __forceinline__ int vs_kind(int ax, int ay, int bx, int by) {
    if (ax == 0 && ay == 0 && bx == 0 && by == 0) return VS_FULL;
    if (!vs_comp_ok(ax) || !vs_comp_ok(ay) || !vs_comp_ok(bx) || !vs_comp_ok(by)) return VS_IGNORED;
    const int s = ax * by - ay * bx;
    if (s > 0) return VS_CONVEX;
    if (s < 0) return VS_REFLEX;
    return ax * bx + ay * by < 0 ? VS_HALF : VS_IGNORED;   // dot == 0 with s == 0: exactly one of a, b is zero
}

// In(d; a, b) for a sector that is not ignored
__device__ __forceinline__ bool vs_in(const vs_sector& s, int dx, int dy) {
    if ((dx == 0 && dy == 0) || s.kind == VS_FULL) return true;
    const int ad = s.ax * dy - s.ay * dx;   // cross(a, d)
    const int db = dx * s.by - dy * s.bx;   // cross(d, b)
    if (s.kind == VS_CONVEX) return ad >= 0 && db > 0;
    if (s.kind == VS_REFLEX) return !(-db >= 0 && -ad > 0);   // cross(b, d) = -cross(d, b), cross(d, a) = -cross(a, d)
    return ad > 0 || (ad == 0 && s.ax * dx + s.ay * dy > 0);
}

__device__ __forceinline__ vs_sector vs_load(const int32_t* __restrict__ sviews, int v) {
    vs_sector s;
    s.ax = sviews[7 * v + 3];
    s.ay = sviews[7 * v + 4];
    s.bx = sviews[7 * v + 5];
    s.by = sviews[7 * v + 6];
    s.kind = vs_kind(s.ax, s.ay, s.bx, s.by);
    return s;
}

// the clipped box of sector row v: vw_view_box of its (cx, cy, r2); an ignored sector sees nothing
__device__ __forceinline__ vw_box vs_view_box(const uint8_t* __restrict__ occ, const int32_t* __restrict__ sviews, int v, const vs_sector& s,
                                              int W, int H) {
    const int32_t row[3] = {sviews[7 * v], sviews[7 * v + 1], s.kind == VS_IGNORED ? -1 : sviews[7 * v + 2]};
    return vw_view_box(occ, row, 0, W, H);
}

// true when no cell of tile t of the box can lie in the sector; uniform across the workgroup
__device__ __forceinline__ bool vs_skip(const vw_box& b, const vs_sector& s, int t) {
    if (s.kind == VS_FULL) return false;
    const int x0 = b.x0 + (t % b.tx) * VW_TILE - b.cx, y0 = b.y0 + (t / b.tx) * VW_TILE - b.cy;   // corner offsets x0 .. x1, y0 .. y1
    const int x1 = x0 + VW_TILE - 1, y1 = y0 + VW_TILE - 1;
    if (x0 <= 0 && x1 >= 0 && y0 <= 0 && y1 >= 0) return false;   // the centre's tile
    int out_a = 0, out_b = 0;   // corners with cross(a, d) < 0; with cross(d, b) <= 0
    int in_cone = 0;            // corners inside the cone from b to a
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dx = (k & 1) ? x1 : x0, dy = (k & 2) ? y1 : y0;
        const int ad = s.ax * dy - s.ay * dx, db = dx * s.by - dy * s.bx;
        out_a += ad < 0;
        out_b += db <= 0;
        in_cone += (db <= 0 && ad < 0);
    }
    if (s.kind == VS_CONVEX) return out_a == 4 || out_b == 4;
    if (s.kind == VS_HALF) return out_a == 4;
    return in_cone == 4;
}

struct vs_dirs {
    int32_t u[SC_VIEW_MAX_BINS][2];
};

// In(d; a, b) for two entries of a valid table that are not the same entry, d != 0
__device__ __forceinline__ bool vs_in_cone(int2 a, int2 b, int dx, int dy) {
    const int s = a.x * b.y - a.y * b.x;
    const int ad = a.x * dy - a.y * dx, db = dx * b.y - dy * b.x;
    if (s > 0) return ad >= 0 && db > 0;
    if (s < 0) return !(db <= 0 && ad < 0);
    return ad > 0 || (ad == 0 && a.x * dx + a.y * dy > 0);
}

}  // namespace

// the heading table's rules (include/sea_current_hip.h): 3 .. SC_VIEW_MAX_BINS entries, components in -32767 .. 32767,
// every entry strictly counter-clockwise of its predecessor by less than half a turn, one turn in all
static bool vs_dirs_ok(const int32_t* dirs, int B) {
    if (!dirs || B < 3 || B > SC_VIEW_MAX_BINS) return false;
    for (int i = 0; i < 2 * B; ++i)
        if (dirs[i] < -32767 || dirs[i] > 32767) return false;
    int leaves = 0;   // entries in the upper half-open plane whose successor is not
    for (int b = 0; b < B; ++b) {
        const int64_t ux = dirs[2 * b], uy = dirs[2 * b + 1], vx = dirs[2 * ((b + 1) % B)], vy = dirs[2 * ((b + 1) % B) + 1];
        if (ux * vy - uy * vx <= 0) return false;
        const bool up = uy > 0 || (uy == 0 && ux > 0), vup = vy > 0 || (vy == 0 && vx > 0);
        leaves += up && !vup;
    }
    return leaves == 1;
}
