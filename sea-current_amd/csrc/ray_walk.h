// ray_walk.h -- the ordered, bounded supercover walk of the range-scan calls (scan.hip; Walk(a, b) in
// include/sea_current_hip.h).  Plain C++ that compiles for the device and for the host: the host build
// is what tests/cpp/scan_walk_check.cpp compares with the C statement (tests/cpp/scan_ref.c) ray by ray.
//
// Column i (0 .. D) of the major axis, doubled coordinates relative to a: t in [max(2i-1, 0), min(2i+1, 2D)], rows
//   rhi(i) = min(floor(((2i+1) m + D) / 2D), m),   rlo(i) = ceil(((2i-1) m - D) / 2D) for i >= 1, 0 for i = 0.
// With n(i) = (2i+1) m + D = q(i) * 2D + rem(i):  rhi(i) = min(q(i), m) and rlo(i) = q(i-1) - (rem(i-1) == 0); n(i+1) =
// n(i) + 2m with 2m <= 2D, so q grows by at most one per column and no division is needed.  rhi - rlo <= 2.  This is the
// recurrence of views.hip's vw_ray; that walker stays where it is: it yields flat indices of cells it knows to lie in the
// grid, four columns at a time and in no order, while this one yields coordinates (the edge test needs them) cell by cell in
// sequence order.  The two share the recurrence and no code.
//
// Bound.  A ray that is not ignored has D, m <= SC_SCAN_MAX_REACH = 16384: n(i) <= (2D+1) m + D <= 32769 * 16384 + 16384
// < 2^30, rem < 2D + 2m <= 2^16, and a coordinate stays within SC_MAX_DIM + SC_SCAN_MAX_REACH of zero: everything fits int32.
#pragma once
#include <stdint.h>

#include "../../include/sea_current_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RW_HD __host__ __device__ __forceinline__
#else
#define RW_HD inline
#endif

// a ray that is not ignored: a inside the grid, |bx - ax| and |by - ay| <= SC_SCAN_MAX_REACH (64-bit: b is any int32)
RW_HD bool rw_ray_ok(int ax, int ay, int bx, int by, int W, int H) {
    if (ax < 0 || ay < 0 || ax >= W || ay >= H) return false;
    const int64_t dx = (int64_t)bx - ax, dy = (int64_t)by - ay;
    return dx >= -SC_SCAN_MAX_REACH && dx <= SC_SCAN_MAX_REACH && dy >= -SC_SCAN_MAX_REACH && dy <= SC_SCAN_MAX_REACH;
}

struct rw_walk {
    int ax, ay, D, m, twoD;
    int Mx, My, mx, my;   // the unit step of the major axis and of the minor axis, in x and y
    int i, q, rem, rlo;   // column i: q, rem of n(i); rlo of column i
    RW_HD void init(int ax_, int ay_, int bx, int by) {
        ax = ax_;
        ay = ay_;
        const int dx = bx - ax, dy = by - ay;   // rw_ray_ok: no overflow
        const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
        const bool xmajor = adx >= ady;
        D = xmajor ? adx : ady;
        m = xmajor ? ady : adx;
        const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
        Mx = xmajor ? sx : 0;
        My = xmajor ? 0 : sy;
        mx = xmajor ? 0 : sx;
        my = xmajor ? sy : 0;
        twoD = 2 * D;
        i = 0;
        // n(0) = m + D < 2D unless m == D (then q = 1, rem = 0); D == 0: one column, row 0
        q = (D > 0 && m == D) ? 1 : 0;
        rem = (D > 0 && m == D) ? 0 : m + D;
        rlo = 0;
    }
    RW_HD bool finished() const { return i > D; }
    RW_HD int rhi() const { return q < m ? q : m; }
    // the cell of row r in column i
    RW_HD void cell(int r, int& x, int& y) const {
        x = ax + i * Mx + r * mx;
        y = ay + i * My + r * my;
    }
    // to column i + 1
    RW_HD void next() {
        rlo = q - (rem == 0 ? 1 : 0);
        rem += 2 * m;
        if (rem >= twoD && twoD > 0) { rem -= twoD; ++q; }
        ++i;
    }
};

// Walk(a, b) cell by cell: visit(cell index) in sequence order until it returns false, a cell lies outside the grid, or
// the walk ends.  The ray must be rw_ray_ok.
template <class F>
RW_HD void rw_each(int ax, int ay, int bx, int by, int W, int H, F&& visit) {
    rw_walk w;
    w.init(ax, ay, bx, by);
    for (; !w.finished(); w.next()) {
        const int rhi = w.rhi();
        for (int r = w.rlo; r <= rhi; ++r) {
            int x, y;
            w.cell(r, x, y);
            if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) return;
            if (!visit(y * W + x)) return;
        }
    }
}
