// waypoints.hip -- A* cell paths -> line-of-sight waypoints (sc_path_waypoints_batch).
//
// The reference's planner returns a short list of sample points and its caller hands that list to from_path
// (examples/test.cpp:284 -> :300).  The grid planner returns every cell of its path instead, and a grid path is mostly
// collinear runs: the tangent rule (sea_current.hpp:347-352) gives NaN there and every cell would become a Bezier leg.
// This kernel shortcuts a cell path to the cells where it has to turn.  Definitions:
//
//   T(c)          d2[c] >= max(r2_clear, 1)                     (the rule of sc_moves_i32_u8 and A*)
//   Visible(a, b) every cell whose closed unit square meets the closed segment between the centres of a and b is
//                 traversable (the segment's supercover: through a corner it needs both side cells, A*'s no-corner-
//                 cutting rule).  Such a segment never leaves the bounding box of a and b.
//   greedy        out = [p0], anchor a = 0; j = the largest index with Visible(p[a], p[k]) for every k in a+1..j;
//                 emit p[j]; stop at j = L-1, else a = j and repeat.
//   merge         before w is appended, the last output point b is dropped while out[-2], b, w are collinear in the
//                 same direction (cross = 0, dot > 0): the supercover of a-w is the union of those of a-b and b-w.
//   reversed      if out[-2], out[-1] = p[a], p[j] are collinear in the reverse direction (cross = 0, dot < 0), j is
//                 lowered (not below a+1) until they are not (a defined treatment; it fires on no path of the tests).
//
// Kernel: one wavefront per path.  The 64 lanes test the candidates a+1 .. a+64 at once, each lane walking its own
// segment's supercover column by column (integer arithmetic only, d2 read from global memory / L2, four columns' loads in
// flight at a time), and a ballot after every round finds the first failure: the wave stops once every lane below it
// has finished; without a failure it moves on by 64.  Validation uses wp_visible, the same walk one cell at a time.  Output points are written with plain stores by lane 0 into
// wp (indices < Wmax) or, when Wmax is too small, into context scratch so that the merge can still look back and the
// needed count is exact.
#include "sc_internal.h"

namespace {

__device__ __forceinline__ bool wp_traversable(const int32_t* __restrict__ d2, int c, int32_t thr) { return d2[c] >= thr; }

// Visible(ca, cb) by columns of the major axis: in column i (0 .. D) of the segment, in doubled coordinates relative to
// a, the segment spans t in [max(2i-1, 0), min(2i+1, 2D)] along the major axis and rises t * m / (2D) on the minor one
// (m = |minor delta| <= D); the cells it meets there are rows ceil((tlo m - D) / 2D) .. floor((thi m + D) / 2D).
__device__ bool wp_visible(const int32_t* __restrict__ d2, int W, int H, int32_t thr, int ca, int cb) {
    const int ax = ca % W, ay = ca / W, bx = cb % W, by = cb / W;
    int dx = bx - ax, dy = by - ay;
    if (dx == 0 && dy == 0) return wp_traversable(d2, ca, thr);
    const bool xmajor = abs(dx) >= abs(dy);
    const int D = xmajor ? abs(dx) : abs(dy), m = xmajor ? abs(dy) : abs(dx);
    const int smaj = (xmajor ? dx : dy) < 0 ? -1 : 1, smin = (xmajor ? dy : dx) < 0 ? -1 : 1;
    const int twoD = 2 * D;
    for (int i = 0; i <= D; ++i) {
        const int tlo = max(2 * i - 1, 0), thi = min(2 * i + 1, twoD);
        const int nlo = tlo * m - D, nhi = thi * m + D;
        const int rlo = nlo <= 0 ? 0 : (nlo + twoD - 1) / twoD, rhi = nhi / twoD;
        for (int r = rlo; r <= rhi; ++r) {
            int x, y;
            if (xmajor) { x = ax + smaj * i; y = ay + smin * r; }
            else { y = ay + smaj * i; x = ax + smin * r; }
            if (x < 0 || y < 0 || x >= W || y >= H) return false;   // not reached for cells of the grid (see above)
            if (!wp_traversable(d2, y * W + x, thr)) return false;
        }
    }
    return true;
}

// The same walk as wp_visible, WP_COLS columns per call with every load of a round issued before any test: a lane's
// columns are independent, so the round costs about one L2 round trip instead of one per column.  Rows per column:
// rlo .. rhi with rhi - rlo <= 2 (three loads, the unused ones repeat rhi).  Every cell lies in the bounding box of the
// two endpoints, hence in the grid; the index guard only keeps a broken invariant from reading outside d2.
#define WP_COLS 4
struct wp_walker {
    int ca, D, m, twoD, sM, sm, i;
    __device__ void init(int W, int a, int b) {
        const int dx = b % W - a % W, dy = b / W - a / W;
        const bool xmajor = abs(dx) >= abs(dy);
        D = xmajor ? abs(dx) : abs(dy);
        m = xmajor ? abs(dy) : abs(dx);
        const int smaj = (xmajor ? dx : dy) < 0 ? -1 : 1, smin = (xmajor ? dy : dx) < 0 ? -1 : 1;
        sM = xmajor ? smaj : smaj * W;   // index step along the major axis
        sm = xmajor ? smin * W : smin;   // index step along the minor axis
        twoD = 2 * D;
        ca = a;
        i = 0;
    }
    __device__ bool finished() const { return i > D; }
    __device__ bool step(const int32_t* __restrict__ d2, int cells, int32_t thr) {
        int32_t v[WP_COLS][3];
#pragma unroll
        for (int c = 0; c < WP_COLS; ++c) {
            const int ii = min(i + c, D);
            int rlo = 0, rhi = 0;
            if (D > 0) {
                const int tlo = max(2 * ii - 1, 0), thi = min(2 * ii + 1, twoD);
                const int nlo = tlo * m - D, nhi = thi * m + D;
                rlo = nlo <= 0 ? 0 : (nlo + twoD - 1) / twoD;
                rhi = nhi / twoD;
            }
            const int base = ca + ii * sM;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int idx = base + min(rlo + r, rhi) * sm;
                v[c][r] = (unsigned)idx < (unsigned)cells ? d2[idx] : -1;
            }
        }
        bool ok = true;
#pragma unroll
        for (int c = 0; c < WP_COLS; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) ok = ok && v[c][r] >= thr;
        i += WP_COLS;
        return ok;
    }
};

// collinearity of a, b, w (cell indices): 0 = not collinear, 1 = same direction, -1 = reverse direction
__device__ __forceinline__ int wp_collinear(int W, int a, int b, int w) {
    const int ux = b % W - a % W, uy = b / W - a / W, vx = w % W - b % W, vy = w / W - b / W;
    if (ux * vy - uy * vx != 0) return 0;
    const int dot = ux * vx + uy * vy;
    return dot > 0 ? 1 : (dot < 0 ? -1 : 0);
}

struct wp_out {
    int32_t* wp;      // [Wmax] of this path
    int32_t* spill;   // [Lmax - Wmax] of this path (indices >= Wmax), or null when Wmax >= Lmax
    int Wmax;
    __device__ int32_t* at(int i) const { return i < Wmax ? wp + i : spill + (i - Wmax); }
};

// kLds: the path row is staged in LDS (Lmax <= WP_LDS_MAX_L), so the serial chain of an anchor step (candidates, the
// chosen cell) waits on LDS instead of L2
#define WP_LDS_MAX_L 16384
template <bool kLds>
__global__ void __launch_bounds__(64)
path_waypoints_kernel(const int32_t* __restrict__ d2, int W, int H, int32_t thr, const int32_t* __restrict__ path,
                      const int32_t* __restrict__ len, const int32_t* __restrict__ astar_status, int Q, int Lmax, int Wmax,
                      int32_t* __restrict__ wp, int32_t* __restrict__ n_wp, int32_t* __restrict__ status, int32_t* __restrict__ spill) {
    const int q = blockIdx.x;
    const int lane = threadIdx.x;
    if (q >= Q) return;
    const int cells = W * H;
    const int32_t* p = path + (size_t)q * Lmax;   // the LDS copy once validated (kLds)
    if (astar_status && astar_status[q] != SC_Q_OK) {
        if (lane == 0) { n_wp[q] = 0; status[q] = astar_status[q]; }
        return;
    }
    const int L = len[q];
    // ---- validate: cells in range, consecutive cells 8-adjacent and mutually visible (A*'s move legality)
    bool bad = L < 1 || L > Lmax;
    if (!bad) {
        for (int i = lane; i < L; i += 64) {
            const int c = p[i];
            if (c < 0 || c >= cells) { bad = true; continue; }
            if (L == 1) { bad = !wp_traversable(d2, c, thr); continue; }
            if (i + 1 < L) {
                const int e = p[i + 1];
                if (e < 0 || e >= cells) { bad = true; continue; }
                const int ddx = abs(e % W - c % W), ddy = abs(e / W - c / W);
                if (max(ddx, ddy) != 1 || !wp_visible(d2, W, H, thr, c, e)) bad = true;
            }
        }
    }
    if (__ballot(bad) != 0ull) {
        if (lane == 0) { n_wp[q] = 0; status[q] = SC_Q_BAD_PATH; }
        return;
    }
    extern __shared__ int32_t wp_lds_path[];
    if (kLds) {
        for (int i = lane; i < L; i += 64) wp_lds_path[i] = p[i];
        __syncthreads();
        p = wp_lds_path;
    }
    const wp_out out{wp + (size_t)q * Wmax, spill ? spill + (size_t)q * (Lmax - Wmax) : nullptr, Wmax};
    // ---- greedy prefix shortcut with the collinear merge; o1 = out[-1], o2 = out[-2] (uniform across the wave)
    int n = 1, o1 = p[0], o2 = -1;
    if (lane == 0) *out.at(0) = o1;
    int a = 0;
    while (a < L - 1) {
        const int ca = o1;   // = p[a]
        int j = -1;
        for (int k0 = a + 1; k0 < L && j < 0; k0 += 64) {
            const int k = k0 + lane;
            wp_walker wk;
            wk.init(W, ca, k < L ? p[k] : ca);
            bool done = k >= L, fail = false;
            // walk in rounds of WP_COLS columns; a lane above the lowest failing lane no longer matters (j only depends
            // on the first failure), so the wave stops as soon as every lane below it has finished
            while (true) {
                if (!done) {
                    fail = !wk.step(d2, cells, thr);
                    done = fail || wk.finished();
                }
                const unsigned long long fm = __ballot(fail);
                const int first = fm ? __ffsll((long long)fm) - 1 : 64;
                const unsigned long long below = first >= 64 ? ~0ull : ((1ull << first) - 1);
                if ((__ballot(!done) & below) == 0ull) {
                    if (fm) j = k0 + first - 1;
                    break;
                }
            }
        }
        if (j < 0) j = L - 1;
        // the reverse-direction rule (lowers j to a cell off the line out[-2], p[a])
        if (o2 >= 0)
            while (j > a + 1 && wp_collinear(W, o2, ca, p[j]) < 0) --j;
        const int w = p[j];
        while (n >= 2 && wp_collinear(W, o2, o1, w) > 0) {   // drop out[-1]
            --n;
            o1 = o2;
            o2 = n >= 2 ? *out.at(n - 2) : -1;
        }
        if (lane == 0) *out.at(n) = w;
        o2 = o1; o1 = w; ++n;
        a = j;
    }
    if (lane == 0) { n_wp[q] = n; status[q] = n <= Wmax ? SC_Q_OK : SC_Q_TRUNCATED; }
}

}  // namespace

extern "C" int sc_path_waypoints_batch(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear, const int32_t* path,
                                       const int32_t* len, const int32_t* astar_status, int Q, int Lmax, int Wmax, int32_t* wp,
                                       int32_t* n_wp, int32_t* status) {
    if (!ctx || !d2 || !path || !len || !wp || !n_wp || !status || W <= 0 || H <= 0 || W > SC_MAX_DIM || H > SC_MAX_DIM || Q < 0 ||
        Lmax <= 0 || Wmax <= 0)
        return SC_ERR_INVALID;
    if (Q == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    int32_t* spill = nullptr;
    if (Wmax < Lmax) {
        int r = sc_scratch_reserve(ctx, &ctx->wp_spill, (size_t)Q * (Lmax - Wmax) * sizeof(int32_t));
        if (r != SC_OK) return r;
        spill = (int32_t*)ctx->wp_spill.p;
    }
    const int32_t thr = r2_clear > 1 ? r2_clear : 1;
    int tk = sc_time_begin(ctx, SC_K_WAYPOINTS);
    if (Lmax <= WP_LDS_MAX_L)
        hipLaunchKernelGGL(path_waypoints_kernel<true>, dim3(Q), dim3(64), (size_t)Lmax * sizeof(int32_t), ctx->stream, d2, W, H, thr, path,
                           len, astar_status, Q, Lmax, Wmax, wp, n_wp, status, spill);
    else
        hipLaunchKernelGGL(path_waypoints_kernel<false>, dim3(Q), dim3(64), 0, ctx->stream, d2, W, H, thr, path, len, astar_status, Q, Lmax,
                           Wmax, wp, n_wp, status, spill);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}
