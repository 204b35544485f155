// tile_label.h -- the tile labeller shared by components.hip (4-connected free space) and frontier.hip (8-connected frontier
// clusters), and the wave shuffles field.hip uses as well.  Device code only, all of it inlined into the callers' kernels.
//
// The machine: one wavefront per 64 x 64 tile, lane = column.  A 64-bit mask per lane says which cells of the column take
// part; the column's 64 labels (tile-local indices y * 64 + lane) stay in registers.  label_tile sweeps the rows down and up
// to a fixed point, count_runs counts the cells of every local set, store_forest writes a forest into the label array, unite
// joins the trees across tile edges and flatten_cell points every cell at its root.  The result, label[c] = the smallest
// linear index of c's set, does not depend on any execution order.  The proofs are in DESIGN.md section 15.2 (the union, the
// counts) and section 22.2 (the fixed point with diagonal links); the conditions they and the compiler rely on stand at
// each routine.
#pragma once
#include "sc_internal.h"

namespace tl {

constexpr int T = 64;                     // tile edge (= wavefront width)
constexpr uint32_t INF = 0xFFFFFFFFu;     // label of a cell outside the mask while the labels are in registers

// ---- wave helpers ----
// lanes whose source lies outside the wave (lane < s going up, lane + s > 63 going down) receive their own value
__device__ __forceinline__ uint32_t shup(uint32_t v, int s) { return (uint32_t)__shfl_up((int)v, s, 64); }
__device__ __forceinline__ uint32_t shdn(uint32_t v, int s) { return (uint32_t)__shfl_down((int)v, s, 64); }
__device__ __forceinline__ uint64_t shup64(uint64_t v) {
    return ((uint64_t)shup((uint32_t)(v >> 32), 1) << 32) | shup((uint32_t)v, 1);
}
__device__ __forceinline__ uint64_t shdn64(uint64_t v) {
    return ((uint64_t)shdn((uint32_t)(v >> 32), 1) << 32) | shdn((uint32_t)v, 1);
}

// Every read of a word that other workgroups of the launch write (the parents of the forest) is a relaxed agent-scope atomic
// load; every write is atomicMin or st_agent.
__device__ __forceinline__ int32_t ld_agent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- the sweep ----
// minimum of v over each run of lanes inside the mask (tmask = ballot of tc, this row's mask bit): segmented min-scans
// left-to-right then right-to-left
__device__ __forceinline__ uint32_t seg_min(uint32_t v, uint64_t tmask, bool tc, int lane) {
    const uint64_t blocked = ~tmask;
    const uint64_t below = blocked & ((1ull << lane) - 1ull);
    const int rs = below ? 64 - __clzll((long long)below) : 0;
    const uint64_t above = lane == 63 ? 0ull : (blocked & (~0ull << (lane + 1)));
    const int re = above ? __ffsll((long long)above) - 2 : 63;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = shup(v, s);
        if (tc && lane - s >= rs) v = min(v, o);
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = shdn(v, s);
        if (tc && lane + s <= re) v = min(v, o);
    }
    return v;
}

// One row step of a sweep: row y takes the minimum with the cells of row yp = y -/+ 1 it touches, then closes its horizontal
// runs; returns whether it changed.  !DIAG (4-connected): the vertical neighbour, where both cells are in the mask; rows is
// not read.  DIAG (8-connected): the vertical and, through two shuffles, the two diagonal neighbours (a cell outside the mask
// holds INF and never wins); rows, wave-uniform, has bit y set where row y has a cell in the mask, and a row without one is
// skipped outright.  y and yp must be compile-time constants: an index into lab the compiler cannot resolve moves the 64
// labels from registers to scratch.
template <bool DIAG>
__device__ __forceinline__ bool row_step(uint32_t (&lab)[T], uint64_t m, uint64_t rows, int y, int yp, int lane, bool force) {
    if (DIAG && !((rows >> y) & 1ull)) return false;
    const bool tc = ((m >> y) & 1ull) != 0;
    const uint32_t old = lab[y];
    uint32_t v = old;
    if (yp >= 0 && yp < T) {
        if constexpr (DIAG) {
            if ((rows >> yp) & 1ull) {
                const uint32_t p = lab[yp];
                const uint32_t pl = shup(p, 1), pr = shdn(p, 1);   // lanes 0 / 63 receive their own p
                if (tc) v = min(v, min(p, min(pl, pr)));
            }
        } else {
            if (tc && ((m >> yp) & 1ull)) v = min(v, lab[yp]);
        }
    }
    if (__ballot(v < old) != 0ull || force) {
        const uint64_t tm = __ballot(tc);
        if (DIAG || tm != 0ull) v = seg_min(v, tm, tc, lane);
    }
    lab[y] = v;
    return __ballot(v < old) != 0ull;
}

// fully unrolled in both directions, so that every index of lab is a constant
template <bool DIAG>
__device__ __forceinline__ bool sweep(uint32_t (&lab)[T], uint64_t m, uint64_t rows, bool down, int lane, bool force) {
    bool c = false;
    if (down) {
#pragma unroll
        for (int y = 0; y < T; ++y) c |= row_step<DIAG>(lab, m, rows, y, y - 1, lane, force);
    } else {
#pragma unroll
        for (int y = T - 1; y >= 0; --y) c |= row_step<DIAG>(lab, m, rows, y, y + 1, lane, force);
    }
    return c;
}

// lab[y] = the smallest y' * 64 + lane' over the cells of the connected set of cell (y, lane) inside the tile, INF outside the
// mask m (bit y of m: row y of this lane's column).  The first sweep closes every run (force); a later sweep works only where
// a label fell.  Labels only fall and remain indices of cells of the own set, and the cell that holds a set's minimum keeps
// it.  A sweep leaves every cell <= its neighbours in the row it came from and every run constant, so a state that the
// opposite sweep leaves unchanged has every cell <= all of its neighbours: constant on every connected set, hence the
// minimum.  That is why the loop ends after a sweep, not the first, that changed nothing.
template <bool DIAG>
__device__ __forceinline__ void label_tile(uint32_t (&lab)[T], uint64_t m, int lane) {
    uint64_t rows = 0;
    if constexpr (DIAG) {
#pragma unroll
        for (int y = 0; y < T; ++y) rows |= (uint64_t)(__ballot((m >> y) & 1ull) != 0ull) << y;
    }
#pragma unroll
    for (int y = 0; y < T; ++y) lab[y] = ((m >> y) & 1ull) ? (uint32_t)(y * T + lane) : INF;
    if (!DIAG && __ballot(m != 0ull) == 0ull) return;   // DIAG: an empty tile has no row to step
    bool down = true;
    for (int k = 0;; ++k) {
        const bool c = sweep<DIAG>(lab, m, rows, down, lane, k == 0);
        if (!c && k >= 1) break;
        down = !down;
    }
}

// ---- counts and the forest ----
// cnt[l] = the number of cells labelled l, for the labels label_tile left; cnt: T * T words of LDS, the wavefront's own.
// One add per horizontal run: its cells share a label.
__device__ __forceinline__ void count_runs(int32_t* cnt, const uint32_t (&lab)[T], uint64_t m, int lane) {
    int32_t* const z = cnt + lane;   // 64 stores off one address
#pragma unroll
    for (int k = 0; k < T; ++k) z[k * 64] = 0;
    wave_lds_sync();
#pragma unroll
    for (int y = 0; y < T; ++y) {
        const bool tc = ((m >> y) & 1ull) != 0;
        const uint64_t tm = __ballot(tc);
        if (tc && (lane == 0 || !((tm >> (lane - 1)) & 1ull))) {
            const uint64_t r = ~(tm >> lane);
            atomicAdd(&cnt[lab[y]], r ? __ffsll((long long)r) - 1 : 64);
        }
    }
    wave_lds_sync();
}

// The forest of the tile at (x0, y0) of a W-wide grid: L[c] = the global index of c's local minimum r (L[r] == r), -1 outside
// the mask; rows >= th and lanes with !colin lie outside the grid.  With S (may be NULL; then cnt is not read) S[c] = the
// cell count of the local set at its minimum, 0 elsewhere: flatten_cell relies on a non-root holding exactly that.
__device__ __forceinline__ void store_forest(int32_t* L, int32_t* S, const int32_t* cnt, const uint32_t (&lab)[T], int W, int x0, int y0,
                                             int th, bool colin, int lane) {
    // Nothing below depends on the grid or on the sweeps, so the compiler would compute the 64 rows' predicates and addresses
    // ahead of the callers' loop over the grids, before the tile's first load, and carry them across all the sweeps in
    // registers the labels need (they end up in AGPRs and in spilled SGPRs).  The empty statement makes the inputs new
    // values here; the lane's cell of row 0 then joins the grid's pointer and a row adds a wave-uniform offset.
    asm volatile("" : "+v"(lane), "+s"(W), "+s"(x0), "+s"(y0), "+s"(th));
    const size_t c0 = (size_t)y0 * W + x0 + (colin ? lane : 0);
    int32_t* const L0 = L + c0;
    int32_t* const S0 = S ? S + c0 : nullptr;
#pragma unroll
    for (int y = 0; y < T; ++y) {
        if (colin && y < th) {
            const uint32_t l = lab[y];
            const bool tc = l != INF;
            L0[y * W] = tc ? (int32_t)((y0 + (int)(l >> 6)) * W + x0 + (int)(l & 63u)) : -1;
            if (S) S0[y * W] = (tc && l == (uint32_t)(y * T + lane)) ? cnt[l] : 0;
        }
    }
    wave_lds_sync();   // cnt is reused by the next grid
}

// ---- union-find across tile edges (Komura / Playne) ----
// A cell's parent is a cell of its own set with an index no larger than its own, and parents only fall: every chain ends.
__device__ __forceinline__ int32_t find(const int32_t* L, int32_t x) {
    for (;;) {
        const int32_t p = ld_agent(L + x);
        if (p == x) return x;
        x = p;
    }
}

// unite the trees of a and b (cells of one grid): the larger root is linked to the smaller; when the atomicMin finds the
// larger root linked meanwhile, the link it displaced (or the one it lost to) is united in turn.  Every interleaving ends in
// one tree per set whose root is the set's minimum.
__device__ __forceinline__ void unite(int32_t* L, int32_t a, int32_t b) {
    for (;;) {
        a = find(L, a);
        b = find(L, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

// Edge i of a grid of W x H cells: the (TY - 1) * W cells above horizontal tile edges (i < ne_h) come first, then the
// (TX - 1) * H cells left of vertical ones.  a: the cell on the near side, b: the cell facing it, b -/+ step: b's neighbours
// along the edge, pos < len: where along the edge, in cells from the grid's border.
struct edge { int a, b, step, pos, len; };
__device__ __forceinline__ edge edge_decode(size_t i, size_t ne_h, int W, int H) {
    if (i < ne_h) {
        const int t = (int)(i / W) + 1, x = (int)(i % W), a = (t * T - 1) * W + x;
        return {a, a + W, 1, x, W};
    }
    const size_t j = i - ne_h;
    const int t = (int)(j / H) + 1, y = (int)(j % H), a = y * W + t * T - 1;
    return {a, a + 1, W, y, H};
}

// The flatten pass for cell c of one grid, after all unions of the launch: follows the parents to the root and stores it (a
// concurrent reader sees the old parent or the root, both ancestors); with S (may be NULL), moves a non-root's count to the
// root and clears its own.  A cell that is not a root receives no adds, so its count is what store_forest wrote and the plain
// read is safe.  Returns whether c is a root.
__device__ __forceinline__ bool flatten_cell(int32_t* L, int32_t* S, size_t c) {
    const int32_t l = ld_agent(L + c);
    if (l < 0) return false;
    const int32_t r = find(L, l);
    if (r != l) st_agent(L + c, r);
    const bool root = r == (int32_t)c;
    if (S && !root) {
        const int32_t s = S[c];
        if (s) {
            atomicAdd(S + r, s);
            S[c] = 0;
        }
    }
    return root;
}

}  // namespace tl
