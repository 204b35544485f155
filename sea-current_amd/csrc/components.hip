// components.hip -- connected components of the traversable cells (sc_components_batch), O(1) reachability from the labels
// (sc_reachable_batch) and A* that never searches a hopeless query (sc_astar_batch_screened).
//
// Definition.  T(c) <=> d2[c] >= max(r2_clear, 1).  Two traversable cells lie in one component iff a chain of orthogonal
// moves through traversable cells joins them.  label[c] = the smallest linear index y * W + x of c's component, -1 where c
// is not traversable: unique, and independent of any execution order.
//   This is exactly A*'s reachability.  A*'s graph (oracle/sc_oracle.h) has 8 moves, but a diagonal move needs both of its
//   orthogonal side cells traversable, so every diagonal move can be replaced by two orthogonal moves through one of them:
//   8-connected reachability under the no-corner-cutting rule equals 4-connected reachability.  Hence for two traversable
//   cells sc_astar_batch finds a path (SC_Q_OK or SC_Q_TRUNCATED) iff their labels are equal.  DESIGN.md section 15.
//
// Kernels: a constant number of launches on one stream, no workgroup waits for another, integer atomics only.  The labelling
// routines are those of tile_label.h, shared with frontier.hip.
//   1. comp_tile_kernel: one wavefront per 64 x 64 tile, lane = column.  It reads its 64 x 64 cells of d2 into one 64-bit
//      traversability mask per lane, runs the 4-connected tile labeller on it (sweeps to the fixed point, labels in
//      registers) and stores the global index of each cell's local minimum (a forest: label[c] = r with label[r] == r) and,
//      at each local minimum, the cell count of the local component.
//   2. comp_border_kernel: one thread per pair of cells that face each other across a tile edge.  Where both are
//      traversable it unites their trees (the lock-free union-find: one tree per component, rooted at its minimum).
//   3. comp_flatten_kernel: every cell follows its parents to the root and stores it; a local minimum that is not the root
//      adds its local count to the root's and clears its own; roots are counted per wavefront (ballot) into ncomp.
//   4. comp_largest_kernel (only when `largest` is asked for): 64-bit atomicMax of size << 32 | ~index over the roots, one
//      per wavefront; comp_largest_out_kernel turns the key into the index.
#include "tile_label.h"

namespace {

using tl::ld_agent;
constexpr int CT = tl::T;   // tile edge

struct comp_args {
    const int32_t* d2;   // [G][H][W]
    int32_t* label;      // [G][H][W]
    int32_t* sz;         // [G][H][W] or NULL
    int G, W, H, TX, TY;
    int32_t thr;
};

// grid (tiles, grids): grids strided
__global__ __launch_bounds__(64) void comp_tile_kernel(comp_args a) {
    __shared__ int32_t cnt[CT * CT];
    const int lane = threadIdx.x;
    const int W = a.W, H = a.H;
    const int tx = blockIdx.x % a.TX, ty = blockIdx.x / a.TX;
    const int x0 = tx * CT, y0 = ty * CT;
    const int tw = min(CT, W - x0), th = min(CT, H - y0);
    const int cx = x0 + lane;
    const bool colin = lane < tw;
    const size_t n = (size_t)W * H;
    for (int gi = blockIdx.y; gi < a.G; gi += gridDim.y) {
        const int32_t* D = a.d2 + (size_t)gi * n;
        int32_t* L = a.label + (size_t)gi * n;
        int32_t* S = a.sz ? a.sz + (size_t)gi * n : nullptr;
        uint64_t m = 0;
#pragma unroll
        for (int y = 0; y < CT; ++y) {
            const bool t = colin && y < th && D[(size_t)(y0 + y) * W + cx] >= a.thr;
            m |= (uint64_t)t << y;
        }
        uint32_t lab[CT];
        tl::label_tile<false>(lab, m, lane);
        if (S) tl::count_runs(cnt, lab, m, lane);
        tl::store_forest(L, S, cnt, lab, W, x0, y0, th, colin, lane);
    }
}

// pairs of cells facing each other across a tile edge: (TY - 1) * W across horizontal edges, then (TX - 1) * H across
// vertical ones.  A pair whose predecessor along the edge (inside the same two tiles) is traversable on both sides joins
// the same two local components as that predecessor: it is skipped.
__global__ __launch_bounds__(256) void comp_border_kernel(int32_t* label, int G, int W, int H, int TX, int TY) {
    const size_t n = (size_t)W * H;
    const size_t ne_h = (size_t)(TY - 1) * W, ne = ne_h + (size_t)(TX - 1) * H;
    for (int gi = blockIdx.y; gi < G; gi += gridDim.y) {
        int32_t* L = label + (size_t)gi * n;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += (size_t)gridDim.x * blockDim.x) {
            const tl::edge e = tl::edge_decode(i, ne_h, W, H);
            const int32_t la = ld_agent(L + e.a);
            if (la < 0) continue;
            const int32_t lb = ld_agent(L + e.b);
            if (lb < 0) continue;
            if (e.pos % CT != 0 && ld_agent(L + e.a - e.step) >= 0 && ld_agent(L + e.b - e.step) >= 0) continue;
            tl::unite(L, la, lb);
        }
    }
}

// grid (ceil(n / 256), grids): grids strided
__global__ __launch_bounds__(256) void comp_flatten_kernel(int32_t* label, int32_t* sz, int32_t* ncomp, int G, int W, int H) {
    const size_t n = (size_t)W * H;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (int gi = blockIdx.y; gi < G; gi += gridDim.y) {
        const bool root = c < n && tl::flatten_cell(label + (size_t)gi * n, sz ? sz + (size_t)gi * n : nullptr, c);
        if (ncomp) {
            const int k = __popcll(__ballot(root));
            if ((threadIdx.x & 63) == 0 && k) atomicAdd(ncomp + gi, k);
        }
    }
}

__global__ __launch_bounds__(256) void comp_largest_kernel(const int32_t* label, const int32_t* sz, unsigned long long* key, int G, int W, int H) {
    const size_t n = (size_t)W * H;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (int gi = blockIdx.y; gi < G; gi += gridDim.y) {
        unsigned long long k = 0;
        if (c < n && label[(size_t)gi * n + c] == (int32_t)c)
            k = ((unsigned long long)(uint32_t)sz[(size_t)gi * n + c] << 32) | (uint32_t)~(uint32_t)c;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), s, 64), lo = (uint32_t)__shfl_xor((int)(uint32_t)k, s, 64);
            const unsigned long long o = ((unsigned long long)hi << 32) | lo;
            k = o > k ? o : k;
        }
        if ((threadIdx.x & 63) == 0 && k) atomicMax(key + gi, k);
    }
}

__global__ void comp_largest_out_kernel(const unsigned long long* key, int32_t* largest, int G) {
    const int gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi < G) largest[gi] = key[gi] ? (int32_t)~(uint32_t)key[gi] : -1;
}

// the status sc_astar_batch gives query q, SC_Q_OK standing for SC_Q_OK and SC_Q_TRUNCATED; grid_ok: qgrid[q] is in range
__device__ __forceinline__ int reach_status(const int32_t* label, int G, const int32_t* qgrid, size_t n, const int32_t* start,
                                            const int32_t* goal, int q, bool& grid_ok) {
    const int gi = qgrid ? qgrid[q] : 0;
    const int s = start[q], t = goal[q];
    grid_ok = gi >= 0 && gi < G;
    if (!grid_ok || s < 0 || t < 0 || (size_t)s >= n || (size_t)t >= n) return SC_Q_BAD_ENDPOINT;
    const int32_t ls = label[(size_t)gi * n + s], lt = label[(size_t)gi * n + t];
    if (ls < 0 || lt < 0) return SC_Q_BAD_ENDPOINT;
    return ls == lt ? SC_Q_OK : SC_Q_NO_PATH;
}

__global__ void reachable_kernel(const int32_t* label, int G, const int32_t* qgrid, int W, int H, const int32_t* start, const int32_t* goal,
                                 int Q, int32_t* status) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    bool grid_ok;
    status[q] = reach_status(label, G, qgrid, (size_t)W * H, start, goal, q, grid_ok);
}

// the starts the search runs on: -1 (a bad endpoint: the search leaves at once with len 0 and cost -1) where the endpoints
// lie in different components, and where the query names no grid
__global__ void screen_mask_kernel(const int32_t* label, int G, const int32_t* qgrid, int W, int H, const int32_t* start,
                                   const int32_t* goal, int Q, int32_t* masked) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    bool grid_ok;
    const int st = reach_status(label, G, qgrid, (size_t)W * H, start, goal, q, grid_ok);
    masked[q] = (st == SC_Q_NO_PATH || !grid_ok) ? -1 : start[q];
}

__global__ void screen_status_kernel(const int32_t* label, int G, const int32_t* qgrid, int W, int H, const int32_t* start,
                                     const int32_t* goal, int Q, int32_t* status) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    bool grid_ok;
    if (reach_status(label, G, qgrid, (size_t)W * H, start, goal, q, grid_ok) == SC_Q_NO_PATH) status[q] = SC_Q_NO_PATH;
}

}  // namespace

static bool components_args_ok(const sc_ctx* ctx, const int32_t* d2, int G, int W, int H, const int32_t* label) {
    return ctx && d2 && label && G > 0 && W > 0 && H > 0 && W <= SC_MAX_DIM && H <= SC_MAX_DIM;
}

static bool reachable_args_ok(const sc_ctx* ctx, const int32_t* label, int G, const int32_t* qgrid, int W, int H, const int32_t* start,
                              const int32_t* goal, int Q, const int32_t* status) {
    return ctx && label && start && goal && status && G > 0 && W > 0 && H > 0 && W <= SC_MAX_DIM && H <= SC_MAX_DIM && Q >= 0 &&
           (qgrid || G == 1);
}

extern "C" int sc_components_batch(sc_ctx* ctx, const int32_t* d2, int G, int W, int H, int32_t r2_clear, int32_t* label, int32_t* size,
                                   int32_t* ncomp, int32_t* largest) {
    if (!components_args_ok(ctx, d2, G, W, H, label)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const int TX = (W + CT - 1) / CT, TY = (H + CT - 1) / CT;
    const size_t n = (size_t)W * H;
    // scratch: the largest keys, then the sizes when `largest` needs them and the caller keeps none
    const size_t o_sz = al256((size_t)G * 8);
    const bool own_sz = largest && !size;
    if (largest) {
        const int r = sc_scratch_reserve(ctx, &ctx->cmp_state, o_sz + (own_sz ? (size_t)G * n * 4 : 0));
        if (r != SC_OK) return r;
    }
    int32_t* sz = own_sz ? (int32_t*)((char*)ctx->cmp_state.p + o_sz) : size;
    unsigned long long* key = largest ? (unsigned long long*)ctx->cmp_state.p : nullptr;
    const unsigned gy = (unsigned)(G < 65535 ? G : 65535);
    const unsigned bx = (unsigned)((n + 255) / 256);
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    if (ncomp) SC_HIP(ctx, hipMemsetAsync(ncomp, 0, (size_t)G * 4, ctx->stream));
    if (key) SC_HIP(ctx, hipMemsetAsync(key, 0, (size_t)G * 8, ctx->stream));
    comp_args a{d2, label, sz, G, W, H, TX, TY, r2_clear > 1 ? r2_clear : 1};
    hipLaunchKernelGGL(comp_tile_kernel, dim3((unsigned)(TX * TY), gy), dim3(64), 0, ctx->stream, a);
    if (TX > 1 || TY > 1) {
        const size_t ne = (size_t)(TY - 1) * W + (size_t)(TX - 1) * H;
        hipLaunchKernelGGL(comp_border_kernel, dim3((unsigned)((ne + 255) / 256), gy), dim3(256), 0, ctx->stream, label, G, W, H, TX, TY);
    }
    hipLaunchKernelGGL(comp_flatten_kernel, dim3(bx, gy), dim3(256), 0, ctx->stream, label, sz, ncomp, G, W, H);
    if (largest) {
        hipLaunchKernelGGL(comp_largest_kernel, dim3(bx, gy), dim3(256), 0, ctx->stream, (const int32_t*)label, (const int32_t*)sz, key, G, W, H);
        hipLaunchKernelGGL(comp_largest_out_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const unsigned long long*)key, largest, G);
    }
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_reachable_batch(sc_ctx* ctx, const int32_t* label, int G, const int32_t* qgrid, int W, int H, const int32_t* start,
                                  const int32_t* goal, int Q, int32_t* status) {
    if (!reachable_args_ok(ctx, label, G, qgrid, W, H, start, goal, Q, status)) return SC_ERR_INVALID;
    if (Q == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    hipLaunchKernelGGL(reachable_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, ctx->stream, label, G, qgrid, W, H, start, goal, Q,
                       status);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_astar_batch_screened(sc_ctx* ctx, const int32_t* d2, const int32_t* label, int G, const int32_t* qgrid, int W, int H,
                                       int32_t r2_clear, const int32_t* start, const int32_t* goal, int Q, int Lmax, int32_t* path,
                                       int32_t* len, int32_t* cost, int32_t* status) {
    if (!reachable_args_ok(ctx, label, G, qgrid, W, H, start, goal, Q, status) || !d2 || !path || !len || !cost || Lmax <= 0)
        return SC_ERR_INVALID;
    if (Q == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    int r = sc_scratch_reserve(ctx, &ctx->cmp_start, (size_t)Q * 4);
    if (r != SC_OK) return r;
    int32_t* masked = (int32_t*)ctx->cmp_start.p;
    const dim3 grid((unsigned)((Q + 255) / 256)), block(256);
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    hipLaunchKernelGGL(screen_mask_kernel, grid, block, 0, ctx->stream, label, G, qgrid, W, H, start, goal, Q, masked);
    sc_time_end(ctx, tk);
    r = qgrid ? sc_astar_batch_multi(ctx, d2, G, qgrid, W, H, r2_clear, masked, goal, Q, Lmax, path, len, cost, status)
              : sc_astar_batch(ctx, d2, W, H, r2_clear, masked, goal, Q, Lmax, path, len, cost, status);
    if (r != SC_OK) return r;
    tk = sc_time_begin(ctx, SC_K_ASTAR);
    hipLaunchKernelGGL(screen_status_kernel, grid, block, 0, ctx->stream, label, G, qgrid, W, H, start, goal, Q, status);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_components_batch_host(sc_ctx* ctx, const int32_t* d2, int G, int W, int H, int32_t r2_clear, int32_t* label,
                                        int32_t* size, int32_t* ncomp, int32_t* largest) {
    if (!components_args_ok(ctx, d2, G, W, H, label)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nb = (size_t)G * W * H * 4, gb = (size_t)G * 4;
    sc_stage st(ctx);
    const int i_d2 = st.in(d2, nb);
    const int o_l = st.out(label, nb), o_s = st.out(size, size ? nb : 0), o_n = st.out(ncomp, gb), o_g = st.out(largest, gb);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_components_batch(ctx, st.dev<const int32_t>(i_d2), G, W, H, r2_clear, st.dev<int32_t>(o_l), size ? st.dev<int32_t>(o_s) : nullptr,
                                ncomp ? st.dev<int32_t>(o_n) : nullptr, largest ? st.dev<int32_t>(o_g) : nullptr);
    return st.finish(r);
}

extern "C" int sc_reachable_batch_host(sc_ctx* ctx, const int32_t* label, int G, const int32_t* qgrid, int W, int H, const int32_t* start,
                                       const int32_t* goal, int Q, int32_t* status) {
    if (!reachable_args_ok(ctx, label, G, qgrid, W, H, start, goal, Q, status)) return SC_ERR_INVALID;
    if (Q == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t qb = (size_t)Q * 4;
    sc_stage st(ctx);
    const int i_l = st.in(label, (size_t)G * W * H * 4), i_q = st.in(qgrid, qb), i_s = st.in(start, qb), i_g = st.in(goal, qb);
    const int o_st = st.out(status, qb);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_reachable_batch(ctx, st.dev<const int32_t>(i_l), G, qgrid ? st.dev<const int32_t>(i_q) : nullptr, W, H, st.dev<const int32_t>(i_s),
                               st.dev<const int32_t>(i_g), Q, st.dev<int32_t>(o_st));
    return st.finish(r);
}
