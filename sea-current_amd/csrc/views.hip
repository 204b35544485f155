// views.hip -- line-of-sight sensing: the known-space mask of views that walls block (sc_known_from_views) and the unknown
// cells a candidate pose would see (sc_view_gain_batch).  DESIGN.md section 23; the definitions are in
// include/sea_current_hip.h.
//
// Definition.  Clear(a, b): every cell whose closed unit square meets the closed segment between the centres of a and b has
// occ == 0 (section 9's Visible with the cell test occ == 0).  vis[c] <=> some view has c in its disc and Clear(centre, c);
// surf[c] <=> occ[c] != 0 and an orthogonal neighbour inside the grid has vis; known = base | vis | surf.
//
// Kernels.  One ray per (view, cell of the view's clipped bounding box); nothing loops over views per grid cell.
//   1. vw_view_kernel: grid (tile slots, views).  A workgroup of 256 takes 16 x 16 tiles of its view's box, strided by the
//      tile slots; a wavefront is an 8 x 8 quarter of the tile, so its 64 rays have nearly the same length and direction.  A
//      lane walks its ray from the centre outward (vw_ray, views_common.h), leaves at its first blocked cell, and the wave
//      leaves when all lanes have.  A visible target stores 1 into the zeroed vis bytes: plain stores, every writer stores
//      the same value.
//   2. vw_combine_kernel: one thread per cell; reads base[c] and writes known[c] of its own cell only (in place is safe).
//   3. vw_gain_kernel: grid (tile slots, candidates), the same ray routine; a wave counts known == 0 and Clear by ballot and
//      popcount over its tiles and adds once into gain[i] (integer atomicAdd; gain was zeroed on the stream before).
// Where occ is read.  Every ray reads its bytes from global memory (L2).  A form that first packed the view's box into a bit
// map in LDS and tested bits there was built and measured: it lost at every size and is not kept.
//
// The walker (views_common.h, shared with sectors.hip) restates section 9's (waypoints.hip) rather than sharing it: that one
// tests d2 >= thr on int32 and divides per column; this one tests bytes and carries quotient and remainder from column to
// column (no division in the loop).  With W, H <= SC_MAX_DIM = 8192 every product fits int32: (2 D + 1) m + D <=
// 2 * 8191^2 + 3 * 8191 < 2^28.
#include "views_common.h"

namespace {

__global__ __launch_bounds__(256) void vw_view_kernel(const uint8_t* __restrict__ occ, const int32_t* __restrict__ views, int W, int H,
                                                      uint8_t* __restrict__ vis) {
    const vw_box b = vw_view_box(occ, views, blockIdx.y, W, H);
    const int cells = W * H;
    for (int t = blockIdx.x; t < b.ntiles; t += gridDim.x) {
        int x, y;
        const int c = vw_target(b, t, W, H, x, y);
        if (c >= 0 && vw_clear(occ, W, cells, b, x, y)) vis[c] = 1;
    }
}

__global__ __launch_bounds__(256) void vw_combine_kernel(const uint8_t* base, const uint8_t* __restrict__ occ, const uint8_t* __restrict__ vis,
                                                         int W, int H, uint8_t* known, uint8_t* occ_seen) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (size_t)W * H) return;
    const int x = (int)(c % W), y = (int)(c / W);
    const uint8_t o = occ[c];
    bool k = (base && base[c] != 0) || vis[c] != 0;
    if (!k && o != 0)
        k = (x > 0 && vis[c - 1]) || (x + 1 < W && vis[c + 1]) || (y > 0 && vis[c - W]) || (y + 1 < H && vis[c + W]);
    known[c] = k ? 1 : 0;
    if (occ_seen) occ_seen[c] = k ? o : 0;
}

__global__ __launch_bounds__(256) void vw_gain_kernel(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ known,
                                                      const int32_t* __restrict__ views, int W, int H, int32_t* __restrict__ gain) {
    const vw_box b = vw_view_box(occ, views, blockIdx.y, W, H);
    const int cells = W * H;
    int n = 0;   // uniform across the wave
    for (int t = blockIdx.x; t < b.ntiles; t += gridDim.x) {
        int x, y;
        const int c = vw_target(b, t, W, H, x, y);
        const bool hit = c >= 0 && known[c] == 0 && vw_clear(occ, W, cells, b, x, y);
        n += __popcll(__ballot(hit));
    }
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(gain + blockIdx.y, n);
}

}  // namespace

// sectors.hip ends its known-space call with the same kernel
int sc_launch_view_combine(sc_ctx* ctx, const uint8_t* base, const uint8_t* occ, const uint8_t* vis, int W, int H, uint8_t* known,
                           uint8_t* occ_seen) {
    const size_t n = (size_t)W * H;
    hipLaunchKernelGGL(vw_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, base, occ, vis, W, H, known, occ_seen);
    return SC_OK;
}

static bool views_args_ok(const sc_ctx* ctx, const uint8_t* occ, const int32_t* views, int R, int W, int H, const uint8_t* known,
                          const uint8_t* occ_seen) {
    return ctx && occ && known && R >= 0 && (views || R == 0) && vw_dims_ok(W, H) && !(occ_seen && (occ_seen == occ || occ_seen == known));
}

static bool gain_args_ok(const sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H,
                         const int32_t* gain) {
    return ctx && occ && known && N >= 0 && ((views && gain) || N == 0) && vw_dims_ok(W, H);
}

extern "C" int sc_known_from_views(sc_ctx* ctx, const uint8_t* base, const uint8_t* occ, const int32_t* views, int R, int W, int H,
                                   uint8_t* known, uint8_t* occ_seen) {
    if (!views_args_ok(ctx, occ, views, R, W, H, known, occ_seen)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    int r = sc_scratch_reserve(ctx, &ctx->vw_vis, al256(n));
    if (r != SC_OK) return r;
    uint8_t* vis = (uint8_t*)ctx->vw_vis.p;
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    SC_HIP(ctx, hipMemsetAsync(vis, 0, n, ctx->stream));
    for (int v0 = 0; v0 < R; v0 += 65535) {   // gridDim.y <= 65535
        const int nv = R - v0 < 65535 ? R - v0 : 65535;
        hipLaunchKernelGGL(vw_view_kernel, dim3(vw_slots(W, H, VW_SLOTS), (unsigned)nv), dim3(256), 0, ctx->stream, occ, views + 3 * (size_t)v0, W,
                           H, vis);
    }
    hipLaunchKernelGGL(vw_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, base, occ, (const uint8_t*)vis, W, H,
                       known, occ_seen);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_view_gain_batch(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H,
                                  int32_t* gain) {
    if (!gain_args_ok(ctx, occ, known, views, N, W, H, gain)) return SC_ERR_INVALID;
    if (N == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    // a few workgroups per candidate when there are few candidates: about 4096 in all, 64 per candidate at most
    const int per = N >= 4096 ? 1 : (4096 / N < 64 ? 4096 / N : 64);
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    SC_HIP(ctx, hipMemsetAsync(gain, 0, (size_t)N * 4, ctx->stream));
    for (int v0 = 0; v0 < N; v0 += 65535) {
        const int nv = N - v0 < 65535 ? N - v0 : 65535;
        hipLaunchKernelGGL(vw_gain_kernel, dim3(vw_slots(W, H, per), (unsigned)nv), dim3(256), 0, ctx->stream, occ, known,
                           views + 3 * (size_t)v0, W, H, gain + v0);
    }
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// ---- host forms ----
extern "C" int sc_known_from_views_host(sc_ctx* ctx, const uint8_t* base, const uint8_t* occ, const int32_t* views, int R, int W, int H,
                                        uint8_t* known, uint8_t* occ_seen) {
    if (!views_args_ok(ctx, occ, views, R, W, H, known, occ_seen)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    sc_stage st(ctx);
    const int i_b = st.in(base, base ? n : 0), i_o = st.in(occ, n), i_v = st.in(views, (size_t)R * 12);
    const int o_k = st.out(known, n), o_s = st.out(occ_seen, occ_seen ? n : 0);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_known_from_views(ctx, base ? st.dev<const uint8_t>(i_b) : nullptr, st.dev<const uint8_t>(i_o), st.dev<const int32_t>(i_v), R, W, H,
                                st.dev<uint8_t>(o_k), occ_seen ? st.dev<uint8_t>(o_s) : nullptr);
    return st.finish(r);
}

extern "C" int sc_view_gain_batch_host(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H,
                                       int32_t* gain) {
    if (!gain_args_ok(ctx, occ, known, views, N, W, H, gain)) return SC_ERR_INVALID;
    if (N == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    sc_stage st(ctx);
    const int i_o = st.in(occ, n), i_k = st.in(known, n), i_v = st.in(views, (size_t)N * 12);
    const int o_g = st.out(gain, (size_t)N * 4);
    int r = st.upload();
    if (r == SC_OK) r = sc_view_gain_batch(ctx, st.dev<const uint8_t>(i_o), st.dev<const uint8_t>(i_k), st.dev<const int32_t>(i_v), N, W, H,
                                           st.dev<int32_t>(o_g));
    return st.finish(r);
}
