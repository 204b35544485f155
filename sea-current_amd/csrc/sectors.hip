// sectors.hip -- sensors with a field of view: the known-space mask of sector views (sc_known_from_sectors), the unknown cells
// a sector pose would see (sc_sector_gain_batch), the gain of every heading of a candidate at the cost of one pass of rays
// (sc_view_gain_headings_batch), and view rows from goal cells (sc_views_from_cells).  DESIGN.md section 27; the definitions
// are in include/sea_current_hip.h.
//
// Definition.  In(d; a, b): the offset d lies in the half-open sector counter-clockwise from direction a (inclusive) to b
// (exclusive); d = 0 and a = b = 0 are true; with s = cross(a, b): s > 0 the two half-planes, s < 0 the complement of the cone
// from b to a, s = 0 and dot < 0 the half-plane of a with the ray of a; anything else is an ignored row.  A sector view sees
// c <=> section 23's vis and In(c - centre; a, b).  Bin b of a heading table u is In(d; u_b, u_{b+1}), d != 0.
//
// Kernels.  The ray routine, the boxes and the tiles are views.hip's (views_common.h); the predicate, a row's box, the tile
// skip and the table live in sectors_common.h, which explore_gain.hip shares.
//   1. vs_view_kernel / vs_gain_kernel: vw_view_kernel / vw_gain_kernel with the predicate on the target.  A workgroup skips a
//      16 x 16 tile when no cell of it can lie in the sector (vs_skip): the four corner offsets lie outside one bounding
//      half-plane (a sector of at most half a turn), or inside the complementary cone (a reflex sector).  Both regions are
//      convex, so the four corners speak for the tile.  The tile that holds the centre is never skipped; the skip is
//      conservative and the predicate alone decides a cell.  sc_known_from_sectors ends with views.hip's vw_combine_kernel.
//   2. vs_hist_kernel: the ray pass of vw_gain_kernel.  A lane that counts finds its bin by halving the table's cones (at most 6
//      steps for 64 bins); the wave takes the first counting lane's bin, ballots the lanes that share it, adds the popcount to
//      the workgroup's LDS histogram and goes on with the rest (an 8 x 8 quarter tile away from the centre spans one to three
//      bins).  At the end the workgroup adds its non-zero bins into hist[i][.], zeroed on the stream: one integer atomicAdd per
//      bin.  The centre's lane stores c0[i] = 1 (one lane of the launch).  The table is a kernel argument, copied to LDS.
//   3. vs_window_kernel: one wave per candidate; the row in LDS, lane h sums its circular window, a butterfly picks the
//      maximum with the smallest heading.
//   4. vs_cells_kernel: one thread per row.
// Every product of the predicate fits int32: components <= 32767, offsets <= 8191, 2 * 32767 * 8191 < 2^30; cross(a, b) and
// dot(a, b) of two table entries reach 2 * 32767^2 < 2^31.
#include "sectors_common.h"

namespace {

__global__ __launch_bounds__(256) void vs_view_kernel(const uint8_t* __restrict__ occ, const int32_t* __restrict__ sviews, int W, int H,
                                                      uint8_t* __restrict__ vis) {
    const vs_sector s = vs_load(sviews, blockIdx.y);
    const vw_box b = vs_view_box(occ, sviews, blockIdx.y, s, W, H);
    const int cells = W * H;
    for (int t = blockIdx.x; t < b.ntiles; t += gridDim.x) {
        if (vs_skip(b, s, t)) continue;
        int x, y;
        const int c = vw_target(b, t, W, H, x, y);
        if (c >= 0 && vs_in(s, x - b.cx, y - b.cy) && vw_clear(occ, W, cells, b, x, y)) vis[c] = 1;
    }
}

__global__ __launch_bounds__(256) void vs_gain_kernel(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ known,
                                                      const int32_t* __restrict__ sviews, int W, int H, int32_t* __restrict__ gain) {
    const vs_sector s = vs_load(sviews, blockIdx.y);
    const vw_box b = vs_view_box(occ, sviews, blockIdx.y, s, W, H);
    const int cells = W * H;
    int n = 0;   // uniform across the wave
    for (int t = blockIdx.x; t < b.ntiles; t += gridDim.x) {
        if (vs_skip(b, s, t)) continue;
        int x, y;
        const int c = vw_target(b, t, W, H, x, y);
        const bool hit = c >= 0 && known[c] == 0 && vs_in(s, x - b.cx, y - b.cy) && vw_clear(occ, W, cells, b, x, y);
        n += __popcll(__ballot(hit));
    }
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(gain + blockIdx.y, n);
}

__global__ __launch_bounds__(256) void vs_hist_kernel(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ known,
                                                      const int32_t* __restrict__ views, int W, int H, const vs_dirs dirs, int B,
                                                      int32_t* __restrict__ hist, int32_t* __restrict__ c0) {
    __shared__ int2 u[SC_VIEW_MAX_BINS];
    __shared__ int lh[SC_VIEW_MAX_BINS];
    if (threadIdx.x < SC_VIEW_MAX_BINS) {
        lh[threadIdx.x] = 0;
        if ((int)threadIdx.x < B) u[threadIdx.x] = make_int2(dirs.u[threadIdx.x][0], dirs.u[threadIdx.x][1]);
    }
    __syncthreads();
    const vw_box b = vw_view_box(occ, views, blockIdx.y, W, H);
    const int cells = W * H;
    const int lane = threadIdx.x & 63;
    for (int t = blockIdx.x; t < b.ntiles; t += gridDim.x) {
        int x, y;
        const int c = vw_target(b, t, W, H, x, y);
        const bool hit = c >= 0 && known[c] == 0 && vw_clear(occ, W, cells, b, x, y);
        const int dx = x - b.cx, dy = y - b.cy;
        const bool centre = dx == 0 && dy == 0;
        if (hit && centre) c0[blockIdx.y] = 1;
        int lo = 0;
        if (hit && !centre) {   // d lies in one of the bins lo .. lo + n - 1; lo + n <= B throughout
            for (int n = B; n > 1;) {
                const int k = n >> 1;
                if (vs_in_cone(u[lo], u[lo + k], dx, dy)) n = k;
                else { lo += k; n -= k; }
            }
        }
        unsigned long long left = __ballot(hit && !centre);
        while (left) {   // uniform across the wave
            const int bin = __shfl(lo, __ffsll((long long)left) - 1);
            const unsigned long long same = left & __ballot(lo == bin);
            if (lane == 0) atomicAdd(&lh[bin], __popcll(same));
            left &= ~same;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < B && lh[threadIdx.x]) atomicAdd(hist + (size_t)blockIdx.y * B + threadIdx.x, lh[threadIdx.x]);
}

// one wave per candidate, four candidates per workgroup
__global__ __launch_bounds__(256) void vs_window_kernel(const int32_t* __restrict__ hist, const int32_t* __restrict__ c0, int N, int B, int span,
                                                        int32_t* __restrict__ gainh, int32_t* __restrict__ best) {
    __shared__ int row[4][SC_VIEW_MAX_BINS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    if (i >= N) return;   // a whole wave; no workgroup barrier below
    if (lane < B) row[wv][lane] = hist[(size_t)i * B + lane];
    wave_lds_sync();
    int g = -1, h = lane;
    if (lane < B) {
        g = c0[i];
        int k = lane;
        for (int j = 0; j < span; ++j) {
            g += row[wv][k];
            k = k + 1 == B ? 0 : k + 1;
        }
        if (gainh) gainh[(size_t)i * B + lane] = g;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int og = __shfl_xor(g, off), oh = __shfl_xor(h, off);
        if (og > g || (og == g && oh < h)) { g = og; h = oh; }
    }
    if (lane == 0) {
        best[2 * (size_t)i] = g;
        best[2 * (size_t)i + 1] = h;
    }
}

__global__ __launch_bounds__(256) void vs_cells_kernel(const int32_t* __restrict__ cell, int N, int W, int H, int32_t r2, int32_t* __restrict__ views) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N) return;
    const int c = cell[i];
    const bool ok = c >= 0 && c < W * H;
    views[3 * i] = ok ? c % W : 0;
    views[3 * i + 1] = ok ? c / W : 0;
    views[3 * i + 2] = ok ? r2 : -1;
}

}  // namespace

static bool sectors_args_ok(const sc_ctx* ctx, const uint8_t* occ, const int32_t* sviews, int R, int W, int H, const uint8_t* known,
                            const uint8_t* occ_seen) {
    return ctx && occ && known && R >= 0 && (sviews || R == 0) && vw_dims_ok(W, H) && !(occ_seen && (occ_seen == occ || occ_seen == known));
}

static bool sector_gain_args_ok(const sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* sviews, int N, int W, int H,
                                const int32_t* gain) {
    return ctx && occ && known && N >= 0 && ((sviews && gain) || N == 0) && vw_dims_ok(W, H);
}

static bool headings_args_ok(const sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H,
                             const int32_t* dirs, int B, int span, const int32_t* best) {
    return ctx && occ && known && N >= 0 && ((views && best) || N == 0) && vw_dims_ok(W, H) && vs_dirs_ok(dirs, B) && span >= 1 && span <= B &&
           (long long)N * B <= (1ll << 30);
}

static bool cells_args_ok(const sc_ctx* ctx, const int32_t* cell, int N, int W, int H, const int32_t* views) {
    return ctx && N >= 0 && ((cell && views) || N == 0) && vw_dims_ok(W, H);
}

extern "C" int sc_known_from_sectors(sc_ctx* ctx, const uint8_t* base, const uint8_t* occ, const int32_t* sviews, int R, int W, int H,
                                     uint8_t* known, uint8_t* occ_seen) {
    if (!sectors_args_ok(ctx, occ, sviews, R, W, H, known, occ_seen)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    int r = sc_scratch_reserve(ctx, &ctx->vw_vis, al256(n));
    if (r != SC_OK) return r;
    uint8_t* vis = (uint8_t*)ctx->vw_vis.p;
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    SC_HIP(ctx, hipMemsetAsync(vis, 0, n, ctx->stream));
    for (int v0 = 0; v0 < R; v0 += 65535) {   // gridDim.y <= 65535
        const int nv = R - v0 < 65535 ? R - v0 : 65535;
        hipLaunchKernelGGL(vs_view_kernel, dim3(vw_slots(W, H, VW_SLOTS), (unsigned)nv), dim3(256), 0, ctx->stream, occ, sviews + 7 * (size_t)v0,
                           W, H, vis);
    }
    sc_launch_view_combine(ctx, base, occ, vis, W, H, known, occ_seen);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// a few workgroups per candidate when there are few candidates: about 4096 in all, 64 per candidate at most
static int vs_per_candidate(int N) { return N >= 4096 ? 1 : (4096 / N < 64 ? 4096 / N : 64); }

extern "C" int sc_sector_gain_batch(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* sviews, int N, int W, int H,
                                    int32_t* gain) {
    if (!sector_gain_args_ok(ctx, occ, known, sviews, N, W, H, gain)) return SC_ERR_INVALID;
    if (N == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const int per = vs_per_candidate(N);
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    SC_HIP(ctx, hipMemsetAsync(gain, 0, (size_t)N * 4, ctx->stream));
    for (int v0 = 0; v0 < N; v0 += 65535) {
        const int nv = N - v0 < 65535 ? N - v0 : 65535;
        hipLaunchKernelGGL(vs_gain_kernel, dim3(vw_slots(W, H, per), (unsigned)nv), dim3(256), 0, ctx->stream, occ, known,
                           sviews + 7 * (size_t)v0, W, H, gain + v0);
    }
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_view_gain_headings_batch(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H,
                                           const int32_t* dirs, int B, int span, int32_t* hist, int32_t* gainh, int32_t* best) {
    if (!headings_args_ok(ctx, occ, known, views, N, W, H, dirs, B, span, best)) return SC_ERR_INVALID;
    if (N == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t c0_bytes = al256((size_t)N * 4), hist_bytes = (size_t)N * B * 4;
    int r = sc_scratch_reserve(ctx, &ctx->vs_state, c0_bytes + (hist ? 0 : al256(hist_bytes)));
    if (r != SC_OK) return r;
    int32_t* c0 = (int32_t*)ctx->vs_state.p;
    if (!hist) hist = (int32_t*)((char*)ctx->vs_state.p + c0_bytes);
    vs_dirs table;
    memset(&table, 0, sizeof table);
    memcpy(table.u, dirs, (size_t)B * 8);
    const int per = vs_per_candidate(N);
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    SC_HIP(ctx, hipMemsetAsync(c0, 0, (size_t)N * 4, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(hist, 0, hist_bytes, ctx->stream));
    for (int v0 = 0; v0 < N; v0 += 65535) {
        const int nv = N - v0 < 65535 ? N - v0 : 65535;
        hipLaunchKernelGGL(vs_hist_kernel, dim3(vw_slots(W, H, per), (unsigned)nv), dim3(256), 0, ctx->stream, occ, known,
                           views + 3 * (size_t)v0, W, H, table, B, hist + (size_t)v0 * B, c0 + v0);
    }
    hipLaunchKernelGGL(vs_window_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, (const int32_t*)hist, (const int32_t*)c0, N, B,
                       span, gainh, best);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_views_from_cells(sc_ctx* ctx, const int32_t* cell, int N, int W, int H, int32_t r2, int32_t* views) {
    if (!cells_args_ok(ctx, cell, N, W, H, views)) return SC_ERR_INVALID;
    if (N == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    hipLaunchKernelGGL(vs_cells_kernel, dim3((unsigned)(((size_t)N + 255) / 256)), dim3(256), 0, ctx->stream, cell, N, W, H, r2, views);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// ---- host forms ----
extern "C" int sc_known_from_sectors_host(sc_ctx* ctx, const uint8_t* base, const uint8_t* occ, const int32_t* sviews, int R, int W, int H,
                                          uint8_t* known, uint8_t* occ_seen) {
    if (!sectors_args_ok(ctx, occ, sviews, R, W, H, known, occ_seen)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    sc_stage st(ctx);
    const int i_b = st.in(base, base ? n : 0), i_o = st.in(occ, n), i_v = st.in(sviews, (size_t)R * 28);
    const int o_k = st.out(known, n), o_s = st.out(occ_seen, occ_seen ? n : 0);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_known_from_sectors(ctx, base ? st.dev<const uint8_t>(i_b) : nullptr, st.dev<const uint8_t>(i_o), st.dev<const int32_t>(i_v), R, W,
                                  H, st.dev<uint8_t>(o_k), occ_seen ? st.dev<uint8_t>(o_s) : nullptr);
    return st.finish(r);
}

extern "C" int sc_sector_gain_batch_host(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* sviews, int N, int W, int H,
                                         int32_t* gain) {
    if (!sector_gain_args_ok(ctx, occ, known, sviews, N, W, H, gain)) return SC_ERR_INVALID;
    if (N == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    sc_stage st(ctx);
    const int i_o = st.in(occ, n), i_k = st.in(known, n), i_v = st.in(sviews, (size_t)N * 28);
    const int o_g = st.out(gain, (size_t)N * 4);
    int r = st.upload();
    if (r == SC_OK) r = sc_sector_gain_batch(ctx, st.dev<const uint8_t>(i_o), st.dev<const uint8_t>(i_k), st.dev<const int32_t>(i_v), N, W, H,
                                             st.dev<int32_t>(o_g));
    return st.finish(r);
}

extern "C" int sc_view_gain_headings_batch_host(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W,
                                                int H, const int32_t* dirs, int B, int span, int32_t* hist, int32_t* gainh, int32_t* best) {
    if (!headings_args_ok(ctx, occ, known, views, N, W, H, dirs, B, span, best)) return SC_ERR_INVALID;
    if (N == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H, nb = (size_t)N * B * 4;
    sc_stage st(ctx);
    const int i_o = st.in(occ, n), i_k = st.in(known, n), i_v = st.in(views, (size_t)N * 12);
    const int o_h = st.out(hist, hist ? nb : 0), o_g = st.out(gainh, gainh ? nb : 0), o_b = st.out(best, (size_t)N * 8);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_view_gain_headings_batch(ctx, st.dev<const uint8_t>(i_o), st.dev<const uint8_t>(i_k), st.dev<const int32_t>(i_v), N, W, H, dirs, B,
                                        span, hist ? st.dev<int32_t>(o_h) : nullptr, gainh ? st.dev<int32_t>(o_g) : nullptr,
                                        st.dev<int32_t>(o_b));
    return st.finish(r);
}

extern "C" int sc_views_from_cells_host(sc_ctx* ctx, const int32_t* cell, int N, int W, int H, int32_t r2, int32_t* views) {
    if (!cells_args_ok(ctx, cell, N, W, H, views)) return SC_ERR_INVALID;
    if (N == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_c = st.in(cell, (size_t)N * 4);
    const int o_v = st.out(views, (size_t)N * 12);
    int r = st.upload();
    if (r == SC_OK) r = sc_views_from_cells(ctx, st.dev<const int32_t>(i_c), N, W, H, r2, st.dev<int32_t>(o_v));
    return st.finish(r);
}
