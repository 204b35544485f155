// scan.hip -- occupancy from range scans: the simulated range sensor (sc_scan_cast_batch) and the clamped log-odds map update
// from beams (sc_logodds_update).  DESIGN.md section 24; the definitions are in include/sea_current_hip.h, the walk in
// ray_walk.h.
//
// Kernels.  One ray per beam; nothing loops over beams per grid cell.
//   1. sn_cast_kernel: one lane per ray.  Consecutive rays of a scan have nearly the same direction and length, so a wave
//      lives and dies together.  A round issues the loads of SN_COLS columns (three rows each) before any test, then tests
//      them in sequence order: the walk is ordered, the first occupied cell is the answer and a cell outside the grid ends
//      the walk, so the bytes of a round cannot be OR-ed as views.hip does.
//   2. sn_mark_kernel: one lane per beam, the same walk cell by cell.  Plain stores of 1 into a zeroed miss byte map and a
//      zeroed hit byte map: every writer stores the same value, so no atomics are needed; two maps because a hit and a miss of
//      one cell by two beams would otherwise race for one byte.
//   3. sn_combine_kernel: one thread per cell: L and the two flags -> Lout, occ_est, known.  It clears the two flags it read,
//      so the maps are all zero again when the call's work is done and the next call needs no memset (a memset per call was
//      measured beside this and lost: DESIGN.md section 24.4).
#include "ray_walk.h"
#include "sc_internal.h"

namespace {

constexpr int SN_COLS = 4;   // columns whose loads are in flight together

// ray k as four 4-byte loads: rays is int32 [N][4] and promises no more than the alignment of an int32
struct sn_ray { int ax, ay, bx, by; };
__device__ __forceinline__ sn_ray sn_load_ray(const int32_t* __restrict__ rays, size_t k) {
    return {rays[4 * k], rays[4 * k + 1], rays[4 * k + 2], rays[4 * k + 3]};
}

__global__ __launch_bounds__(256) void sn_cast_kernel(const uint8_t* __restrict__ occ, const int32_t* __restrict__ rays, int N, int W, int H,
                                                      int32_t* __restrict__ hit) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;   // the launch has ceil(N / 256) workgroups: one ray per lane
    if (k >= (size_t)N) return;
    const sn_ray ry = sn_load_ray(rays, k);
    int res = SC_SCAN_IGNORED;
    if (rw_ray_ok(ry.ax, ry.ay, ry.bx, ry.by, W, H) && occ[ry.ay * W + ry.ax] == 0) {
        rw_walk w;
        w.init(ry.ax, ry.ay, ry.bx, ry.by);
        res = SC_SCAN_NO_RETURN;
        bool done = false;
        while (!done && !w.finished()) {
            // code: the cell, -1 for a row the column does not have, -2 for a cell outside the grid (never loaded)
            int code[SN_COLS][3];
            uint32_t v[SN_COLS][3];
#pragma unroll
            for (int c = 0; c < SN_COLS; ++c) {
                const bool live = !w.finished();
                const int rhi = w.rhi();
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    int x, y;
                    w.cell(w.rlo + r, x, y);
                    const bool in = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
                    code[c][r] = !(live && w.rlo + r <= rhi) ? -1 : in ? y * W + x : -2;
                    v[c][r] = code[c][r] >= 0 ? occ[code[c][r]] : 0u;
                }
                w.next();
            }
#pragma unroll
            for (int c = 0; c < SN_COLS; ++c)
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    if (!done) {
                        if (code[c][r] == -2) done = true;
                        else if (code[c][r] >= 0 && v[c][r] != 0) { res = code[c][r]; done = true; }
                    }
        }
    }
    hit[k] = res;
}

__global__ __launch_bounds__(256) void sn_mark_kernel(const int32_t* __restrict__ rays, const int32_t* __restrict__ hit, int N, int W, int H,
                                                      uint8_t* __restrict__ miss, uint8_t* __restrict__ hitmap) {
    const int cells = W * H;
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (size_t)N) return;
    const sn_ray ry = sn_load_ray(rays, k);
    const int h = hit[k];
    if (!rw_ray_ok(ry.ax, ry.ay, ry.bx, ry.by, W, H) || h < SC_SCAN_NO_RETURN || h >= cells) return;   // ignored
    if (h >= 0) hitmap[h] = 1;
    // every cell is inside the grid when it is stored to: rw_each ends the walk at the first one that is not
    rw_each(ry.ax, ry.ay, ry.bx, ry.by, W, H, [&](int c) {
        if (c == h) return false;
        miss[c] = 1;
        return true;
    });
}

__global__ __launch_bounds__(256) void sn_combine_kernel(const int32_t* L, uint8_t* __restrict__ miss, uint8_t* __restrict__ hitmap, int cells,
                                                         int32_t l_hit, int32_t l_miss, int32_t l_clamp, int32_t t_occ, int32_t t_free,
                                                         int32_t* Lout, uint8_t* __restrict__ occ_est, uint8_t* __restrict__ known) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (size_t)cells) return;
    const uint8_t mi = miss[c], hi = hitmap[c];
    long long l = L ? L[c] : 0;
    l += hi ? (long long)l_hit : mi ? -(long long)l_miss : 0;
    const int32_t o = (int32_t)(l < -(long long)l_clamp ? -(long long)l_clamp : l > l_clamp ? (long long)l_clamp : l);
    Lout[c] = o;
    if (occ_est) occ_est[c] = o >= t_occ ? 1 : 0;
    if (known) known[c] = (o >= t_occ || o <= -t_free) ? 1 : 0;
    if (mi) miss[c] = 0;
    if (hi) hitmap[c] = 0;
}

}  // namespace

static bool sn_dims_ok(int W, int H) { return W >= 1 && W <= SC_MAX_DIM && H >= 1 && H <= SC_MAX_DIM; }

static bool cast_args_ok(const sc_ctx* ctx, const uint8_t* occ, const int32_t* rays, int N, int W, int H, const int32_t* hit) {
    return ctx && occ && hit && N >= 0 && (rays || N == 0) && sn_dims_ok(W, H);
}

static bool update_args_ok(const sc_ctx* ctx, const int32_t* L, const int32_t* rays, const int32_t* hit, int N, int W, int H, int32_t l_hit,
                           int32_t l_miss, int32_t l_clamp, int32_t t_occ, int32_t t_free, const int32_t* Lout, const uint8_t* occ_est,
                           const uint8_t* known) {
    if (!ctx || !Lout || N < 0 || ((!rays || !hit) && N > 0) || !sn_dims_ok(W, H)) return false;
    if (l_hit < 0 || l_miss < 0 || l_clamp < 0 || l_clamp > (1 << 30) || t_occ < 1 || t_free < 1) return false;
    const void *e = occ_est, *k = known;
    if (e && (e == k || e == (const void*)L || e == (const void*)Lout)) return false;
    if (k && (k == (const void*)L || k == (const void*)Lout)) return false;
    return true;
}

// one lane per beam: ceil(N / 256) workgroups, at most 2^23 for an int N, which a grid dimension holds
static unsigned sn_beam_blocks(int N) { return (unsigned)(((size_t)N + 255) / 256); }

extern "C" int sc_scan_cast_batch(sc_ctx* ctx, const uint8_t* occ, const int32_t* rays, int N, int W, int H, int32_t* hit) {
    if (!cast_args_ok(ctx, occ, rays, N, W, H, hit)) return SC_ERR_INVALID;
    if (N == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    hipLaunchKernelGGL(sn_cast_kernel, dim3(sn_beam_blocks(N)), dim3(256), 0, ctx->stream, occ, rays, N, W, H, hit);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_logodds_update(sc_ctx* ctx, const int32_t* L, const int32_t* rays, const int32_t* hit, int N, int W, int H, int32_t l_hit,
                                 int32_t l_miss, int32_t l_clamp, int32_t t_occ, int32_t t_free, int32_t* Lout, uint8_t* occ_est,
                                 uint8_t* known) {
    if (!update_args_ok(ctx, L, rays, hit, N, W, H, l_hit, l_miss, l_clamp, t_occ, t_free, Lout, occ_est, known)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H, stride = al256(n);
    // the two flag maps: miss at 0, hit at stride.  A buffer that has just been allocated is zeroed once (sn_flags_zeroed says
    // that this memset was enqueued; one that failed is tried again by the next call); after that the combine pass leaves
    // every byte it read zero again, and a call only ever sets bytes its own combine pass reads.
    const void* before = ctx->sn_flags.p;
    const size_t before_bytes = ctx->sn_flags.bytes;
    int r = sc_scratch_reserve(ctx, &ctx->sn_flags, 2 * stride);
    if (r != SC_OK) return r;
    uint8_t *miss = (uint8_t*)ctx->sn_flags.p, *hitmap = miss + stride;
    if (ctx->sn_flags.p != before || ctx->sn_flags.bytes != before_bytes) ctx->sn_flags_zeroed = false;
    if (!ctx->sn_flags_zeroed) {
        SC_HIP(ctx, hipMemsetAsync(ctx->sn_flags.p, 0, ctx->sn_flags.bytes, ctx->stream));
        ctx->sn_flags_zeroed = true;
    }
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    if (N > 0) hipLaunchKernelGGL(sn_mark_kernel, dim3(sn_beam_blocks(N)), dim3(256), 0, ctx->stream, rays, hit, N, W, H, miss, hitmap);
    hipLaunchKernelGGL(sn_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, L, miss, hitmap, (int)n, l_hit, l_miss,
                       l_clamp, t_occ, t_free, Lout, occ_est, known);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// ---- host forms ----
extern "C" int sc_scan_cast_batch_host(sc_ctx* ctx, const uint8_t* occ, const int32_t* rays, int N, int W, int H, int32_t* hit) {
    if (!cast_args_ok(ctx, occ, rays, N, W, H, hit)) return SC_ERR_INVALID;
    if (N == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_o = st.in(occ, (size_t)W * H), i_r = st.in(rays, (size_t)N * 16);
    const int o_h = st.out(hit, (size_t)N * 4);
    int r = st.upload();
    if (r == SC_OK) r = sc_scan_cast_batch(ctx, st.dev<const uint8_t>(i_o), st.dev<const int32_t>(i_r), N, W, H, st.dev<int32_t>(o_h));
    return st.finish(r);
}

extern "C" int sc_logodds_update_host(sc_ctx* ctx, const int32_t* L, const int32_t* rays, const int32_t* hit, int N, int W, int H,
                                      int32_t l_hit, int32_t l_miss, int32_t l_clamp, int32_t t_occ, int32_t t_free, int32_t* Lout,
                                      uint8_t* occ_est, uint8_t* known) {
    if (!update_args_ok(ctx, L, rays, hit, N, W, H, l_hit, l_miss, l_clamp, t_occ, t_free, Lout, occ_est, known)) return SC_ERR_INVALID;
    const size_t n = (size_t)W * H;
    for (int k = 0; k < N; ++k)
        if (hit[k] < SC_SCAN_IGNORED || (int64_t)hit[k] >= (int64_t)n) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_l = st.in(L, L ? n * 4 : 0), i_r = st.in(rays, (size_t)N * 16), i_h = st.in(hit, (size_t)N * 4);
    const int o_l = st.out(Lout, n * 4), o_e = st.out(occ_est, occ_est ? n : 0), o_k = st.out(known, known ? n : 0);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_logodds_update(ctx, L ? st.dev<const int32_t>(i_l) : nullptr, st.dev<const int32_t>(i_r), st.dev<const int32_t>(i_h), N, W, H, l_hit,
                              l_miss, l_clamp, t_occ, t_free, st.dev<int32_t>(o_l), occ_est ? st.dev<uint8_t>(o_e) : nullptr,
                              known ? st.dev<uint8_t>(o_k) : nullptr);
    return st.finish(r);
}
