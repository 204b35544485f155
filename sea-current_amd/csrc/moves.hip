// moves.hip -- legal-move masks for A* (gfx950): one byte per cell, bit d set where the step in direction d is allowed.
// A cell is traversable where the EDT's d2 (edt.hip) is at least the squared clearance asked for; a diagonal step also
// needs both cells beside it.  Also the clearance penalty of the weighted cost fields (sc_clearance_penalty_u8).
#include "sc_internal.h"

__global__ void __launch_bounds__(256)
moves_kernel(const int32_t* __restrict__ d2, int W, int Hall, int H, int32_t rmin, uint8_t* __restrict__ moves) {
    // Hall = G * H rows: G grids of H rows stacked; a cell's neighbours are looked up inside its own grid only
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int yall = blockIdx.y;
    if (x >= W) return;
    const int y = yall % H;
    const int32_t* r1 = d2 + (size_t)yall * W;
    bool t[3][3];
#pragma unroll
    for (int j = -1; j <= 1; ++j)
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            int xx = x + i, yy = y + j;
            t[j + 1][i + 1] = xx >= 0 && xx < W && yy >= 0 && yy < H && r1[(ptrdiff_t)j * W + xx] >= rmin;
        }
    uint32_t m = 0;
    if (t[1][1]) {
        // d: dx = {1,-1,0,0,1,-1,1,-1}, dy = {0,0,1,-1,1,1,-1,-1}
        m |= (uint32_t)t[1][2] << 0;
        m |= (uint32_t)t[1][0] << 1;
        m |= (uint32_t)t[2][1] << 2;
        m |= (uint32_t)t[0][1] << 3;
        m |= (uint32_t)(t[2][2] && t[1][2] && t[2][1]) << 4;
        m |= (uint32_t)(t[2][0] && t[1][0] && t[2][1]) << 5;
        m |= (uint32_t)(t[0][2] && t[1][2] && t[0][1]) << 6;
        m |= (uint32_t)(t[0][0] && t[1][0] && t[0][1]) << 7;
    }
    moves[(size_t)yall * W + x] = (uint8_t)m;
}

// The same, four cells per thread (W a multiple of 4, rows 16-byte aligned): the three rows come in as 16-byte loads plus
// the two cells beside them, the four masks leave as one dword -- the one-cell form moves 5 B/cell at 0.8 TB/s (a byte per
// thread and store), this one is bound by the d2 reads.
__global__ void __launch_bounds__(256)
moves4_kernel(const int32_t* __restrict__ d2, int W, int Hall, int H, int32_t rmin, uint8_t* __restrict__ moves) {
    const int x = 4 * (blockIdx.x * 256 + threadIdx.x);
    const int yall = blockIdx.y;
    if (x >= W) return;
    const int y = yall % H;
    const int32_t* r1 = d2 + (size_t)yall * W;
    uint32_t t[3] = {0u, 0u, 0u};          // bit i + 1 of t[j + 1]: cell (x + i, y + j) is traversable, i = -1 .. 4
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
        const int yy = y + j;
        if (yy < 0 || yy >= H) continue;
        const int32_t* r = r1 + (ptrdiff_t)j * W;
        const int4 v = *reinterpret_cast<const int4*>(r + x);
        const int32_t l = x > 0 ? r[x - 1] : 0, q = x + 4 < W ? r[x + 4] : 0;      // 0 < rmin: outside the grid is blocked
        t[j + 1] = (uint32_t)(l >= rmin) | (uint32_t)(v.x >= rmin) << 1 | (uint32_t)(v.y >= rmin) << 2 | (uint32_t)(v.z >= rmin) << 3 |
                   (uint32_t)(v.w >= rmin) << 4 | (uint32_t)(q >= rmin) << 5;
    }
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t a = t[0] >> i, c = t[1] >> i, b = t[2] >> i;   // rows y - 1, y, y + 1; bit 0 = x - 1, bit 1 = x, bit 2 = x + 1
        uint32_t m = 0;
        if (c & 2u) {
            // d: dx = {1,-1,0,0,1,-1,1,-1}, dy = {0,0,1,-1,1,1,-1,-1}
            const uint32_t E = (c >> 2) & 1u, Wt = c & 1u, S = (b >> 1) & 1u, N = (a >> 1) & 1u;
            m = E | Wt << 1 | S << 2 | N << 3 | (((b >> 2) & 1u) & E & S) << 4 | ((b & 1u) & Wt & S) << 5 | (((a >> 2) & 1u) & E & N) << 6 |
                ((a & 1u) & Wt & N) << 7;
        }
        out |= m << (8 * i);
    }
    *reinterpret_cast<uint32_t*>(moves + (size_t)yall * W + x) = out;
}

// ... and four rows per thread as well (H a multiple of 4: a block of rows stays inside its grid): six rows read for four
// written instead of twelve.
__global__ void __launch_bounds__(256)
moves4x4_kernel(const int32_t* __restrict__ d2, int W, int Hall, int H, int32_t rmin, uint8_t* __restrict__ moves) {
    const int x = 4 * (blockIdx.x * 256 + threadIdx.x);
    const int yall0 = 4 * blockIdx.y;
    if (x >= W) return;
    const int y0 = yall0 % H;
    const int32_t* r1 = d2 + (size_t)yall0 * W;
    uint32_t t[6];                          // rows y0 - 1 .. y0 + 4; bit i + 1: cell x + i is traversable, i = -1 .. 4
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int yy = y0 + j - 1;
        t[j] = 0u;
        if (yy < 0 || yy >= H) continue;
        const int32_t* r = r1 + (ptrdiff_t)(j - 1) * W;
        const int4 v = *reinterpret_cast<const int4*>(r + x);
        const int32_t l = x > 0 ? r[x - 1] : 0, q = x + 4 < W ? r[x + 4] : 0;
        t[j] = (uint32_t)(l >= rmin) | (uint32_t)(v.x >= rmin) << 1 | (uint32_t)(v.y >= rmin) << 2 | (uint32_t)(v.z >= rmin) << 3 |
               (uint32_t)(v.w >= rmin) << 4 | (uint32_t)(q >= rmin) << 5;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t out = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t a = t[k] >> i, c = t[k + 1] >> i, b = t[k + 2] >> i;
            uint32_t m = 0;
            if (c & 2u) {
                const uint32_t E = (c >> 2) & 1u, Wt = c & 1u, S = (b >> 1) & 1u, N = (a >> 1) & 1u;
                m = E | Wt << 1 | S << 2 | N << 3 | (((b >> 2) & 1u) & E & S) << 4 | ((b & 1u) & Wt & S) << 5 | (((a >> 2) & 1u) & E & N) << 6 |
                    ((a & 1u) & Wt & N) << 7;
            }
            out |= m << (8 * i);
        }
        *reinterpret_cast<uint32_t*>(moves + (size_t)(yall0 + k) * W + x) = out;
    }
}

int sc_launch_moves(sc_ctx* ctx, const int32_t* d2, int W, int Hall, int H, int32_t r2, uint8_t* moves) {
    int32_t rmin = r2 > 1 ? r2 : 1;
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    if (W % 4 == 0 && H % 4 == 0 && ((uintptr_t)d2 & 15) == 0 && ((uintptr_t)moves & 3) == 0)
        hipLaunchKernelGGL(moves4x4_kernel, dim3((W / 4 + 255) / 256, Hall / 4), dim3(256), 0, ctx->stream, d2, W, Hall, H, rmin, moves);
    else if (W % 4 == 0 && ((uintptr_t)d2 & 15) == 0 && ((uintptr_t)moves & 3) == 0)
        hipLaunchKernelGGL(moves4_kernel, dim3((W / 4 + 255) / 256, Hall), dim3(256), 0, ctx->stream, d2, W, Hall, H, rmin, moves);
    else
        hipLaunchKernelGGL(moves_kernel, dim3((W + 255) / 256, Hall), dim3(256), 0, ctx->stream, d2, W, Hall, H, rmin, moves);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_moves_i32_u8(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear, uint8_t* moves) {
    if (!ctx || !d2 || !moves || W <= 0 || H <= 0 || W > SC_MAX_DIM || H > SC_MAX_DIM) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return sc_launch_moves(ctx, d2, W, H, H, r2_clear, moves);
}

// ---- clearance penalty (costmap of sc_cost_field_weighted_batch) ----------------------------------------------------
// exact floor square root: fp64 sqrt is within one of it for v < 2^53, integer compares settle the rest
__host__ __device__ static inline int64_t isqrt64(int64_t v) {
    int64_t r = (int64_t)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// pen = pen_max * (s10 - isqrt(100 d2)) / s10 for thr <= d2 < r2_soft, 0 elsewhere; one thread per cell
__global__ void __launch_bounds__(256)
clearance_penalty_kernel(const int32_t* __restrict__ d2, size_t n, int32_t thr, int32_t r2_soft, int64_t s10, int pen_max,
                         uint8_t* __restrict__ pen) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t d = d2[i];
    uint8_t p = 0;
    if (d >= thr && d < r2_soft) p = (uint8_t)(((int64_t)pen_max * (s10 - isqrt64(100ll * d))) / s10);
    pen[i] = p;
}

extern "C" int sc_clearance_penalty_u8(sc_ctx* ctx, const int32_t* d2, int W, int H, int batch, int32_t r2_clear, int32_t r2_soft,
                                       int pen_max, uint8_t* pen) {
    if (!ctx || !d2 || !pen || W <= 0 || H <= 0 || W > SC_MAX_DIM || H > SC_MAX_DIM || batch <= 0 || pen_max < 0 || pen_max > 255 ||
        r2_soft < 1)
        return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)batch * W * H;
    if ((n + 255) / 256 > 0x7FFFFFFFull) return SC_ERR_INVALID;
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    hipLaunchKernelGGL(clearance_penalty_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d2, n,
                       r2_clear > 1 ? r2_clear : 1, r2_soft, isqrt64(100ll * r2_soft), pen_max, pen);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_clearance_penalty_u8_host(sc_ctx* ctx, const int32_t* d2, int W, int H, int batch, int32_t r2_clear, int32_t r2_soft,
                                            int pen_max, uint8_t* pen) {
    if (!ctx || !d2 || !pen || W <= 0 || H <= 0 || W > SC_MAX_DIM || H > SC_MAX_DIM || batch <= 0 || pen_max < 0 || pen_max > 255 ||
        r2_soft < 1)
        return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)batch * W * H;
    sc_stage st(ctx);
    const int i_d2 = st.in(d2, n * 4), o_pen = st.out(pen, n);
    int r = st.upload();
    if (r == SC_OK) r = sc_clearance_penalty_u8(ctx, st.dev<const int32_t>(i_d2), W, H, batch, r2_clear, r2_soft, pen_max, st.dev<uint8_t>(o_pen));
    return st.finish(r);
}
