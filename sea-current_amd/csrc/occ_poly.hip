// occ_poly.hip -- occupancy grids from polygon obstacles (sc_occ_from_polygons): the successor header's host
// occupancy_grid::rasterize (sea_current.hpp), byte for byte, on the device.  The rule is written out in
// include/sea_current_hip.h; DESIGN.md section 11 has the kernel and its measurements.
//
// Built with -ffp-contract=off: every float expression below is the host's, step for step (correctly rounded division,
// the float sqrt as (float)sqrt(double)), so no multiply-add may fuse.
//
// Two launches on the context's stream:
//   prep  one wavefront per obstacle: its box (obs_box, or min/max of its lines) and the range of cell rows it can touch
//         (the fill rows of its box when closed, and cy of both ends of every edge's sample chain).
//   rows  one wavefront per (grid, row), grid-stride: the row lives in LDS, seeded from base or zeros; the wave walks its
//         grid's obstacles 64 at a time, keeps those whose row range holds the row, paints their fill (the crossings of
//         the row's centre line, compacted into LDS, counted per cell) and the samples of their edges that land in the
//         row (a contiguous k range, found by binary search), and stores the row once.
#include "sc_internal.h"

#define OCC_XCAP 1024           // crossings a wave holds in LDS; more are folded into per-cell parity bytes first
#define OCC_MAX_SAMPLES 16777216  // 2^24: the contract's bound on an edge's n (a clamp that only matters outside it)

// clamp((int)floor((v - lo) / res), 0, n - 1), clamped in float before the conversion so that no input converts out of
// range (the same value as the header's int clamp for every input in the contract)
__device__ __forceinline__ int occ_cell(float v, float lo, float res, int n) {
    const float f = floorf((v - lo) / res);
    return (int)fminf(fmaxf(f, 0.0f), (float)(n - 1));
}

__global__ void __launch_bounds__(64)
occ_poly_prep_kernel(const float4* __restrict__ lines, int n_lines, const int32_t* __restrict__ obs_off, int n_obs,
                     const float4* __restrict__ obs_box, const uint8_t* __restrict__ obs_closed, int H, float y_min, float res_y,
                     float4* __restrict__ box_out, int2* __restrict__ rows_out) {
    const int lane = threadIdx.x;
    for (int o = blockIdx.x; o < n_obs; o += gridDim.x) {
        const int e0 = min(max(obs_off[o], 0), n_lines), e1 = min(max(obs_off[o + 1], e0), n_lines);
        float xmax = -INFINITY, xmin = INFINITY, ymax = -INFINITY, ymin = INFINITY;
        int r0 = H, r1 = -1;
        for (int e = e0 + lane; e < e1; e += 64) {
            const float4 l = lines[e];
            xmax = fmaxf(xmax, fmaxf(l.x, l.z)); xmin = fminf(xmin, fminf(l.x, l.z));
            ymax = fmaxf(ymax, fmaxf(l.y, l.w)); ymin = fminf(ymin, fminf(l.y, l.w));
            // the edge's samples run from y(0) = a.y to y(n) = a.y + dy (not always b.y in float); cy is monotone in k
            const int ra = occ_cell(l.y, y_min, res_y, H), rb = occ_cell(l.y + (l.w - l.y), y_min, res_y, H);
            r0 = min(r0, min(ra, rb));
            r1 = max(r1, max(ra, rb));
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            xmax = fmaxf(xmax, __shfl_xor(xmax, s)); xmin = fminf(xmin, __shfl_xor(xmin, s));
            ymax = fmaxf(ymax, __shfl_xor(ymax, s)); ymin = fminf(ymin, __shfl_xor(ymin, s));
            r0 = min(r0, __shfl_xor(r0, s)); r1 = max(r1, __shfl_xor(r1, s));
        }
        const float4 B = obs_box ? obs_box[o] : make_float4(xmax, xmin, ymax, ymin);   // bound_rect order
        if (e1 > e0 && (!obs_closed || obs_closed[o])) {
            r0 = min(r0, occ_cell(B.w, y_min, res_y, H));
            r1 = max(r1, occ_cell(B.z, y_min, res_y, H));
        }
        if (e1 <= e0) { r0 = H; r1 = -1; }   // no edges: skipped
        if (lane == 0) {
            box_out[o] = B;
            rows_out[o] = make_int2(r0, r1);
        }
    }
}

__global__ void __launch_bounds__(64)
occ_poly_rows_kernel(const uint8_t* base, int G, int W, int H, float x_min, float y_min, float res_x, float res_y,
                     const float4* __restrict__ lines, int n_lines, const int32_t* __restrict__ obs_off, int n_obs,
                     const uint8_t* __restrict__ obs_closed, const int32_t* __restrict__ grid_off, const float4* __restrict__ box,
                     const int2* __restrict__ rows, uint8_t* occ) {
    extern __shared__ __align__(16) uint8_t occ_smem[];
    const int Wp = (W + 15) & ~15;
    uint8_t* row = occ_smem;                               // [Wp] the row being painted
    uint8_t* par = occ_smem + Wp;                          // [Wp] crossing parity of cells, when a row has > OCC_XCAP crossings
    float* xs = reinterpret_cast<float*>(occ_smem + 2 * Wp);   // [OCC_XCAP] crossings of the row's centre line
    const int lane = threadIdx.x;
    const uint64_t lt = (1ull << lane) - 1ull;
    const float hstep = 0.5f * (res_y < res_x ? res_y : res_x);
    const bool w4 = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(occ) | reinterpret_cast<uintptr_t>(base)) & 3) == 0;
    const int64_t nrows = (int64_t)G * H;
    for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int g = (int)(r / H), iy = (int)(r % H);
        const size_t ro = (size_t)r * W;
        if (w4) {
            for (int x = lane; x < W / 4; x += 64)
                reinterpret_cast<uint32_t*>(row)[x] = base ? reinterpret_cast<const uint32_t*>(base + ro)[x] : 0u;
        } else {
            for (int x = lane; x < W; x += 64) row[x] = base ? base[ro + x] : (uint8_t)0;
        }
        __syncthreads();
        const float py = y_min + ((float)iy + 0.5f) * res_y;
        const int ob0 = grid_off ? min(max(grid_off[g], 0), n_obs) : 0;
        const int ob1 = grid_off ? min(max(grid_off[g + 1], ob0), n_obs) : n_obs;
        for (int oc = ob0; oc < ob1; oc += 64) {
            bool hit = false;
            if (oc + lane < ob1) {
                const int2 rr = rows[oc + lane];
                hit = rr.x <= iy && iy <= rr.y;
            }
            uint64_t om = __ballot(hit);
            while (om) {
                const int o = oc + __ffsll((long long)om) - 1;
                om &= om - 1;
                const int e0 = min(max(obs_off[o], 0), n_lines), e1 = min(max(obs_off[o + 1], e0), n_lines);
                const float4 B = box[o];   // x_max, x_min, y_max, y_min
                const bool fill = (!obs_closed || obs_closed[o]) && iy >= occ_cell(B.w, y_min, res_y, H) &&
                                  iy <= occ_cell(B.z, y_min, res_y, H) && py <= B.z && py >= B.w;
                const int ix0 = occ_cell(B.y, x_min, res_x, W), ix1 = occ_cell(B.x, x_min, res_x, W);
                int nx = 0;
                bool folded = false;
                // count the crossings right of each cell centre of ix0 .. ix1; the parity of the count so far goes to `par`
                // (fin == false) or, on the last pass, the cells inside are set (fin == true)
                auto fold = [&](bool fin) {
                    __syncthreads();
                    for (int x = ix0 + lane; x <= ix1; x += 64) {
                        const float px = x_min + ((float)x + 0.5f) * res_x;
                        int c = 0;
                        for (int i = 0; i < nx; ++i) c += px < xs[i];
                        const int p = (c & 1) ^ (folded ? par[x] : 0);
                        if (!fin) par[x] = (uint8_t)p;
                        else if (p && px <= B.x && px >= B.y) row[x] = 1;
                    }
                    __syncthreads();
                };
                for (int c = e0; c < e1; c += 64) {
                    const int e = c + lane;
                    const bool v = e < e1;
                    const float4 l = v ? lines[e] : make_float4(0.f, 0.f, 0.f, 0.f);
                    if (fill) {
                        const bool cr = v && ((l.y > py) != (l.w > py));
                        float xi = 0.f;
                        if (cr) xi = l.x + (py - l.y) * (l.z - l.x) / (l.w - l.y);
                        const uint64_t cm = __ballot(cr);
                        const int cnt = __popcll(cm);
                        if (nx + cnt > OCC_XCAP) { fold(false); folded = true; nx = 0; }
                        if (cr) xs[nx + __popcll(cm & lt)] = xi;
                        nx += cnt;
                    }
                    const int ra = occ_cell(l.y, y_min, res_y, H), rb = occ_cell(l.y + (l.w - l.y), y_min, res_y, H);
                    uint64_t em = __ballot(v && min(ra, rb) <= iy && iy <= max(ra, rb));
                    while (em) {
                        const int j = __ffsll((long long)em) - 1;
                        em &= em - 1;
                        const float4 q = lines[c + j];
                        const float ax = q.x, ay = q.y, dx = q.z - q.x, dy = q.w - q.y;
                        const float s2 = dx * dx + dy * dy;
                        const float len = (float)sqrt((double)s2);
                        const int n = (int)fminf(fmaxf(ceilf(len / hstep), 1.0f), (float)OCC_MAX_SAMPLES);
                        const float fn = (float)n;
                        const bool up = !(dy < 0.f);
                        // first k in [from, n] whose row is at or past `target` in the edge's direction (n + 1: none)
                        auto first_at = [&](int from, int target) {
                            int lo = from, hi = n + 1;
                            while (lo < hi) {
                                const int mid = (lo + hi) >> 1;
                                const int rk = occ_cell(ay + dy * ((float)mid / fn), y_min, res_y, H);
                                if (up ? rk >= target : rk <= target) hi = mid;
                                else lo = mid + 1;
                            }
                            return lo;
                        };
                        const int k0 = first_at(0, iy), k1 = first_at(k0, up ? iy + 1 : iy - 1);
                        for (int k = k0 + lane; k < k1; k += 64)
                            row[occ_cell(ax + dx * ((float)k / fn), x_min, res_x, W)] = 1;
                    }
                }
                if (fill) fold(true);
            }
        }
        __syncthreads();
        if (w4) {
            for (int x = lane; x < W / 4; x += 64) reinterpret_cast<uint32_t*>(occ + ro)[x] = reinterpret_cast<const uint32_t*>(row)[x];
        } else {
            for (int x = lane; x < W; x += 64) occ[ro + x] = row[x];
        }
        __syncthreads();
    }
}

static bool occ_args_ok(sc_ctx* ctx, int G, int W, int H, float x_min, float y_min, float res_x, float res_y, const float* lines,
                        int n_lines, const int32_t* obs_off, int n_obs, const int32_t* grid_off, const uint8_t* occ) {
    return ctx && occ && G >= 1 && G <= 65535 && W > 0 && H > 0 && W <= SC_MAX_DIM && H <= SC_MAX_DIM && n_lines >= 0 &&
           n_obs >= 0 && (n_lines == 0 || lines) && (n_obs == 0 || obs_off) && (G == 1 || grid_off) && std::isfinite(x_min) &&
           std::isfinite(y_min) && std::isfinite(res_x) && std::isfinite(res_y) && res_x > 0.f && res_y > 0.f;
}

extern "C" int sc_occ_from_polygons(sc_ctx* ctx, const uint8_t* base, int G, int W, int H, float x_min, float y_min, float res_x,
                                    float res_y, const float* lines, int n_lines, const int32_t* obs_off, int n_obs, const float* obs_box,
                                    const uint8_t* obs_closed, const int32_t* grid_off, uint8_t* occ) {
    if (!occ_args_ok(ctx, G, W, H, x_min, y_min, res_x, res_y, lines, n_lines, obs_off, n_obs, grid_off, occ)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (n_obs > 0) {
        const int r = sc_scratch_reserve(ctx, &ctx->occ_prep, al256((size_t)n_obs * 16) + (size_t)n_obs * 8);
        if (r != SC_OK) return r;
    }
    float4* pbox = (float4*)ctx->occ_prep.p;
    int2* prow = n_obs > 0 ? (int2*)((char*)ctx->occ_prep.p + al256((size_t)n_obs * 16)) : nullptr;
    int tk = sc_time_begin(ctx, SC_K_OCC);
    if (n_obs > 0)
        hipLaunchKernelGGL(occ_poly_prep_kernel, dim3((unsigned)min(n_obs, 65536)), dim3(64), 0, ctx->stream, (const float4*)lines,
                           n_lines, obs_off, n_obs, (const float4*)obs_box, obs_closed, H, y_min, res_y, pbox, prow);
    const int64_t nrows = (int64_t)G * H;
    const size_t lds = 2 * (size_t)((W + 15) & ~15) + 4 * OCC_XCAP;
    hipLaunchKernelGGL(occ_poly_rows_kernel, dim3((unsigned)std::min<int64_t>(nrows, 16384)), dim3(64), lds, ctx->stream, base, G, W, H, x_min,
                       y_min, res_x, res_y, (const float4*)lines, n_lines, obs_off, n_obs, obs_closed, grid_off, (const float4*)pbox, prow,
                       occ);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// the contract of the header comment, on host data: offsets in order, coordinates finite, cell coordinates within 2^30,
// every edge's sample count within 2^24
static bool occ_contract_ok(int G, int W, int H, float x_min, float y_min, float res_x, float res_y, const float* lines, int n_lines,
                            const int32_t* obs_off, int n_obs, const float* obs_box, const int32_t* grid_off) {
    const float lim = 1073741824.0f;
    auto in_x = [&](float v) { const float c = (v - x_min) / res_x; return std::isfinite(v) && c >= -lim && c <= lim; };
    auto in_y = [&](float v) { const float c = (v - y_min) / res_y; return std::isfinite(v) && c >= -lim && c <= lim; };
    if (n_obs > 0) {
        if (obs_off[0] < 0) return false;
        for (int o = 0; o < n_obs; ++o)
            if (obs_off[o + 1] < obs_off[o]) return false;
        if (obs_off[n_obs] > n_lines) return false;
    }
    if (grid_off) {
        if (grid_off[0] < 0 || grid_off[G] > n_obs) return false;
        for (int g = 0; g < G; ++g)
            if (grid_off[g + 1] < grid_off[g]) return false;
    }
    const float hstep = 0.5f * (res_y < res_x ? res_y : res_x);
    for (int e = 0; e < n_lines; ++e) {
        const float* l = lines + 4 * (size_t)e;
        if (!in_x(l[0]) || !in_y(l[1]) || !in_x(l[2]) || !in_y(l[3])) return false;
        const float dx = l[2] - l[0], dy = l[3] - l[1];
        const float s2 = dx * dx + dy * dy;
        const float q = std::ceil((float)std::sqrt((double)s2) / hstep);
        if (!(q <= (float)OCC_MAX_SAMPLES)) return false;
    }
    if (obs_box)
        for (int o = 0; o < n_obs; ++o) {
            const float* b = obs_box + 4 * (size_t)o;
            if (!in_x(b[0]) || !in_x(b[1]) || !in_y(b[2]) || !in_y(b[3])) return false;
        }
    return true;
}

extern "C" int sc_occ_from_polygons_host(sc_ctx* ctx, const uint8_t* base, int G, int W, int H, float x_min, float y_min, float res_x,
                                         float res_y, const float* lines, int n_lines, const int32_t* obs_off, int n_obs, const float* obs_box,
                                         const uint8_t* obs_closed, const int32_t* grid_off, uint8_t* occ) {
    if (!occ_args_ok(ctx, G, W, H, x_min, y_min, res_x, res_y, lines, n_lines, obs_off, n_obs, grid_off, occ) ||
        !occ_contract_ok(G, W, H, x_min, y_min, res_x, res_y, lines, n_lines, obs_off, n_obs, obs_box, grid_off))
        return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)G * H * W;
    const bool obs = n_obs > 0;
    sc_stage st(ctx);
    const int io_occ = st.in(base, cells), i_l = st.in(lines, (size_t)n_lines * 16), i_off = st.in(obs_off, obs ? (size_t)(n_obs + 1) * 4 : 0),
              i_box = st.in(obs_box, (size_t)n_obs * 16), i_cl = st.in(obs_closed, (size_t)n_obs), i_g = st.in(grid_off, (size_t)(G + 1) * 4);
    st.back(io_occ, occ, cells);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_occ_from_polygons(ctx, base ? st.dev<const uint8_t>(io_occ) : nullptr, G, W, H, x_min, y_min, res_x, res_y,
                                 n_lines > 0 ? st.dev<const float>(i_l) : nullptr, n_lines, obs ? st.dev<const int32_t>(i_off) : nullptr, n_obs,
                                 obs && obs_box ? st.dev<const float>(i_box) : nullptr, obs && obs_closed ? st.dev<const uint8_t>(i_cl) : nullptr,
                                 grid_off ? st.dev<const int32_t>(i_g) : nullptr, st.dev<uint8_t>(io_occ));
    return st.finish(r);
}
