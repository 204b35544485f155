// smooth.hip -- the post-planner sequence of the reference's service (examples/zmq_test.cpp:66-93) for P paths in one
// call: from_path -> arclength -> gen_vel_prof<1> along the arclength -> resample(nudge) -> angular velocity.
//
// The numerical work is done by the library's own kernels (bezier.hip, toppra.hip), so every value is the one those
// entry points give on the same inputs.  What this file adds is the bookkeeping between them, on the device: checks of
// the input, the scan of the legs and the compaction of the control points, the per-path arclength sum and TOPP-RA
// inputs, the sample counts with their scan and the capacity test, and the angular velocity.  Nothing is read back:
// launches are sized by P, P*(n_max-1) and the sample capacity, and kernels read the real counts on the device.
//
// Compiled with -ffp-contract=off: sc_cells_to_points_batch must give occupancy_grid::centre_of's float32 bits.
#include "sc_internal.h"

#include <math.h>

#define SM_THREADS 1024   // the one-workgroup scans: P <= SC_SMOOTH_MAX_PATHS, at most 64 paths per thread

// exclusive scan of one value per thread over the workgroup; *total = the sum of all
__device__ __forceinline__ long long block_exscan(long long v, long long* total) {
    __shared__ long long s_w[SM_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    long long base = 0, tot = 0;
    for (int w = 0; w < SM_THREADS / 64; ++w) { if (w < wave) base += s_w[w]; tot += s_w[w]; }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

// 1a. input checks, one wavefront per path: npts_eff[p] = npts[p] if the path is usable, else 0 (from_path then writes
//     zeros for it); status BAD_INPUT / OK
__global__ void __launch_bounds__(256)
smooth_check_kernel(const float* __restrict__ path, const int32_t* __restrict__ npts, int P, int n_max, int32_t* __restrict__ npts_eff,
                    int32_t* __restrict__ status) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= P) return;   // wave-uniform
    const int n = npts[p];
    bool ok = n >= 2 && n <= n_max;
    if (ok) {
        const float* w = path + (size_t)p * n_max * 2;
        bool bad = false;
        for (int i = lane; i < 2 * n; i += 64) bad |= !isfinite(w[i]);
        ok = __ballot(bad) == 0ull;
    }
    if (lane == 0) { npts_eff[p] = ok ? n : 0; status[p] = ok ? SC_SMOOTH_OK : SC_SMOOTH_BAD_INPUT; }
}

// 1b. the scan of the legs: seg_off [P+1]
__global__ void __launch_bounds__(SM_THREADS)
smooth_seg_scan_kernel(const int32_t* __restrict__ npts_eff, int P, int32_t* __restrict__ seg_off) {
    const int c = (P + SM_THREADS - 1) / SM_THREADS;
    const int p0 = min(P, (int)threadIdx.x * c), p1 = min(P, p0 + c);
    long long sum = 0;
    for (int p = p0; p < p1; ++p) { const int n = npts_eff[p]; sum += n > 0 ? n - 1 : 0; }
    long long tot;
    long long base = block_exscan(sum, &tot);
    for (int p = p0; p < p1; ++p) {
        seg_off[p] = (int32_t)base;
        const int n = npts_eff[p];
        base += n > 0 ? n - 1 : 0;
    }
    if (threadIdx.x == 0) seg_off[P] = (int32_t)tot;
}

// 2. from_path's [P][n_max-1] control points -> the legs back to back, one thread per (path, leg)
__global__ void __launch_bounds__(256)
smooth_compact_kernel(const float* __restrict__ padded, const int32_t* __restrict__ npts_eff, const int32_t* __restrict__ seg_off, int P,
                      int n_max, float* __restrict__ ctrl) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)P * (n_max - 1)) return;
    const int p = (int)(gid / (n_max - 1)), i = (int)(gid % (n_max - 1));
    if (i >= npts_eff[p] - 1) return;
    const float* src = padded + (size_t)gid * 8;
    float* dst = ctrl + ((size_t)seg_off[p] + i) * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = src[k];
}

// 3. per path, one wavefront: arclength = the float32 sum of the legs in leg order (bezier_spline::arclength; the lanes
//    load, the sum runs through the loaded values one by one), NONFINITE, and the TOPP-RA inputs of
//    gen_vel_prof<1>(arclength, 0, 0, 0, limits); paths already failed get a harmless problem
__global__ void __launch_bounds__(256)
smooth_toppra_inputs_kernel(const float* __restrict__ ctrl, const float* __restrict__ seg_len, const int32_t* __restrict__ seg_off,
                            const double* __restrict__ limits, int P, int32_t* __restrict__ status, float* __restrict__ arclength,
                            double* __restrict__ tp) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= P) return;   // wave-uniform
    int st = status[p];
    float AL = 0.f;
    if (st == SC_SMOOTH_OK) {
        const int s0 = seg_off[p], ns = seg_off[p + 1] - s0;
        for (int base = 0; base < ns; base += 64) {
            const float v = base + lane < ns ? seg_len[s0 + base + lane] : 0.f;
            const int m = min(64, ns - base);
            for (int j = 0; j < m; ++j) {
                const float x = __shfl(v, j);
                AL = (base == 0 && j == 0) ? x : AL + x;
            }
        }
        bool bad = false;
        const float* c = ctrl + (size_t)s0 * 8;
        for (int k = lane; k < 8 * ns; k += 64) bad |= !isfinite(c[k]);
        if (__ballot(bad) != 0ull || !isfinite(AL)) st = SC_SMOOTH_NONFINITE;
        if (lane == 0) status[p] = st;
    }
    if (lane != 0) return;
    arclength[p] = AL;
    const bool ok = st == SC_SMOOTH_OK;
    tp[p] = 0.0;                                          // p0
    tp[(size_t)P + p] = ok ? (double)AL : 1.0;            // p1
    tp[(size_t)2 * P + p] = 0.0;                          // v0
    tp[(size_t)3 * P + p] = 0.0;                          // v1
    tp[(size_t)4 * P + p] = ok ? limits[4 * (size_t)p] : -1.0;       // vel_min
    tp[(size_t)5 * P + p] = ok ? limits[4 * (size_t)p + 1] : 1.0;    // vel_max
    tp[(size_t)6 * P + p] = ok ? limits[4 * (size_t)p + 2] : -1.0;   // acc_min
    tp[(size_t)7 * P + p] = ok ? limits[4 * (size_t)p + 3] : 1.0;    // acc_max
}

// 4. sample counts by the sampler's rule (toppra_sample_kernel: knots whose time increment is below 1e-8 are dropped,
//    T = the time of the last knot kept, length = ceil(T / dt)), their scan, the capacity test; roff = offsets with the
//    slots of truncated paths emptied (what the resample reads)
#define SM_NEARLY_ZERO 1e-8   // TP_NEARLY_ZERO of toppra.hip
__global__ void __launch_bounds__(SM_THREADS)
smooth_count_scan_kernel(const double* __restrict__ t, const int32_t* __restrict__ tstat, int P, int N, double dt, long long cap,
                         int32_t* __restrict__ status, int32_t* __restrict__ length, int32_t* __restrict__ offsets,
                         int32_t* __restrict__ roff, int64_t* __restrict__ needed) {
    __shared__ int s_first;   // offset of the first truncated path
    if (threadIdx.x == 0) s_first = INT32_MAX;
    const int c = (P + SM_THREADS - 1) / SM_THREADS;
    const int p0 = min(P, (int)threadIdx.x * c), p1 = min(P, p0 + c);
    long long sum = 0;
    for (int p = p0; p < p1; ++p) {
        int st = status[p], len = 0;
        if (st == SC_SMOOTH_OK) {
            if (tstat[p] != 0) st = SC_SMOOTH_TOPPRA_FAILED;
            else {
                const double* tp = t + (size_t)p * (N + 1);
                int i = N;
                while (i > 0 && !(tp[i] - tp[i - 1] >= SM_NEARLY_ZERO)) --i;
                const double q = ceil(tp[i] / dt);
                if (q >= 0.0 && q <= 2147483647.0) len = (int)q;
                else st = SC_SMOOTH_TOPPRA_FAILED;
            }
            status[p] = st;
        }
        length[p] = len;
        sum += len;
    }
    long long tot;
    long long off = block_exscan(sum, &tot);   // its barriers also order s_first's initialisation
    for (int p = p0; p < p1; ++p) {
        const int len = length[p];
        offsets[p] = (int32_t)min(off, (long long)INT32_MAX);
        if (len > 0 && off + len > cap) {
            status[p] = SC_SMOOTH_TRUNCATED;
            atomicMin(&s_first, (int)min(off, (long long)INT32_MAX));   // the first one has off <= cap <= INT32_MAX
        }
        off += len;
    }
    __syncthreads();
    const long long first = s_first;
    for (int p = p0; p < p1; ++p) roff[p] = (int32_t)min((long long)offsets[p], first);
    if (threadIdx.x == 0) {
        offsets[P] = (int32_t)min(tot, (long long)INT32_MAX);
        roff[P] = (int32_t)min(tot, first);
        *needed = tot;
    }
}

// 5. EMPTY_SEGMENT from the resample's status, and ang_vel = vel * curvature over the samples written
__global__ void __launch_bounds__(256)
smooth_finish_kernel(const int32_t* __restrict__ rstat, const int32_t* __restrict__ roff, int P, int32_t* __restrict__ status,
                     int32_t* __restrict__ length, const float* __restrict__ vel, const float* __restrict__ curv, float* __restrict__ ang_vel) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid < P && status[gid] == SC_SMOOTH_OK && rstat[gid] != 0) { status[gid] = SC_SMOOTH_EMPTY_SEGMENT; length[gid] = 0; }
    if (!ang_vel) return;
    const int M = roff[P];
    for (int i = gid; i < M; i += gridDim.x * 256) ang_vel[i] = vel[i] * curv[i];
}

// what sc_smooth_paths_limited_batch adds to the sequence: per-stage limits between the arclength and TOPP-RA
struct sm_limited {
    const double* dyn;
    int J;
    sc_speed_frame fr;
    double* vmax_stage;
    float* min_clear;
};

// what sc_smooth_paths_clear_batch adds to the limited sequence: the repair of legs that hit the grid, between the
// compaction and the arclength
struct sm_clear {
    int32_t r2_clear;
    int max_level;
    uint8_t* level;
    int32_t *leg_min, *rounds;
};

// the repair's verdict enters after NONFINITE has been decided: a COLLIDES path gets a harmless TOPP-RA problem
__global__ void __launch_bounds__(256)
smooth_collides_kernel(const int32_t* __restrict__ cstat, int P, int32_t* __restrict__ status, double* __restrict__ tp) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P || status[p] != SC_SMOOTH_OK || cstat[p] != SC_SMOOTH_COLLIDES) return;
    status[p] = SC_SMOOTH_COLLIDES;
    tp[(size_t)P + p] = 1.0;
    tp[(size_t)4 * P + p] = -1.0;
    tp[(size_t)5 * P + p] = 1.0;
    tp[(size_t)6 * P + p] = -1.0;
    tp[(size_t)7 * P + p] = 1.0;
}

// the sequence of the entry points; lt NULL: one constant limit per path; cl (only with lt and its grid): the repair
static int smooth_run(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits, float start_angle,
                      const float* lines, int nlines, float dt, int N, int nsub, int64_t sample_capacity, float* ctrl, int32_t* seg_off,
                      float* arclength, int32_t* length, int32_t* offsets, int32_t* status, int64_t* needed, double* time, float* pos,
                      float* vel, float* acc, float* pts, float* curvature, float* ang_vel, float* tpar, int32_t* seg, const sm_limited* lt,
                      const sm_clear* cl = nullptr) {
    if (!ctx || !path || !npts || !limits || !ctrl || !seg_off || !arclength || !length || !offsets || !status || !needed || !pos || !pts ||
        P <= 0 || P > SC_SMOOTH_MAX_PATHS || n_max < 2 || (long long)P * (n_max - 1) > INT32_MAX / 8 || nlines < 0 || (nlines > 0 && !lines) ||
        !(dt > 0.f) || !isfinite(dt) || N <= 0 || nsub <= 0 || nsub > SC_RESAMPLE_MAX_NSUB || sample_capacity < 0 ||
        sample_capacity > INT32_MAX)
        return SC_ERR_INVALID;
    if (lt && (!sc_speed_args_ok(lt->J, lt->dyn, lt->fr) || (long long)P * ((long long)N + 1) > INT32_MAX)) return SC_ERR_INVALID;
    if (cl && (!lt || !sc_curve_grid_ok(lt->fr, cl->r2_clear) || cl->max_level < 1 || cl->max_level > SC_CURVE_MAX_LEVEL ||
               n_max - 1 > SC_CURVE_MAX_LEGS))
        return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const int Smax = P * (n_max - 1);
    const long long cap = sample_capacity;
    int r = sc_scratch_reserve(ctx, &ctx->sm_ctrl, (size_t)Smax * 32);
    if (r == SC_OK) r = sc_scratch_reserve(ctx, &ctx->sm_cum, al256((size_t)Smax * (nsub + 1) * 4) + (size_t)Smax * 4);
    const size_t tp_in = (size_t)8 * P, oK = tp_in, ox = oK + (size_t)P * (N + 1) * 2, ot = ox + (size_t)P * (N + 1),
                 ou = ot + (size_t)P * (N + 1), tp_words = ou + (size_t)P * N;
    if (r == SC_OK) r = sc_scratch_reserve(ctx, &ctx->sm_tp, tp_words * 8);
    if (r == SC_OK) r = sc_scratch_reserve(ctx, &ctx->sm_int, (size_t)((cl ? 5 : 4) * P + 1) * 4);
    const bool need_vel = ang_vel && !vel, need_curv = ang_vel && !curvature;
    if (r == SC_OK && (need_vel || need_curv)) r = sc_scratch_reserve(ctx, &ctx->sm_smp, (size_t)2 * (cap > 0 ? cap : 1) * 4);
    if (r == SC_OK && lt) r = sc_scratch_reserve(ctx, &ctx->sm_vlim, (size_t)2 * P * (N + 1) * 8);
    if (r != SC_OK) return r;
    float* padded = (float*)ctx->sm_ctrl.p;
    float* cum = (float*)ctx->sm_cum.p;
    float* seg_len = (float*)((char*)ctx->sm_cum.p + al256((size_t)Smax * (nsub + 1) * 4));
    double* tp = (double*)ctx->sm_tp.p;
    int32_t* npts_eff = (int32_t*)ctx->sm_int.p;
    int32_t *tstat = npts_eff + P, *rstat = tstat + P, *roff = rstat + P, *cstat = roff + P + 1;
    float* vel_o = need_vel ? (float*)ctx->sm_smp.p : vel;
    float* curv_o = need_curv ? (float*)ctx->sm_smp.p + (cap > 0 ? cap : 1) : curvature;

    int tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(smooth_check_kernel, dim3((P + 3) / 4), dim3(256), 0, ctx->stream, path, npts, P, n_max, npts_eff, status);
    hipLaunchKernelGGL(smooth_seg_scan_kernel, dim3(1), dim3(SM_THREADS), 0, ctx->stream, (const int32_t*)npts_eff, P, seg_off);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    r = sc_bezier_from_path_batch(ctx, path, npts_eff, P, n_max, start_angle, lines, nlines, padded);
    if (r != SC_OK) return r;
    tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(smooth_compact_kernel, dim3((Smax + 255) / 256), dim3(256), 0, ctx->stream, (const float*)padded, (const int32_t*)npts_eff,
                       (const int32_t*)seg_off, P, n_max, ctrl);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    if (cl) {   // in place; its verdict waits in cstat until NONFINITE has been decided on the repaired legs
        r = sc_launch_curve_clear(ctx, ctrl, ctrl, seg_off, status, P, lt->fr, cl->r2_clear, cl->max_level, cl->level, cl->rounds, cl->leg_min,
                                  cstat);
        if (r != SC_OK) return r;
    }
    r = sc_launch_arclength(ctx, ctrl, Smax, nsub, cum, seg_len, seg_off + P);
    if (r != SC_OK) return r;
    tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(smooth_toppra_inputs_kernel, dim3((P + 3) / 4), dim3(256), 0, ctx->stream, (const float*)ctrl, (const float*)seg_len,
                       (const int32_t*)seg_off, limits, P, status, arclength, tp);
    if (cl) hipLaunchKernelGGL(smooth_collides_kernel, dim3((P + 255) / 256), dim3(256), 0, ctx->stream, (const int32_t*)cstat, P, status, tp);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    const double *p0 = tp, *p1 = tp + P, *v0 = tp + 2 * (size_t)P, *v1 = tp + 3 * (size_t)P;
    if (lt) {
        // status is read and written in place: every thread of a path's workgroup derives the same value from what it reads,
        // before or after the one store
        double* vlo = (double*)ctx->sm_vlim.p;
        double* vhi = vlo + (size_t)P * (N + 1);
        r = sc_launch_speed_limits(ctx, ctrl, cum, seg_off, arclength, status, P, nsub, N, lt->J, limits, lt->dyn, lt->fr, n_max - 1, vlo, vhi,
                                   lt->vmax_stage, lt->min_clear, status);
        if (r != SC_OK) return r;
        r = sc_toppra_hermite_batch(ctx, P, 1, N, p0, p1, v0, v1, vlo, vhi, 1, tp + 6 * (size_t)P, tp + 7 * (size_t)P, 0.0, 0.0, tp + oK,
                                    tp + ox, tp + ou, tp + ot, tstat);
    } else
        r = sc_toppra_hermite_batch(ctx, P, 1, N, p0, p1, v0, v1, tp + 4 * (size_t)P, tp + 5 * (size_t)P, 0, tp + 6 * (size_t)P,
                                    tp + 7 * (size_t)P, 0.0, 0.0, tp + oK, tp + ox, tp + ou, tp + ot, tstat);
    if (r != SC_OK) return r;
    tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(smooth_count_scan_kernel, dim3(1), dim3(SM_THREADS), 0, ctx->stream, (const double*)(tp + ot), (const int32_t*)tstat, P, N,
                       (double)dt, cap, status, length, offsets, roff, needed);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    r = sc_launch_toppra_sample_packed(ctx, P, 1, N, p0, p1, v0, v1, tp + ox, tp + ot, (double)dt, offsets, length, status, pos, vel_o, acc,
                                       time);
    if (r != SC_OK) return r;
    r = sc_launch_resample(ctx, ctrl, cum, arclength, seg_off, P, Smax, nsub, pos, roff, 1, pts, tpar, seg, curv_o, rstat, seg_off + P);
    if (r != SC_OK) return r;
    long long gb = (cap + 255) / 256;
    if (gb > 2048) gb = 2048;
    if (gb < (P + 255) / 256) gb = (P + 255) / 256;
    tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(smooth_finish_kernel, dim3((unsigned)gb), dim3(256), 0, ctx->stream, (const int32_t*)rstat, (const int32_t*)roff, P, status,
                       length, (const float*)vel_o, (const float*)curv_o, ang_vel);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_smooth_paths_batch(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits,
                                     float start_angle, const float* lines, int nlines, float dt, int N, int nsub, int64_t sample_capacity,
                                     float* ctrl, int32_t* seg_off, float* arclength, int32_t* length, int32_t* offsets, int32_t* status,
                                     int64_t* needed, double* time, float* pos, float* vel, float* acc, float* pts, float* curvature,
                                     float* ang_vel, float* tpar, int32_t* seg) {
    return smooth_run(ctx, path, npts, P, n_max, limits, start_angle, lines, nlines, dt, N, nsub, sample_capacity, ctrl, seg_off, arclength,
                      length, offsets, status, needed, time, pos, vel, acc, pts, curvature, ang_vel, tpar, seg, nullptr);
}

extern "C" int sc_smooth_paths_limited_batch(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits,
                                             float start_angle, const float* lines, int nlines, float dt, int N, int nsub,
                                             int64_t sample_capacity, float* ctrl, int32_t* seg_off, float* arclength, int32_t* length,
                                             int32_t* offsets, int32_t* status, int64_t* needed, double* time, float* pos, float* vel,
                                             float* acc, float* pts, float* curvature, float* ang_vel, float* tpar, int32_t* seg,
                                             const double* dyn, int J, const int32_t* d2, int W, int H, float x_min, float y_min, float res_x,
                                             float res_y, double* vmax_stage, float* min_clear) {
    const sm_limited lt{dyn, J, {d2, W, H, x_min, y_min, res_x, res_y}, vmax_stage, min_clear};
    return smooth_run(ctx, path, npts, P, n_max, limits, start_angle, lines, nlines, dt, N, nsub, sample_capacity, ctrl, seg_off, arclength,
                      length, offsets, status, needed, time, pos, vel, acc, pts, curvature, ang_vel, tpar, seg, &lt);
}

extern "C" int sc_smooth_paths_clear_batch(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits,
                                           float start_angle, const float* lines, int nlines, float dt, int N, int nsub, int64_t sample_capacity,
                                           float* ctrl, int32_t* seg_off, float* arclength, int32_t* length, int32_t* offsets, int32_t* status,
                                           int64_t* needed, double* time, float* pos, float* vel, float* acc, float* pts, float* curvature,
                                           float* ang_vel, float* tpar, int32_t* seg, const double* dyn, int J, const int32_t* d2, int W, int H,
                                           float x_min, float y_min, float res_x, float res_y, double* vmax_stage, float* min_clear,
                                           int32_t r2_clear, int max_level, uint8_t* level, int32_t* leg_min_d2, int32_t* rounds) {
    const sm_limited lt{dyn, J, {d2, W, H, x_min, y_min, res_x, res_y}, vmax_stage, min_clear};
    const sm_clear cl{r2_clear, max_level, level, leg_min_d2, rounds};
    return smooth_run(ctx, path, npts, P, n_max, limits, start_angle, lines, nlines, dt, N, nsub, sample_capacity, ctrl, seg_off, arclength,
                      length, offsets, status, needed, time, pos, vel, acc, pts, curvature, ang_vel, tpar, seg, &lt, &cl);
}

// the host form of all three; lt (host pointers) NULL: sc_smooth_paths_batch_host; cl (host pointers) only with lt
static int smooth_run_host(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits, float start_angle,
                           const float* lines, int nlines, float dt, int N, int nsub, int64_t sample_capacity, float* ctrl,
                           int32_t* seg_off, float* arclength, int32_t* length, int32_t* offsets, int32_t* status, int64_t* needed,
                           double* time, float* pos, float* vel, float* acc, float* pts, float* curvature, float* ang_vel, float* tpar,
                           int32_t* seg, const sm_limited* lt, const sm_clear* cl = nullptr) {
    if (!ctx || !path || !npts || !limits || !ctrl || !seg_off || !arclength || !length || !offsets || !status || !needed || !pos || !pts ||
        P <= 0 || P > SC_SMOOTH_MAX_PATHS || n_max < 2 || (long long)P * (n_max - 1) > INT32_MAX / 8 || nlines < 0 || (nlines > 0 && !lines) ||
        sample_capacity < 0 || sample_capacity > INT32_MAX)
        return SC_ERR_INVALID;
    if (lt && (N <= 0 || (long long)P * ((long long)N + 1) > INT32_MAX || !sc_speed_args_ok(lt->J, lt->dyn, lt->fr) ||
               !sc_speed_dyn_ok(lt->dyn, P)))
        return SC_ERR_INVALID;
    if (cl && (!lt || !lt->fr.d2)) return SC_ERR_INVALID;   // smooth_run checks the rest
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t S = (size_t)P * (n_max - 1), M = sample_capacity > 0 ? (size_t)sample_capacity : 1, pb = (size_t)P * 4;
    sc_stage st(ctx);
    const bool grid = lt && lt->fr.d2;
    const int i_dyn = st.in(lt ? lt->dyn : nullptr, lt ? pb * 8 : 0), i_d2 = st.in(grid ? lt->fr.d2 : nullptr, grid ? (size_t)lt->fr.W * lt->fr.H * 4 : 0),
              o_vs = st.out(lt ? lt->vmax_stage : nullptr, lt && lt->vmax_stage ? (size_t)P * (N + 1) * 8 : 0),
              o_mc = st.out(lt ? lt->min_clear : nullptr, lt && lt->min_clear ? pb : 0);
    const int i_path = st.in(path, (size_t)P * n_max * 8), i_npts = st.in(npts, pb), i_lim = st.in(limits, pb * 8),
              i_l = st.in(lines, (size_t)nlines * 16);
    const int o_ctrl = st.out(nullptr, S * 32), o_so = st.out(seg_off, pb + 4), o_al = st.out(arclength, pb), o_len = st.out(length, pb),
              o_off = st.out(offsets, pb + 4), o_st = st.out(status, pb), o_need = st.out(needed, 8);
    // per-sample outputs (room only for those the caller wants), downloaded once the counts are known
    auto smp = [&](const void* h, size_t elem) { return st.out(nullptr, h ? M * elem : 0); };
    const int o_time = smp(time, 8), o_pos = smp(pos, 4), o_vel = smp(vel, 4), o_acc = smp(acc, 4), o_pts = smp(pts, 8), o_cv = smp(curvature, 4),
              o_ang = smp(ang_vel, 4), o_tpar = smp(tpar, 4), o_seg = smp(seg, 4);
    // the repair's outputs: per leg and waypoint, downloaded once the counts are known
    const int o_lv = st.out(nullptr, cl && cl->level ? S + P : 0), o_lm = st.out(nullptr, cl && cl->leg_min ? S * 4 : 0),
              o_rd = st.out(cl ? cl->rounds : nullptr, cl && cl->rounds ? pb : 0);
    int r = st.upload();
    sm_limited dl{};
    if (lt) {
        dl = *lt;
        dl.dyn = st.dev<const double>(i_dyn);
        dl.fr.d2 = grid ? st.dev<const int32_t>(i_d2) : nullptr;
        dl.vmax_stage = lt->vmax_stage ? st.dev<double>(o_vs) : nullptr;
        dl.min_clear = lt->min_clear ? st.dev<float>(o_mc) : nullptr;
    }
    sm_clear dc{};
    if (cl) {
        dc = *cl;
        dc.level = cl->level ? st.dev<uint8_t>(o_lv) : nullptr;
        dc.leg_min = cl->leg_min ? st.dev<int32_t>(o_lm) : nullptr;
        dc.rounds = cl->rounds ? st.dev<int32_t>(o_rd) : nullptr;
    }
    if (r == SC_OK)
        r = smooth_run(ctx, st.dev<const float>(i_path), st.dev<const int32_t>(i_npts), P, n_max, st.dev<const double>(i_lim), start_angle,
                                  nlines > 0 ? st.dev<const float>(i_l) : nullptr, nlines, dt, N, nsub, sample_capacity, st.dev<float>(o_ctrl),
                                  st.dev<int32_t>(o_so), st.dev<float>(o_al), st.dev<int32_t>(o_len), st.dev<int32_t>(o_off), st.dev<int32_t>(o_st),
                                  st.dev<int64_t>(o_need), time ? st.dev<double>(o_time) : nullptr, st.dev<float>(o_pos),
                                  vel ? st.dev<float>(o_vel) : nullptr, acc ? st.dev<float>(o_acc) : nullptr, st.dev<float>(o_pts),
                                  curvature ? st.dev<float>(o_cv) : nullptr, ang_vel ? st.dev<float>(o_ang) : nullptr,
                                  tpar ? st.dev<float>(o_tpar) : nullptr, seg ? st.dev<int32_t>(o_seg) : nullptr, lt ? &dl : nullptr,
                                  cl ? &dc : nullptr);
    r = st.finish(r);
    if (r != SC_OK) return r;
    // the samples written: up to the first truncated path
    size_t Mw = (size_t)offsets[P];
    for (int p = 0; p < P; ++p)
        if (status[p] == SC_SMOOTH_TRUNCATED) { Mw = (size_t)offsets[p]; break; }
    if (Mw > (size_t)sample_capacity) Mw = (size_t)sample_capacity;
    st.back(o_ctrl, ctrl, (size_t)seg_off[P] * 32);
    st.back(o_time, time, Mw * 8); st.back(o_pos, pos, Mw * 4); st.back(o_vel, vel, Mw * 4); st.back(o_acc, acc, Mw * 4);
    st.back(o_pts, pts, Mw * 8); st.back(o_cv, curvature, Mw * 4); st.back(o_ang, ang_vel, Mw * 4); st.back(o_tpar, tpar, Mw * 4);
    st.back(o_seg, seg, Mw * 4);
    if (cl) { st.back(o_lv, cl->level, (size_t)seg_off[P] + P); st.back(o_lm, cl->leg_min, (size_t)seg_off[P] * 4); }
    return st.finish(SC_OK);
}

extern "C" int sc_smooth_paths_batch_host(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits,
                                          float start_angle, const float* lines, int nlines, float dt, int N, int nsub,
                                          int64_t sample_capacity, float* ctrl, int32_t* seg_off, float* arclength, int32_t* length,
                                          int32_t* offsets, int32_t* status, int64_t* needed, double* time, float* pos, float* vel,
                                          float* acc, float* pts, float* curvature, float* ang_vel, float* tpar, int32_t* seg) {
    return smooth_run_host(ctx, path, npts, P, n_max, limits, start_angle, lines, nlines, dt, N, nsub, sample_capacity, ctrl, seg_off,
                           arclength, length, offsets, status, needed, time, pos, vel, acc, pts, curvature, ang_vel, tpar, seg, nullptr);
}

extern "C" int sc_smooth_paths_limited_batch_host(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits,
                                                  float start_angle, const float* lines, int nlines, float dt, int N, int nsub,
                                                  int64_t sample_capacity, float* ctrl, int32_t* seg_off, float* arclength, int32_t* length,
                                                  int32_t* offsets, int32_t* status, int64_t* needed, double* time, float* pos, float* vel,
                                                  float* acc, float* pts, float* curvature, float* ang_vel, float* tpar, int32_t* seg,
                                                  const double* dyn, int J, const int32_t* d2, int W, int H, float x_min, float y_min,
                                                  float res_x, float res_y, double* vmax_stage, float* min_clear) {
    const sm_limited lt{dyn, J, {d2, W, H, x_min, y_min, res_x, res_y}, vmax_stage, min_clear};
    return smooth_run_host(ctx, path, npts, P, n_max, limits, start_angle, lines, nlines, dt, N, nsub, sample_capacity, ctrl, seg_off,
                           arclength, length, offsets, status, needed, time, pos, vel, acc, pts, curvature, ang_vel, tpar, seg, &lt);
}

extern "C" int sc_smooth_paths_clear_batch_host(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits,
                                                float start_angle, const float* lines, int nlines, float dt, int N, int nsub,
                                                int64_t sample_capacity, float* ctrl, int32_t* seg_off, float* arclength, int32_t* length,
                                                int32_t* offsets, int32_t* status, int64_t* needed, double* time, float* pos, float* vel,
                                                float* acc, float* pts, float* curvature, float* ang_vel, float* tpar, int32_t* seg,
                                                const double* dyn, int J, const int32_t* d2, int W, int H, float x_min, float y_min,
                                                float res_x, float res_y, double* vmax_stage, float* min_clear, int32_t r2_clear,
                                                int max_level, uint8_t* level, int32_t* leg_min_d2, int32_t* rounds) {
    const sm_limited lt{dyn, J, {d2, W, H, x_min, y_min, res_x, res_y}, vmax_stage, min_clear};
    const sm_clear cl{r2_clear, max_level, level, leg_min_d2, rounds};
    return smooth_run_host(ctx, path, npts, P, n_max, limits, start_angle, lines, nlines, dt, N, nsub, sample_capacity, ctrl, seg_off,
                           arclength, length, offsets, status, needed, time, pos, vel, acc, pts, curvature, ang_vel, tpar, seg, &lt, &cl);
}

// cells of sc_path_waypoints_batch -> float points (occupancy_grid::centre_of), one thread per (path, point)
__global__ void __launch_bounds__(256)
cells_to_points_kernel(const int32_t* __restrict__ wp, const int32_t* __restrict__ n_wp, const int32_t* __restrict__ status, int Q, int Wmax,
                       int W, float x_min, float y_min, float res_x, float res_y, const float* __restrict__ starts,
                       const float* __restrict__ goals, float* __restrict__ path, int32_t* __restrict__ npts) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)Q * Wmax) return;
    const int q = (int)(gid / Wmax), i = (int)(gid % Wmax);
    const int n = n_wp[q];
    const bool ok = (!status || status[q] == SC_Q_OK) && n >= 1 && n <= Wmax;
    const bool ends = starts != nullptr;
    int np = ok ? n : 0;
    if (ok && ends && n < 2) np = Wmax >= 2 ? 2 : 0;
    if (i == 0) npts[q] = np;
    if (i >= np) return;
    float x, y;
    if (ends && i == 0) { x = starts[2 * (size_t)q]; y = starts[2 * (size_t)q + 1]; }
    else if (ends && i == np - 1) { x = goals[2 * (size_t)q]; y = goals[2 * (size_t)q + 1]; }
    else {
        const int c = wp[(size_t)q * Wmax + i];
        x = sc_cell_centre(c % W, x_min, res_x);
        y = sc_cell_centre(c / W, y_min, res_y);
    }
    path[((size_t)q * Wmax + i) * 2] = x;
    path[((size_t)q * Wmax + i) * 2 + 1] = y;
}

extern "C" int sc_cells_to_points_batch(sc_ctx* ctx, const int32_t* wp, const int32_t* n_wp, const int32_t* status, int Q, int Wmax, int W,
                                        float x_min, float y_min, float res_x, float res_y, const float* starts, const float* goals, float* path,
                                        int32_t* npts) {
    if (!ctx || !wp || !n_wp || !path || !npts || Q <= 0 || Wmax <= 0 || W <= 0 || (!starts) != (!goals)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const long long n = (long long)Q * Wmax;
    int tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(cells_to_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, wp, n_wp, status, Q, Wmax, W, x_min,
                       y_min, res_x, res_y, starts, goals, path, npts);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}
