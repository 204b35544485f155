// curve.hip -- smoothed curves against the distance map: a sampled test of which cells a Bezier leg visits
// (sc_curve_clearance_batch) and the repair that halves the tangents at the ends of a hitting leg until no leg hits
// (sc_curve_clear_batch; the definition is in include/sea_current_hip.h and DESIGN.md section 21).
//
// What the test guarantees: no SAMPLE of a leg that passes lies in a cell with d2 < max(r2_clear, 1) or outside the map,
// and no point of the curve lies further than a quarter of a cell (min(res_x, res_y) / 4, along the curve) from a sample.
// It is a sampled test of cell membership, not a swept-disc proof: the curve may cut the corner of a blocked cell between
// two samples by less than that quarter cell.
//
// Both kernels run one 256-thread workgroup per path.  A leg is evaluated by one wavefront: the lanes stride over the
// samples, each evaluates the point in fp64 (bez_eval), fetches d2 and keeps a running minimum and its lowest hitting
// sample; a wave reduction follows.  The workgroup's wavefronts take the legs in turn.  The repair keeps the level-0
// control points, the levels and the per-leg flags of its path in LDS and runs every round inside the kernel: a batch is
// one launch and nothing is read back.  The rounds are Jacobi: __syncthreads() separates the evaluation of a round from
// its level update, so no result depends on the order of the wavefronts.
//
// Compiled with -ffp-contract=off: the NumPy twin of the tests states the same products and sums without fused
// multiply-adds.
#include "sc_internal.h"

#include <math.h>

#define CV_THREADS 256
#define CV_WAVES (CV_THREADS / 64)
#define CV_N_CLAMP (1 << 20)   // samples of a leg at the most; a leg that needs more hits

struct cv_grid {
    const int32_t* d2;
    int W, H;
    double x_min, y_min, res_x, res_y, h;   // h = min(res_x, res_y)
    int32_t r2c;                            // max(r2_clear, 1)
};

__device__ __forceinline__ int cv_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

// One wavefront evaluates the leg c [4][2] (every lane passes the same values): mn = the minimum of d2 over its samples,
// t_hit = the parameter of its lowest hitting sample (0 when only the sample count or the length make it hit, -1 when it
// does not hit).  Returns whether the leg hits.  All results are wave-uniform.
__device__ __forceinline__ bool cv_leg(const cv_grid& g, const float* c, int lane, int32_t& mn, float& t_hit) {
    double Lp = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double dx = (double)c[2 * j + 2] - (double)c[2 * j], dy = (double)c[2 * j + 3] - (double)c[2 * j + 1];
        const double l = __dsqrt_rn(dx * dx + dy * dy);
        Lp = j == 0 ? l : Lp + l;
    }
    const double q = ceil(6.0 * Lp / g.h);
    bool forced = false;
    int n;
    if (!isfinite(Lp)) { n = 1; forced = true; }
    else if (q > (double)CV_N_CLAMP) { n = CV_N_CLAMP; forced = true; }
    else n = q < 1.0 ? 1 : (int)q;
    int32_t m = INT32_MAX;
    int kf = INT32_MAX;
    for (int k = lane; k <= n; k += 64) {
        const double t = (double)k / (double)n;
        double x, y;
        bez_eval(c, t, 0, x, y);
        const double fx = (x - g.x_min) / g.res_x, fy = (y - g.y_min) / g.res_y;
        int32_t v = 0;   // not finite (every comparison fails) or outside the map: a hit
        if (fx >= 0.0 && fy >= 0.0 && fx < (double)g.W && fy < (double)g.H) v = g.d2[(size_t)(int)fy * g.W + (int)fx];
        m = min(m, v);
        if (v < g.r2c) kf = min(kf, k);
    }
    m = cv_wave_min(m);
    kf = cv_wave_min(kf);
    mn = m;
    const bool hit = forced || m < g.r2c;
    t_hit = !hit ? -1.f : (kf == INT32_MAX ? 0.f : (float)((double)kf / (double)n));
    return hit;
}

struct cv_check_args {
    const float* ctrl;
    const int32_t *seg_off, *status;
    cv_grid g;
    int32_t *leg_min, *path_min, *hit_legs, *hit_leg;
    float* hit_t;
};

// the check alone: wavefront w of path p's workgroup takes legs w, w + 4, ...
__global__ void __launch_bounds__(CV_THREADS) curve_clearance_kernel(cv_check_args a) {
    __shared__ int32_t s_min[CV_WAVES], s_cnt[CV_WAVES], s_leg[CV_WAVES];
    __shared__ float s_t[CV_WAVES];
    const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s0 = a.seg_off[p], ns = s0 >= 0 ? a.seg_off[p + 1] - s0 : 0;
    if (a.status && a.status[p] != SC_SMOOTH_OK) {   // the whole workgroup leaves, before the barrier
        if (threadIdx.x == 0) {
            if (a.path_min) a.path_min[p] = 0;
            if (a.hit_legs) a.hit_legs[p] = 0;
            if (a.hit_leg) a.hit_leg[p] = -1;
            if (a.hit_t) a.hit_t[p] = -1.f;
        }
        return;
    }
    int32_t pm = INT32_MAX, cnt = 0, first = INT32_MAX;
    float first_t = -1.f;
    for (int i = wave; i < ns; i += CV_WAVES) {
        const float* g_c = a.ctrl + ((size_t)s0 + i) * 8;
        float c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = g_c[k];
        int32_t mn;
        float t;
        const bool hit = cv_leg(a.g, c, lane, mn, t);
        if (lane == 0 && a.leg_min) a.leg_min[s0 + i] = mn;
        pm = min(pm, mn);
        if (hit) {
            ++cnt;
            if (first == INT32_MAX) { first = i; first_t = t; }   // the legs of a wavefront ascend
        }
    }
    if (lane == 0) { s_min[wave] = pm; s_cnt[wave] = cnt; s_leg[wave] = first; s_t[wave] = first_t; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CV_WAVES; ++w) {
            pm = min(pm, s_min[w]);
            cnt += s_cnt[w];
            if (s_leg[w] < first) { first = s_leg[w]; first_t = s_t[w]; }
        }
        if (a.path_min) a.path_min[p] = pm;   // INT32_MAX for a path without legs
        if (a.hit_legs) a.hit_legs[p] = cnt;
        if (a.hit_leg) a.hit_leg[p] = first == INT32_MAX ? -1 : first;
        if (a.hit_t) a.hit_t[p] = first == INT32_MAX ? -1.f : first_t;
    }
}

struct cv_clear_args {
    const float* ctrl_in;
    float* ctrl_out;
    const int32_t *seg_off, *status;
    cv_grid g;
    int max_level;
    uint8_t* level;
    int32_t *rounds, *leg_min, *status_out;
};

// control points of leg i at the levels of its two waypoints, from the level-0 points c0 (fp64 on the widened floats)
__device__ __forceinline__ void cv_leg_ctrl(const float* c0, int la, int lb, float* c) {
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = c0[k];
    if (la > 0) {
        const double s = ldexp(1.0, -la);
        c[2] = (float)((double)c0[0] + s * ((double)c0[2] - (double)c0[0]));
        c[3] = (float)((double)c0[1] + s * ((double)c0[3] - (double)c0[1]));
    }
    if (lb > 0) {
        const double s = ldexp(1.0, -lb);
        c[4] = (float)((double)c0[6] - s * ((double)c0[6] - (double)c0[4]));
        c[5] = (float)((double)c0[7] - s * ((double)c0[7] - (double)c0[5]));
    }
}

// the repair: every round of path p inside its workgroup
__global__ void __launch_bounds__(CV_THREADS) curve_clear_kernel(cv_clear_args a) {
    __shared__ float s_c0[SC_CURVE_MAX_LEGS * 8];      // the level-0 control points (ctrl_out may be ctrl_in)
    __shared__ int32_t s_min[SC_CURVE_MAX_LEGS];
    __shared__ uint8_t s_lv[SC_CURVE_MAX_LEGS + 1];    // level of every waypoint
    __shared__ uint8_t s_chg[SC_CURVE_MAX_LEGS + 1];   // its level changed in this round
    __shared__ uint8_t s_leg[SC_CURVE_MAX_LEGS];       // bit 0: the leg hit when it was last evaluated, bit 1: it must be evaluated again
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s0 = a.seg_off[p], ns = a.seg_off[p + 1] - s0;
    int st = a.status ? a.status[p] : SC_SMOOTH_OK;
    if (st == SC_SMOOTH_OK && (s0 < 0 || ns < 0 || ns > SC_CURVE_MAX_LEGS)) st = SC_SMOOTH_BAD_INPUT;
    // status_out may be status itself: every thread derives the same st from what it reads, before or after the store
    if (st != SC_SMOOTH_OK) {   // block-uniform: the whole workgroup leaves, before the first barrier
        if (s0 >= 0 && ns >= 0) {   // a path without legs still owns the slot of one waypoint
            if (a.ctrl_out != a.ctrl_in)
                for (int i = tid; i < ns * 8; i += CV_THREADS) a.ctrl_out[(size_t)s0 * 8 + i] = a.ctrl_in[(size_t)s0 * 8 + i];
            if (a.level)
                for (int j = tid; j <= ns; j += CV_THREADS) a.level[(size_t)s0 + p + j] = 0;
        }
        if (tid == 0) {
            if (a.rounds) a.rounds[p] = 0;
            if (a.status_out) a.status_out[p] = st;
        }
        return;
    }
    for (int i = tid; i < ns * 8; i += CV_THREADS) s_c0[i] = a.ctrl_in[(size_t)s0 * 8 + i];
    for (int j = tid; j <= ns; j += CV_THREADS) s_lv[j] = 0;
    for (int i = tid; i < ns; i += CV_THREADS) s_leg[i] = 2;
    __syncthreads();
    int r = 0;
    bool resolved = false;
    for (;; ++r) {   // at most max_level * (ns + 1) + 1 rounds: every round but the last raises a level
        for (int i = wave; i < ns; i += CV_WAVES) {
            if (!(s_leg[i] & 2)) continue;   // wave-uniform
            float c[8];
            cv_leg_ctrl(s_c0 + (size_t)i * 8, s_lv[i], s_lv[i + 1], c);
            int32_t mn;
            float t;
            const bool hit = cv_leg(a.g, c, lane, mn, t);
            if (lane == 0) { s_min[i] = mn; s_leg[i] = hit; }
        }
        __syncthreads();
        int any = 0;
        for (int i = tid; i < ns; i += CV_THREADS) any |= s_leg[i] & 1;
        if (!__syncthreads_or(any)) { resolved = true; break; }
        int chg = 0;
        for (int j = tid; j <= ns; j += CV_THREADS) {   // only thread j's owner reads and writes s_lv[j]
            const bool bump = (j > 0 && (s_leg[j - 1] & 1)) || (j < ns && (s_leg[j] & 1));
            const int lv = s_lv[j], nl = bump ? min(lv + 1, a.max_level) : lv;
            s_chg[j] = nl != lv;
            s_lv[j] = (uint8_t)nl;
            chg |= nl != lv;
        }
        if (!__syncthreads_or(chg)) { resolved = false; break; }
        for (int i = tid; i < ns; i += CV_THREADS) s_leg[i] = (s_leg[i] & 1) | ((s_chg[i] | s_chg[i + 1]) << 1);
        __syncthreads();
    }
    // every thread left the loop at the same barrier; the levels are those of the last evaluation
    for (int i = tid; i < ns; i += CV_THREADS) {
        float c[8];
        cv_leg_ctrl(s_c0 + (size_t)i * 8, s_lv[i], s_lv[i + 1], c);
        float* o = a.ctrl_out + ((size_t)s0 + i) * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = c[k];
        if (a.leg_min) a.leg_min[s0 + i] = s_min[i];
    }
    if (a.level)
        for (int j = tid; j <= ns; j += CV_THREADS) a.level[(size_t)s0 + p + j] = s_lv[j];
    if (tid == 0) {
        if (a.rounds) a.rounds[p] = r;
        if (a.status_out) a.status_out[p] = resolved ? SC_SMOOTH_OK : SC_SMOOTH_COLLIDES;
    }
}

int sc_curve_grid_ok(const sc_speed_frame& fr, int32_t r2_clear) {
    return fr.d2 && r2_clear >= 0 && sc_frame_ok(fr);
}

static cv_grid cv_make_grid(const sc_speed_frame& fr, int32_t r2_clear) {
    return cv_grid{fr.d2, fr.W, fr.H, (double)fr.x_min, (double)fr.y_min, (double)fr.res_x, (double)fr.res_y,
                   (double)fminf(fr.res_x, fr.res_y), r2_clear > 1 ? r2_clear : 1};
}

static int cv_launch_check(sc_ctx* ctx, const float* ctrl, const int32_t* seg_off, const int32_t* status, int P, const sc_speed_frame& fr,
                           int32_t r2_clear, int32_t* leg_min, int32_t* path_min, int32_t* hit_legs, int32_t* hit_leg, float* hit_t) {
    cv_check_args a{ctrl, seg_off, status, cv_make_grid(fr, r2_clear), leg_min, path_min, hit_legs, hit_leg, hit_t};
    int tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(curve_clearance_kernel, dim3(P), dim3(CV_THREADS), 0, ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

int sc_launch_curve_clear(sc_ctx* ctx, const float* ctrl_in, float* ctrl_out, const int32_t* seg_off, const int32_t* status, int P,
                          const sc_speed_frame& fr, int32_t r2_clear, int max_level, uint8_t* level, int32_t* rounds, int32_t* leg_min,
                          int32_t* status_out) {
    cv_clear_args a{ctrl_in, ctrl_out, seg_off, status, cv_make_grid(fr, r2_clear), max_level, level, rounds, leg_min, status_out};
    int tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(curve_clear_kernel, dim3(P), dim3(CV_THREADS), 0, ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

static bool cv_check_invalid(sc_ctx* ctx, const float* ctrl, const int32_t* seg_off, int P, const sc_speed_frame& fr, int32_t r2_clear,
                             const void* o0, const void* o1, const void* o2, const void* o3, const void* o4) {
    return !ctx || !ctrl || !seg_off || P <= 0 || P > SC_SMOOTH_MAX_PATHS || !sc_curve_grid_ok(fr, r2_clear) || (!o0 && !o1 && !o2 && !o3 && !o4);
}

extern "C" int sc_curve_clearance_batch(sc_ctx* ctx, const float* ctrl, const int32_t* seg_off, const int32_t* status, int P,
                                        const int32_t* d2, int W, int H, float x_min, float y_min, float res_x, float res_y, int32_t r2_clear,
                                        int32_t* leg_min_d2, int32_t* path_min_d2, int32_t* hit_legs, int32_t* hit_leg, float* hit_t) {
    const sc_speed_frame fr{d2, W, H, x_min, y_min, res_x, res_y};
    if (cv_check_invalid(ctx, ctrl, seg_off, P, fr, r2_clear, leg_min_d2, path_min_d2, hit_legs, hit_leg, hit_t)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return cv_launch_check(ctx, ctrl, seg_off, status, P, fr, r2_clear, leg_min_d2, path_min_d2, hit_legs, hit_leg, hit_t);
}

// seg_off on the host: starts at or above 0 and does not decrease; the legs of a path at most max_legs (0: any number)
static bool cv_seg_off_ok(const int32_t* seg_off, int P, int max_legs) {
    if (seg_off[0] < 0) return false;
    for (int p = 0; p < P; ++p)
        if (seg_off[p + 1] < seg_off[p] || (max_legs > 0 && seg_off[p + 1] - seg_off[p] > max_legs)) return false;
    return true;
}

extern "C" int sc_curve_clearance_batch_host(sc_ctx* ctx, const float* ctrl, const int32_t* seg_off, const int32_t* status, int P,
                                             const int32_t* d2, int W, int H, float x_min, float y_min, float res_x, float res_y,
                                             int32_t r2_clear, int32_t* leg_min_d2, int32_t* path_min_d2, int32_t* hit_legs, int32_t* hit_leg,
                                             float* hit_t) {
    const sc_speed_frame fr{d2, W, H, x_min, y_min, res_x, res_y};
    if (cv_check_invalid(ctx, ctrl, seg_off, P, fr, r2_clear, leg_min_d2, path_min_d2, hit_legs, hit_leg, hit_t)) return SC_ERR_INVALID;
    if (!cv_seg_off_ok(seg_off, P, 0)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t S = (size_t)seg_off[P], pb = (size_t)P * 4;
    sc_stage st(ctx);
    const int i_ctrl = st.in(ctrl, S * 32), i_so = st.in(seg_off, pb + 4), i_st = st.in(status, status ? pb : 0),
              i_d2 = st.in(d2, (size_t)W * H * 4);
    // the entries of skipped paths' legs are not written: the caller's values go up first
    const int o_lm = st.in(status ? leg_min_d2 : nullptr, leg_min_d2 ? S * 4 : 0), o_pm = st.out(path_min_d2, path_min_d2 ? pb : 0),
              o_hl = st.out(hit_legs, hit_legs ? pb : 0), o_hf = st.out(hit_leg, hit_leg ? pb : 0), o_ht = st.out(hit_t, hit_t ? pb : 0);
    st.back(o_lm, leg_min_d2, S * 4);
    int r = st.upload();
    if (r == SC_OK) {
        const sc_speed_frame dfr{st.dev<const int32_t>(i_d2), W, H, x_min, y_min, res_x, res_y};
        r = cv_launch_check(ctx, st.dev<const float>(i_ctrl), st.dev<const int32_t>(i_so), status ? st.dev<const int32_t>(i_st) : nullptr, P,
                            dfr, r2_clear, leg_min_d2 ? st.dev<int32_t>(o_lm) : nullptr, path_min_d2 ? st.dev<int32_t>(o_pm) : nullptr,
                            hit_legs ? st.dev<int32_t>(o_hl) : nullptr, hit_leg ? st.dev<int32_t>(o_hf) : nullptr,
                            hit_t ? st.dev<float>(o_ht) : nullptr);
    }
    return st.finish(r);
}

static bool cv_clear_invalid(sc_ctx* ctx, const float* ctrl_in, const float* ctrl_out, const int32_t* seg_off, int P,
                             const sc_speed_frame& fr, int32_t r2_clear, int max_level) {
    return !ctx || !ctrl_in || !ctrl_out || !seg_off || P <= 0 || P > SC_SMOOTH_MAX_PATHS || !sc_curve_grid_ok(fr, r2_clear) ||
           max_level < 1 || max_level > SC_CURVE_MAX_LEVEL;
}

extern "C" int sc_curve_clear_batch(sc_ctx* ctx, const float* ctrl_in, const int32_t* seg_off, const int32_t* status, int P,
                                    const int32_t* d2, int W, int H, float x_min, float y_min, float res_x, float res_y, int32_t r2_clear,
                                    int max_level, float* ctrl_out, uint8_t* level, int32_t* rounds, int32_t* leg_min_d2,
                                    int32_t* status_out) {
    const sc_speed_frame fr{d2, W, H, x_min, y_min, res_x, res_y};
    if (cv_clear_invalid(ctx, ctrl_in, ctrl_out, seg_off, P, fr, r2_clear, max_level)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return sc_launch_curve_clear(ctx, ctrl_in, ctrl_out, seg_off, status, P, fr, r2_clear, max_level, level, rounds, leg_min_d2, status_out);
}

extern "C" int sc_curve_clear_batch_host(sc_ctx* ctx, const float* ctrl_in, const int32_t* seg_off, const int32_t* status, int P,
                                         const int32_t* d2, int W, int H, float x_min, float y_min, float res_x, float res_y,
                                         int32_t r2_clear, int max_level, float* ctrl_out, uint8_t* level, int32_t* rounds,
                                         int32_t* leg_min_d2, int32_t* status_out) {
    const sc_speed_frame fr{d2, W, H, x_min, y_min, res_x, res_y};
    if (cv_clear_invalid(ctx, ctrl_in, ctrl_out, seg_off, P, fr, r2_clear, max_level)) return SC_ERR_INVALID;
    if (!cv_seg_off_ok(seg_off, P, SC_CURVE_MAX_LEGS)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t S = (size_t)seg_off[P], pb = (size_t)P * 4;
    sc_stage st(ctx);
    // one device copy serves as ctrl_in and ctrl_out (the in-place form)
    const int i_so = st.in(seg_off, pb + 4), i_st = st.in(status, status ? pb : 0), i_d2 = st.in(d2, (size_t)W * H * 4);
    const int o_ctrl = st.in(ctrl_in, S * 32), o_lv = st.out(level, level ? S + P : 0), o_rd = st.out(rounds, rounds ? pb : 0),
              o_lm = st.in(status ? leg_min_d2 : nullptr, leg_min_d2 ? S * 4 : 0),   // skipped paths leave their legs' entries as they are
              o_st = st.out(status_out, status_out ? pb : 0);
    st.back(o_ctrl, ctrl_out, S * 32);
    st.back(o_lm, leg_min_d2, S * 4);
    int r = st.upload();
    if (r == SC_OK) {
        const sc_speed_frame dfr{st.dev<const int32_t>(i_d2), W, H, x_min, y_min, res_x, res_y};
        r = sc_launch_curve_clear(ctx, st.dev<const float>(o_ctrl), st.dev<float>(o_ctrl), st.dev<const int32_t>(i_so),
                                  status ? st.dev<const int32_t>(i_st) : nullptr, P, dfr, r2_clear, max_level,
                                  level ? st.dev<uint8_t>(o_lv) : nullptr, rounds ? st.dev<int32_t>(o_rd) : nullptr,
                                  leg_min_d2 ? st.dev<int32_t>(o_lm) : nullptr, status_out ? st.dev<int32_t>(o_st) : nullptr);
    }
    return st.finish(r);
}
