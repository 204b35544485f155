// speed.hip -- per-stage speed limits of TOPP-RA from the curvature of a path's Bezier legs and from its clearance in a
// distance map (sc_speed_limits_batch; the definition is in include/sea_current_hip.h and DESIGN.md section 13).
//
// One 256-thread workgroup per path.  The path's leg prefix B (fp64), control points and arclength tables are staged in
// LDS when they fit the launch's budget, otherwise every sample reads them from global memory (L2-resident: the
// arclength kernel has just written them).  Threads stride over (stage, sample) pairs, SP_CHUNK stages at a time; the
// minimum of a stage is taken by an LDS atomicMin on the fp64 bit pattern as unsigned 64-bit (every candidate is >= 0 or
// +inf, where that order is the numeric one), so no result depends on the order of the threads.
//
// Compiled with -ffp-contract=off: the NumPy twin of the tests states the same products and sums without fused
// multiply-adds.
#include "sc_internal.h"

#include <math.h>

#define SP_THREADS 256
#define SP_CHUNK 256                  // stages reduced per pass
#define SP_LDS_BUDGET (64 * 1024)     // dynamic LDS of a workgroup at the most: two workgroups per CU
#define SP_HEAD ((SP_CHUNK + 2) * 8)  // stage minima [SP_CHUNK] | minimum clearance | pad, in front of the staged tables
#define SP_INF_BITS 0x7FF0000000000000ull

static inline size_t sp_al16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ static inline size_t sp_stage_need(size_t ns, int nsub) {
    return (((ns + 1) * 8 + 15) & ~(size_t)15) + ns * 32 + ns * (size_t)(nsub + 1) * 4;
}

struct sp_args {
    const float *ctrl, *cum;
    const int32_t *seg_off;
    const float* arclength;
    const int32_t* status;
    int P, nsub, N, J;
    const double *limits, *dyn;
    const int32_t* d2;
    int W, H;
    double x_min, y_min, res_x, res_y, cell;   // cell = min(res_x, res_y)
    unsigned stage_bytes;                       // LDS behind SP_HEAD
    double *vlo, *vhi, *vhi_copy;
    float* min_clear;
    int32_t* status_out;
};

// gridpoint i of gen_vel_prof<1>(AL, 0, 0, 0, ...): the Hermite path from 0 to AL with zero end tangents
__device__ __forceinline__ double sp_gridpoint(double AL, int i, int N) {
    const double s = (double)i / N;
    return AL * (3 * s * s - 2 * s * s * s);
}

// the (stage, sample) pairs of one path.  STAGED: B, ctrl and cum are the LDS copies, else ctrl and cum are the path's rows
// in global memory and the leg is found by running B up leg by leg (the same sums in the same order).
template <bool STAGED>
__device__ __forceinline__ void sp_path(const sp_args& a, int p, int ns, const double* B, const float* ctrl, const float* cum,
                                        unsigned long long* s_min, unsigned long long* s_clear, unsigned long long* s_zero) {
    const int tid = threadIdx.x, N = a.N, J = a.J, K = 2 * J + 1, nsub = a.nsub, row = nsub + 1;
    const double AL = (double)a.arclength[p];
    const double vel_min = a.limits[4 * (size_t)p], vel_max = a.limits[4 * (size_t)p + 1];
    const double om = a.dyn[4 * (size_t)p], alat = a.dyn[4 * (size_t)p + 1], cf = a.dyn[4 * (size_t)p + 2], cg = a.dyn[4 * (size_t)p + 3];
    const bool clear_on = a.d2 != nullptr && isfinite(cf);
    double my_clear = INFINITY;
    for (int c0 = 0; c0 <= N; c0 += SP_CHUNK) {
        const int nst = min(SP_CHUNK, N + 1 - c0);
        for (int i = tid; i < nst; i += SP_THREADS) s_min[i] = SP_INF_BITS;
        __syncthreads();
        for (int pair = tid; pair < nst * K; pair += SP_THREADS) {
            const int li = pair / K, j = pair % K - J, i = c0 + li;
            // the window of stage i reaches half way to its neighbours
            const double ai = sp_gridpoint(AL, i, N);
            double x;
            if (j < 0) {
                const double lo = i == 0 ? ai : (sp_gridpoint(AL, i - 1, N) + ai) / 2;
                x = ai + ((double)j / J) * (ai - lo);
            } else {
                const double hi = i == N ? ai : (ai + sp_gridpoint(AL, i + 1, N)) / 2;
                x = ai + ((double)j / J) * (hi - ai);
            }
            x = !(x > 0.0) ? 0.0 : (x > AL ? AL : x);
            // position -> (leg, t)
            int leg = 0;
            double Bj = 0.0;
            if (STAGED) {
                int lo = 0, hi = ns + 1;   // the number of B_j <= x, B [ns+1] non-decreasing with B_0 = 0
                while (lo < hi) { const int m = (lo + hi) >> 1; if (B[m] <= x) lo = m + 1; else hi = m; }
                leg = min(max(lo - 1, 0), ns - 1);
                Bj = B[leg];
            } else {
                while (leg < ns - 1) {
                    const double nb = Bj + (double)cum[(size_t)leg * row + nsub];
                    if (!(nb <= x)) break;
                    Bj = nb;
                    ++leg;
                }
            }
            const float* tab = cum + (size_t)leg * row;
            const double len = (double)tab[nsub];
            double r = x - Bj;
            r = !(r > 0.0) ? 0.0 : (r > len ? len : r);
            int klo = 0, khi = nsub + 1;   // the number of c_k <= r
            while (klo < khi) { const int m = (klo + khi) >> 1; if ((double)tab[m] <= r) klo = m + 1; else khi = m; }
            const int k = min(max(klo - 1, 0), nsub - 1);
            const double ck = (double)tab[k], den = (double)tab[k + 1] - ck;
            const double f = den > 0.0 ? (r - ck) / den : 0.0;
            double t = ((double)k + f) / nsub;
            t = !(t > 0.0) ? 0.0 : (t > 1.0 ? 1.0 : t);
            const float* c = ctrl + (size_t)leg * 8;
            double ax, ay, bx, by;
            bez_eval(c, t, 1, ax, ay);
            bez_eval(c, t, 2, bx, by);
            const double q = ax * ax + ay * ay;
            double kappa = fabs(ax * by - ay * bx) / (q * sqrt(q));
            if (!isfinite(kappa)) kappa = 0.0;
            double v = INFINITY;
            if (kappa > 0.0) v = fmin(om / kappa, sqrt(alat / kappa));
            if (clear_on) {
                double px, py;
                bez_eval(c, t, 0, px, py);
                double fx = (px - a.x_min) / a.res_x - 0.5, fy = (py - a.y_min) / a.res_y - 0.5;
                fx = !(fx > 0.0) ? 0.0 : (fx > (double)(a.W - 1) ? (double)(a.W - 1) : fx);   // NaN -> 0: the gathers stay in the grid
                fy = !(fy > 0.0) ? 0.0 : (fy > (double)(a.H - 1) ? (double)(a.H - 1) : fy);
                const int ix = min((int)fx, max(a.W - 2, 0)), iy = min((int)fy, max(a.H - 2, 0));
                const int ix1 = min(ix + 1, a.W - 1), iy1 = min(iy + 1, a.H - 1);
                const double ux = fx - ix, uy = fy - iy;
                const int32_t* r0 = a.d2 + (size_t)iy * a.W;
                const int32_t* r1 = a.d2 + (size_t)iy1 * a.W;
                const double d00 = a.cell * sqrt((double)max(r0[ix], 0)), d01 = a.cell * sqrt((double)max(r0[ix1], 0));
                const double d10 = a.cell * sqrt((double)max(r1[ix], 0)), d11 = a.cell * sqrt((double)max(r1[ix1], 0));
                const double e0 = d00 * (1.0 - ux) + d01 * ux, e1 = d10 * (1.0 - ux) + d11 * ux;
                const double cl = e0 * (1.0 - uy) + e1 * uy;
                my_clear = fmin(my_clear, cl);
                v = fmin(v, cf + cg * cl);
            }
            if (v < INFINITY) atomicMin(&s_min[li], (unsigned long long)__double_as_longlong(v));
        }
        __syncthreads();
        for (int li = tid; li < nst; li += SP_THREADS) {
            const double m = __longlong_as_double((long long)s_min[li]);
            const double out = m < vel_max ? m : vel_max;   // no term below vel_max: vel_max's own bits
            if (m < vel_max && !(m > 0.0) && c0 + li > 0 && c0 + li < N) *s_zero = 1ull;   // a term stops the path inside
            const size_t o = (size_t)p * (N + 1) + c0 + li;
            a.vhi[o] = out;
            if (a.vhi_copy) a.vhi_copy[o] = out;
            if (a.vlo) a.vlo[o] = vel_min;
        }
        __syncthreads();
    }
    if (my_clear < INFINITY) atomicMin(s_clear, (unsigned long long)__double_as_longlong(my_clear));
}

__global__ void __launch_bounds__(SP_THREADS) speed_limits_kernel(sp_args a) {
    extern __shared__ __align__(16) unsigned char sp_lds[];
    unsigned long long* s_min = reinterpret_cast<unsigned long long*>(sp_lds);
    unsigned long long* s_clear = s_min + SP_CHUNK;
    unsigned long long* s_zero = s_clear + 1;   // != 0: an interior stage whose limit a term brought to 0
    const int tid = threadIdx.x, p = blockIdx.x, N = a.N;
    const int s0 = a.seg_off[p], ns = a.seg_off[p + 1] - s0;
    int st = a.status ? a.status[p] : SC_SMOOTH_OK;
    if (st == SC_SMOOTH_OK) {
        const double om = a.dyn[4 * (size_t)p], alat = a.dyn[4 * (size_t)p + 1], cf = a.dyn[4 * (size_t)p + 2], cg = a.dyn[4 * (size_t)p + 3];
        const bool dyn_ok = om > 0.0 && alat > 0.0 && cf >= 0.0 && cg >= 0.0 && isfinite(cg);   // a NaN fails its comparison
        if (!dyn_ok || ns < 1 || s0 < 0) st = SC_SMOOTH_BAD_INPUT;
        else if (!isfinite(a.arclength[p])) st = SC_SMOOTH_NONFINITE;
    }
    // status_out may be status itself: every thread derives the same st from what it reads, before or after the store
    if (st != SC_SMOOTH_OK) {   // block-uniform, before the first barrier: a harmless finite problem
        if (tid == 0 && a.status_out) a.status_out[p] = st;
        for (int i = tid; i <= N; i += SP_THREADS) {
            const size_t o = (size_t)p * (N + 1) + i;
            a.vhi[o] = 1.0;
            if (a.vhi_copy) a.vhi_copy[o] = 1.0;
            if (a.vlo) a.vlo[o] = -1.0;
        }
        if (tid == 0 && a.min_clear) a.min_clear[p] = 0.f;
        return;
    }
    if (tid == 0) { *s_clear = SP_INF_BITS; *s_zero = 0ull; }
    const float* g_ctrl = a.ctrl + (size_t)s0 * 8;
    const float* g_cum = a.cum + (size_t)s0 * (a.nsub + 1);
    const bool staged = sp_stage_need((size_t)ns, a.nsub) <= (size_t)a.stage_bytes;
    if (staged) {
        double* B = reinterpret_cast<double*>(sp_lds + SP_HEAD);
        float* l_ctrl = reinterpret_cast<float*>(sp_lds + SP_HEAD + ((((size_t)ns + 1) * 8 + 15) & ~(size_t)15));
        float* l_cum = l_ctrl + (size_t)ns * 8;
        const int row = a.nsub + 1;
        if (tid == 0) {   // B_{j+1} = B_j + seg_len[j] in leg order
            double b = 0.0;
            B[0] = 0.0;
            for (int j = 0; j < ns; ++j) { b += (double)g_cum[(size_t)j * row + a.nsub]; B[j + 1] = b; }
        }
        for (int i = tid; i < ns * 8; i += SP_THREADS) l_ctrl[i] = g_ctrl[i];
        for (int i = tid; i < ns * row; i += SP_THREADS) l_cum[i] = g_cum[i];
        __syncthreads();
        sp_path<true>(a, p, ns, B, l_ctrl, l_cum, s_min, s_clear, s_zero);
    } else {
        __syncthreads();
        sp_path<false>(a, p, ns, nullptr, g_ctrl, g_cum, s_min, s_clear, s_zero);
    }
    __syncthreads();
    if (tid == 0) {
        if (a.min_clear) a.min_clear[p] = (float)__longlong_as_double((long long)*s_clear);
        // The parametriser gives an interval of zero speed 5 s (as the reference's does) where no finite time exists, so a
        // stage the clearance term stops is decided here: no profile passes it.
        if (a.status_out) a.status_out[p] = *s_zero ? SC_SMOOTH_TOPPRA_FAILED : SC_SMOOTH_OK;
    }
}

int sc_speed_args_ok(int J, const double* dyn, const sc_speed_frame& fr) {
    if (!dyn || J < 1 || J > SC_SPEED_MAX_J) return 0;
    if (fr.d2 && !sc_frame_ok(fr)) return 0;
    return 1;
}

int sc_launch_speed_limits(sc_ctx* ctx, const float* ctrl, const float* cum, const int32_t* seg_off, const float* arclength,
                           const int32_t* status, int P, int nsub, int N, int J, const double* limits, const double* dyn,
                           const sc_speed_frame& fr, int ns_bound, double* vlo, double* vhi, double* vhi_copy, float* min_clear,
                           int32_t* status_out) {
    size_t stage = SP_LDS_BUDGET - SP_HEAD;
    if (ns_bound > 0 && sp_stage_need((size_t)ns_bound, nsub) < stage) stage = sp_al16(sp_stage_need((size_t)ns_bound, nsub));
    sp_args a{ctrl, cum, seg_off, arclength, status, P, nsub, N, J, limits, dyn, fr.d2, fr.W, fr.H, (double)fr.x_min, (double)fr.y_min,
              (double)fr.res_x, (double)fr.res_y, (double)fminf(fr.res_x, fr.res_y), (unsigned)stage, vlo, vhi, vhi_copy, min_clear, status_out};
    int tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(speed_limits_kernel, dim3(P), dim3(SP_THREADS), SP_HEAD + stage, ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

static bool sp_invalid(sc_ctx* ctx, const float* ctrl, const float* cum, const int32_t* seg_off, const float* arclength, int P, int nsub,
                       int N, int J, const double* limits, const double* dyn, const sc_speed_frame& fr, const double* vhi) {
    return !ctx || !ctrl || !cum || !seg_off || !arclength || !limits || !vhi || P <= 0 || P > SC_SMOOTH_MAX_PATHS || nsub <= 0 ||
           nsub > SC_RESAMPLE_MAX_NSUB || N <= 0 || (long long)P * ((long long)N + 1) > INT32_MAX || !sc_speed_args_ok(J, dyn, fr);
}

extern "C" int sc_speed_limits_batch(sc_ctx* ctx, const float* ctrl, const float* cum, const int32_t* seg_off, const float* arclength,
                                     const int32_t* status, int P, int nsub, int N, int J, const double* limits, const double* dyn,
                                     const int32_t* d2, int W, int H, float x_min, float y_min, float res_x, float res_y, double* vhi,
                                     float* min_clear, int32_t* status_out) {
    const sc_speed_frame fr{d2, W, H, x_min, y_min, res_x, res_y};
    if (sp_invalid(ctx, ctrl, cum, seg_off, arclength, P, nsub, N, J, limits, dyn, fr, vhi)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return sc_launch_speed_limits(ctx, ctrl, cum, seg_off, arclength, status, P, nsub, N, J, limits, dyn, fr, 0, nullptr, vhi, nullptr,
                                  min_clear, status_out);
}

// the contract of dyn, as the kernel decides it per path
int sc_speed_dyn_ok(const double* dyn, int P) {
    for (int p = 0; p < P; ++p) {
        const double* d = dyn + 4 * (size_t)p;
        if (!(d[0] > 0.0) || !(d[1] > 0.0) || !(d[2] >= 0.0) || !(d[3] >= 0.0) || !isfinite(d[3])) return 0;
    }
    return 1;
}

extern "C" int sc_speed_limits_batch_host(sc_ctx* ctx, const float* ctrl, const float* cum, const int32_t* seg_off, const float* arclength,
                                          const int32_t* status, int P, int nsub, int N, int J, const double* limits, const double* dyn,
                                          const int32_t* d2, int W, int H, float x_min, float y_min, float res_x, float res_y, double* vhi,
                                          float* min_clear, int32_t* status_out) {
    const sc_speed_frame fr{d2, W, H, x_min, y_min, res_x, res_y};
    if (sp_invalid(ctx, ctrl, cum, seg_off, arclength, P, nsub, N, J, limits, dyn, fr, vhi)) return SC_ERR_INVALID;
    if (seg_off[0] < 0) return SC_ERR_INVALID;
    for (int p = 0; p < P; ++p)
        if (seg_off[p + 1] < seg_off[p]) return SC_ERR_INVALID;
    if (!sc_speed_dyn_ok(dyn, P)) return SC_ERR_INVALID;
    for (int i = 0; i < 4 * P; ++i)
        if (isnan(limits[i])) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t S = (size_t)seg_off[P], pb = (size_t)P * 4, nv = (size_t)P * (N + 1) * 8;
    sc_stage st(ctx);
    const int i_ctrl = st.in(ctrl, S * 32), i_cum = st.in(cum, S * (nsub + 1) * 4), i_so = st.in(seg_off, pb + 4), i_al = st.in(arclength, pb),
              i_st = st.in(status, status ? pb : 0), i_lim = st.in(limits, pb * 8), i_dyn = st.in(dyn, pb * 8),
              i_d2 = st.in(d2, d2 ? (size_t)W * H * 4 : 0);
    const int o_v = st.out(vhi, nv), o_mc = st.out(min_clear, min_clear ? pb : 0), o_st = st.out(status_out, status_out ? pb : 0);
    int r = st.upload();
    if (r == SC_OK) {
        const sc_speed_frame dfr{d2 ? st.dev<const int32_t>(i_d2) : nullptr, W, H, x_min, y_min, res_x, res_y};
        r = sc_launch_speed_limits(ctx, st.dev<const float>(i_ctrl), st.dev<const float>(i_cum), st.dev<const int32_t>(i_so),
                                   st.dev<const float>(i_al), status ? st.dev<const int32_t>(i_st) : nullptr, P, nsub, N, J,
                                   st.dev<const double>(i_lim), st.dev<const double>(i_dyn), dfr, 0, nullptr, st.dev<double>(o_v), nullptr,
                                   min_clear ? st.dev<float>(o_mc) : nullptr, status_out ? st.dev<int32_t>(o_st) : nullptr);
    }
    return st.finish(r);
}
