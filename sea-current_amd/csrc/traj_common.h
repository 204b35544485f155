// traj_common.h -- what the files that read timed paths agree on, stated once: the conflict predicate, the radius contract,
// the size and clock limits, the packed timed paths with their checks, staging and knots launcher, and the scratch behind
// knots the caller passes none of.  Included by traj.hip, traj_sched.hip and tplan.hip.
#pragma once
#include "sc_internal.h"

#include <math.h>

// ---- limits ----
#define SC_TRAJ_MAX_TICKS 65535
#define SC_TRAJ_MAX_KNOTS (1ll << 26)
#define SC_TRAJ_MAX_PATHS 16384
#define SC_TRAJ_SCHED_MAX_PATHS 8192   // the delay schedules: traj_schedule_kernel keeps one int32 slot per path in LDS (32 KiB)

// P, K and P * (K + 1) in range
static inline bool sc_traj_size_ok(int P, int K, int max_paths = SC_TRAJ_MAX_PATHS) {
    return P >= 1 && P <= max_paths && K >= 1 && K <= SC_TRAJ_MAX_TICKS && (long long)P * ((long long)K + 1) <= SC_TRAJ_MAX_KNOTS;
}

// the common clock: tick k is at T0 + k * dt_c, k = 0 .. K
struct sc_traj_clock { double T0, dt_c; int K; };

static inline bool sc_traj_clock_ok(const sc_traj_clock& ck) { return isfinite(ck.dt_c) && ck.dt_c > 0.0 && isfinite(ck.T0); }

// ---- the radius contract ----
__host__ __device__ __forceinline__ bool sc_traj_radius_ok(double r) { return isfinite(r) && r >= 0.0; }

static inline bool sc_traj_radius_outside(const double* radius, int n) {
    for (int i = 0; i < n; ++i)
        if (!sc_traj_radius_ok(radius[i])) return true;
    return false;
}

// ---- the packed timed paths (the smoother's outputs) ----
struct sc_traj_paths {
    const double* time;
    const float* pts;
    const int32_t *offsets, *length, *status;   // status may be NULL: all OK
    const double* t0;                           // may be NULL: 0
    const int32_t* flags;                       // may be NULL: 3
    int P;
};

// what every call that reads timed paths on a clock refuses
static inline bool sc_traj_input_invalid(const sc_ctx* ctx, const sc_traj_paths& pa, const sc_traj_clock& ck, int max_paths = SC_TRAJ_MAX_PATHS) {
    return !ctx || !pa.time || !pa.pts || !pa.offsets || !pa.length || !sc_traj_size_ok(pa.P, ck.K, max_paths) || !sc_traj_clock_ok(ck);
}

// host pointers: what a device form would read out of range, or mark SC_TRAJ_BAD from the per-path arguments alone
static inline bool sc_traj_paths_outside(const sc_traj_paths& pa) {
    if (pa.offsets[0] < 0) return true;
    for (int p = 0; p < pa.P; ++p) {
        if (pa.offsets[p + 1] < pa.offsets[p]) return true;
        if (pa.t0 && !isfinite(pa.t0[p])) return true;
        if (pa.flags && (pa.flags[p] < 0 || pa.flags[p] > 3)) return true;
    }
    for (int p = 0; p < pa.P; ++p)
        if ((!pa.status || pa.status[p] == SC_SMOOTH_OK) && pa.length[p] >= 1 && (long long)pa.offsets[p] + pa.length[p] > pa.offsets[pa.P]) return true;
    return false;
}

// The seven arrays of host paths into seven consecutive slots of a `_host` call's stage: the first of them.
static inline int sc_traj_stage_paths(sc_stage& st, const sc_traj_paths& h) {
    const size_t M = (size_t)h.offsets[h.P], pb = (size_t)h.P * 4;
    const int first = st.in(h.time, M * 8);
    st.in(h.pts, M * 8), st.in(h.offsets, pb + 4), st.in(h.length, pb);
    st.in(h.status, h.status ? pb : 0), st.in(h.t0, h.t0 ? pb * 2 : 0), st.in(h.flags, h.flags ? pb : 0);
    return first;
}

// after st.upload(): the same paths on the device; an array the caller passed none of stays NULL
static inline sc_traj_paths sc_traj_staged_paths(const sc_stage& st, int i, const sc_traj_paths& h) {
    return sc_traj_paths{st.dev<const double>(i), st.dev<const float>(i + 1), st.dev<const int32_t>(i + 2), st.dev<const int32_t>(i + 3),
                         h.status ? st.dev<const int32_t>(i + 4) : nullptr, h.t0 ? st.dev<const double>(i + 5) : nullptr,
                         h.flags ? st.dev<const int32_t>(i + 6) : nullptr, h.P};
}

// the knots kernel (traj.hip): device pointers, checked by the caller, the device set
__attribute__((visibility("hidden"))) int sc_traj_launch_knots(sc_ctx* ctx, const sc_traj_paths& pa, const sc_traj_clock& ck, double* knots,
                                                              int32_t* tstatus);

// knots / tstatus the caller of a fleet call passed none of: into ctx->traj_knots
static inline int sc_traj_scratch_knots(sc_ctx* ctx, int P, int K, double** knots, int32_t** tstatus) {
    const size_t kb = *knots ? 0 : al256((size_t)P * (K + 1) * 16), sb = *tstatus ? 0 : al256((size_t)P * 4);
    if (kb + sb) {
        int r = sc_scratch_reserve(ctx, &ctx->traj_knots, kb + sb);
        if (r != SC_OK) return r;
        if (!*knots) *knots = (double*)ctx->traj_knots.p;
        if (!*tstatus) *tstatus = (int32_t*)((char*)ctx->traj_knots.p + kb);
    }
    return SC_OK;
}

// an OK path whose radius r is outside the contract becomes SC_TRAJ_BAD, in every call that reads a radius (one thread per path)
__device__ __forceinline__ void sc_traj_mark_radius(int32_t* tstatus, int p, double r) {
    if (tstatus[p] == SC_TRAJ_OK && !sc_traj_radius_ok(r)) tstatus[p] = SC_TRAJ_BAD;
}

__device__ __forceinline__ double sc_clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// The predicate of the path conflicts (the definition in include/sea_current_hip.h): on one interval
// of two linear motions whose difference goes from d0 to d1, the squared closest approach m2 at the clamped parameter lam; a
// pair conflicts on the interval when m2 < R^2.  aa, bb and lam are what the entry time of a conflict goes on from.  A knot
// that is absent is (NaN, NaN): m2 is then NaN and fails every comparison.
// This is the only statement of the operation order that the NumPy twins state product by product, and the objects of the
// three files that call it are built with -ffp-contract=off: no product and sum fuse, so the pair kernel, the table kernel
// and the reserve kernel compute the same bits from the same knots.
struct sc_traj_approach { double m2, aa, bb, lam; };

__device__ __forceinline__ sc_traj_approach sc_traj_closest(double d0x, double d0y, double d1x, double d1y) {
    const double ex = d1x - d0x, ey = d1y - d0y;
    const double aa = ex * ex + ey * ey;
    const double bb = d0x * ex + d0y * ey;
    const double lam = aa > 0.0 ? sc_clampd(-bb / aa, 0.0, 1.0) : 0.0;
    const double px = d0x + lam * ex, py = d0y + lam * ey;
    return sc_traj_approach{px * px + py * py, aa, bb, lam};
}
