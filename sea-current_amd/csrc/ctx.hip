// ctx.hip -- context, stream, scratch, launch timing and the `_host` convenience wrappers.
#include "sc_internal.h"
#include <stdlib.h>

extern "C" int sc_abi_version(void) { return SC_ABI_VERSION; }

extern "C" const char* sc_status_string(int s) {
    switch (s) {
        case SC_OK: return "ok";
        case SC_ERR_INVALID: return "invalid argument";
        case SC_ERR_HIP: return "HIP runtime error";
        case SC_ERR_NOMEM: return "out of device memory";
        case SC_ERR_NO_DEVICE: return "no usable device";
        default: return "unknown status";
    }
}

extern "C" const char* sc_last_error(const sc_ctx* ctx) { return ctx ? ctx->err : "null context"; }

extern "C" int sc_ctx_create(int device, sc_ctx** out) {
    if (!out) return SC_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return SC_ERR_NO_DEVICE;
    sc_ctx* c = new sc_ctx();
    c->device = device;
    // with the stream the status block (sc_status_word) and its pinned mirror: zeroed, and waited for, before anything can be enqueued
    const size_t sb = SC_ST_COUNT * sizeof(int32_t);
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void**)&c->status, sb) != hipSuccess || hipMemsetAsync(c->status, 0, sb, c->own_stream) != hipSuccess ||
        hipStreamSynchronize(c->own_stream) != hipSuccess ||
        hipHostMalloc((void**)&c->status_host, sb, hipHostMallocDefault) != hipSuccess) {
        (void)hipFree(c->status);
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
        delete c;
        return SC_ERR_HIP;
    }
    c->stream = c->own_stream;
    // scratch the A* slots of this context may take, in GiB (a slot = one resident wavefront's g array, closed bitmap and rings)
    if (const char* e = getenv("SC_ASTAR_SLOT_GB")) { const long v = atol(e); if (v >= 1 && v <= 256) c->astar_slot_budget = (size_t)v << 30; }
    // workgroups the pair kernel of the path conflicts aims for (the tests lower it so that small fleets walk several tick
    // chunks and column tiles per workgroup)
    if (const char* e = getenv("SC_TRAJ_WORKGROUPS")) { const long v = atol(e); if (v >= 1 && v <= 65536) c->traj_wg_target = (int)v; }
    // the shift table evaluates every pair, also those whose boxes are too far apart to meet (the tests compare the two)
    if (const char* e = getenv("SC_TRAJ_SCHED_NOSKIP")) c->traj_sched_noskip = atol(e) == 1;
    // space-time plans: GiB of layer scratch a group of queries may take, and the layers one launch of the step kernel advances
    // (the tests set both: several groups, and every blocking from 1 to 16)
    if (const char* e = getenv("SC_TPLAN_GB")) { const double v = atof(e); if (v > 0.0 && v <= 64.0) c->tplan_budget = (size_t)(v * 1073741824.0); }
    if (const char* e = getenv("SC_TPLAN_LAYERS")) { const long v = atol(e); if (v >= 1 && v <= 16) c->tplan_layers = (int)v; }
    *out = c;
    return SC_OK;
}

extern "C" int sc_ctx_destroy(sc_ctx* ctx) {
    if (!ctx) return SC_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)sc_comm_destroy(ctx);
    for (auto& p : ctx->pending) { if (!p.shared_a) (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->wait_ev) (void)hipEventDestroy(ctx->wait_ev);
    (void)hipStreamDestroy(ctx->own_stream);
    (void)hipFree(ctx->status); (void)hipHostFree(ctx->status_host);
    delete ctx;   // the scratch buffers free themselves
    return SC_OK;
}

extern "C" int sc_ctx_set_stream(sc_ctx* ctx, void* s) {
    if (!ctx) return SC_ERR_INVALID;
    ctx->stream = (hipStream_t)s;
    return SC_OK;
}

extern "C" int sc_ctx_use_own_stream(sc_ctx* ctx) {
    if (!ctx) return SC_ERR_INVALID;
    ctx->stream = ctx->own_stream;
    return SC_OK;
}

int sc_allow_big_lds(sc_ctx* ctx, const void* kernel, int bytes) {
    if (ctx->big_lds_done.count(kernel)) return SC_OK;
    SC_HIP(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    ctx->big_lds_done.insert(kernel);
    return SC_OK;
}

int sc_stream_wait(sc_ctx* ctx) {
    if (!ctx->wait_ev) SC_HIP(ctx, hipEventCreateWithFlags(&ctx->wait_ev, hipEventBlockingSync | hipEventDisableTiming));
    SC_HIP(ctx, hipEventRecord(ctx->wait_ev, ctx->stream));
    SC_HIP(ctx, hipEventSynchronize(ctx->wait_ev));
    return SC_OK;
}

extern "C" int sc_ctx_synchronize(sc_ctx* ctx) {
    if (!ctx) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t sb = SC_ST_COUNT * sizeof(int32_t);
    // what the launches since the last synchronisation met (sc_status_word): ONE copy, in front of the event the wait sleeps on
    const hipError_t status_copy = ctx->status_armed ? hipMemcpyAsync(ctx->status_host, ctx->status, sb, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
    const int r = sc_stream_wait(ctx);   // whatever the copy did: the caller's work is waited for
    if (r != SC_OK || !ctx->status_armed) return r;
    SC_HIP(ctx, status_copy);
    ctx->status_armed = false;
    const int32_t* st = ctx->status_host;
    int32_t any = 0;
    for (int i = 0; i < SC_ST_COUNT; ++i) any |= st[i];
    // cleared in stream order, ahead of any later launch; the outcome is looked at last, so that nothing hides a fault
    const hipError_t status_clear = any ? hipMemsetAsync(ctx->status, 0, sb, ctx->stream) : hipSuccess;
    // A* bucket rings overflowed (the overflowed queries were rerun with 16x the space on the device): larger rings from now on
    if (st[SC_ST_ASTAR_OVERFLOW] && ctx->astar_cap < (1 << 22)) ctx->astar_cap *= 4;
    sc_edt_open_mode_update(ctx, st[SC_ST_EDT_OPEN_SEEN], st[SC_ST_EDT_OPEN_STILL]);
    // the wide-row EDT kernel's wavefronts wait for one another with bounded spins: one that ran out left rows unwritten
    if (st[SC_ST_EDT_FAULT]) {
        snprintf(ctx->err, sizeof(ctx->err), "edt_band_wide_kernel: a wait between the wavefronts of a workgroup ran out; the distances of that call are incomplete");
        return SC_ERR_HIP;
    }
    SC_HIP(ctx, status_clear);
    return SC_OK;
}

int sc_scratch_reserve(sc_ctx* ctx, sc_scratch* s, size_t bytes) {
    if (bytes <= s->bytes) return SC_OK;
    if (s->p) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        SC_HIP(ctx, hipFree(s->p));
        ctx->scratch_total -= s->bytes;
        s->p = nullptr;
        s->bytes = 0;
    }
    SC_HIP(ctx, hipMalloc(&s->p, bytes));
    s->bytes = bytes;
    ctx->scratch_total += bytes;
    return SC_OK;
}

extern "C" int sc_ctx_scratch_bytes(sc_ctx* ctx, int64_t* bytes) {
    if (!ctx || !bytes) return SC_ERR_INVALID;
    *bytes = (int64_t)ctx->scratch_total;
    return SC_OK;
}

int sc_stage::upload() {
    const int r = sc_scratch_reserve(ctx_, &ctx_->host_stage, end_);
    if (r != SC_OK) return r;
    for (const copy& c : up_) SC_HIP(ctx_, hipMemcpyAsync(dev<char>(c.slot), c.host, c.bytes, hipMemcpyHostToDevice, ctx_->stream));
    up_.clear();
    return SC_OK;
}

int sc_stage::finish(int r) {
    auto download = [&]() -> int {
        for (const copy& c : down_) SC_HIP(ctx_, hipMemcpyAsync(c.host, dev<char>(c.slot), c.bytes, hipMemcpyDeviceToHost, ctx_->stream));
        return SC_OK;
    };
    if (r == SC_OK) r = download();
    down_.clear();
    if (r == SC_OK) return sc_ctx_synchronize(ctx_);
    (void)hipStreamSynchronize(ctx_->stream);
    return r;
}

// ---- timing ---------------------------------------------------------------
static hipEvent_t get_event(sc_ctx* ctx) {
    if (!ctx->ev_pool.empty()) {
        hipEvent_t e = ctx->ev_pool.back();
        ctx->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) e = nullptr;
    return e;
}

int sc_time_begin(sc_ctx* ctx, int kid) {
    if (!ctx->timing) return -1;
    sc_ctx::pending_ev p{kid, get_event(ctx), get_event(ctx)};
    if (!p.a || !p.b) {   // no event to be had: this launch goes untimed
        if (p.a) ctx->ev_pool.push_back(p.a);
        if (p.b) ctx->ev_pool.push_back(p.b);
        return -1;
    }
    (void)hipEventRecord(p.a, ctx->stream);
    ctx->pending.push_back(p);
    return (int)ctx->pending.size() - 1;
}

void sc_time_end(sc_ctx* ctx, int token) {
    if (token < 0) return;
    (void)hipEventRecord(ctx->pending[token].b, ctx->stream);
}

// end of bracket `token` and begin of a bracket for `kid` with ONE event record (back-to-back kernels)
int sc_time_chain(sc_ctx* ctx, int token, int kid) {
    if (token < 0) return -1;
    (void)hipEventRecord(ctx->pending[token].b, ctx->stream);
    sc_ctx::pending_ev p{kid, ctx->pending[token].b, get_event(ctx)};
    if (!p.b) return -1;
    p.shared_a = true;
    ctx->pending.push_back(p);
    return (int)ctx->pending.size() - 1;
}

static void drain_timing(sc_ctx* ctx) {
    for (auto& p : ctx->pending) {
        float ms = 0.f;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            ctx->t_ms[p.kid] += ms;
            ctx->t_n[p.kid] += 1;
        }
        if (!p.shared_a) ctx->ev_pool.push_back(p.a);
        ctx->ev_pool.push_back(p.b);
    }
    ctx->pending.clear();
}

extern "C" int sc_ctx_set_timing(sc_ctx* ctx, int enable) {
    if (!ctx) return SC_ERR_INVALID;
    drain_timing(ctx);
    ctx->timing = enable ? 1 : 0;
    return SC_OK;
}

extern "C" int sc_ctx_reset_timing(sc_ctx* ctx) {
    if (!ctx) return SC_ERR_INVALID;
    drain_timing(ctx);
    for (int i = 0; i < SC_K_COUNT; ++i) { ctx->t_ms[i] = 0; ctx->t_n[i] = 0; }
    return SC_OK;
}

extern "C" int sc_ctx_get_timing(sc_ctx* ctx, int kid, double* total_ms, int64_t* launches) {
    if (!ctx || kid < 0 || kid >= SC_K_COUNT) return SC_ERR_INVALID;
    drain_timing(ctx);
    if (total_ms) *total_ms = ctx->t_ms[kid];
    if (launches) *launches = ctx->t_n[kid];
    return SC_OK;
}

// ---- host wrappers: argument checks, then sc_stage (sc_internal.h) around the device form ---------------------------
extern "C" int sc_edt_u8_i32_host(sc_ctx* ctx, const uint8_t* occ, int W, int H, int batch, int32_t* d2) {
    if (!ctx || !occ || !d2 || W <= 0 || H <= 0 || batch <= 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H * batch;
    sc_stage st(ctx);
    const int i_occ = st.in(occ, n), o_d2 = st.out(d2, n * 4);
    int r = st.upload();
    if (r == SC_OK) r = sc_edt_u8_i32(ctx, st.dev<const uint8_t>(i_occ), W, H, batch, st.dev<int32_t>(o_d2));
    return st.finish(r);
}

extern "C" int sc_astar_batch_host(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2,
                                   const int32_t* start, const int32_t* goal, int Q, int Lmax,
                                   int32_t* path, int32_t* len, int32_t* cost, int32_t* status) {
    if (!ctx || !d2 || !start || !goal || !path || !len || !cost || !status || W <= 0 || H <= 0 || Q < 0 || Lmax <= 0)
        return SC_ERR_INVALID;
    if (Q == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H, qb = (size_t)Q * 4;
    sc_stage st(ctx);
    const int i_d2 = st.in(d2, n * 4), i_s = st.in(start, qb), i_g = st.in(goal, qb);
    const int o_path = st.out(path, qb * Lmax), o_len = st.out(len, qb), o_cost = st.out(cost, qb), o_st = st.out(status, qb);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_astar_batch(ctx, st.dev<const int32_t>(i_d2), W, H, r2, st.dev<const int32_t>(i_s), st.dev<const int32_t>(i_g), Q, Lmax,
                           st.dev<int32_t>(o_path), st.dev<int32_t>(o_len), st.dev<int32_t>(o_cost), st.dev<int32_t>(o_st));
    return st.finish(r);
}

extern "C" int sc_path_waypoints_batch_host(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear, const int32_t* path,
                                            const int32_t* len, const int32_t* astar_status, int Q, int Lmax, int Wmax, int32_t* wp,
                                            int32_t* n_wp, int32_t* status) {
    if (!ctx || !d2 || !path || !len || !wp || !n_wp || !status || W <= 0 || H <= 0 || Q < 0 || Lmax <= 0 || Wmax <= 0)
        return SC_ERR_INVALID;
    if (Q == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H, qb = (size_t)Q * 4;
    sc_stage st(ctx);
    const int i_d2 = st.in(d2, n * 4), i_p = st.in(path, qb * Lmax), i_len = st.in(len, qb), i_as = st.in(astar_status, qb);
    const int o_wp = st.out(wp, qb * Wmax), o_n = st.out(n_wp, qb), o_st = st.out(status, qb);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_path_waypoints_batch(ctx, st.dev<const int32_t>(i_d2), W, H, r2_clear, st.dev<const int32_t>(i_p), st.dev<const int32_t>(i_len),
                                    astar_status ? st.dev<const int32_t>(i_as) : nullptr, Q, Lmax, Wmax, st.dev<int32_t>(o_wp),
                                    st.dev<int32_t>(o_n), st.dev<int32_t>(o_st));
    return st.finish(r);
}

extern "C" int sc_toppra_hermite_batch_host(sc_ctx* ctx, int P, int dof, int N,
                                            const double* p0, const double* p1, const double* v0, const double* v1,
                                            const double* vlim_lo, const double* vlim_hi, int vlim_per_stage,
                                            const double* alim_lo, const double* alim_hi,
                                            double sd_start, double sd_end,
                                            double* K, double* x, double* u, double* t, int32_t* status) {
    if (!ctx || P <= 0 || dof <= 0 || N <= 0 || !p0 || !p1 || !v0 || !v1 || !vlim_lo || !vlim_hi || !alim_lo ||
        !alim_hi || !K || !x || !u || !t || !status)
        return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pd = (size_t)P * dof * 8, vl = vlim_per_stage ? pd * (N + 1) : pd, kb = (size_t)P * (N + 1) * 8;
    sc_stage st(ctx);
    const int i_p0 = st.in(p0, pd), i_p1 = st.in(p1, pd), i_v0 = st.in(v0, pd), i_v1 = st.in(v1, pd), i_vlo = st.in(vlim_lo, vl),
              i_vhi = st.in(vlim_hi, vl), i_alo = st.in(alim_lo, pd), i_ahi = st.in(alim_hi, pd);
    const int o_K = st.out(K, 2 * kb), o_x = st.out(x, kb), o_u = st.out(u, (size_t)P * N * 8), o_t = st.out(t, kb),
              o_st = st.out(status, (size_t)P * 4);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_toppra_hermite_batch(ctx, P, dof, N, st.dev<const double>(i_p0), st.dev<const double>(i_p1), st.dev<const double>(i_v0),
                                    st.dev<const double>(i_v1), st.dev<const double>(i_vlo), st.dev<const double>(i_vhi), vlim_per_stage,
                                    st.dev<const double>(i_alo), st.dev<const double>(i_ahi), sd_start, sd_end, st.dev<double>(o_K),
                                    st.dev<double>(o_x), st.dev<double>(o_u), st.dev<double>(o_t), st.dev<int32_t>(o_st));
    return st.finish(r);
}

extern "C" int sc_toppra_sample_batch_host(sc_ctx* ctx, int P, int dof, int N,
                                           const double* p0, const double* p1, const double* v0, const double* v1,
                                           const double* x, const double* t, double dt, int max_len,
                                           float* pos, float* vel, float* acc, double* times, int32_t* length) {
    if (!ctx || P <= 0 || dof <= 0 || N <= 0 || max_len <= 0 || !p0 || !p1 || !v0 || !v1 || !x || !t || !pos ||
        !vel || !acc || !times || !length)
        return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pd = (size_t)P * dof * 8, xs = (size_t)P * (N + 1) * 8, fb = (size_t)P * dof * max_len * 4;
    sc_stage st(ctx);
    const int i_p0 = st.in(p0, pd), i_p1 = st.in(p1, pd), i_v0 = st.in(v0, pd), i_v1 = st.in(v1, pd), i_x = st.in(x, xs), i_t = st.in(t, xs);
    const int o_pos = st.out(pos, fb), o_vel = st.out(vel, fb), o_acc = st.out(acc, fb), o_tim = st.out(times, (size_t)P * max_len * 8),
              o_len = st.out(length, (size_t)P * 4);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_toppra_sample_batch(ctx, P, dof, N, st.dev<const double>(i_p0), st.dev<const double>(i_p1), st.dev<const double>(i_v0),
                                   st.dev<const double>(i_v1), st.dev<const double>(i_x), st.dev<const double>(i_t), dt, max_len,
                                   st.dev<float>(o_pos), st.dev<float>(o_vel), st.dev<float>(o_acc), st.dev<double>(o_tim),
                                   st.dev<int32_t>(o_len));
    return st.finish(r);
}

extern "C" int sc_bezier_from_path_batch_host(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, float start_angle,
                                              const float* lines, int nlines, float* ctrl) {
    if (!ctx || !path || !npts || !ctrl || P <= 0 || n_max < 2 || nlines < 0 || (nlines > 0 && !lines)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_path = st.in(path, (size_t)P * n_max * 8), i_npts = st.in(npts, (size_t)P * 4), i_l = st.in(lines, (size_t)nlines * 16);
    const int o_ctrl = st.out(ctrl, (size_t)P * (n_max - 1) * 32);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_bezier_from_path_batch(ctx, st.dev<const float>(i_path), st.dev<const int32_t>(i_npts), P, n_max, start_angle,
                                      nlines ? st.dev<const float>(i_l) : nullptr, nlines, st.dev<float>(o_ctrl));
    return st.finish(r);
}

extern "C" int sc_bezier_arclength_batch_host(sc_ctx* ctx, const float* ctrl, int S, int nsub, float* cum, float* seg_len) {
    if (!ctx || !ctrl || !cum || !seg_len || S <= 0 || nsub <= 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_ctrl = st.in(ctrl, (size_t)S * 32), o_cum = st.out(cum, (size_t)S * (nsub + 1) * 4), o_len = st.out(seg_len, (size_t)S * 4);
    int r = st.upload();
    if (r == SC_OK) r = sc_bezier_arclength_batch(ctx, st.dev<const float>(i_ctrl), S, nsub, st.dev<float>(o_cum), st.dev<float>(o_len));
    return st.finish(r);
}

extern "C" int sc_bezier_resample_batch_host(sc_ctx* ctx, const float* ctrl, const float* cum, const float* arclength,
                                             const int32_t* seg_off, int B, int S, int nsub, float* profile_pos, const int32_t* prof_off,
                                             int nudge, float* pts, float* tpar, int32_t* seg, float* curvature, int32_t* status) {
    if (!ctx || !ctrl || !cum || !arclength || !seg_off || !profile_pos || !prof_off || !status || B <= 0 || S <= 0 || nsub <= 0)
        return SC_ERR_INVALID;
    if (seg_off[B] != S || seg_off[0] != 0 || prof_off[0] != 0 || prof_off[B] < 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t M = (size_t)prof_off[B], bb = (size_t)B * 4;
    sc_stage st(ctx);
    const int i_ctrl = st.in(ctrl, (size_t)S * 32), i_cum = st.in(cum, (size_t)S * (nsub + 1) * 4), i_al = st.in(arclength, bb),
              i_so = st.in(seg_off, bb + 4), i_po = st.in(prof_off, bb + 4), io_pp = st.in(profile_pos, M * 4);
    st.back(io_pp, profile_pos, M * 4);
    const int o_pts = st.out(pts, M * 8), o_t = st.out(tpar, M * 4), o_sg = st.out(seg, M * 4), o_cv = st.out(curvature, M * 4),
              o_st = st.out(status, bb);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_bezier_resample_batch(ctx, st.dev<const float>(i_ctrl), st.dev<const float>(i_cum), st.dev<const float>(i_al),
                                     st.dev<const int32_t>(i_so), B, S, nsub, st.dev<float>(io_pp), st.dev<const int32_t>(i_po), nudge,
                                     pts ? st.dev<float>(o_pts) : nullptr, tpar ? st.dev<float>(o_t) : nullptr,
                                     seg ? st.dev<int32_t>(o_sg) : nullptr, curvature ? st.dev<float>(o_cv) : nullptr, st.dev<int32_t>(o_st));
    return st.finish(r);
}

extern "C" int sc_bezier_eval_batch_host(sc_ctx* ctx, const float* ctrl, int S, const int32_t* seg, const float* t, int M, int order,
                                         float* out) {
    if (!ctx || !ctrl || !seg || !t || !out || S <= 0 || M <= 0) return SC_ERR_INVALID;
    for (int i = 0; i < M; ++i)
        if (seg[i] < 0 || seg[i] >= S) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_ctrl = st.in(ctrl, (size_t)S * 32), i_seg = st.in(seg, (size_t)M * 4), i_t = st.in(t, (size_t)M * 4), o = st.out(out, (size_t)M * 8);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_bezier_eval_batch(ctx, st.dev<const float>(i_ctrl), st.dev<const int32_t>(i_seg), st.dev<const float>(i_t), M, order, st.dev<float>(o));
    return st.finish(r);
}

extern "C" int sc_bezier_shrink_tangent_batch_host(sc_ctx* ctx, const float* T, const float* Wp, int M, float k, const float* lines, int nlines,
                                                   float* out) {
    if (!ctx || !T || !Wp || !out || M <= 0 || nlines < 0 || (nlines > 0 && !lines)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_T = st.in(T, (size_t)M * 8), i_W = st.in(Wp, (size_t)M * 8), i_l = st.in(lines, (size_t)nlines * 16), o = st.out(out, (size_t)M * 8);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_bezier_shrink_tangent_batch(ctx, st.dev<const float>(i_T), st.dev<const float>(i_W), M, k,
                                           nlines ? st.dev<const float>(i_l) : nullptr, nlines, st.dev<float>(o));
    return st.finish(r);
}

extern "C" int sc_fmt_star_batch_host(sc_ctx* ctx, const float* samples, int n, const float* starts, const float* goals, int Q, float rn,
                                      const float* lines, int E, int Lmax, float* path, int32_t* len, float* cost, int32_t* status) {
    if (!ctx || !samples || !starts || !goals || !path || !len || !cost || !status || n < 0 || Q < 0 || E < 0 || (E > 0 && !lines) ||
        Lmax <= 0)
        return SC_ERR_INVALID;
    if (Q == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t qb = (size_t)Q * 4;
    sc_stage st(ctx);
    const int i_s = st.in(samples, (size_t)n * 8), i_st = st.in(starts, 2 * qb), i_g = st.in(goals, 2 * qb), i_l = st.in(lines, (size_t)E * 16);
    const int o_p = st.out(path, 2 * qb * Lmax), o_len = st.out(len, qb), o_c = st.out(cost, qb), o_st = st.out(status, qb);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_fmt_star_batch(ctx, st.dev<const float>(i_s), n, st.dev<const float>(i_st), st.dev<const float>(i_g), Q, rn, st.dev<const float>(i_l),
                              E, Lmax, st.dev<float>(o_p), st.dev<int32_t>(o_len), st.dev<float>(o_c), st.dev<int32_t>(o_st));
    return st.finish(r);
}

extern "C" int sc_bezier_curve_batch_host(sc_ctx* ctx, const float* ctrl, int S, int degree, const int32_t* seg, const float* t, int M, float* out) {
    if (!ctx || !ctrl || !seg || !t || !out || S <= 0 || M <= 0 || degree < 1 || degree > SC_BEZIER_MAX_DEGREE) return SC_ERR_INVALID;
    for (int i = 0; i < M; ++i)
        if (seg[i] < 0 || seg[i] >= S) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_ctrl = st.in(ctrl, (size_t)S * (degree + 1) * 8), i_seg = st.in(seg, (size_t)M * 4), i_t = st.in(t, (size_t)M * 4),
              o = st.out(out, (size_t)M * 8);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_bezier_curve_batch(ctx, st.dev<const float>(i_ctrl), degree, st.dev<const int32_t>(i_seg), st.dev<const float>(i_t), M, st.dev<float>(o));
    return st.finish(r);
}

extern "C" int sc_chebfit_batch_host(sc_ctx* ctx, const float* x, const float* y, const int32_t* off, int B, int degree, float* coef, float* xrange) {
    if (!ctx || !x || !y || !off || !coef || !xrange || B <= 0 || degree < 1 || degree > SC_CHEB_MAX_DEGREE || off[0] != 0 || off[B] <= 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)off[B];
    sc_stage st(ctx);
    const int i_x = st.in(x, n * 4), i_y = st.in(y, n * 4), i_off = st.in(off, (size_t)(B + 1) * 4);
    const int o_c = st.out(coef, (size_t)B * degree * 4), o_r = st.out(xrange, (size_t)B * 8);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_chebfit_batch(ctx, st.dev<const float>(i_x), st.dev<const float>(i_y), st.dev<const int32_t>(i_off), B, (int)n, degree,
                             st.dev<float>(o_c), st.dev<float>(o_r));
    return st.finish(r);
}

extern "C" int sc_chebeval_batch_host(sc_ctx* ctx, const float* x, const int32_t* off, int B, int degree, const float* coef, const float* xrange,
                                      float* y) {
    if (!ctx || !x || !off || !coef || !xrange || !y || B <= 0 || degree < 1 || degree > SC_CHEB_MAX_DEGREE || off[0] != 0 || off[B] <= 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)off[B];
    sc_stage st(ctx);
    const int i_x = st.in(x, n * 4), i_off = st.in(off, (size_t)(B + 1) * 4), i_c = st.in(coef, (size_t)B * degree * 4),
              i_r = st.in(xrange, (size_t)B * 8), o_y = st.out(y, n * 4);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_chebeval_batch(ctx, st.dev<const float>(i_x), st.dev<const int32_t>(i_off), B, degree, st.dev<const float>(i_c),
                              st.dev<const float>(i_r), st.dev<float>(o_y));
    return st.finish(r);
}
