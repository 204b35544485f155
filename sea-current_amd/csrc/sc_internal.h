// sc_internal.h -- context, scratch and launch-timing plumbing shared by the HIP sources.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "../../include/sea_current_hip.h"

// a grow-only device buffer of a context (sc_scratch_reserve); freed with the context
struct sc_scratch {
    void* p = nullptr;
    size_t bytes = 0;
    sc_scratch() = default;
    sc_scratch(const sc_scratch&) = delete;
    sc_scratch& operator=(const sc_scratch&) = delete;
    ~sc_scratch() { if (p) (void)hipFree(p); }
};

static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// What a context's launches tell its host: int32 words of ctx->status (device, one block per context) that kernels only ever
// set to 1 and that sc_ctx_synchronize copies into ctx->status_host, acts on and clears.
enum sc_status_word {
    SC_ST_ASTAR_OVERFLOW,   // A*: a bucket ring overflowed (the query was rerun with 16x the space): later calls start with 4x the rings
    SC_ST_EDT_OPEN_SEEN,    // EDT, rows of 513 .. 1024 pixels: a row of edt_band_k16_kernel<.., false> took the 32-bit fallback (open space)
    SC_ST_EDT_OPEN_STILL,   // the same widths: a row of the OPEN build took the site search
    SC_ST_EDT_FAULT,        // EDT, rows wider than 1024: a wavefront's bounded wait ran out, the distances of that call are incomplete
    SC_ST_COUNT
};

// hidden: the library's own types; their (inline) members are not part of the exported symbols
struct __attribute__((visibility("hidden"))) sc_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t wait_ev = nullptr;   // blocking-sync event: host waits sleep instead of spinning (one host thread per context in flight)
    int32_t *status = nullptr, *status_host = nullptr;   // [SC_ST_COUNT] on the device (zeroed) and its pinned mirror: created and freed with the context
    bool status_armed = false;       // a launch that can set a status word has been enqueued since the last sc_ctx_synchronize
    char err[256] = {0};
    // timing
    int timing = 0;
    struct pending_ev { int kid; hipEvent_t a, b; bool shared_a = false; };
    std::vector<pending_ev> pending;
    std::vector<hipEvent_t> ev_pool;
    double t_ms[SC_K_COUNT] = {0};
    int64_t t_n[SC_K_COUNT] = {0};
    // scratch: grow-only, reserved through sc_scratch_reserve (which keeps scratch_total), freed by the destructors
    size_t scratch_total = 0;
    sc_scratch host_stage;  // the _host wrappers' device copies (sc_stage), one call at a time
    sc_scratch astar_ends;  // sc_astar_gfield: int32 start, goal, len, path[1] of its one query
    sc_scratch colbits;     // EDT: uint32 [batch][nb][W]
    sc_scratch updown;      // EDT, rows wider than 1024 and rows of 513 .. 1024 in open-space mode: uint32 [batch][nb][W], rows to the nearest obstacle in the bands above / below
    sc_scratch edt_flags;   // EDT, rows wider than 1024: int32 [2][batch][bands], != 0 where a windowed pass gave a band up
    sc_scratch moves;       // A*: uint8 [H][W]
    sc_scratch gslots;      // A*: uint32 [S][g cells] (4 x 4-cell tiles)
    sc_scratch closed;      // A*: uint32 [S][bitmap words] closed set, one bit per cell (32 x 16-cell tiles)
    sc_scratch buckets;     // A*: uint32 [S][32][cap]
    sc_scratch qstats;      // A*: int32 expanded[Q] | queue order[Q] | overflow list[Q]
    sc_scratch actr;        // A*: int32 [16], [0 .. 3] queue / overflow counters of a launch ([4 .. 15] reserved, read 0)
    sc_scratch bez_tang;    // Bezier: double [P][n_max][2] tangents
    sc_scratch bez_gl;      // Bezier: 32 Gauss-Legendre nodes + 32 weights
    sc_scratch bez_seginfo; // resample: int4 [S] (first sample, last sample, spline, segment in spline)
    sc_scratch cheb_a;      // chebfit: double [rows][degree + 1], the [T | y] matrices of a batch
    sc_scratch fmt_nbr;     // FMT*: uint16 [n][256] samples in range of every sample | int32 count [n] | int32 overflow
    sc_scratch gather_msg;  // gather: this rank's message, every rank's messages, local offsets
    sc_scratch wp_spill;    // waypoints: int32 [Q][Lmax - Wmax] output points past Wmax (needed count of a truncated path)
    sc_scratch sm_ctrl;     // smoothing: float [P][n_max-1][4][2] control points of from_path before compaction
    sc_scratch sm_cum;      // smoothing: float [P (n_max-1)][nsub+1] arclength tables | float [P (n_max-1)] segment lengths
    sc_scratch sm_tp;       // smoothing: fp64 TOPP-RA inputs p0 p1 v0 v1 vlo vhi alo ahi [P] | K [P][N+1][2] x t [P][N+1] u [P][N]
    sc_scratch sm_int;      // smoothing: int32 npts [P] | TOPP-RA status [P] | resample status [P] | resample offsets [P+1] | repair status [P] (sc_smooth_paths_clear_batch)
    sc_scratch sm_smp;      // smoothing: float vel | curvature [capacity] when the caller wants ang_vel without them
    sc_scratch sm_vlim;     // smoothing with per-stage limits: fp64 vlo [P][N+1] | vhi [P][N+1]
    sc_scratch occ_prep;    // polygon occupancy: float4 box [n_obs] | int2 cell-row range [n_obs] of every obstacle
    sc_scratch fld_mask;    // cost fields: uint64 [G][tile rows][W] traversability of 64 rows per column
    sc_scratch fld_mask_old; // field repair: the same masks of the old map
    sc_scratch fld_state;   // cost fields: int32 ok [F] | stamp [F][tiles] | seeded [F][tiles] | list0, list1 [F * tiles] | ctr [rounds + 1] | left [jumps + 1]
                            // a repair lays it out anew: ok | stamp | seeded | list0, list1 | ctr | rstamp [F][tiles] | rctr [raise rounds + 1] | gflag [G][tiles] | gcount [G] | rlist0, rlist1 [F * tiles]
    sc_scratch cmp_state;   // components: int32 [G][H][W] sizes when the caller passes none | uint64 [G] largest keys
    sc_scratch cmp_start;   // screened A*: int32 [Q] the starts, -1 where the endpoints lie in different components
    sc_scratch traj_part;   // path conflicts: partial results [P][slots] of the pair kernel | uint32 [P][ceil(P/32)] when the caller passes no matrix
    sc_scratch traj_knots;  // sc_fleet_conflicts_batch without the caller's buffers: fp64 knots [P][K+1][2] | int32 tstatus [P]
    sc_scratch traj_box;    // delay schedules: fp64 [P][4] box of every path's present knots
    sc_scratch traj_table;  // sc_fleet_schedule_batch without the caller's table: uint64 [P][P]
    sc_scratch assign_t;    // assignment with more rows than columns: int32 [B][C][R], the transposed cost matrices
    sc_scratch assign_cost; // sc_fleet_assign_batch without the caller's matrix: int32 [R][F]
    sc_scratch tp_planes;   // space-time plans: uint32 [8][H][Wq], plane d = the cells with bit d of the move byte set
    sc_scratch tp_reach;    // space-time plans without the caller's reach: uint32 [B_g][L][H][Wq], the layers of one group of queries
    sc_scratch tp_state;    // space-time plans: per-query state [B_g] | int32 path [B_g][L] when only the knots are wanted
    sc_scratch fr_state;    // frontiers: int32 [G][H][W] labels when the caller passes none | int32 [G][H][W] sizes, then slots, at the roots | int32 [G][blocks] listed roots per 256 cells
    sc_scratch fr_key;      // frontier cost matrix: uint64 [F][Cmax] keys g << 32 | cell
    sc_scratch fr_fleet;    // sc_fleet_explore_batch: the intermediate arrays the caller passes none of
    sc_scratch vw_vis;      // line-of-sight sensing: uint8 [H][W], 1 where a view of the call sees the free cell
    sc_scratch vs_state;    // gain per heading: int32 c0 [N] | int32 hist [N][B] when the caller passes none
    sc_scratch sn_flags;    // range scans: uint8 [2][al256(W H)] miss and hit flags of one sc_logodds_update; all zero between calls
    sc_scratch mt_cost;     // scan matching: uint16 [H+2][W+2] + 1, the cost map of one call inside a border of unk, then a cell of 0
    sc_scratch mt_part;     // scan matching: {uint64 key, int32 count, pad} [S][R][tiles of 256 candidates]
    sc_scratch mw_pyr;      // wide scan matching: the pooled cost maps of levels 1 .. top, uint16 [H+m+1][W+m+1] each, and the half-way map of a level
    sc_scratch mw_state;    // wide scan matching: uint64 parents [2][S][max_nodes] | int32 bounds [S][max_nodes] | uint64 keys [S][R] | int32 counts [S][16] | int32 U [S][8]
    sc_scratch fp_sat;      // footprint mask: int32 [H+1][W+1] | int32 [W+H][W+H], the summed-area tables of one grid's blocked cells over (x, y) and over (x + y, y - x)
    sc_scratch pose_state;  // pose fields: int32 ok [F] | stamp [F][tiles] | list0, list1 [F * tiles] | ctr [rounds + 1]
    sc_scratch car_state;   // car fields: the layout of pose_state
    sc_scratch eg_state;    // goals by gain: state words | kw [H][W] when the caller keeps none | vis [2][H][W] | views [N][3] | best [N][2] | hist [N][B] | c0 [N] | assigned [R] | taken [N] | cost [R][N] | partials
    sc_scratch eg_centre;   // sc_frontier_centres: uint64 [G][Cmax] smallest keys
    sc_scratch eg_fleet;    // sc_fleet_explore_gain_batch: the intermediate arrays the caller passes none of
    int astar_cap = 1 << 16;         // ring entries per bucket (power of two)
    size_t astar_slot_budget = (size_t)96 << 30;  // bytes of g + bitmap + ring scratch this context may take (SC_ASTAR_SLOT_GB), further bounded by what the device has free; 4096^2: 96 GiB = 1966 slots measured best (48: -34 %, 160: -17 %)
    int traj_wg_target = 4096;      // path conflicts: workgroups a launch of the pair kernel aims for (16 per CU; SC_TRAJ_WORKGROUPS)
    bool traj_sched_noskip = false; // delay schedules: evaluate the pairs the box test would skip (SC_TRAJ_SCHED_NOSKIP=1; the tests prove the skip exact with it)
    size_t tplan_budget = (size_t)8 << 30;   // space-time plans: bytes of tp_reach a group of queries may take (SC_TPLAN_GB, 1 .. 64)
    int tplan_layers = 16;          // space-time plans: layers a launch of the step kernel advances, 1 .. 16 (SC_TPLAN_LAYERS); no output depends on it
    bool sn_flags_zeroed = false;   // range scans: the memset of the current sn_flags buffer has been enqueued
    int last_Q = 0;
    void* comm = nullptr;           // ncclComm_t of sc_allgather_paths
    bool comm_owned = false;
    int comm_ranks = 0, comm_rank = 0;
    int64_t gather_bytes = 0;       // bytes every rank received in the last gather
    std::set<const void*> big_lds_done;   // kernels whose dynamic-LDS limit this context has raised on its device
    int cu_count = 0;               // compute units of the device (0: not asked yet)
    bool edt_open_mode = false;     // EDT, rows of 513 .. 1024 pixels: this context has seen open space -> the band kernel's build with the site search
    bool edt_open_launched = false; // that build has been launched since the last sc_ctx_synchronize
    int astar_waves = 0;            // wavefronts an A* launch keeps resident (0: not yet determined)
    int astar_dual = -1;   // queries the two-wavefront A* kernel keeps resident (-1: not asked yet, 0: off)
    int astar_dual_lat = -1;   // the same for its latency build (larger LDS ring: fewer per CU)
};

#define SC_HIP(ctx, call)                                                                  \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            snprintf((ctx)->err, sizeof((ctx)->err), "%s:%d %s -> %s", __FILE__, __LINE__, #call, \
                     hipGetErrorString(e_));                                               \
            return e_ == hipErrorOutOfMemory ? SC_ERR_NOMEM : SC_ERR_HIP;                  \
        }                                                                                  \
    } while (0)

int sc_scratch_reserve(sc_ctx* ctx, sc_scratch* s, size_t bytes);

// The device copies of one `_host` call: slots laid out 256-byte aligned in ctx->host_stage.
//   sc_stage st(ctx);
//   const int i = st.in(src, bytes), o = st.out(dst, bytes);   // src / dst null: slot only, no copy
//   int r = st.upload();                                       // reserve, enqueue the uploads
//   if (r == SC_OK) r = sc_device_form(ctx, st.dev<const T>(i), ..., st.dev<T>(o));
//   return st.finish(r);                                       // ok: downloads + sc_ctx_synchronize
// Every slot, an empty one included, owns at least 256 bytes, so dev() is never null: a wrapper that hands the device
// form a null pointer says so at the call site.  finish() with an error waits for the stream (ignoring the outcome of
// the wait) and returns the error: no copy or kernel is left using the buffer when the next call reuses it.
class __attribute__((visibility("hidden"))) sc_stage {
  public:
    explicit sc_stage(sc_ctx* ctx) : ctx_(ctx) {}
    int in(const void* src, size_t bytes) {
        const int i = slot(bytes);
        if (src && bytes) up_.push_back({i, const_cast<void*>(src), bytes});
        return i;
    }
    int out(void* dst, size_t bytes) {
        const int i = slot(bytes);
        back(i, dst, bytes);
        return i;
    }
    // download `bytes` of slot i to dst at the next finish(); dst null or bytes 0: nothing
    void back(int i, void* dst, size_t bytes) {
        if (dst && bytes) down_.push_back({i, dst, bytes});
    }
    int upload();
    template <class T> T* dev(int i) const { return (T*)((char*)ctx_->host_stage.p + off_[i]); }
    int finish(int r);

  private:
    struct copy { int slot; void* host; size_t bytes; };
    int slot(size_t bytes) {
        off_.push_back(end_);
        end_ += al256(bytes ? bytes : 1);
        return (int)off_.size() - 1;
    }
    sc_ctx* ctx_;
    size_t end_ = 0;
    std::vector<size_t> off_;
    std::vector<copy> up_, down_;
};

// RAII-free timing bracket: t = sc_time_begin(ctx, kid); launch...; sc_time_end(ctx, t)
int sc_time_begin(sc_ctx* ctx, int kid);
void sc_time_end(sc_ctx* ctx, int token);
int sc_time_chain(sc_ctx* ctx, int token, int kid);

// kernels' host launchers (defined in the respective .hip files)
int sc_launch_edt(sc_ctx* ctx, const uint8_t* occ, int W, int H, int batch, int32_t* d2);
int sc_launch_moves(sc_ctx* ctx, const int32_t* d2, int W, int Hall, int H, int32_t r2, uint8_t* moves);   // Hall / H grids of H rows, stacked
// S_dev (may be NULL): a device count; blocks of segments at or past it exit (launches sized by an upper bound)
int sc_launch_arclength(sc_ctx* ctx, const float* ctrl, int S, int nsub, float* cum, float* seg_len, const int32_t* S_dev);
int sc_launch_resample(sc_ctx* ctx, const float* ctrl, const float* cum, const float* arclength, const int32_t* seg_off, int B, int S,
                       int nsub, float* profile_pos, const int32_t* prof_off, int nudge, float* pts, float* tpar, int32_t* seg,
                       float* curvature, int32_t* status, const int32_t* S_dev);
// per-stage speed limits (speed.hip); the grid of one call: d2 NULL = none
struct sc_speed_frame {
    const int32_t* d2;
    int W, H;
    float x_min, y_min, res_x, res_y;
};
// the frames every call accepts: dimensions 1 .. SC_MAX_DIM, a finite origin, finite resolutions > 0 (d2 is the caller's matter)
static inline bool sc_frame_ok(const sc_speed_frame& fr) {
    return fr.W >= 1 && fr.W <= SC_MAX_DIM && fr.H >= 1 && fr.H <= SC_MAX_DIM && isfinite(fr.x_min) && isfinite(fr.y_min) &&
           isfinite(fr.res_x) && fr.res_x > 0.f && isfinite(fr.res_y) && fr.res_y > 0.f;
}
// ns_bound: an upper bound of the legs of one path (sizes the LDS the kernel stages a path's tables in), <= 0: not known.
// vlo (may be NULL) receives vel_min per stage, vhi_copy (may be NULL) a second copy of vhi.
int sc_launch_speed_limits(sc_ctx* ctx, const float* ctrl, const float* cum, const int32_t* seg_off, const float* arclength,
                           const int32_t* status, int P, int nsub, int N, int J, const double* limits, const double* dyn,
                           const sc_speed_frame& fr, int ns_bound, double* vlo, double* vhi, double* vhi_copy, float* min_clear,
                           int32_t* status_out);
// argument checks shared by the entry points that take dyn, J and a grid
int sc_speed_args_ok(int J, const double* dyn, const sc_speed_frame& fr);
// the contract of dyn [P][4] on the host (the _host forms refuse what the kernel would mark SC_SMOOTH_BAD_INPUT)
int sc_speed_dyn_ok(const double* dyn, int P);
// curve.hip: the repair of curves that hit the grid (d2 required); status_out may be status, ctrl_out may be ctrl_in
int sc_curve_grid_ok(const sc_speed_frame& fr, int32_t r2_clear);
int sc_launch_curve_clear(sc_ctx* ctx, const float* ctrl_in, float* ctrl_out, const int32_t* seg_off, const int32_t* status, int P,
                          const sc_speed_frame& fr, int32_t r2_clear, int max_level, uint8_t* level, int32_t* rounds, int32_t* leg_min,
                          int32_t* status_out);
int sc_launch_toppra_sample_packed(sc_ctx* ctx, int P, int dof, int N, const double* p0, const double* p1, const double* v0,
                                   const double* v1, const double* x, const double* t, double dt, const int32_t* offsets,
                                   const int32_t* plen, const int32_t* skip, float* pos, float* vel, float* acc, double* times);

// Raise a kernel's dynamic-LDS limit (> 64 KiB needs hipFuncSetAttribute, which is per DEVICE): once per context, i.e.
// once per device and host thread -- a process-wide flag would leave a second GPU's copy of the kernel at the default
// and be written by several threads at once.
int sc_allow_big_lds(sc_ctx* ctx, const void* kernel, int bytes);

// wait for everything enqueued on the context's stream without burning a host core
int sc_stream_wait(sc_ctx* ctx);
void sc_edt_open_mode_update(sc_ctx* ctx, int32_t seen, int32_t still);   // the two open-space status words -> ctx->edt_open_mode (edt.hip; host only)

#ifdef __HIPCC__
__device__ __forceinline__ void wave_lds_sync() {
    // LDS operations of one wave execute in issue order; only the compiler must not reorder them.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the float32 centre of cell i of an axis with origin o and resolution r (occupancy_grid::centre_of), rounding by rounding
__device__ __forceinline__ float sc_cell_centre(int i, float o, float r) { return __fadd_rn(o, __fmul_rn(__fadd_rn((float)i, 0.5f), r)); }

// point (order 0), hodograph (1) or second derivative (2) of the cubic Bezier c [4][2] at parameter s, in fp64
__device__ __forceinline__ void bez_eval(const float* c, double s, int order, double& ox, double& oy) {
    const double r = 1 - s;
    double o[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const double p0 = c[a], p1 = c[2 + a], p2 = c[4 + a], p3 = c[6 + a];
        if (order == 0) o[a] = r * r * r * p0 + 3 * r * r * s * p1 + 3 * r * s * s * p2 + s * s * s * p3;
        else if (order == 1) o[a] = 3 * (r * r * (p1 - p0) + 2 * r * s * (p2 - p1) + s * s * (p3 - p2));
        else o[a] = 6 * (r * (p2 - 2 * p1 + p0) + s * (p3 - 2 * p2 + p1));
    }
    ox = o[0]; oy = o[1];
}
#endif
