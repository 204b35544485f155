// tplan.hip -- re-planning in (cell, time) around the scheduled fleet: reservations rasterised from timed paths, an exact
// earliest-arrival search on the time-expanded grid, and the two chained (sc_traj_reserve_batch, sc_tplan_batch,
// sc_fleet_replan_batch; the definition is in include/sea_current_hip.h and DESIGN.md section 20).
//
// Reserve: a wavefront per (path, interval).  It clips the capsule's cell box to the grid, widens it to whole 32-cell words,
// and walks it two words at a time: lane = cell, the predicate of the path conflicts (sc_traj_closest) per cell, __ballot, and the
// lanes 0 and 32 OR their halves into layers k and k+1.  The box is a superset of the hit cells (its margin covers the
// float32 rounding of the cell centres), so the result equals the definition, which tests every cell.
// Planes: one pass over the move bytes, __ballot per direction: plane d = the cells with bit d of the move byte set.
// Step: the layer update is a 3 x 3 bit dilation.  Legal moves are symmetric (s -> c is legal iff c -> s is: the same two
// side cells guard a diagonal both ways), so "some s in reach with bit d of moves[s] set and s + delta_d == c" is
// "c - delta_d in reach and bit opp(d) of moves[c] set": a thread needs the planes of its own word only and keeps them in
// registers for all the layers of a launch.  A workgroup owns a tile of TP_TH rows x TP_TW words of one query, loads it with a
// halo of h rows and one word into LDS and advances up to h layers, reading one reservation word and writing one reach word
// per layer; what the missing neighbours beyond the halo spoil moves inwards one cell per layer and never reaches the
// interior.  Launches are ordered on the stream: nothing waits across workgroups.
// Arrival: the thread that owns the goal's word tests the goal's bit after each layer and stores the layer once (a single
// writer).  Workgroups of later launches read it and leave; a workgroup never acts on a value of its own launch (that value
// is larger than the launch's base layer), so every layer up to the arrival is complete.
// Read-out: one thread per query walks back from (goal, arrive), waits first, then the directions in order.
//
// Compiled with -ffp-contract=off: the reservation predicate is the one of traj.hip (sc_traj_closest of traj_common.h), without fused multiply-adds.
#include "traj_common.h"

#define TP_TW 8                      // interior words of a tile (256 cells)
#define TP_TH 64                     // interior rows of a tile
#define TP_HMAX 16                   // layers per launch, at most: the halo of one word (32 cells) and h rows covers them
#define TP_LW (TP_TW + 2)            // tile words with the halo
#define TP_SW (TP_LW + 2)            // LDS row: a zero word on either side, so that neighbours are read without a test
#define TP_ROWS_MAX (TP_TH + 2 * TP_HMAX)
#define TP_THREADS 256
#define TP_WPT ((TP_ROWS_MAX * TP_LW + TP_THREADS - 1) / TP_THREADS)   // tile words per thread
#define TP_MAX_B 65536
#define TP_MAX_L 65536

// per-query state of a search (context scratch)
struct tp_q {
    int32_t start, goal, t_start, t_min;   // t_min = max(t_start, t_hold)
    int32_t arr;                           // -1: searching, >= 0: the arrival layer, -2: no search (status says why)
    int32_t status;
};

// ---- reserve ---------------------------------------------------------------------------------------------------------
struct tp_reserve_args {
    const double* knots;
    int32_t* tstatus;          // may be NULL: all OK
    const double* radius;
    const int32_t* select;     // may be NULL: all
    int P, K;
    double pad;
    sc_speed_frame fr;         // d2 is not read
    int Wq, margin;
    uint32_t* res;
};

__global__ void __launch_bounds__(256) tplan_reserve_kernel(tp_reserve_args a) {
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // (path, interval), wavefront-uniform
    if (item >= (long long)a.P * a.K) return;
    const int q = (int)(item / a.K), k = (int)(item % a.K);
    const double r = a.radius[q];
    if (!sc_traj_radius_ok(r)) {   // every wavefront of q leaves on the radius alone
        if (a.tstatus && k == 0 && lane == 0) sc_traj_mark_radius(a.tstatus, q, r);
        return;
    }
    if ((a.tstatus && a.tstatus[q] != SC_TRAJ_OK) || (a.select && a.select[q] == 0)) return;
    const double* kn = a.knots + ((size_t)q * (a.K + 1) + k) * 2;
    const double ax = kn[0], ay = kn[1], bx = kn[2], by = kn[3];
    if (isnan(ax) || isnan(ay) || isnan(bx) || isnan(by)) return;
    const double R = r + a.pad, RR = R * R;
    // the cell box: centres within R of the segment's box, `margin` cells wider than the exact one
    const sc_speed_frame& f = a.fr;
    const double fx0 = ((fmin(ax, bx) - R) - (double)f.x_min) / (double)f.res_x - 0.5, fx1 = ((fmax(ax, bx) + R) - (double)f.x_min) / (double)f.res_x - 0.5;
    const double fy0 = ((fmin(ay, by) - R) - (double)f.y_min) / (double)f.res_y - 0.5, fy1 = ((fmax(ay, by) + R) - (double)f.y_min) / (double)f.res_y - 0.5;
    if (!(fx1 >= fx0) || !(fy1 >= fy0)) return;   // not finite
    const int x0 = (int)sc_clampd(floor(fx0) - a.margin, 0.0, (double)f.W), x1 = (int)sc_clampd(ceil(fx1) + a.margin, -1.0, (double)(f.W - 1));
    const int y0 = (int)sc_clampd(floor(fy0) - a.margin, 0.0, (double)f.H), y1 = (int)sc_clampd(ceil(fy1) + a.margin, -1.0, (double)(f.H - 1));
    if (x1 < x0 || y1 < y0) return;
    const int w0 = x0 >> 5, nw = (x1 >> 5) - w0 + 1;        // words of a box row
    const int np = (nw + 1) >> 1;                           // word pairs of a box row
    const size_t layer = (size_t)f.H * a.Wq;
    uint32_t* l0 = a.res + (size_t)k * layer;
    const long long n = (long long)(y1 - y0 + 1) * np;
    for (long long i = 0; i < n; ++i) {                     // wavefront-uniform
        const int y = y0 + (int)(i / np), w = w0 + 2 * (int)(i % np) + (lane >> 5);
        const int x = w * 32 + (lane & 31);
        bool hit = false;
        if (x >= x0 && x <= x1) {
            const double cx = (double)sc_cell_centre(x, f.x_min, f.res_x), cy = (double)sc_cell_centre(y, f.y_min, f.res_y);
            hit = sc_traj_closest(ax - cx, ay - cy, bx - cx, by - cy).m2 < RR;
        }
        const unsigned long long m = __ballot(hit);
        const uint32_t word = (uint32_t)(m >> (lane & 32));
        if ((lane & 31) == 0 && word) {
            uint32_t* p = l0 + (size_t)y * a.Wq + w;
            atomicOr(p, word);
            atomicOr(p + layer, word);
        }
    }
}

// ---- planes ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tplan_planes_kernel(const uint8_t* __restrict__ moves, int W, int H, int Wq, uint32_t* __restrict__ planes) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, lane = threadIdx.x & 63;
    const uint32_t b = x < W ? moves[(size_t)y * W + x] : 0u;
    const int w = (x >> 5);   // the word of this lane's half of the wavefront
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const unsigned long long m = __ballot((b >> d) & 1u);
        if ((lane & 31) == 0 && w < Wq) planes[((size_t)d * H + y) * Wq + w] = (uint32_t)(m >> (lane & 32));
    }
}

// ---- search ----------------------------------------------------------------------------------------------------------
struct tp_init_args {
    const int32_t* d2;
    int W, H, Wq, L;
    int32_t rmin;
    const uint32_t* res;   // may be NULL
    const int32_t *start, *goal, *t_start;
    int hold;
    tp_q* qs;
};

// one workgroup per query: the status that needs no search, t_hold from the goal's column of res
__global__ void __launch_bounds__(256) tplan_init_kernel(tp_init_args a) {
    __shared__ int s_last[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int s = a.start[b], g = a.goal[b], ts = a.t_start ? a.t_start[b] : 0;
    const int cells = a.W * a.H;
    const size_t layer = (size_t)a.H * a.Wq;
    const bool ends_ok = s >= 0 && s < cells && g >= 0 && g < cells && ts >= 0 && ts < a.L && a.d2[s] >= a.rmin && a.d2[g] >= a.rmin;   // block-uniform
    int last = -1;   // the last layer at which the goal is reserved
    if (ends_ok && a.hold && a.res) {
        const size_t gw = (size_t)(g / a.W) * a.Wq + ((g % a.W) >> 5);
        const uint32_t gb = 1u << ((g % a.W) & 31);
        for (int t = tid; t < a.L; t += 256)
            if (a.res[t * layer + gw] & gb) last = t;   // ascending per thread
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) last = max(last, __shfl_xor(last, o));
    if ((tid & 63) == 0) s_last[tid >> 6] = last;
    __syncthreads();
    if (tid != 0) return;
    last = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
    tp_q o;
    o.start = s; o.goal = g; o.t_start = ts;
    const int t_hold = last + 1;
    o.t_min = ts > t_hold ? ts : t_hold;
    o.arr = -2;
    if (!ends_ok) o.status = SC_TP_BAD_ENDPOINT;
    else {
        const size_t sw = (size_t)(s / a.W) * a.Wq + ((s % a.W) >> 5);
        if (a.res && (a.res[ts * layer + sw] >> ((s % a.W) & 31) & 1u)) o.status = SC_TP_START_BLOCKED;
        else {
            o.status = SC_TP_NO_PATH;   // until a layer holds the goal
            o.arr = -1;
            if (s == g && ts >= t_hold) { o.arr = ts; o.status = SC_TP_OK; }
        }
    }
    a.qs[b] = o;
}

// reach[t_start] = {start}: the whole layer is written
__global__ void __launch_bounds__(256) tplan_seed_kernel(const tp_q* __restrict__ qs, int W, size_t layer, int L, uint32_t* __restrict__ reach) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= layer) return;
    const tp_q q = qs[blockIdx.y];
    if (q.arr == -2) return;
    const int Wq = (W + 31) >> 5;
    const size_t sw = (size_t)(q.start / W) * Wq + ((q.start % W) >> 5);
    reach[((size_t)blockIdx.y * L + q.t_start) * layer + i] = i == sw ? 1u << ((q.start % W) & 31) : 0u;
}

struct tp_step_args {
    const uint32_t* planes;   // [8][H][Wq]
    const uint32_t* res;      // [L][H][Wq], may be NULL
    uint32_t* reach;          // [B_g][L][H][Wq]
    tp_q* qs;
    int W, H, Wq, L, tiles_x;
    int t0, n, h;             // this launch: layers t0 + 1 .. t0 + n from layer t0; halo rows
};

__global__ void __launch_bounds__(TP_THREADS) tplan_step_kernel(tp_step_args a) {
    __shared__ uint32_t s_r[2][(TP_ROWS_MAX + 2) * TP_SW];
    const int b = blockIdx.y, tid = threadIdx.x;
    const tp_q q = a.qs[b];
    const int base = q.t_start > a.t0 ? q.t_start : a.t0;
    if (q.arr == -2 || (q.arr >= 0 && q.arr <= base)) return;   // block-uniform; an arrival of this launch is > base
    const int t_end = a.t0 + a.n;
    if (base >= t_end) return;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const int nrows = TP_TH + 2 * a.h, nwords = nrows * TP_LW;
    const size_t layer = (size_t)a.H * a.Wq;
    uint32_t* rq = a.reach + (size_t)b * a.L * layer;
    for (int i = tid; i < 2 * (TP_ROWS_MAX + 2) * TP_SW; i += TP_THREADS) (&s_r[0][0])[i] = 0u;
    __syncthreads();
    // the goal's word, when this tile's interior holds it
    const int gx = q.goal % a.W, gy_goal = q.goal / a.W;
    uint32_t pl[TP_WPT][8];
    size_t goff[TP_WPT];
    int sidx[TP_WPT];
    bool in[TP_WPT], inner[TP_WPT], is_goal[TP_WPT];
#pragma unroll
    for (int j = 0; j < TP_WPT; ++j) {
        const int idx = tid + j * TP_THREADS;
        const int ly = idx / TP_LW, lw = idx % TP_LW;
        const int gy = ty * TP_TH - a.h + ly, gw = tx * TP_TW - 1 + lw;
        in[j] = idx < nwords && gy >= 0 && gy < a.H && gw >= 0 && gw < a.Wq;
        inner[j] = in[j] && ly >= a.h && ly < a.h + TP_TH && lw >= 1 && lw <= TP_TW;
        is_goal[j] = inner[j] && gy == gy_goal && gw == (gx >> 5);
        goff[j] = in[j] ? (size_t)gy * a.Wq + gw : 0;
        sidx[j] = (ly + 1) * TP_SW + lw + 1;
        // plane of the opposite direction: 0 <-> 1, 2 <-> 3, 4 <-> 7, 5 <-> 6
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int od = d < 4 ? (d ^ 1) : 11 - d;
            pl[j][d] = in[j] ? a.planes[(size_t)od * layer + goff[j]] : 0u;
        }
        if (in[j]) s_r[0][sidx[j]] = rq[(size_t)base * layer + goff[j]];
    }
    const uint32_t gbit = 1u << (gx & 31);
    bool found = false;
    int cur = 0;
    uint32_t rs[TP_WPT];   // the reservation words of layer t, loaded one layer ahead
#pragma unroll
    for (int j = 0; j < TP_WPT; ++j) rs[j] = (in[j] && a.res) ? a.res[(size_t)(base + 1) * layer + goff[j]] : 0u;
    for (int t = base + 1; t <= t_end; ++t) {
        uint32_t rn[TP_WPT];
#pragma unroll
        for (int j = 0; j < TP_WPT; ++j) rn[j] = (in[j] && a.res && t < t_end) ? a.res[(size_t)(t + 1) * layer + goff[j]] : 0u;
        __syncthreads();   // layer t - 1 is in s_r[cur]; s_r[cur ^ 1] has been read
        const uint32_t* s = s_r[cur];
        uint32_t* o = s_r[cur ^ 1];
#pragma unroll
        for (int j = 0; j < TP_WPT; ++j) {
            if (!in[j]) continue;
            const int i = sidx[j];
            const uint32_t ul = s[i - TP_SW - 1], uc = s[i - TP_SW], ur = s[i - TP_SW + 1];   // row y - 1
            const uint32_t ml = s[i - 1], mc = s[i], mr = s[i + 1];
            const uint32_t dl = s[i + TP_SW - 1], dc = s[i + TP_SW], dr = s[i + TP_SW + 1];   // row y + 1
            // d: dx = {1,-1,0,0,1,-1,1,-1}, dy = {0,0,1,-1,1,1,-1,-1}; a step in direction d comes from (x - dx, y - dy)
            uint32_t v = mc;
            v |= ((mc << 1) | (ml >> 31)) & pl[j][0];
            v |= ((mc >> 1) | (mr << 31)) & pl[j][1];
            v |= uc & pl[j][2];
            v |= dc & pl[j][3];
            v |= ((uc << 1) | (ul >> 31)) & pl[j][4];
            v |= ((uc >> 1) | (ur << 31)) & pl[j][5];
            v |= ((dc << 1) | (dl >> 31)) & pl[j][6];
            v |= ((dc >> 1) | (dr << 31)) & pl[j][7];
            v &= ~rs[j];
            o[i] = v;
            if (inner[j]) rq[(size_t)t * layer + goff[j]] = v;
            if (is_goal[j] && !found && t >= q.t_min && (v & gbit)) {
                found = true;
                a.qs[b].arr = t;
                a.qs[b].status = SC_TP_OK;
            }
        }
        cur ^= 1;
#pragma unroll
        for (int j = 0; j < TP_WPT; ++j) rs[j] = rn[j];
    }
}

struct tp_read_args {
    const tp_q* qs;
    const uint32_t* reach;
    const uint8_t* moves;
    int W, H, Wq, L, B;
    int32_t *path, *len, *arrive, *status;   // of this group; path may be NULL
};

__device__ __forceinline__ bool tp_bit(const uint32_t* layer, int Wq, int x, int y) { return layer[(size_t)y * Wq + (x >> 5)] >> (x & 31) & 1u; }

__global__ void __launch_bounds__(64) tplan_read_kernel(tp_read_args a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const tp_q q = a.qs[b];
    const bool ok = q.status == SC_TP_OK;
    a.status[b] = q.status;
    if (a.arrive) a.arrive[b] = ok ? q.arr : -1;
    if (a.len) a.len[b] = ok ? q.arr - q.t_start + 1 : 0;
    if (!ok || !a.path) return;
    const size_t layer = (size_t)a.H * a.Wq;
    const uint32_t* rq = a.reach + (size_t)b * a.L * layer;
    int32_t* path = a.path + (size_t)b * a.L;
    int x = q.goal % a.W, y = q.goal / a.W;
    path[q.arr - q.t_start] = q.goal;
    for (int t = q.arr; t > q.t_start; --t) {
        const uint32_t* prev = rq + (size_t)(t - 1) * layer;
        if (!tp_bit(prev, a.Wq, x, y)) {   // no wait: the first direction whose source was reached and may step here
            int px = x, py = y;
            for (int d = 0; d < 8; ++d) {
                const int dx = (0xA2 >> d & 1) ? -1 : ((0x51 >> d & 1) ? 1 : 0);        // {1,-1,0,0,1,-1,1,-1}
                const int dy = (0x34 >> d & 1) ? 1 : ((0xC8 >> d & 1) ? -1 : 0);        // {0,0,1,-1,1,1,-1,-1}
                const int sx = x - dx, sy = y - dy;
                if (sx < 0 || sx >= a.W || sy < 0 || sy >= a.H) continue;
                if (tp_bit(prev, a.Wq, sx, sy) && (a.moves[(size_t)sy * a.W + sx] >> d & 1)) { px = sx; py = sy; break; }
            }
            x = px; y = py;
        }
        path[t - 1 - q.t_start] = y * a.W + x;
    }
}

struct tp_knots_args {
    const tp_q* qs;
    const int32_t* path;
    int L, B, hold;
    sc_speed_frame fr;
    double* knots_out;
};

__global__ void __launch_bounds__(256) tplan_knots_kernel(tp_knots_args a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.B * a.L) return;
    const int b = (int)(i / a.L), t = (int)(i % a.L);
    const tp_q q = a.qs[b];
    int c = -1;
    if (q.status == SC_TP_OK && t >= q.t_start) {
        if (t <= q.arr) c = a.path[(size_t)b * a.L + t - q.t_start];
        else if (a.hold) c = q.goal;
    }
    double x = NAN, y = NAN;
    if (c >= 0) { x = (double)sc_cell_centre(c % a.fr.W, a.fr.x_min, a.fr.res_x); y = (double)sc_cell_centre(c / a.fr.W, a.fr.y_min, a.fr.res_y); }
    a.knots_out[2 * i] = x;
    a.knots_out[2 * i + 1] = y;
}

// ---- host ------------------------------------------------------------------------------------------------------------
// the grid of a call is a sc_speed_frame: a reservation reads no d2, a plan the origin and the resolutions only for knots_out
static bool tp_reserve_invalid(sc_ctx* ctx, const double* knots, int P, int K, const double* radius, double pad, const sc_speed_frame& fr,
                               const uint32_t* res) {
    return !ctx || !knots || !radius || !res || !sc_traj_size_ok(P, K) || !isfinite(pad) || pad < 0.0 || !sc_frame_ok(fr);
}

static bool tp_plan_invalid(sc_ctx* ctx, const sc_speed_frame& fr, int L, const int32_t* start, const int32_t* goal, int B,
                            const int32_t* status, const double* knots_out) {
    return !ctx || !fr.d2 || !start || !goal || !status || fr.W < 1 || fr.H < 1 || fr.W > SC_MAX_DIM || fr.H > SC_MAX_DIM || L < 1 ||
           L > TP_MAX_L || B < 1 || B > TP_MAX_B || (knots_out && !sc_frame_ok(fr));
}

static int tp_launch_reserve(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius, const int32_t* select,
                             double pad, const sc_speed_frame& fr, uint32_t* res) {
    // cells the float32 rounding of a centre can move it by, plus one for floor / ceil and one to spare
    const double span_x = fabs((double)fr.x_min) + (double)fr.W * fr.res_x, span_y = fabs((double)fr.y_min) + (double)fr.H * fr.res_y;
    double m = fmax(span_x / fr.res_x, span_y / fr.res_y) * 0x1p-22 + 2.0;
    if (!(m < 16384.0)) m = 16384.0;
    tp_reserve_args a{knots, tstatus, radius, select, P, K, pad, fr, (fr.W + 31) / 32, (int)ceil(m), res};
    const long long items = (long long)P * K;
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    hipLaunchKernelGGL(tplan_reserve_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// moves and planes of (d2, r2_clear) into the context's scratch
static int tp_prepare_grid(sc_ctx* ctx, const sc_speed_frame& fr, int32_t r2_clear) {
    const int W = fr.W, H = fr.H, Wq = (W + 31) / 32;
    int r = sc_scratch_reserve(ctx, &ctx->moves, (size_t)W * H);
    if (r == SC_OK) r = sc_scratch_reserve(ctx, &ctx->tp_planes, (size_t)8 * H * Wq * 4);
    if (r != SC_OK) return r;
    r = sc_launch_moves(ctx, fr.d2, W, H, H, r2_clear, (uint8_t*)ctx->moves.p);
    if (r != SC_OK) return r;
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    hipLaunchKernelGGL(tplan_planes_kernel, dim3((W + 255) / 256, H), dim3(256), 0, ctx->stream, (const uint8_t*)ctx->moves.p, W, H, Wq,
                       (uint32_t*)ctx->tp_planes.p);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// queries a group may hold: the budget when the layers live in scratch, and a launch's grid limits
static int tp_group_size(sc_ctx* ctx, int W, int H, int L, int B, bool own_reach, int* out) {
    const int Wq = (W + 31) / 32;
    const size_t per_q = (size_t)L * H * Wq * 4;
    const long long tiles = (long long)((Wq + TP_TW - 1) / TP_TW) * ((H + TP_TH - 1) / TP_TH);
    long long g = B;
    if (own_reach) {
        if (per_q > ctx->tplan_budget) {
            snprintf(ctx->err, sizeof(ctx->err), "sc_tplan: the layers of one query need %zu bytes, the budget (SC_TPLAN_GB) is %zu", per_q,
                     ctx->tplan_budget);
            return SC_ERR_INVALID;
        }
        g = (long long)(ctx->tplan_budget / per_q);
    }
    if (g > 32768) g = 32768;
    if (g > (1ll << 22) / tiles) g = (1ll << 22) / tiles;   // workgroups of a step launch
    if (g < 1) g = 1;
    *out = (int)(g < B ? g : B);
    return SC_OK;
}

// the search of queries [0, Bg) with their layers at `reach`; tp_prepare_grid has run.  path may be NULL unless knots_out is given.
static int tp_launch_group(sc_ctx* ctx, const sc_speed_frame& fr, int32_t r2_clear, const uint32_t* res, int L, const int32_t* start,
                           const int32_t* goal, const int32_t* t_start, int Bg, int hold, int32_t* path, int32_t* len, int32_t* arrive,
                           int32_t* status, double* knots_out, uint32_t* reach, tp_q* qs) {
    const int W = fr.W, H = fr.H, Wq = (W + 31) / 32, h = ctx->tplan_layers;
    const size_t layer = (size_t)H * Wq;
    const int tiles_x = (Wq + TP_TW - 1) / TP_TW, tiles_y = (H + TP_TH - 1) / TP_TH;
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    tp_init_args ia{fr.d2, W, H, Wq, L, r2_clear > 1 ? r2_clear : 1, res, start, goal, t_start, hold, qs};
    hipLaunchKernelGGL(tplan_init_kernel, dim3(Bg), dim3(256), 0, ctx->stream, ia);
    hipLaunchKernelGGL(tplan_seed_kernel, dim3((unsigned)((layer + 255) / 256), Bg), dim3(256), 0, ctx->stream, (const tp_q*)qs, W, layer, L, reach);
    for (int t0 = 0; t0 < L - 1; t0 += h) {
        tp_step_args sa{(const uint32_t*)ctx->tp_planes.p, res, reach, qs, W, H, Wq, L, tiles_x, t0, (L - 1 - t0) < h ? (L - 1 - t0) : h, h};
        hipLaunchKernelGGL(tplan_step_kernel, dim3(tiles_x * tiles_y, Bg), dim3(TP_THREADS), 0, ctx->stream, sa);
    }
    tp_read_args ra{qs, reach, (const uint8_t*)ctx->moves.p, W, H, Wq, L, Bg, path, len, arrive, status};
    hipLaunchKernelGGL(tplan_read_kernel, dim3((Bg + 63) / 64), dim3(64), 0, ctx->stream, ra);
    if (knots_out) {
        tp_knots_args ka{qs, path, L, Bg, hold, fr, knots_out};
        hipLaunchKernelGGL(tplan_knots_kernel, dim3((unsigned)(((long long)Bg * L + 255) / 256)), dim3(256), 0, ctx->stream, ka);
    }
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// scratch of a plan: the group's layers when the caller passes none, the query states, the paths when only the knots are wanted
struct tp_scratch {
    int Bg;
    uint32_t* reach;   // the caller's or scratch
    bool own_reach;
    tp_q* qs;
    int32_t* path;     // scratch for Bg queries, NULL when the caller's is used
};

static int tp_make_scratch(sc_ctx* ctx, int W, int H, int L, int B, bool seq, uint32_t* reach, bool need_path, tp_scratch* s) {
    const size_t per_q = (size_t)L * H * ((W + 31) / 32) * 4;
    s->own_reach = !reach;
    int r = tp_group_size(ctx, W, H, L, seq ? 1 : B, s->own_reach, &s->Bg);
    if (r != SC_OK) return r;
    if (s->own_reach) {
        r = sc_scratch_reserve(ctx, &ctx->tp_reach, per_q * s->Bg);
        if (r != SC_OK) return r;
    }
    const size_t qb = al256((size_t)s->Bg * sizeof(tp_q)), pb = need_path ? (size_t)s->Bg * L * 4 : 0;
    r = sc_scratch_reserve(ctx, &ctx->tp_state, qb + pb);
    if (r != SC_OK) return r;
    s->reach = reach ? reach : (uint32_t*)ctx->tp_reach.p;
    s->qs = (tp_q*)ctx->tp_state.p;
    s->path = need_path ? (int32_t*)((char*)ctx->tp_state.p + qb) : nullptr;
    return SC_OK;
}

// queries [b0, b0 + n) of a call, n <= s.Bg
static int tp_run(sc_ctx* ctx, const tp_scratch& s, const sc_speed_frame& fr, int32_t r2_clear, const uint32_t* res, int L,
                  const int32_t* start, const int32_t* goal, const int32_t* t_start, int b0, int n, int hold, int32_t* path, int32_t* len,
                  int32_t* arrive, int32_t* status, double* knots_out) {
    const size_t per_q = (size_t)L * fr.H * ((fr.W + 31) / 32);
    return tp_launch_group(ctx, fr, r2_clear, res, L, start + b0, goal + b0, t_start ? t_start + b0 : nullptr, n, hold,
                           path ? path + (size_t)b0 * L : s.path, len ? len + b0 : nullptr, arrive ? arrive + b0 : nullptr, status + b0,
                           knots_out ? knots_out + (size_t)b0 * L * 2 : nullptr, s.own_reach ? s.reach : s.reach + (size_t)b0 * per_q, s.qs);
}

extern "C" int sc_traj_reserve_batch(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius,
                                     const int32_t* select, double pad, int W, int H, float x_min, float y_min, float res_x, float res_y,
                                     uint32_t* res) {
    const sc_speed_frame fr{nullptr, W, H, x_min, y_min, res_x, res_y};
    if (tp_reserve_invalid(ctx, knots, P, K, radius, pad, fr, res)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return tp_launch_reserve(ctx, knots, tstatus, P, K, radius, select, pad, fr, res);
}

extern "C" int sc_tplan_batch(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear, const uint32_t* res, int L, const int32_t* start,
                              const int32_t* goal, const int32_t* t_start, int B, int hold, int32_t* path, int32_t* len, int32_t* arrive,
                              int32_t* status, double* knots_out, float x_min, float y_min, float res_x, float res_y, uint32_t* reach) {
    const sc_speed_frame fr{d2, W, H, x_min, y_min, res_x, res_y};
    if (tp_plan_invalid(ctx, fr, L, start, goal, B, status, knots_out)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    tp_scratch s;
    int r = tp_make_scratch(ctx, W, H, L, B, false, reach, knots_out && !path, &s);
    if (r == SC_OK) r = tp_prepare_grid(ctx, fr, r2_clear);
    for (int b0 = 0; r == SC_OK && b0 < B; b0 += s.Bg)
        r = tp_run(ctx, s, fr, r2_clear, res, L, start, goal, t_start, b0, B - b0 < s.Bg ? B - b0 : s.Bg, hold != 0, path, len, arrive, status,
                   knots_out);
    return r;
}

extern "C" int sc_fleet_replan_batch(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius,
                                     const int32_t* select, double pad, int W, int H, float x_min, float y_min, float res_x, float res_y,
                                     uint32_t* res, const int32_t* d2, int32_t r2_clear, int L, const int32_t* start, const int32_t* goal,
                                     const int32_t* t_start, int B, int hold, int32_t* path, int32_t* len, int32_t* arrive, int32_t* status,
                                     double* knots_out, uint32_t* reach, const double* r_new, int sequential) {
    const sc_speed_frame fr{d2, W, H, x_min, y_min, res_x, res_y};
    if (tp_reserve_invalid(ctx, knots, P, K, radius, pad, fr, res) || tp_plan_invalid(ctx, fr, L, start, goal, B, status, knots_out) ||
        L != K + 1 || (sequential && (!r_new || !knots_out)))
        return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    tp_scratch s;
    int r = tp_make_scratch(ctx, W, H, L, B, sequential != 0, reach, knots_out && !path, &s);
    if (r == SC_OK) r = tp_prepare_grid(ctx, fr, r2_clear);
    if (r == SC_OK) r = tp_launch_reserve(ctx, knots, tstatus, P, K, radius, select, pad, fr, res);
    const int step = sequential ? 1 : s.Bg;
    for (int b0 = 0; r == SC_OK && b0 < B; b0 += step) {
        r = tp_run(ctx, s, fr, r2_clear, res, L, start, goal, t_start, b0, B - b0 < step ? B - b0 : step, hold != 0, path, len, arrive, status,
                   knots_out);
        // prioritised planning: robot b0's row joins the reservations (a failed plan is NaN rows and reserves nothing)
        if (r == SC_OK && sequential)
            r = tp_launch_reserve(ctx, knots_out + (size_t)b0 * L * 2, nullptr, 1, K, r_new + b0, nullptr, pad, fr, res);
    }
    return r;
}

// ---- host forms ----
extern "C" int sc_traj_reserve_batch_host(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius,
                                          const int32_t* select, double pad, int W, int H, float x_min, float y_min, float res_x, float res_y,
                                          uint32_t* res) {
    const sc_speed_frame fr{nullptr, W, H, x_min, y_min, res_x, res_y};
    if (tp_reserve_invalid(ctx, knots, P, K, radius, pad, fr, res) || sc_traj_radius_outside(radius, P)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pb = (size_t)P * 4, rb = (size_t)(K + 1) * H * ((W + 31) / 32) * 4;
    sc_stage st(ctx);
    const int i_k = st.in(knots, (size_t)P * (K + 1) * 16), i_s = st.in(tstatus, tstatus ? pb : 0), i_r = st.in(radius, pb * 2),
              i_sel = st.in(select, select ? pb : 0), i_res = st.in(res, rb);
    st.back(i_s, tstatus, pb);
    st.back(i_res, res, rb);
    int r = st.upload();
    if (r == SC_OK)
        r = tp_launch_reserve(ctx, st.dev<const double>(i_k), tstatus ? st.dev<int32_t>(i_s) : nullptr, P, K, st.dev<const double>(i_r),
                              select ? st.dev<const int32_t>(i_sel) : nullptr, pad, fr, st.dev<uint32_t>(i_res));
    return st.finish(r);
}

extern "C" int sc_tplan_batch_host(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear, const uint32_t* res, int L,
                                   const int32_t* start, const int32_t* goal, const int32_t* t_start, int B, int hold, int32_t* path,
                                   int32_t* len, int32_t* arrive, int32_t* status, double* knots_out, float x_min, float y_min, float res_x,
                                   float res_y, uint32_t* reach) {
    if (tp_plan_invalid(ctx, sc_speed_frame{d2, W, H, x_min, y_min, res_x, res_y}, L, start, goal, B, status, knots_out)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bb = (size_t)B * 4, layer = (size_t)H * ((W + 31) / 32) * 4;
    sc_stage st(ctx);
    const int i_d = st.in(d2, (size_t)W * H * 4), i_res = st.in(res, res ? layer * L : 0), i_s = st.in(start, bb), i_g = st.in(goal, bb),
              i_t = st.in(t_start, t_start ? bb : 0);
    const int o_p = st.out(path, path ? bb * L : 0), o_l = st.out(len, len ? bb : 0), o_a = st.out(arrive, arrive ? bb : 0),
              o_s = st.out(status, bb), o_k = st.out(knots_out, knots_out ? (size_t)B * L * 16 : 0), o_r = st.out(reach, reach ? layer * L * B : 0);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_tplan_batch(ctx, st.dev<const int32_t>(i_d), W, H, r2_clear, res ? st.dev<const uint32_t>(i_res) : nullptr, L,
                           st.dev<const int32_t>(i_s), st.dev<const int32_t>(i_g), t_start ? st.dev<const int32_t>(i_t) : nullptr, B, hold,
                           path ? st.dev<int32_t>(o_p) : nullptr, len ? st.dev<int32_t>(o_l) : nullptr, arrive ? st.dev<int32_t>(o_a) : nullptr,
                           st.dev<int32_t>(o_s), knots_out ? st.dev<double>(o_k) : nullptr, x_min, y_min, res_x, res_y,
                           reach ? st.dev<uint32_t>(o_r) : nullptr);
    return st.finish(r);
}

extern "C" int sc_fleet_replan_batch_host(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius,
                                          const int32_t* select, double pad, int W, int H, float x_min, float y_min, float res_x, float res_y,
                                          uint32_t* res, const int32_t* d2, int32_t r2_clear, int L, const int32_t* start, const int32_t* goal,
                                          const int32_t* t_start, int B, int hold, int32_t* path, int32_t* len, int32_t* arrive,
                                          int32_t* status, double* knots_out, uint32_t* reach, const double* r_new, int sequential) {
    const sc_speed_frame fr{d2, W, H, x_min, y_min, res_x, res_y};
    if (tp_reserve_invalid(ctx, knots, P, K, radius, pad, fr, res) || tp_plan_invalid(ctx, fr, L, start, goal, B, status, knots_out) ||
        L != K + 1 || (sequential && (!r_new || !knots_out)) || sc_traj_radius_outside(radius, P) ||
        (r_new && sc_traj_radius_outside(r_new, B)))
        return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pb = (size_t)P * 4, bb = (size_t)B * 4, layer = (size_t)H * ((W + 31) / 32) * 4;
    sc_stage st(ctx);
    const int i_k = st.in(knots, (size_t)P * (K + 1) * 16), i_ts = st.in(tstatus, tstatus ? pb : 0), i_r = st.in(radius, pb * 2),
              i_sel = st.in(select, select ? pb : 0), i_res = st.in(res, layer * L), i_d = st.in(d2, (size_t)W * H * 4), i_s = st.in(start, bb),
              i_g = st.in(goal, bb), i_t = st.in(t_start, t_start ? bb : 0), i_rn = st.in(r_new, r_new ? bb * 2 : 0);
    st.back(i_ts, tstatus, pb);
    st.back(i_res, res, layer * L);
    const int o_p = st.out(path, path ? bb * L : 0), o_l = st.out(len, len ? bb : 0), o_a = st.out(arrive, arrive ? bb : 0),
              o_s = st.out(status, bb), o_k = st.out(knots_out, knots_out ? (size_t)B * L * 16 : 0), o_r = st.out(reach, reach ? layer * L * B : 0);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_fleet_replan_batch(ctx, st.dev<const double>(i_k), tstatus ? st.dev<int32_t>(i_ts) : nullptr, P, K, st.dev<const double>(i_r),
                                  select ? st.dev<const int32_t>(i_sel) : nullptr, pad, W, H, x_min, y_min, res_x, res_y,
                                  st.dev<uint32_t>(i_res), st.dev<const int32_t>(i_d), r2_clear, L, st.dev<const int32_t>(i_s),
                                  st.dev<const int32_t>(i_g), t_start ? st.dev<const int32_t>(i_t) : nullptr, B, hold,
                                  path ? st.dev<int32_t>(o_p) : nullptr, len ? st.dev<int32_t>(o_l) : nullptr,
                                  arrive ? st.dev<int32_t>(o_a) : nullptr, st.dev<int32_t>(o_s), knots_out ? st.dev<double>(o_k) : nullptr,
                                  reach ? st.dev<uint32_t>(o_r) : nullptr, r_new ? st.dev<const double>(i_rn) : nullptr, sequential);
    return st.finish(r);
}
