// traj_sched.hip -- delay schedules for timed paths: the shift-conflict table, the priority greedy that reads start slots off
// it, and the shifted knots (sc_traj_shift_table_batch, sc_traj_schedule_batch, sc_traj_shift_knots_batch,
// sc_fleet_schedule_batch; the definition is in include/sea_current_hip.h and DESIGN.md section 18).
//
// Boxes: one wavefront per path takes the box of its present knots, marks a radius outside the contract SC_TRAJ_BAD and
// writes the diagonal entry of the table.
// Table: a one-wavefront workgroup owns a pair (lo < hi) at a time and lane = relative shift r = lane - (D-1); when 2D-1 <= 31
// the two halves of the wavefront own a pair each, when 2D-1 <= 15 its four quarters.  Both knot rows stream through LDS in
// chunks of TS_CHUNK ticks behind a halo of (D-1) * stride ticks; lane r reads lo[max(k - max(r,0) * stride, 0)] and hi[max(k - max(-r,0) * stride, 0)] and
// carries one "has conflicted" flag over k.  After the last chunk the ballot of the flags is table[lo][hi] and its bit
// reversal table[hi][lo]: no atomics, no partials.  Only m2 of section 17 is evaluated (one division per interval, no square
// root).  A pair whose boxes are at least R apart writes 0 without touching the ticks.
// LDS layout: x and y of a row apart (8-byte reads, banked over the two 32-lane halves), element i at slot i + i / 32: the
// lanes with r > 0 read stride elements apart, and without the pad an even stride would put them 2, 4, .. 32 deep on a bank.
// A halo beyond TS_HALO_LDS ticks does not fit: those calls read the rows from global memory with the same loop.
// Schedule: one workgroup, the slots in LDS, walks order; per step every thread ORs the windows of its columns of row p, one
// wave reduction and an LDS combine follow, thread 0 takes the lowest free bit.  The next row is loaded before the current
// one reduces (its address does not depend on the decision).
//
// Compiled with -ffp-contract=off: the predicate is section 17's, product by product (sc_traj_closest of traj_common.h).
#include "traj_common.h"

#define TS_MAX_PATHS SC_TRAJ_SCHED_MAX_PATHS
#define TS_CHUNK 64             // intervals of a chunk
#define TS_HALO_LDS 512         // the largest (D-1) * stride the LDS path takes: 4 rows * 2 * 8 B * 596 slots = 37.3 KiB
#define TS_LDS_BYTES 49152      // what a launch takes at most: four pairs per wavefront become two when their rows need more
#define TS_BOX_SLACK 0x1p-48    // see ts_gap2
#define TS_SCHED_THREADS 1024
#define TS_SCHED_COLS (TS_MAX_PATHS / TS_SCHED_THREADS)
#define TS_KN_THREADS 256

struct ts_box { double x0, x1, y0, y1; };   // min / max of the present knots; +inf / -inf when there is none

struct ts_box_args {
    const double* knots;
    int32_t* tstatus;
    const double* radius;
    int P, K;
    ts_box* box;
    uint64_t* table;
};

__global__ void __launch_bounds__(64) traj_box_kernel(ts_box_args a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const double* k = a.knots + (size_t)p * (a.K + 1) * 2;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int i = lane; i <= a.K; i += 64) {
        const double x = k[2 * (size_t)i], y = k[2 * (size_t)i + 1];
        if (x == x && y == y) {
            x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
            y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double ax0 = __shfl_xor(x0, s), ax1 = __shfl_xor(x1, s), ay0 = __shfl_xor(y0, s), ay1 = __shfl_xor(y1, s);
        x0 = ax0 < x0 ? ax0 : x0; x1 = ax1 > x1 ? ax1 : x1;
        y0 = ay0 < y0 ? ay0 : y0; y1 = ay1 > y1 ? ay1 : y1;
    }
    if (lane != 0) return;
    sc_traj_mark_radius(a.tstatus, p, a.radius[p]);
    a.box[p] = ts_box{x0, x1, y0, y1};
    a.table[(size_t)p * a.P + p] = 0;
}

// The squared gap between two boxes, shrunk so that no interval of the pair can have m2 below it.  In real numbers every
// difference hi - lo of two knots is at least the gap g per axis; rounding keeps d0, d1 >= fl(g), and the point d0 + lam * e
// of the predicate can undershoot the smaller of d0, d1 by the rounding of e = d1 - d0 and of the sum: at most 2^-51 of the
// span w (the far edges' distance, >= |d0|, |d1|, |e| / 2).  Taking 2^-48 * w off g leaves a margin of 7 * 2^-51 * w, which
// also covers the roundings of the two sums of squares.  A path without a present knot has an infinite gap.
__device__ __forceinline__ double ts_gap2(const ts_box& a, const ts_box& b) {
    const double lx = a.x0 > b.x0 ? a.x0 : b.x0, hx = a.x1 < b.x1 ? a.x1 : b.x1;
    const double ly = a.y0 > b.y0 ? a.y0 : b.y0, hy = a.y1 < b.y1 ? a.y1 : b.y1;
    const double wx = (a.x1 > b.x1 ? a.x1 : b.x1) - (a.x0 < b.x0 ? a.x0 : b.x0);
    const double wy = (a.y1 > b.y1 ? a.y1 : b.y1) - (a.y0 < b.y0 ? a.y0 : b.y0);
    double gx = (lx - hx) - TS_BOX_SLACK * wx, gy = (ly - hy) - TS_BOX_SLACK * wy;
    gx = gx > 0.0 ? gx : 0.0;
    gy = gy > 0.0 ? gy : 0.0;
    return gx * gx + gy * gy;
}

struct ts_table_args {
    const double* knots;
    const int32_t* tstatus;   // after traj_box_kernel
    const double* radius;
    const int32_t* group;
    const ts_box* box;
    int P, K, D, stride, noskip;
    int per;                  // pairs a wavefront owns at a time: 1, 2 or 4 groups of 64 / per lanes, 2D-1 <= 64 / per
    long long pairs;          // P (P-1) / 2
    int slots;                // LDS doubles per coordinate of a row (LDS build)
    uint64_t* table;
};

__device__ __forceinline__ int ts_pad(int i) { return i + (i >> 5); }

// pair t of the triangle, rows first: t = hi (hi-1) / 2 + lo, lo < hi
__device__ __forceinline__ void ts_pair(long long t, int& lo, int& hi) {
    int h = (int)((1.0 + sqrt(1.0 + 8.0 * (double)t)) * 0.5);
    while ((long long)h * (h - 1) / 2 > t) --h;
    while ((long long)(h + 1) * h / 2 <= t) ++h;
    hi = h;
    lo = (int)(t - (long long)h * (h - 1) / 2);
}

template <bool LDS>
__global__ void __launch_bounds__(64) traj_shift_table_kernel(ts_table_args a) {
    extern __shared__ double ts_smem[];   // LDS build: [group][lo, hi][x, y][slots]
    const int lane = threadIdx.x, P = a.P, K = a.K, D = a.D, nb = 2 * D - 1;
    const int per = a.per, width = 64 / per, part = lane / width, sub = lane % width;
    const int r = sub < nb ? sub - (D - 1) : 0;
    const int sl = (r > 0 ? r : 0) * a.stride, sh = (r < 0 ? -r : 0) * a.stride;   // <= (D-1) * stride <= K
    const int H = (D - 1) * a.stride;
    double* s_lo = ts_smem + (size_t)part * 4 * a.slots;
    double* s_hi = s_lo + 2 * (size_t)a.slots;
    for (long long w = blockIdx.x; w * per < a.pairs; w += gridDim.x) {
        const long long t = w * per + part;
        int lo = 0, hi = 1;
        bool live = false;
        double RR = 0.0;
        if (t < a.pairs) {
            ts_pair(t, lo, hi);
            live = a.tstatus[lo] == SC_TRAJ_OK && a.tstatus[hi] == SC_TRAJ_OK;
            if (live && a.group) { const int g = a.group[lo]; live = !(g >= 0 && g == a.group[hi]); }
            if (live) {
                const double R = a.radius[lo] + a.radius[hi];
                RR = R * R;
                if (!a.noskip) live = ts_gap2(a.box[lo], a.box[hi]) < RR;
            }
        }
        const double* klo = a.knots + (size_t)lo * (K + 1) * 2;
        const double* khi = a.knots + (size_t)hi * (K + 1) * 2;
        const bool on = live && sub < nb;
        bool hit = false;
        if (__ballot(live)) {   // wavefront-uniform from here: every group walks the chunks, a dead one computes nothing
            double d0x = 0.0, d0y = 0.0;
            for (int kc = 0; kc < K; kc += TS_CHUNK) {
                const int ke = min(K, kc + TS_CHUNK), base = kc - H;
                if (LDS) {
                    __syncthreads();   // the previous chunk has been read
                    if (live) {
                        const int n = ke - base + 1;   // elements base .. ke
                        for (int e = sub; e < n; e += width) {
                            const int gi = base + e;
                            if (gi < 0) continue;
                            const double2 vl = *(const double2*)(klo + 2 * (size_t)gi), vh = *(const double2*)(khi + 2 * (size_t)gi);
                            const int s = ts_pad(e);
                            s_lo[s] = vl.x; s_lo[a.slots + s] = vl.y;
                            s_hi[s] = vh.x; s_hi[a.slots + s] = vh.y;
                        }
                    }
                    __syncthreads();
                }
                if (on) {
                    if (kc == 0) {   // tick 0: nobody has started
                        d0x = khi[0] - klo[0];
                        d0y = khi[1] - klo[1];
                    }
                    for (int k = kc; k < ke; ++k) {
                        const int il = max(k + 1 - sl, 0), ih = max(k + 1 - sh, 0);
                        double lx, ly, hx, hy;
                        if (LDS) {
                            const int pl = ts_pad(il - base), ph = ts_pad(ih - base);
                            lx = s_lo[pl]; ly = s_lo[a.slots + pl];
                            hx = s_hi[ph]; hy = s_hi[a.slots + ph];
                        } else {
                            lx = klo[2 * (size_t)il]; ly = klo[2 * (size_t)il + 1];
                            hx = khi[2 * (size_t)ih]; hy = khi[2 * (size_t)ih + 1];
                        }
                        const double d1x = hx - lx, d1y = hy - ly;
                        hit |= sc_traj_closest(d0x, d0y, d1x, d1y).m2 < RR;
                        d0x = d1x;
                        d0y = d1y;
                    }
                }
                if (!__ballot(on && !hit)) break;   // every shift of every live pair has conflicted
            }
        }
        const uint64_t all = __ballot(on && hit);
        if (sub == 0 && t < a.pairs) {
            const uint64_t word = per == 1 ? all : (all >> (width * part)) & ((1ull << width) - 1);
            a.table[(size_t)lo * P + hi] = word;
            a.table[(size_t)hi * P + lo] = __brevll(word) >> (64 - nb);
        }
    }
}

struct ts_sched_args {
    const uint64_t* table;
    const int32_t* tstatus;
    int P, D;
    const int32_t *order, *jmax;
    int32_t *slot, *counts;
};

__global__ void __launch_bounds__(TS_SCHED_THREADS) traj_schedule_kernel(ts_sched_args a) {
    __shared__ int32_t s_slot[TS_MAX_PATHS];
    __shared__ uint32_t s_busy[TS_SCHED_THREADS / 64];
    __shared__ int32_t s_cnt[4];
    const int tid = threadIdx.x, P = a.P, D = a.D;
    const uint32_t dmask = D >= 32 ? 0xffffffffu : (1u << D) - 1u;
    for (int q = tid; q < P; q += TS_SCHED_THREADS) s_slot[q] = SC_SLOT_UNNAMED;
    if (tid < 4) s_cnt[tid] = 0;
    uint64_t cur[TS_SCHED_COLS], nxt[TS_SCHED_COLS];
    int p = a.order ? a.order[0] : 0;
    const bool in0 = p >= 0 && p < P;
#pragma unroll
    for (int j = 0; j < TS_SCHED_COLS; ++j) {
        const int q = tid + j * TS_SCHED_THREADS;
        cur[j] = in0 && q < P ? a.table[(size_t)p * P + q] : 0;
    }
    __syncthreads();
    for (int i = 0; i < P; ++i) {
        const int pn = i + 1 < P ? (a.order ? a.order[i + 1] : i + 1) : -1;
        const bool inn = pn >= 0 && pn < P;
#pragma unroll
        for (int j = 0; j < TS_SCHED_COLS; ++j) {   // the next row: in flight while this one reduces
            const int q = tid + j * TS_SCHED_THREADS;
            nxt[j] = inn && q < P ? a.table[(size_t)pn * P + q] : 0;
        }
        // block-uniform: s_slot[p] was last written before the barrier that ended the previous step
        if (p >= 0 && p < P && s_slot[p] == SC_SLOT_UNNAMED) {
            const int jm = a.jmax ? a.jmax[p] : D - 1;
            const bool ok = a.tstatus[p] == SC_TRAJ_OK;
            uint32_t busy = 0;
            if (ok && jm >= 0) {
#pragma unroll
                for (int j = 0; j < TS_SCHED_COLS; ++j) {
                    const int q = tid + j * TS_SCHED_THREADS;
                    const int sq = q < P ? s_slot[q] : -1;
                    if (sq >= 0) busy |= (uint32_t)(cur[j] >> (D - 1 - sq));
                }
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) busy |= __shfl_xor(busy, s);
                if ((tid & 63) == 0) s_busy[tid >> 6] = busy;
            }
            __syncthreads();   // s_busy written, every read of s_slot done
            if (tid == 0) {
                int sl;
                if (!ok) sl = SC_SLOT_NOT_OK;
                else if (jm < 0) sl = 0;
                else {
                    busy = 0;
                    for (int v = 0; v < TS_SCHED_THREADS / 64; ++v) busy |= s_busy[v];
                    const int top = jm < D - 1 ? jm : D - 1;
                    const uint32_t allow = top >= 31 ? 0xffffffffu : (1u << (top + 1)) - 1u;
                    const uint32_t open = ~busy & dmask & allow;
                    sl = open ? __ffs(open) - 1 : SC_SLOT_UNRESOLVED;
                }
                s_slot[p] = sl;
            }
            __syncthreads();
        }
        p = pn;
#pragma unroll
        for (int j = 0; j < TS_SCHED_COLS; ++j) cur[j] = nxt[j];
    }
    int c[4] = {0, 0, 0, 0};
    for (int q = tid; q < P; q += TS_SCHED_THREADS) {
        const int s = s_slot[q];
        a.slot[q] = s;
        ++c[s == 0 ? 0 : (s > 0 ? 1 : (s == SC_SLOT_UNRESOLVED ? 2 : 3))];
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) c[v] += __shfl_xor(c[v], s);
        if ((tid & 63) == 0 && c[v]) atomicAdd(&s_cnt[v], c[v]);
    }
    __syncthreads();
    if (tid < 4) a.counts[tid] = s_cnt[tid];
}

__global__ void __launch_bounds__(TS_KN_THREADS) traj_shift_knots_kernel(const double* knots, int P, int K, const int32_t* slot, int stride,
                                                                         double* out) {
    const int p = blockIdx.y, k = blockIdx.x * TS_KN_THREADS + threadIdx.x;
    if (k > K) return;
    const int s = slot[p];
    double2 v = make_double2(NAN, NAN);
    if (s >= 0) {
        const long long src = (long long)k - (long long)s * stride;
        v = *(const double2*)(knots + ((size_t)p * (K + 1) + (size_t)(src > 0 ? src : 0)) * 2);
    }
    *(double2*)(out + ((size_t)p * (K + 1) + k) * 2) = v;
}

// ---- launches ----
static bool ts_size_invalid(int P, int K) { return !sc_traj_size_ok(P, K, TS_MAX_PATHS); }

static bool ts_slots_invalid(int D, int stride, int K) {
    return D < 1 || D > 32 || stride < 1 || (long long)(D - 1) * stride > K;
}

static int ts_launch_table(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius, const int32_t* group, int D,
                           int stride, uint64_t* table) {
    int r = sc_scratch_reserve(ctx, &ctx->traj_box, al256((size_t)P * sizeof(ts_box)));
    if (r != SC_OK) return r;
    ts_box* box = (ts_box*)ctx->traj_box.p;
    int tk = sc_time_begin(ctx, SC_K_SMOOTH);
    ts_box_args b{knots, tstatus, radius, P, K, box, table};
    hipLaunchKernelGGL(traj_box_kernel, dim3(P), dim3(64), 0, ctx->stream, b);
    const long long pairs = (long long)P * (P - 1) / 2;
    if (pairs > 0) {
        const int H = (D - 1) * stride, nb = 2 * D - 1, elems = TS_CHUNK + 1 + H;
        const bool lds = H <= TS_HALO_LDS;
        ts_table_args a{knots, tstatus, radius, group, box, P, K, D, stride, ctx->traj_sched_noskip ? 1 : 0, nb <= 15 ? 4 : (nb <= 31 ? 2 : 1),
                        pairs, lds ? elems + (elems >> 5) + 1 : 0, table};
        if (lds && (size_t)a.per * 4 * a.slots * sizeof(double) > TS_LDS_BYTES) a.per = 2;   // at most 2 * 32 B * 596 = 37.3 KiB
        const long long waves = (pairs + a.per - 1) / a.per;
        const int grid = (int)(waves < 65536 ? waves : 65536);   // a wavefront walks its share of the triangle
        if (lds)
            hipLaunchKernelGGL(traj_shift_table_kernel<true>, dim3(grid), dim3(64), (size_t)a.per * 4 * a.slots * sizeof(double), ctx->stream, a);
        else
            hipLaunchKernelGGL(traj_shift_table_kernel<false>, dim3(grid), dim3(64), 0, ctx->stream, a);
    }
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

static int ts_launch_schedule(sc_ctx* ctx, const uint64_t* table, const int32_t* tstatus, int P, int D, const int32_t* order,
                              const int32_t* jmax, int32_t* slot, int32_t* counts) {
    ts_sched_args a{table, tstatus, P, D, order, jmax, slot, counts};
    int tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(traj_schedule_kernel, dim3(1), dim3(TS_SCHED_THREADS), 0, ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

static int ts_launch_shift(sc_ctx* ctx, const double* knots, int P, int K, const int32_t* slot, int stride, double* knots_out) {
    int tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(traj_shift_knots_kernel, dim3((K + TS_KN_THREADS) / TS_KN_THREADS, P), dim3(TS_KN_THREADS), 0, ctx->stream, knots, P, K,
                       slot, stride, knots_out);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_traj_shift_table_batch(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius,
                                         const int32_t* group, int D, int stride, uint64_t* table) {
    if (!ctx || !knots || !tstatus || !radius || !table || ts_size_invalid(P, K) || ts_slots_invalid(D, stride, K)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return ts_launch_table(ctx, knots, tstatus, P, K, radius, group, D, stride, table);
}

extern "C" int sc_traj_schedule_batch(sc_ctx* ctx, const uint64_t* table, const int32_t* tstatus, int P, int D, const int32_t* order,
                                      const int32_t* jmax, int32_t* slot, int32_t* counts) {
    if (!ctx || !table || !tstatus || !slot || !counts || P < 1 || P > TS_MAX_PATHS || D < 1 || D > 32) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return ts_launch_schedule(ctx, table, tstatus, P, D, order, jmax, slot, counts);
}

extern "C" int sc_traj_shift_knots_batch(sc_ctx* ctx, const double* knots, int P, int K, const int32_t* slot, int stride, double* knots_out) {
    if (!ctx || !knots || !slot || !knots_out || ts_size_invalid(P, K) || stride < 1) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return ts_launch_shift(ctx, knots, P, K, slot, stride, knots_out);
}

static bool ts_fleet_invalid(sc_ctx* ctx, const sc_traj_paths& pa, const sc_traj_clock& ck, const double* radius, int D, int stride,
                             const int32_t* slot, const int32_t* counts) {
    return sc_traj_input_invalid(ctx, pa, ck, TS_MAX_PATHS) || !radius || !slot || !counts || ts_slots_invalid(D, stride, ck.K);
}

// the four launches; every pointer is a device pointer and present, except knots_out (ts_fleet_invalid covers sc_traj_knots_batch's checks)
static int ts_launch_fleet(sc_ctx* ctx, const sc_traj_paths& pa, const sc_traj_clock& ck, double* knots, int32_t* tstatus, const double* radius,
                           const int32_t* group, int D, int stride, uint64_t* table, const int32_t* order, const int32_t* jmax, int32_t* slot,
                           int32_t* counts, double* knots_out) {
    int r = sc_traj_launch_knots(ctx, pa, ck, knots, tstatus);
    if (r == SC_OK) r = ts_launch_table(ctx, knots, tstatus, pa.P, ck.K, radius, group, D, stride, table);
    if (r == SC_OK) r = ts_launch_schedule(ctx, table, tstatus, pa.P, D, order, jmax, slot, counts);
    if (r == SC_OK && knots_out) r = ts_launch_shift(ctx, knots, pa.P, ck.K, slot, stride, knots_out);
    return r;
}

extern "C" int sc_fleet_schedule_batch(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets, const int32_t* length,
                                       const int32_t* status, int P, const double* t0, const int32_t* flags, double T0, double dt_c, int K,
                                       double* knots, int32_t* tstatus, const double* radius, const int32_t* group, int D, int stride,
                                       uint64_t* table, const int32_t* order, const int32_t* jmax, int32_t* slot, int32_t* counts,
                                       double* knots_out) {
    const sc_traj_paths pa{time, pts, offsets, length, status, t0, flags, P};
    const sc_traj_clock ck{T0, dt_c, K};
    if (ts_fleet_invalid(ctx, pa, ck, radius, D, stride, slot, counts)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    int r = sc_traj_scratch_knots(ctx, P, K, &knots, &tstatus);
    if (r == SC_OK && !table) r = sc_scratch_reserve(ctx, &ctx->traj_table, al256((size_t)P * P * 8));
    if (r != SC_OK) return r;
    if (!table) table = (uint64_t*)ctx->traj_table.p;
    return ts_launch_fleet(ctx, pa, ck, knots, tstatus, radius, group, D, stride, table, order, jmax, slot, counts, knots_out);
}

// ---- host forms ----
extern "C" int sc_traj_shift_table_batch_host(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius,
                                              const int32_t* group, int D, int stride, uint64_t* table) {
    if (!ctx || !knots || !tstatus || !radius || !table || ts_size_invalid(P, K) || ts_slots_invalid(D, stride, K)) return SC_ERR_INVALID;
    if (sc_traj_radius_outside(radius, P)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pb = (size_t)P * 4;
    sc_stage st(ctx);
    const int i_k = st.in(knots, (size_t)P * (K + 1) * 16), i_s = st.in(tstatus, pb), i_r = st.in(radius, pb * 2),
              i_g = st.in(group, group ? pb : 0);
    st.back(i_s, tstatus, pb);
    const int o_t = st.out(table, (size_t)P * P * 8);
    int r = st.upload();
    if (r == SC_OK)
        r = ts_launch_table(ctx, st.dev<const double>(i_k), st.dev<int32_t>(i_s), P, K, st.dev<const double>(i_r),
                            group ? st.dev<const int32_t>(i_g) : nullptr, D, stride, st.dev<uint64_t>(o_t));
    return st.finish(r);
}

extern "C" int sc_traj_schedule_batch_host(sc_ctx* ctx, const uint64_t* table, const int32_t* tstatus, int P, int D, const int32_t* order,
                                           const int32_t* jmax, int32_t* slot, int32_t* counts) {
    if (!ctx || !table || !tstatus || !slot || !counts || P < 1 || P > TS_MAX_PATHS || D < 1 || D > 32) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pb = (size_t)P * 4;
    sc_stage st(ctx);
    const int i_t = st.in(table, (size_t)P * P * 8), i_s = st.in(tstatus, pb), i_o = st.in(order, order ? pb : 0),
              i_j = st.in(jmax, jmax ? pb : 0);
    const int o_s = st.out(slot, pb), o_c = st.out(counts, 16);
    int r = st.upload();
    if (r == SC_OK)
        r = ts_launch_schedule(ctx, st.dev<const uint64_t>(i_t), st.dev<const int32_t>(i_s), P, D, order ? st.dev<const int32_t>(i_o) : nullptr,
                               jmax ? st.dev<const int32_t>(i_j) : nullptr, st.dev<int32_t>(o_s), st.dev<int32_t>(o_c));
    return st.finish(r);
}

extern "C" int sc_traj_shift_knots_batch_host(sc_ctx* ctx, const double* knots, int P, int K, const int32_t* slot, int stride,
                                              double* knots_out) {
    if (!ctx || !knots || !slot || !knots_out || ts_size_invalid(P, K) || stride < 1) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t kb = (size_t)P * (K + 1) * 16;
    sc_stage st(ctx);
    const int i_k = st.in(knots, kb), i_s = st.in(slot, (size_t)P * 4), o_k = st.out(knots_out, kb);
    int r = st.upload();
    if (r == SC_OK) r = ts_launch_shift(ctx, st.dev<const double>(i_k), P, K, st.dev<const int32_t>(i_s), stride, st.dev<double>(o_k));
    return st.finish(r);
}

extern "C" int sc_fleet_schedule_batch_host(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets, const int32_t* length,
                                            const int32_t* status, int P, const double* t0, const int32_t* flags, double T0, double dt_c,
                                            int K, double* knots, int32_t* tstatus, const double* radius, const int32_t* group, int D,
                                            int stride, uint64_t* table, const int32_t* order, const int32_t* jmax, int32_t* slot,
                                            int32_t* counts, double* knots_out) {
    const sc_traj_paths pa{time, pts, offsets, length, status, t0, flags, P};
    const sc_traj_clock ck{T0, dt_c, K};
    if (ts_fleet_invalid(ctx, pa, ck, radius, D, stride, slot, counts)) return SC_ERR_INVALID;
    if (sc_traj_radius_outside(radius, P) || sc_traj_paths_outside(pa)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pb = (size_t)P * 4, kb = (size_t)P * (K + 1) * 16;
    sc_stage st(ctx);
    const int i_pa = sc_traj_stage_paths(st, pa);
    const int i_r = st.in(radius, pb * 2), i_g = st.in(group, group ? pb : 0), i_or = st.in(order, order ? pb : 0),
              i_j = st.in(jmax, jmax ? pb : 0);
    const int o_k = st.out(knots, kb), o_s = st.out(tstatus, pb), o_t = st.out(table, (size_t)P * P * 8);   // slots even when not copied back
    const int o_sl = st.out(slot, pb), o_c = st.out(counts, 16), o_ko = st.out(knots_out, knots_out ? kb : 0);
    int r = st.upload();
    if (r == SC_OK)
        r = ts_launch_fleet(ctx, sc_traj_staged_paths(st, i_pa, pa), ck, st.dev<double>(o_k), st.dev<int32_t>(o_s), st.dev<const double>(i_r),
                            group ? st.dev<const int32_t>(i_g) : nullptr, D, stride, st.dev<uint64_t>(o_t),
                            order ? st.dev<const int32_t>(i_or) : nullptr, jmax ? st.dev<const int32_t>(i_j) : nullptr, st.dev<int32_t>(o_sl),
                            st.dev<int32_t>(o_c), knots_out ? st.dev<double>(o_ko) : nullptr);
    return st.finish(r);
}
