// traj.hip -- conflicts between timed paths: who comes within a robot's width of whom, when, and how close (sc_traj_knots_batch,
// sc_traj_conflicts_batch, sc_fleet_conflicts_batch; the definition is in include/sea_current_hip.h and DESIGN.md section 17).
//
// Knots: one thread per (path, tick) finds the path's position on the common clock by a binary search in its `time`; every
// workgroup of a path also validates the path (the first writes tstatus).
// Pairs: a one-wavefront workgroup owns TJ_ROWS row paths (one per lane), walks its share of the tick chunks and, inside a
// chunk, its share of the column tiles.  A lane keeps its row's TJ_CHUNK + 1 knots of the chunk in registers; the knots of a
// tile's TJ_COLS columns are staged in LDS, where all lanes read the same column knot (a broadcast read).  Both (p, q) and
// (q, p) are evaluated: every quantity of the definition is unchanged when the difference vectors change sign, so the two
// agree bit for bit.  A knot that is absent is (NaN, NaN): the interval's m2 is then NaN and fails both comparisons, which
// is how "compared only when all four knots are present" is decided without a branch.
// Combination: each workgroup leaves one partial (earliest conflict, closest approach, each with the smallest partner that
// attains it) per row in scratch and ORs its conflict bits into the matrix; a reduce kernel takes the lexicographic minima
// of a path's partials and counts its row of the matrix.  Minima, ORs and counts only: no output depends on the order of
// execution.
//
// Compiled with -ffp-contract=off: the NumPy twin of the tests states the same products and sums without fused
// multiply-adds.  The predicate, the radius contract, the limits and the packed paths are traj_common.h's.
#include "traj_common.h"

#include <limits.h>

#define TJ_KN_THREADS 256
#define TJ_ROWS 64          // row paths of a workgroup: the lanes of its one wavefront
#define TJ_COLS 32          // column paths of a tile: one word of the bit matrix
#define TJ_CHUNK 16         // intervals of a chunk: 4 * (TJ_CHUNK + 1) registers of row knots per lane, no scratch
// (the workgroups a launch aims for, 4096 = 16 per CU unless SC_TRAJ_WORKGROUPS says otherwise, are ctx->traj_wg_target:
// columns and tick chunks are split to reach it)

struct tj_part {   // what one workgroup found for one row path
    double first, sep2;
    int32_t first_with, sep_with;   // INT_MAX: none
};

struct tj_knots_args { sc_traj_paths pa; sc_traj_clock ck; double* knots; int32_t* tstatus; };

__global__ void __launch_bounds__(TJ_KN_THREADS) traj_knots_kernel(tj_knots_args a) {
    const int p = blockIdx.y, tid = threadIdx.x, K = a.ck.K;
    const int n = a.pa.length[p];
    int st = ((a.pa.status && a.pa.status[p] != SC_SMOOTH_OK) || n < 1) ? SC_TRAJ_SKIPPED : SC_TRAJ_OK;
    const size_t o = st == SC_TRAJ_OK ? (size_t)a.pa.offsets[p] : 0;
    const double* t = a.pa.time + o;
    const float* xy = a.pa.pts + 2 * o;
    const double d = a.pa.t0 ? a.pa.t0[p] : 0.0;
    int bad = 0;
    if (st == SC_TRAJ_OK) {
        if (!isfinite(d)) bad = 1;
        for (int i = tid; i < n; i += TJ_KN_THREADS) {
            const double ti = t[i];
            if (!isfinite(ti) || !isfinite(xy[2 * i]) || !isfinite(xy[2 * i + 1])) bad = 1;
            if (i + 1 < n && t[i + 1] < ti) bad = 1;
        }
    }
    if (__syncthreads_or(bad)) st = SC_TRAJ_BAD;   // block-uniform
    if (blockIdx.x == 0 && tid == 0) a.tstatus[p] = st;
    const int k = blockIdx.x * TJ_KN_THREADS + tid;
    if (k > K) return;
    double x = NAN, y = NAN;
    if (st == SC_TRAJ_OK) {
        const int fl = a.pa.flags ? a.pa.flags[p] : 3;
        const double tau = a.ck.T0 + (double)k * a.ck.dt_c;
        const double u = tau - d;
        if (u < t[0]) {
            if (fl & 1) { x = (double)xy[0]; y = (double)xy[1]; }
        } else if (u > t[n - 1]) {
            if (fl & 2) { x = (double)xy[2 * (size_t)(n - 1)]; y = (double)xy[2 * (size_t)(n - 1) + 1]; }
        } else if (n == 1) {
            x = (double)xy[0]; y = (double)xy[1];
        } else {
            int lo = 0, hi = n;   // the number of time[i] <= u
            while (lo < hi) { const int m = (lo + hi) >> 1; if (t[m] <= u) lo = m + 1; else hi = m; }
            const int j = min(max(lo - 1, 0), n - 2);
            const double tj = t[j], den = t[j + 1] - tj;
            const double f = den > 0.0 ? (u - tj) / den : 0.0;
            const double ax = (double)xy[2 * (size_t)j], ay = (double)xy[2 * (size_t)j + 1];
            const double bx = (double)xy[2 * (size_t)j + 2], by = (double)xy[2 * (size_t)j + 3];
            x = ax + f * (bx - ax);
            y = ay + f * (by - ay);
        }
    }
    double* out = a.knots + ((size_t)p * (K + 1) + k) * 2;
    out[0] = x;
    out[1] = y;
}

struct tj_pair_args {
    const double* knots;
    const int32_t* tstatus;
    const double* radius;
    const int32_t* group;
    int P;
    sc_traj_clock ck;
    int coltiles, G, chunks_per_split, slots;   // grid: (G column shares, row tiles, tick splits); slots = G * splits
    tj_part* part;      // [P][slots]
    uint32_t* matrix;   // [P][nw], zeroed; may be NULL
    int nw;
};

__device__ __forceinline__ bool tj_path_ok(const tj_pair_args& a, int p) {
    return a.tstatus[p] == SC_TRAJ_OK && sc_traj_radius_ok(a.radius[p]);
}

__global__ void __launch_bounds__(TJ_ROWS) traj_pairs_kernel(tj_pair_args a) {
    __shared__ double2 s_col[TJ_COLS][TJ_CHUNK + 1];
    __shared__ double s_rad[TJ_COLS];
    __shared__ int32_t s_grp[TJ_COLS], s_ok[TJ_COLS];
    const int lane = threadIdx.x, P = a.P, K = a.ck.K;
    const int row = blockIdx.y * TJ_ROWS + lane;
    const bool row_ok = row < P && tj_path_ok(a, row);
    const double rrad = row_ok ? a.radius[row] : 0.0;
    const int rgrp = (a.group && row < P) ? a.group[row] : -1;
    const double* rk = a.knots + (size_t)(row < P ? row : 0) * (K + 1) * 2;
    double bf = INFINITY, bs = INFINITY;
    int bfw = INT_MAX, bsw = INT_MAX;
    const int k_begin = blockIdx.z * a.chunks_per_split * TJ_CHUNK;
    const int k_end = min(K, k_begin + a.chunks_per_split * TJ_CHUNK);
    for (int kc = k_begin; kc < k_end; kc += TJ_CHUNK) {
        double rx[TJ_CHUNK + 1], ry[TJ_CHUNK + 1];   // the row's knots kc .. kc + TJ_CHUNK; past K: absent
#pragma unroll
        for (int i = 0; i <= TJ_CHUNK; ++i) {
            const bool in = row_ok && kc + i <= K;
            rx[i] = in ? rk[2 * (size_t)(kc + i)] : NAN;
            ry[i] = in ? rk[2 * (size_t)(kc + i) + 1] : NAN;
        }
        for (int ct = blockIdx.x; ct < a.coltiles; ct += a.G) {
            const int c0 = ct * TJ_COLS, ncol = min(TJ_COLS, P - c0);
            __syncthreads();   // the previous tile has been read
            if (lane < ncol) {
                const int q = c0 + lane;
                const bool okq = tj_path_ok(a, q);
                s_ok[lane] = okq;
                s_rad[lane] = okq ? a.radius[q] : 0.0;
                s_grp[lane] = a.group ? a.group[q] : -1;
            }
            for (int e = lane; e < ncol * (TJ_CHUNK + 1); e += TJ_ROWS) {
                const int c = e / (TJ_CHUNK + 1), i = e % (TJ_CHUNK + 1);
                double2 v = make_double2(NAN, NAN);
                if (kc + i <= K) {
                    const double* ck = a.knots + ((size_t)(c0 + c) * (K + 1) + kc + i) * 2;
                    v = make_double2(ck[0], ck[1]);
                }
                s_col[c][i] = v;
            }
            __syncthreads();
            uint32_t word = 0;
            for (int c = 0; c < ncol; ++c) {
                if (!s_ok[c]) continue;   // wavefront-uniform
                const int q = c0 + c;
                const double R = rrad + s_rad[c];
                const double RR = R * R;
                double m2min = INFINITY, tfirst = INFINITY;
                double2 ck = s_col[c][0];
                double d0x = ck.x - rx[0], d0y = ck.y - ry[0];
#pragma unroll
                for (int i = 0; i < TJ_CHUNK; ++i) {
                    ck = s_col[c][i + 1];
                    const double d1x = ck.x - rx[i + 1], d1y = ck.y - ry[i + 1];
                    const sc_traj_approach ap = sc_traj_closest(d0x, d0y, d1x, d1y);
                    if (ap.m2 < m2min) m2min = ap.m2;
                    if (ap.m2 < RR) {   // rare: the entry time of the conflict
                        const double cc = d0x * d0x + d0y * d0y;
                        double lc = 0.0;
                        if (!(cc < RR)) {
                            double disc = ap.bb * ap.bb - ap.aa * (cc - RR);
                            disc = disc > 0.0 ? disc : 0.0;
                            lc = sc_clampd((-ap.bb - sqrt(disc)) / ap.aa, 0.0, ap.lam);
                        }
                        const double tau = a.ck.T0 + (double)(kc + i) * a.ck.dt_c;
                        const double tt = tau + lc * a.ck.dt_c;
                        if (tt < tfirst) tfirst = tt;
                    }
                    d0x = d1x;
                    d0y = d1y;
                }
                const bool compared = row_ok && q != row && !(rgrp == s_grp[c] && rgrp >= 0);
                if (compared) {
                    if (tfirst < bf || (tfirst == bf && q < bfw)) { bf = tfirst; bfw = q; }
                    if (m2min < bs || (m2min == bs && q < bsw)) { bs = m2min; bsw = q; }
                    if (tfirst < INFINITY) word |= 1u << c;
                }
            }
            if (word && a.matrix) atomicOr(&a.matrix[(size_t)row * a.nw + ct], word);
        }
    }
    if (row < P) {
        tj_part& o = a.part[(size_t)row * a.slots + (size_t)blockIdx.z * a.G + blockIdx.x];
        o.first = bf;
        o.sep2 = bs;
        o.first_with = bf < INFINITY ? bfw : INT_MAX;
        o.sep_with = bs < INFINITY ? bsw : INT_MAX;
    }
}

// what a conflicts call reports; each may be NULL
struct tj_report {
    double *first_t, *min_sep;
    int32_t *first_with, *min_with, *n_conf;
    uint32_t* conflict;   // [P][ceil(P / TJ_COLS)]
};

struct tj_reduce_args {
    const tj_part* part;
    int slots;
    const uint32_t* matrix;
    int nw;
    const double* radius;
    double sep_cap;
    int32_t* tstatus;
    tj_report o;   // conflict is not read: matrix is it, or scratch
};

// lexicographic minimum of (value, partner) across the wavefront
__device__ __forceinline__ void tj_wave_min(double& v, int& w) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = __shfl_xor(v, s);
        const int ow = __shfl_xor(w, s);
        if (ov < v || (ov == v && ow < w)) { v = ov; w = ow; }
    }
}

__global__ void __launch_bounds__(64) traj_reduce_kernel(tj_reduce_args a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    double bf = INFINITY, bs = INFINITY;
    int bfw = INT_MAX, bsw = INT_MAX, cnt = 0;
    for (int s = lane; s < a.slots; s += 64) {
        const tj_part v = a.part[(size_t)p * a.slots + s];
        if (v.first < bf || (v.first == bf && v.first_with < bfw)) { bf = v.first; bfw = v.first_with; }
        if (v.sep2 < bs || (v.sep2 == bs && v.sep_with < bsw)) { bs = v.sep2; bsw = v.sep_with; }
    }
    if (a.matrix)
        for (int w = lane; w < a.nw; w += 64) cnt += __popc(a.matrix[(size_t)p * a.nw + w]);
    tj_wave_min(bf, bfw);
    tj_wave_min(bs, bsw);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s);
    if (lane != 0) return;
    sc_traj_mark_radius(a.tstatus, p, a.radius[p]);
    const double ms = sqrt(bs);
    const bool rep = ms < a.sep_cap;
    if (a.o.first_t) a.o.first_t[p] = bf;
    if (a.o.first_with) a.o.first_with[p] = bf < INFINITY ? bfw : -1;
    if (a.o.min_sep) a.o.min_sep[p] = rep ? ms : INFINITY;
    if (a.o.min_with) a.o.min_with[p] = rep ? bsw : -1;
    if (a.o.n_conf) a.o.n_conf[p] = cnt;
}

static bool tj_conf_invalid(sc_ctx* ctx, int P, const sc_traj_clock& ck, const double* radius, double sep_cap) {
    return !ctx || !radius || !sc_traj_size_ok(P, ck.K) || !sc_traj_clock_ok(ck) || isnan(sep_cap) || !(sep_cap > 0.0);
}

int sc_traj_launch_knots(sc_ctx* ctx, const sc_traj_paths& pa, const sc_traj_clock& ck, double* knots, int32_t* tstatus) {
    tj_knots_args a{pa, ck, knots, tstatus};
    int tk = sc_time_begin(ctx, SC_K_SMOOTH);
    hipLaunchKernelGGL(traj_knots_kernel, dim3((ck.K + TJ_KN_THREADS) / TJ_KN_THREADS, pa.P), dim3(TJ_KN_THREADS), 0, ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// how a launch of the pair kernel is split, and the scratch it needs
struct tj_plan {
    int rowtiles, coltiles, G, splits, chunks_per_split, slots, nw;
    size_t part_bytes, matrix_bytes;
};

static tj_plan tj_make_plan(const sc_ctx* ctx, int P, int K, bool own_matrix) {
    tj_plan pl;
    pl.rowtiles = (P + TJ_ROWS - 1) / TJ_ROWS;
    pl.coltiles = (P + TJ_COLS - 1) / TJ_COLS;
    const int chunks = (K + TJ_CHUNK - 1) / TJ_CHUNK;
    const int want = (ctx->traj_wg_target + pl.rowtiles - 1) / pl.rowtiles;   // G * splits <= want
    pl.G = pl.coltiles < want ? pl.coltiles : want;
    int s = want / pl.G;
    if (s > chunks) s = chunks;
    pl.chunks_per_split = (chunks + s - 1) / s;
    pl.splits = (chunks + pl.chunks_per_split - 1) / pl.chunks_per_split;
    pl.slots = pl.G * pl.splits;
    pl.nw = pl.coltiles;
    pl.part_bytes = al256((size_t)P * pl.slots * sizeof(tj_part));
    pl.matrix_bytes = own_matrix ? al256((size_t)P * pl.nw * 4) : 0;
    return pl;
}

// the pair and the reduce kernel behind a report; scratch: ctx->traj_part
static int tj_launch_conflicts(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, const sc_traj_clock& ck, const double* radius,
                               const int32_t* group, double sep_cap, const tj_report& o) {
    const tj_plan pl = tj_make_plan(ctx, P, ck.K, !o.conflict && o.n_conf);
    const int reserved = sc_scratch_reserve(ctx, &ctx->traj_part, pl.part_bytes + pl.matrix_bytes);
    if (reserved != SC_OK) return reserved;
    tj_part* part = (tj_part*)ctx->traj_part.p;
    uint32_t* matrix = o.conflict ? o.conflict : (o.n_conf ? (uint32_t*)((char*)ctx->traj_part.p + pl.part_bytes) : nullptr);
    if (matrix) SC_HIP(ctx, hipMemsetAsync(matrix, 0, (size_t)P * pl.nw * 4, ctx->stream));
    int tk = sc_time_begin(ctx, SC_K_SMOOTH);
    tj_pair_args a{knots, tstatus, radius, group, P, ck, pl.coltiles, pl.G, pl.chunks_per_split, pl.slots, part, matrix, pl.nw};
    hipLaunchKernelGGL(traj_pairs_kernel, dim3(pl.G, pl.rowtiles, pl.splits), dim3(TJ_ROWS), 0, ctx->stream, a);
    tj_reduce_args r{part, pl.slots, matrix, pl.nw, radius, sep_cap, tstatus, o};
    hipLaunchKernelGGL(traj_reduce_kernel, dim3(P), dim3(64), 0, ctx->stream, r);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_traj_knots_batch(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets, const int32_t* length,
                                   const int32_t* status, int P, const double* t0, const int32_t* flags, double T0, double dt_c, int K,
                                   double* knots, int32_t* tstatus) {
    const sc_traj_paths pa{time, pts, offsets, length, status, t0, flags, P};
    const sc_traj_clock ck{T0, dt_c, K};
    if (sc_traj_input_invalid(ctx, pa, ck) || !knots || !tstatus) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return sc_traj_launch_knots(ctx, pa, ck, knots, tstatus);
}

extern "C" int sc_traj_conflicts_batch(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, double T0, double dt_c,
                                       const double* radius, const int32_t* group, double sep_cap, double* first_t, int32_t* first_with,
                                       double* min_sep, int32_t* min_with, int32_t* n_conf, uint32_t* conflict) {
    const sc_traj_clock ck{T0, dt_c, K};
    if (tj_conf_invalid(ctx, P, ck, radius, sep_cap) || !knots || !tstatus) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return tj_launch_conflicts(ctx, knots, tstatus, P, ck, radius, group, sep_cap, tj_report{first_t, min_sep, first_with, min_with, n_conf, conflict});
}

extern "C" int sc_fleet_conflicts_batch(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets, const int32_t* length,
                                        const int32_t* status, int P, const double* t0, const int32_t* flags, double T0, double dt_c, int K,
                                        double* knots, int32_t* tstatus, const double* radius, const int32_t* group, double sep_cap,
                                        double* first_t, int32_t* first_with, double* min_sep, int32_t* min_with, int32_t* n_conf,
                                        uint32_t* conflict) {
    const sc_traj_paths pa{time, pts, offsets, length, status, t0, flags, P};
    const sc_traj_clock ck{T0, dt_c, K};
    if (sc_traj_input_invalid(ctx, pa, ck) || tj_conf_invalid(ctx, P, ck, radius, sep_cap)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    int r = sc_traj_scratch_knots(ctx, P, K, &knots, &tstatus);
    if (r == SC_OK) r = sc_traj_launch_knots(ctx, pa, ck, knots, tstatus);
    if (r != SC_OK) return r;
    return tj_launch_conflicts(ctx, knots, tstatus, P, ck, radius, group, sep_cap, tj_report{first_t, min_sep, first_with, min_with, n_conf, conflict});
}

// ---- host forms ----
// a report's slots in a stage, in the order of its members; tj_report_dev, after st.upload(): the report on the device
static int tj_stage_report(sc_stage& st, const tj_report& h, int P) {
    const size_t pb = (size_t)P * 4;
    const int first = st.out(h.first_t, h.first_t ? pb * 2 : 0);
    st.out(h.min_sep, h.min_sep ? pb * 2 : 0), st.out(h.first_with, h.first_with ? pb : 0), st.out(h.min_with, h.min_with ? pb : 0);
    st.out(h.n_conf, h.n_conf ? pb : 0), st.out(h.conflict, h.conflict ? (size_t)P * ((P + TJ_COLS - 1) / TJ_COLS) * 4 : 0);
    return first;
}

static tj_report tj_report_dev(const sc_stage& st, int i, const tj_report& h) {
    return tj_report{h.first_t ? st.dev<double>(i) : nullptr,         h.min_sep ? st.dev<double>(i + 1) : nullptr,
                     h.first_with ? st.dev<int32_t>(i + 2) : nullptr, h.min_with ? st.dev<int32_t>(i + 3) : nullptr,
                     h.n_conf ? st.dev<int32_t>(i + 4) : nullptr,     h.conflict ? st.dev<uint32_t>(i + 5) : nullptr};
}

extern "C" int sc_traj_knots_batch_host(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets, const int32_t* length,
                                        const int32_t* status, int P, const double* t0, const int32_t* flags, double T0, double dt_c,
                                        int K, double* knots, int32_t* tstatus) {
    const sc_traj_paths pa{time, pts, offsets, length, status, t0, flags, P};
    const sc_traj_clock ck{T0, dt_c, K};
    if (sc_traj_input_invalid(ctx, pa, ck) || !knots || !tstatus || sc_traj_paths_outside(pa)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_pa = sc_traj_stage_paths(st, pa);
    const int o_k = st.out(knots, (size_t)P * (K + 1) * 16), o_s = st.out(tstatus, (size_t)P * 4);
    int r = st.upload();
    if (r == SC_OK) r = sc_traj_launch_knots(ctx, sc_traj_staged_paths(st, i_pa, pa), ck, st.dev<double>(o_k), st.dev<int32_t>(o_s));
    return st.finish(r);
}

extern "C" int sc_traj_conflicts_batch_host(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, double T0, double dt_c,
                                            const double* radius, const int32_t* group, double sep_cap, double* first_t,
                                            int32_t* first_with, double* min_sep, int32_t* min_with, int32_t* n_conf, uint32_t* conflict) {
    const sc_traj_clock ck{T0, dt_c, K};
    const tj_report out{first_t, min_sep, first_with, min_with, n_conf, conflict};
    if (tj_conf_invalid(ctx, P, ck, radius, sep_cap) || !knots || !tstatus || sc_traj_radius_outside(radius, P)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pb = (size_t)P * 4;
    sc_stage st(ctx);
    const int i_k = st.in(knots, (size_t)P * (K + 1) * 16), i_s = st.in(tstatus, pb), i_r = st.in(radius, pb * 2),
              i_g = st.in(group, group ? pb : 0);
    st.back(i_s, tstatus, pb);
    const int o_rep = tj_stage_report(st, out, P);
    int r = st.upload();
    if (r == SC_OK)
        r = tj_launch_conflicts(ctx, st.dev<const double>(i_k), st.dev<int32_t>(i_s), P, ck, st.dev<const double>(i_r),
                                group ? st.dev<const int32_t>(i_g) : nullptr, sep_cap, tj_report_dev(st, o_rep, out));
    return st.finish(r);
}

extern "C" int sc_fleet_conflicts_batch_host(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets,
                                             const int32_t* length, const int32_t* status, int P, const double* t0, const int32_t* flags,
                                             double T0, double dt_c, int K, double* knots, int32_t* tstatus, const double* radius,
                                             const int32_t* group, double sep_cap, double* first_t, int32_t* first_with, double* min_sep,
                                             int32_t* min_with, int32_t* n_conf, uint32_t* conflict) {
    const sc_traj_paths pa{time, pts, offsets, length, status, t0, flags, P};
    const sc_traj_clock ck{T0, dt_c, K};
    const tj_report out{first_t, min_sep, first_with, min_with, n_conf, conflict};
    if (sc_traj_input_invalid(ctx, pa, ck) || tj_conf_invalid(ctx, P, ck, radius, sep_cap)) return SC_ERR_INVALID;
    if (sc_traj_paths_outside(pa) || sc_traj_radius_outside(radius, P)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pb = (size_t)P * 4;
    sc_stage st(ctx);
    const int i_pa = sc_traj_stage_paths(st, pa);
    const int i_r = st.in(radius, pb * 2), i_g = st.in(group, group ? pb : 0);
    const int o_k = st.out(knots, (size_t)P * (K + 1) * 16), o_s = st.out(tstatus, pb);   // slots even when not copied back
    const int o_rep = tj_stage_report(st, out, P);
    int r = st.upload();
    if (r == SC_OK) r = sc_traj_launch_knots(ctx, sc_traj_staged_paths(st, i_pa, pa), ck, st.dev<double>(o_k), st.dev<int32_t>(o_s));
    if (r == SC_OK)
        r = tj_launch_conflicts(ctx, st.dev<const double>(o_k), st.dev<int32_t>(o_s), P, ck, st.dev<const double>(i_r),
                                group ? st.dev<const int32_t>(i_g) : nullptr, sep_cap, tj_report_dev(st, o_rep, out));
    return st.finish(r);
}
