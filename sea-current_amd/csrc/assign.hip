// assign.hip -- robots to goals: the cost matrix taken out of cost fields and the optimal one-to-one matching on it
// (sc_field_cost_matrix, sc_assign_batch, sc_fleet_assign_batch; the definition is in include/sea_current_hip.h and DESIGN.md
// section 19).
//
// Matrix: one thread per (robot, field).
// Matching: one workgroup per problem, thread j owns post j (a column, or a row when R > C: a transpose kernel then writes the
// matrix posts-contiguous into scratch first, so that the scan of a line stays one coalesced read).  minv, way, used, v and p of
// post j live in thread j's registers; u [n], a mirror of p [m] and the reduction slots live in LDS.  Nothing crosses
// workgroups, there are no spin waits and no atomics.
// The deltas are applied lazily.  With D = the sum of the deltas of the current line so far, a post keeps raw = minv + D.  A new
// line i0 is scanned right after the post j0 that led to it was marked, when u[i0] still has its value from the start of the
// line, so raw candidates are a[i0][j] - u[i0] - v[j] + D and comparing raw values is comparing minv.  The minimum of raw over
// the unused posts is the new D (delta = that minimum - the old D).  A post marked at D = Dm has received D_end - Dm by the end of
// the line: v[j] -= D_end - Dm and u[p[j]] += D_end - Dm, u[i] += D_end, once per line.  Integers: exactly the eager form.
// raw < 2^53 (the tests watch the C reference's largest value), so (raw << 10) | j fits 64 bits and one unsigned min-reduction
// gives D and the lowest post among equals.  A step is: scan, wave reduction, one LDS slot per wave, one barrier, every thread
// reads the slots (double-buffered by step parity, hence one barrier and not two), the next line from the LDS mirror of p.
// BLOCK = 64 is one wavefront: no barrier at all, and the matrix (at most 64 x 64) sits in LDS.
// Work is bounded: line i takes at most i + 1 passes (it can mark the i paired posts and one free one), n (n + 1) / 2 in all.
#include "sc_internal.h"

#define AS_MAX_DIM SC_ASSIGN_MAX_DIM
#define AS_BIG SC_ASSIGN_BIG
#define AS_NONE (-1)
#define AS_RAW_INF ((1ll << 53) - 1)
#define AS_MAT_THREADS 256

struct as_matrix_args {
    const int32_t* g;
    int F, R;
    long long cells;
    const int32_t *cell, *col_cost;
    int32_t* cost;
};

__global__ void __launch_bounds__(AS_MAT_THREADS) field_cost_matrix_kernel(as_matrix_args a) {
    const long long t = (long long)blockIdx.x * AS_MAT_THREADS + threadIdx.x;
    if (t >= (long long)a.R * a.F) return;
    const int r = (int)(t / a.F), f = (int)(t % a.F);
    const int c = a.cell[r];
    int32_t out = SC_FIELD_INF;
    if (c >= 0 && c < a.cells) {
        const int32_t gv = a.g[(size_t)f * a.cells + c];
        if (gv != SC_FIELD_INF) {
            const long long s = (long long)gv + (a.col_cost ? a.col_cost[f] : 0);
            out = s > INT32_MAX - 1 ? INT32_MAX - 1 : (int32_t)s;
        }
    }
    a.cost[t] = out;
}

// [B][R][C] -> [B][C][R] through a padded 32 x 32 LDS tile
__global__ void __launch_bounds__(256) assign_transpose_kernel(const int32_t* in, int R, int C, int32_t* out) {
    __shared__ int32_t tile[32][33];
    const int32_t* src = in + (size_t)blockIdx.z * R * C;
    int32_t* dst = out + (size_t)blockIdx.z * R * C;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int k = ty; k < 32; k += 8)
        if (r0 + k < R && c0 + tx < C) tile[k][tx] = src[(size_t)(r0 + k) * C + c0 + tx];
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (c0 + k < C && r0 + tx < R) dst[(size_t)(c0 + k) * R + r0 + tx] = tile[tx][k];
}

struct as_args {
    const int32_t* lines;   // [B][n][m]: the caller's cost [B][R][C], or its transpose when R > C
    int n, m, swap;         // n lines <= m posts
    int32_t *col_of, *row_of;
    int64_t *u, *v, *info;
};

template <int BLOCK>
__device__ __forceinline__ void as_sync() {
    if (BLOCK == 64) wave_lds_sync();
    else __syncthreads();
}

__device__ __forceinline__ unsigned long long as_wave_min(unsigned long long k) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = __shfl_xor(k, s);
        k = o < k ? o : k;
    }
    return k;
}

__device__ __forceinline__ long long as_wave_sum(long long k) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) k += __shfl_xor(k, s);
    return k;
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) assign_kernel(as_args a) {
    constexpr int WAVES = BLOCK / 64;
    constexpr bool MAT_LDS = BLOCK == 64;
    __shared__ int64_t s_u[BLOCK];
    __shared__ int32_t s_p[BLOCK];
    __shared__ int32_t s_way[BLOCK];
    __shared__ unsigned long long s_key[2][WAVES];
    __shared__ long long s_sum[2][WAVES];
    __shared__ int32_t s_mat[MAT_LDS ? 64 * 64 : 1];

    const int j = threadIdx.x, n = a.n, m = a.m, b = blockIdx.x;
    const int32_t* A = a.lines + (size_t)b * n * m;
    const bool post = j < m;

    // a negative entry anywhere: the problem is bad.  The single-wavefront build keeps the matrix it has just read.
    int neg = 0;
    for (int k = j; k < n * m; k += BLOCK) {
        const int32_t c = A[k];
        neg |= c < 0;
        if (MAT_LDS) s_mat[k] = c;
    }
    s_u[j] = 0;
    s_p[j] = AS_NONE;
    int bad;
    if constexpr (BLOCK == 64) { bad = __any(neg); wave_lds_sync(); }
    else bad = __syncthreads_or(neg);

    int64_t v = 0;
    int32_t p = AS_NONE;
    long long steps = 0;
    if (!bad) {
        for (int i = 0; i < n; ++i) {
            int64_t raw = AS_RAW_INF, Dm = 0, D = 0;
            int32_t way = AS_NONE;
            bool used = !post;
            int i0 = i, j0 = AS_NONE;
            for (int pass = 0; pass <= i; ++pass) {   // at most i + 1 passes: the bound on work
                const int64_t u0 = s_u[i0];
                if (!used) {
                    const int32_t c = MAT_LDS ? s_mat[i0 * m + j] : A[(size_t)i0 * m + j];
                    const int64_t cur = (c == SC_FIELD_INF ? AS_BIG : (int64_t)c) - u0 - v + D;
                    if (cur < raw) { raw = cur; way = j0; }
                }
                unsigned long long key = used ? ~0ull : ((unsigned long long)raw << 10) | (unsigned)j;
                key = as_wave_min(key);
                if (BLOCK > 64) {
                    const int par = pass & 1;
                    if ((j & 63) == 0) s_key[par][j >> 6] = key;
                    __syncthreads();
#pragma unroll
                    for (int w = 0; w < WAVES; ++w) {
                        const unsigned long long o = s_key[par][w];
                        key = o < key ? o : key;
                    }
                }
                ++steps;
                const int j1 = (int)(key & 1023);
                D = (int64_t)(key >> 10);
                if (j == j1) { used = true; Dm = D; }
                j0 = j1;
                const int nxt = s_p[j1];
                if (nxt == AS_NONE) break;
                i0 = nxt;
            }
            // settle the line: the duals, then the pairs along way
            if (post && used) {
                const int64_t d = D - Dm;
                v -= d;
                if (p != AS_NONE) s_u[p] += d;   // p is one-to-one: no two threads meet on a line
                s_way[j] = way;
            }
            if (j == 0) s_u[i] += D;             // line i is not paired yet: nobody else touches it
            as_sync<BLOCK>();
            if (j == 0) {
                int q = j0;
                for (int k = 0; k <= i && q != AS_NONE; ++k) {
                    const int w = s_way[q];
                    s_p[q] = w == AS_NONE ? i : s_p[w];
                    q = w;
                }
            }
            as_sync<BLOCK>();
            p = s_p[j];
        }
    }

    // outputs in the caller's orientation
    int real = 0;
    long long cost_of = 0;
    if (!bad && post && p != AS_NONE) {
        const int32_t c = MAT_LDS ? s_mat[p * m + j] : A[(size_t)p * m + j];
        real = c != SC_FIELD_INF;
        cost_of = real ? c : 0;
    }
    int32_t* post_pair = (a.swap ? a.col_of : a.row_of);
    int32_t* line_pair = (a.swap ? a.row_of : a.col_of);
    int64_t* post_dual = (a.swap ? a.u : a.v);
    int64_t* line_dual = (a.swap ? a.v : a.u);
    const size_t po = (size_t)b * m, lo = (size_t)b * n;
    if (post) {
        if (post_pair) post_pair[po + j] = real ? p : -1;
        if (post_dual) post_dual[po + j] = bad ? 0 : v;
        if (!bad && p != AS_NONE && line_pair) line_pair[lo + p] = real ? j : -1;   // every line is paired with exactly one post
    }
    if (j < n) {
        if (bad && line_pair) line_pair[lo + j] = -1;
        if (line_dual) line_dual[lo + j] = bad ? 0 : s_u[j];
    }
    long long cnt = as_wave_sum(real), tot = as_wave_sum(cost_of);
    if (BLOCK > 64) {
        if ((j & 63) == 0) { s_sum[0][j >> 6] = cnt; s_sum[1][j >> 6] = tot; }
        __syncthreads();
        cnt = tot = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) { cnt += s_sum[0][w]; tot += s_sum[1][w]; }
    }
    if (j == 0) {
        int64_t* info = a.info + (size_t)b * 4;
        info[0] = cnt; info[1] = tot; info[2] = bad ? 0 : steps; info[3] = bad ? SC_ASSIGN_BAD : SC_ASSIGN_OK;
    }
}

// ---- launches ----
static bool as_dims_invalid(int R, int C) { return R < 1 || R > AS_MAX_DIM || C < 1 || C > AS_MAX_DIM; }

static bool as_matrix_invalid(sc_ctx* ctx, const int32_t* g, int F, int W, int H, const int32_t* cell, int R) {
    return !ctx || !g || !cell || F < 1 || R < 1 || W < 1 || W > SC_MAX_DIM || H < 1 || H > SC_MAX_DIM || (long long)R * F > (1ll << 30);
}

static int as_launch_matrix(sc_ctx* ctx, const int32_t* g, int F, int W, int H, const int32_t* cell, int R, const int32_t* col_cost,
                            int32_t* cost) {
    as_matrix_args a{g, F, R, (long long)W * H, cell, col_cost, cost};
    const long long total = (long long)R * F;
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    hipLaunchKernelGGL(field_cost_matrix_kernel, dim3((unsigned)((total + AS_MAT_THREADS - 1) / AS_MAT_THREADS)), dim3(AS_MAT_THREADS), 0,
                       ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

static int as_launch_assign(sc_ctx* ctx, const int32_t* cost, int B, int R, int C, int32_t* col_of, int32_t* row_of, int64_t* u, int64_t* v,
                            int64_t* info) {
    const bool swap = R > C;
    const int n = swap ? C : R, m = swap ? R : C;
    const int32_t* lines = cost;
    if (swap) {
        int r = sc_scratch_reserve(ctx, &ctx->assign_t, al256((size_t)B * R * C * 4));
        if (r != SC_OK) return r;
        lines = (const int32_t*)ctx->assign_t.p;
    }
    as_args a{lines, n, m, swap ? 1 : 0, col_of, row_of, u, v, info};
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    for (int b0 = 0; b0 < B; b0 += 65535) {   // grid z of the transpose
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        if (swap)
            hipLaunchKernelGGL(assign_transpose_kernel, dim3((C + 31) / 32, (R + 31) / 32, nb), dim3(256), 0, ctx->stream,
                               cost + (size_t)b0 * R * C, R, C, (int32_t*)ctx->assign_t.p + (size_t)b0 * R * C);
    }
    if (m <= 64) hipLaunchKernelGGL(assign_kernel<64>, dim3(B), dim3(64), 0, ctx->stream, a);
    else if (m <= 256) hipLaunchKernelGGL(assign_kernel<256>, dim3(B), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(assign_kernel<1024>, dim3(B), dim3(1024), 0, ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

static bool as_assign_invalid(sc_ctx* ctx, const int32_t* cost, int B, int R, int C, const int32_t* col_of, const int64_t* info) {
    return !ctx || !cost || !col_of || !info || B < 0 || as_dims_invalid(R, C);
}

extern "C" int sc_field_cost_matrix(sc_ctx* ctx, const int32_t* g, int F, int W, int H, const int32_t* cell, int R, const int32_t* col_cost,
                                    int32_t* cost) {
    if (as_matrix_invalid(ctx, g, F, W, H, cell, R) || !cost) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return as_launch_matrix(ctx, g, F, W, H, cell, R, col_cost, cost);
}

extern "C" int sc_assign_batch(sc_ctx* ctx, const int32_t* cost, int B, int R, int C, int32_t* col_of, int32_t* row_of, int64_t* u, int64_t* v,
                               int64_t* info) {
    if (as_assign_invalid(ctx, cost, B, R, C, col_of, info)) return SC_ERR_INVALID;
    if (B == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return as_launch_assign(ctx, cost, B, R, C, col_of, row_of, u, v, info);
}

extern "C" int sc_fleet_assign_batch(sc_ctx* ctx, const int32_t* g, int F, int W, int H, const int32_t* cell, int R, const int32_t* col_cost,
                                     int32_t* cost, int32_t* col_of, int32_t* row_of, int64_t* u, int64_t* v, int64_t* info) {
    if (as_matrix_invalid(ctx, g, F, W, H, cell, R) || !col_of || !info || as_dims_invalid(R, F)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (!cost) {
        int r = sc_scratch_reserve(ctx, &ctx->assign_cost, al256((size_t)R * F * 4));
        if (r != SC_OK) return r;
        cost = (int32_t*)ctx->assign_cost.p;
    }
    int r = as_launch_matrix(ctx, g, F, W, H, cell, R, col_cost, cost);
    if (r == SC_OK) r = as_launch_assign(ctx, cost, 1, R, F, col_of, row_of, u, v, info);
    return r;
}

// ---- host forms ----
// what the kernels cannot refuse: a field value below 0 (the contract of g in sc_field_paths_batch) and a column cost outside
// 0 .. SC_FIELD_SEED_COST_MAX
static bool as_matrix_data_invalid(const int32_t* g, int F, int W, int H, const int32_t* col_cost) {
    const size_t cells = (size_t)F * W * H;
    for (size_t k = 0; k < cells; ++k)
        if (g[k] < 0) return true;
    if (col_cost)
        for (int f = 0; f < F; ++f)
            if (col_cost[f] < 0 || col_cost[f] > SC_FIELD_SEED_COST_MAX) return true;
    return false;
}

extern "C" int sc_field_cost_matrix_host(sc_ctx* ctx, const int32_t* g, int F, int W, int H, const int32_t* cell, int R,
                                         const int32_t* col_cost, int32_t* cost) {
    if (as_matrix_invalid(ctx, g, F, W, H, cell, R) || !cost) return SC_ERR_INVALID;
    if (as_matrix_data_invalid(g, F, W, H, col_cost)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_g = st.in(g, (size_t)F * W * H * 4), i_c = st.in(cell, (size_t)R * 4), i_cc = st.in(col_cost, col_cost ? (size_t)F * 4 : 0);
    const int o_m = st.out(cost, (size_t)R * F * 4);
    int r = st.upload();
    if (r == SC_OK)
        r = as_launch_matrix(ctx, st.dev<const int32_t>(i_g), F, W, H, st.dev<const int32_t>(i_c), R,
                             col_cost ? st.dev<const int32_t>(i_cc) : nullptr, st.dev<int32_t>(o_m));
    return st.finish(r);
}

extern "C" int sc_assign_batch_host(sc_ctx* ctx, const int32_t* cost, int B, int R, int C, int32_t* col_of, int32_t* row_of, int64_t* u,
                                    int64_t* v, int64_t* info) {
    if (as_assign_invalid(ctx, cost, B, R, C, col_of, info)) return SC_ERR_INVALID;
    if (B == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const size_t rb = (size_t)B * R, cb = (size_t)B * C;
    const int i_m = st.in(cost, rb * C * 4);
    const int o_co = st.out(col_of, rb * 4), o_ro = st.out(row_of, row_of ? cb * 4 : 0), o_u = st.out(u, u ? rb * 8 : 0),
              o_v = st.out(v, v ? cb * 8 : 0), o_i = st.out(info, (size_t)B * 32);
    int r = st.upload();
    if (r == SC_OK)
        r = as_launch_assign(ctx, st.dev<const int32_t>(i_m), B, R, C, st.dev<int32_t>(o_co), row_of ? st.dev<int32_t>(o_ro) : nullptr,
                             u ? st.dev<int64_t>(o_u) : nullptr, v ? st.dev<int64_t>(o_v) : nullptr, st.dev<int64_t>(o_i));
    return st.finish(r);
}

extern "C" int sc_fleet_assign_batch_host(sc_ctx* ctx, const int32_t* g, int F, int W, int H, const int32_t* cell, int R,
                                          const int32_t* col_cost, int32_t* cost, int32_t* col_of, int32_t* row_of, int64_t* u, int64_t* v,
                                          int64_t* info) {
    if (as_matrix_invalid(ctx, g, F, W, H, cell, R) || !col_of || !info || as_dims_invalid(R, F)) return SC_ERR_INVALID;
    if (as_matrix_data_invalid(g, F, W, H, col_cost)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_g = st.in(g, (size_t)F * W * H * 4), i_c = st.in(cell, (size_t)R * 4), i_cc = st.in(col_cost, col_cost ? (size_t)F * 4 : 0);
    const int o_m = st.out(cost, (size_t)R * F * 4);   // a slot even when not copied back
    const int o_co = st.out(col_of, (size_t)R * 4), o_ro = st.out(row_of, row_of ? (size_t)F * 4 : 0), o_u = st.out(u, u ? (size_t)R * 8 : 0),
              o_v = st.out(v, v ? (size_t)F * 8 : 0), o_i = st.out(info, 32);
    int r = st.upload();
    if (r == SC_OK)
        r = as_launch_matrix(ctx, st.dev<const int32_t>(i_g), F, W, H, st.dev<const int32_t>(i_c), R,
                             col_cost ? st.dev<const int32_t>(i_cc) : nullptr, st.dev<int32_t>(o_m));
    if (r == SC_OK)
        r = as_launch_assign(ctx, st.dev<const int32_t>(o_m), 1, R, F, st.dev<int32_t>(o_co), row_of ? st.dev<int32_t>(o_ro) : nullptr,
                             u ? st.dev<int64_t>(o_u) : nullptr, v ? st.dev<int64_t>(o_v) : nullptr, st.dev<int64_t>(o_i));
    return st.finish(r);
}
