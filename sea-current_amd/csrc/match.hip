// match.hip -- scan matching: the pose of a scan against the map (sc_scan_match_batch).  DESIGN.md section 25; the definition
// is in include/sea_current_hip.h.
//
// The work is S R (2wx+1)(2wy+1) N cell lookups, each read by exactly one candidate: nothing to stage, only coalescing and
// parallelism.  Kernels, all integer, no atomics:
//   1. mt_cost_kernel (match_common.h, shared with match_wide.hip): one thread per cell of the padded cost map, uint16 [H+2][W+2] plus one cell that holds 0: the grid's
//      cost (min(d2, cap), unk where unknown) inside a one-cell border of unk.  The score kernel clamps a coordinate to the
//      border, so it has no off-grid branch and every load lies inside the map by construction; an absent point reads the
//      zero cell.
//   2. mt_score_kernel: one workgroup per (scan, rotation, tile of 256 candidates).  Candidates are numbered dy-major, so the
//      64 lanes of a wave run along dx and read consecutive cells of a row (of a few rows when the window is narrower than a
//      wave).  A lane holds 4 candidates in registers; a point's coordinates are uniform across the wave, and so is the test
//      whether the point stays inside the grid over the whole window: then a load's index is one add.  The workgroup's waves
//      split the points (wave w takes the groups of MT_UNROLL points w, w + WAVES, ...) and add their partial sums through
//      LDS: the sums are integers, so the split cannot change them.  4 waves when the launch has MT_FEW workgroups or more,
//      16 below that.  The workgroup then leaves its smallest key and the number of its candidates at that score.
//   3. mt_pick_kernel: one workgroup per scan: the smallest key over rotations and tiles, the ties (a partial's count only
//      counts when its score is the minimum) and the present points of the chosen rotation.
#include "match_common.h"

namespace {

constexpr int MT_TILE = 256;     // candidates per workgroup: 4 per lane
constexpr int MT_PER_LANE = 4;
constexpr int MT_UNROLL = 4;     // points whose loads are in flight together
constexpr size_t MT_FEW = 512;   // workgroups below which a launch leaves most of the machine idle (2 per compute unit)

struct mt_part { unsigned long long key; int32_t count; int32_t pad; };   // key = score << 32 | (dx^2 + dy^2) << 16 | dyi << 8 | dxi

// WAVES wavefronts share the points of one tile of candidates: 4 when the launch fills the machine without it, 16 when it has
// few workgroups (one scan of a mapping loop), where the time is the chain of a wave's rounds of loads.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void mt_score_kernel(const uint16_t* __restrict__ cost, const int32_t* __restrict__ pts,
                                                              const int32_t* __restrict__ centre, int s0, int R, int N, int W, int H, int wx,
                                                              int wy, int tiles, mt_part* __restrict__ part, int32_t* __restrict__ score) {
    __shared__ uint32_t sums[WAVES][MT_TILE];
    __shared__ unsigned long long keys[MT_TILE];
    const int ndx = 2 * wx + 1, ncand = ndx * (2 * wy + 1);
    const int tile = blockIdx.x % tiles, sr = blockIdx.x / tiles;   // sr = (s - s0) R + r
    const int s = s0 + sr / R, r = sr % R;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform, and the compiler is told so: the points are scalar loads
    const size_t srg = (size_t)s * R + r;
    const int cx = centre[2 * s], cy = centre[2 * s + 1];
    // the candidate this thread reduces and writes: the first 256 threads have one
    const bool reducer = tid < MT_TILE && tile * MT_TILE + tid < ncand;
    const int mine = tile * MT_TILE + (tid & (MT_TILE - 1));
    if (!mt_centre_ok(cx) || !mt_centre_ok(cy)) {   // uniform: the whole workgroup leaves
        if (score && reducer) score[srg * ncand + mine] = 0;
        return;
    }
    // this lane's candidates: tile * 256 + j * 64 + lane; one past the window computes a harmless in-range sum
    const int Wp = W + 2, zero_cell = Wp * (H + 2);
    int bx[MT_PER_LANE], by[MT_PER_LANE];
    uint32_t base[MT_PER_LANE], acc[MT_PER_LANE];
#pragma unroll
    for (int j = 0; j < MT_PER_LANE; ++j) {
        const int c = min(tile * MT_TILE + j * 64 + lane, ncand - 1);
        bx[j] = cx + c % ndx - wx;
        by[j] = cy + c / ndx - wy;
        base[j] = (uint32_t)((by[j] + 1) * Wp + bx[j] + 1);   // the candidate's own cell in the padded map (meaningless while it lies outside)
        acc[j] = 0;
    }
    const int32_t* __restrict__ p = pts + srg * (size_t)N * 2;
    // |cx + dx + px| <= 8192 + 2 * 16384 + 64: sums of coordinates stay far inside int32.  A lane's sum is at most
    // 32767 * 65536 = 2 147 418 112 < 2^31 over all N points, so every partial sum and the total fit uint32 and int32.
    for (int k0 = wave * MT_UNROLL; k0 < N; k0 += WAVES * MT_UNROLL) {
        uint32_t v[MT_UNROLL][MT_PER_LANE];
#pragma unroll
        for (int u = 0; u < MT_UNROLL; ++u) {
            const int k = min(k0 + u, N - 1);
            const int px = p[2 * k], py = p[2 * k + 1];
            const bool present = k0 + u < N && !mt_absent(px) && !mt_absent(py);   // uniform
            // uniform: the point lies inside the grid for every candidate of the window.  Then nothing is clamped, and
            // the cell is the candidate's own plus one offset for the whole wave: one add per load
            const bool inside = present && cx - wx + px >= 0 && cx + wx + px < W && cy - wy + py >= 0 && cy + wy + py < H;
            if (inside) {
                const uint32_t off = (uint32_t)(py * Wp + px);
#pragma unroll
                for (int j = 0; j < MT_PER_LANE; ++j) v[u][j] = cost[base[j] + off];   // in [Wp + 1, Wp (H + 1) - 1)
            } else {
#pragma unroll
                for (int j = 0; j < MT_PER_LANE; ++j) {
                    // clamped to the border: -1 .. W and -1 .. H, so the index lies in [0, Wp (H + 2)); an absent point reads 0
                    const int x = min(max(present ? bx[j] + px : 0, -1), W), y = min(max(present ? by[j] + py : 0, -1), H);
                    const int idx = present ? (y + 1) * Wp + (x + 1) : zero_cell;
                    v[u][j] = cost[idx];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < MT_UNROLL; ++u)
#pragma unroll
            for (int j = 0; j < MT_PER_LANE; ++j) acc[j] += v[u][j];
    }
#pragma unroll
    for (int j = 0; j < MT_PER_LANE; ++j) sums[wave][j * 64 + lane] = acc[j];
    __syncthreads();
    uint32_t total = 0;
    unsigned long long key = ~0ull;
    if (tid < MT_TILE) {
#pragma unroll
        for (int w = 0; w < WAVES; ++w) total += sums[w][tid];
        if (reducer) {
            const int dxi = mine % ndx, dyi = mine / ndx, dx = dxi - wx, dy = dyi - wy;
            key = (unsigned long long)total << 32 | (unsigned long long)(dx * dx + dy * dy) << 16 | (unsigned)dyi << 8 | (unsigned)dxi;
            if (score) score[srg * ncand + mine] = (int32_t)total;
        }
        keys[tid] = key;
    }
    __syncthreads();
    for (int h = MT_TILE / 2; h > 0; h >>= 1) {
        if (tid < h) keys[tid] = min(keys[tid], keys[tid + h]);
        __syncthreads();
    }
    const unsigned long long best = keys[0];   // the tile's first candidate exists, so best is a key
    const int n_min = __syncthreads_count(reducer && total == (uint32_t)(best >> 32));
    if (tid == 0) part[srg * tiles + tile] = {best, n_min, 0};
}

__global__ __launch_bounds__(256) void mt_pick_kernel(const mt_part* __restrict__ part, const int32_t* __restrict__ pts,
                                                      const int32_t* __restrict__ centre, int R, int N, int wx, int wy, int tiles,
                                                      int32_t* __restrict__ best) {
    __shared__ mt_key keys[256];
    __shared__ int cnt[256];
    const int s = blockIdx.x, tid = threadIdx.x;
    int32_t* out = best + (size_t)s * 6;
    const int cx = centre[2 * s], cy = centre[2 * s + 1];
    if (!mt_centre_ok(cx) || !mt_centre_ok(cy)) {
        if (tid < 6) out[tid] = tid == 0 ? SC_MATCH_IGNORED : 0;
        return;
    }
    const mt_part* __restrict__ ps = part + (size_t)s * R * tiles;
    const int n = R * tiles;
    mt_key mk = {~0ull, ~0u};
    for (int i = tid; i < n; i += 256) {
        const unsigned long long key = ps[i].key;
        const mt_key k = {(key >> 32) << 32 | ((key >> 16) & 0xffffu) << 8 | (unsigned)(i / tiles), (uint32_t)(key & 0xffffu)};
        if (mt_less(k, mk)) mk = k;
    }
    keys[tid] = mk;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h && mt_less(keys[tid + h], keys[tid])) keys[tid] = keys[tid + h];
        __syncthreads();
    }
    const mt_key bk = keys[0];
    const uint32_t smin = (uint32_t)(bk.k1 >> 32);
    const int r = (int)(bk.k1 & 0xffu);
    // ties: n <= 256 * 66 partials of at most 256 candidates each, far inside int32
    int ties = 0, present = 0;
    for (int i = tid; i < n; i += 256)
        if ((uint32_t)(ps[i].key >> 32) == smin) ties += ps[i].count;
    const int32_t* __restrict__ p = pts + ((size_t)s * R + r) * (size_t)N * 2;
    for (int k = tid; k < N; k += 256) present += !mt_absent(p[2 * k]) && !mt_absent(p[2 * k + 1]);
    __syncthreads();
    cnt[tid] = ties;
    keys[tid].k2 = (uint32_t)present;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            cnt[tid] += cnt[tid + h];
            keys[tid].k2 += keys[tid + h].k2;
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = r;
        out[1] = (int)(bk.k2 & 0xffu) - wx;
        out[2] = (int)(bk.k2 >> 8) - wy;
        out[3] = (int32_t)smin;
        out[4] = (int32_t)keys[0].k2;
        out[5] = cnt[0];
    }
}

}  // namespace

static bool match_args_ok(const sc_ctx* ctx, const int32_t* d2, const int32_t* pts, const int32_t* centre, int S, int R, int N, int W, int H,
                          int wx, int wy, int32_t d2_cap, int32_t unk, const int32_t* best, const int32_t* score) {
    if (!ctx || !d2 || !pts || !centre || !best || S < 0) return false;
    if (R < 1 || R > SC_MATCH_MAX_ROT || N < 1 || N > SC_MATCH_MAX_POINTS || W < 1 || W > SC_MAX_DIM || H < 1 || H > SC_MAX_DIM) return false;
    if (wx < 0 || wx > SC_MATCH_MAX_HALF || wy < 0 || wy > SC_MATCH_MAX_HALF || d2_cap < 1 || d2_cap > 32767 || unk < 0 || unk > d2_cap)
        return false;
    return score != best;
}

extern "C" int sc_scan_match_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre, int S,
                                   int R, int N, int W, int H, int wx, int wy, int32_t d2_cap, int32_t unk, int32_t* best, int32_t* score) {
    if (!match_args_ok(ctx, d2, pts, centre, S, R, N, W, H, wx, wy, d2_cap, unk, best, score)) return SC_ERR_INVALID;
    if (S == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const int ncand = (2 * wx + 1) * (2 * wy + 1), tiles = (ncand + MT_TILE - 1) / MT_TILE;   // at most 66 tiles
    const int cells = (W + 2) * (H + 2) + 1;
    int r = sc_scratch_reserve(ctx, &ctx->mt_cost, (size_t)cells * 2);
    if (r == SC_OK) r = sc_scratch_reserve(ctx, &ctx->mt_part, (size_t)S * R * tiles * sizeof(mt_part));
    if (r != SC_OK) return r;
    uint16_t* cost = (uint16_t*)ctx->mt_cost.p;
    mt_part* part = (mt_part*)ctx->mt_part.p;
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    hipLaunchKernelGGL(mt_cost_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, d2, known, W, H, d2_cap, unk, cost);
    // a launch takes as many scans as keep its workgroups below 2^30: R * tiles <= 256 * 66
    const int per_launch = (1 << 30) / (R * tiles);
    for (int s0 = 0; s0 < S; s0 += per_launch) {
        const int ns = S - s0 < per_launch ? S - s0 : per_launch;
        // fewer than MT_FEW workgroups: 16 wavefronts share a tile's points, else 4
        if ((size_t)ns * R * tiles < MT_FEW)
            hipLaunchKernelGGL(mt_score_kernel<16>, dim3((unsigned)ns * R * tiles), dim3(1024), 0, ctx->stream, cost, pts, centre, s0, R, N, W, H,
                               wx, wy, tiles, part, score);
        else
            hipLaunchKernelGGL(mt_score_kernel<4>, dim3((unsigned)ns * R * tiles), dim3(256), 0, ctx->stream, cost, pts, centre, s0, R, N, W, H, wx,
                               wy, tiles, part, score);
    }
    hipLaunchKernelGGL(mt_pick_kernel, dim3((unsigned)S), dim3(256), 0, ctx->stream, part, pts, centre, R, N, wx, wy, tiles, best);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_scan_match_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre,
                                        int S, int R, int N, int W, int H, int wx, int wy, int32_t d2_cap, int32_t unk, int32_t* best,
                                        int32_t* score) {
    if (!match_args_ok(ctx, d2, pts, centre, S, R, N, W, H, wx, wy, d2_cap, unk, best, score)) return SC_ERR_INVALID;
    if (S == 0) return SC_OK;
    for (int s = 0; s < S; ++s)
        if (!mt_centre_ok(centre[2 * s]) || !mt_centre_ok(centre[2 * s + 1])) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H, vol = (size_t)S * R * (2 * wx + 1) * (2 * wy + 1);
    sc_stage st(ctx);
    const int i_d = st.in(d2, n * 4), i_k = st.in(known, known ? n : 0), i_p = st.in(pts, (size_t)S * R * N * 8), i_c = st.in(centre, (size_t)S * 8);
    const int o_b = st.out(best, (size_t)S * 24), o_s = st.out(score, score ? vol * 4 : 0);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_scan_match_batch(ctx, st.dev<const int32_t>(i_d), known ? st.dev<const uint8_t>(i_k) : nullptr, st.dev<const int32_t>(i_p),
                                st.dev<const int32_t>(i_c), S, R, N, W, H, wx, wy, d2_cap, unk, st.dev<int32_t>(o_b),
                                score ? st.dev<int32_t>(o_s) : nullptr);
    return st.finish(r);
}
