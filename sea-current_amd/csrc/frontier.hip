// frontier.hip -- exploration frontiers: the known-space mask (sc_known_from_discs, sc_d2_known_i32), the frontier cells and
// their 8-connected clusters (sc_frontier_batch), the robots x clusters cost matrix (sc_frontier_cost_matrix) and a goal per
// robot (sc_fleet_explore_batch).  DESIGN.md section 22; the definitions are in include/sea_current_hip.h.
//
// Definition.  Fr(c) <=> known[c] != 0 and d2[c] >= max(r2_clear, 1) and one of c's four orthogonal neighbours inside the grid
// has known == 0.  A cluster is an 8-connected set of frontier cells; label[c] = the smallest linear index of c's cluster, -1
// where c is no frontier cell: unique, and independent of any execution order.
//
// Kernels of sc_frontier_batch: eight launches at most on one stream, whatever the map; no workgroup waits for another;
// integer atomics only.
//   1. fr_init_kernel: the cluster rows read -1 / 0, ncl reads 0.
//   2. fr_tile_kernel: one wavefront per 64 x 64 tile, lane = column.  The unknown cells of the column, of the rows above and
//      below the tile (one byte per lane) and of the columns left and right of it (lane = row, one ballot each) give the
//      known cells that touch unknown space; d2 is read for those only.  A tile with none leaves after that ballot (it
//      still writes its -1 labels).  Otherwise the 8-connected tile labeller of tile_label.h runs on the mask (sweeps to the
//      fixed point, labels in registers) and stores the forest (global index of the tile-local minimum) and, at each local
//      minimum, the local cell count.
//   3. fr_border_kernel: one thread per cell along the near side of a tile edge; where it is a frontier cell it unites its
//      tree with those of the (up to three) cells it touches across the edge, diagonal ones and tile corners included:
//      the lock-free union-find of tile_label.h (atomicMin of the smaller root into the larger root's slot).
//   4. fr_flatten_kernel: every cell follows its parents to the root and stores it; local counts are added to the root's;
//      roots are counted into ncl[g][1].
//   5. fr_count_kernel / 6. fr_scan_kernel / 7. fr_rank_kernel: the listed clusters (size >= min_size) in ascending order of
//      representative: listed roots per block of 256 cells, an exclusive scan of the block counts (one workgroup per grid),
//      then rank = block offset + the rank inside the block (ballots).  The root of column k < Cmax writes rep, csize, the
//      box of its own cell, and its column into the size scratch.
//   8. fr_slot_kernel (only when slot, cbox or csum is asked for): every frontier cell reads its root's column, stores it,
//      and adds itself to the box (atomicMin / atomicMax) and to the coordinate sums (64-bit atomicAdd).
#include "tile_label.h"

namespace {

using tl::ld_agent;
constexpr int FT = tl::T;                  // tile edge
constexpr int FR_BLOCK = 256;              // cells per block of the count / rank kernels
constexpr int FR_SCAN = 1024;              // threads of the scan kernel

struct fr_args {
    const int32_t* d2;     // [G][H][W]
    const uint8_t* known;  // [G][H][W]
    int32_t* label;        // [G][H][W]
    int32_t* sz;           // [G][H][W]
    int G, W, H, TX, TY;
    int32_t thr;
};

// grid (tiles, grids): grids strided
__global__ __launch_bounds__(64) void fr_tile_kernel(fr_args a) {
    __shared__ int32_t cnt[FT * FT];
    const int lane = threadIdx.x;
    const int W = a.W, H = a.H;
    const int tx = blockIdx.x % a.TX, ty = blockIdx.x / a.TX;
    const int x0 = tx * FT, y0 = ty * FT;
    const int tw = min(FT, W - x0), th = min(FT, H - y0);
    const int cx = x0 + lane;
    const bool colin = lane < tw;
    const size_t n = (size_t)W * H;
    for (int gi = blockIdx.y; gi < a.G; gi += gridDim.y) {
        const int32_t* D = a.d2 + (size_t)gi * n;
        const uint8_t* K = a.known + (size_t)gi * n;
        int32_t* L = a.label + (size_t)gi * n;
        int32_t* S = a.sz + (size_t)gi * n;
        // the column's known / unknown cells, the cells just outside the tile
        uint64_t kn = 0, unk = 0;
#pragma unroll
        for (int y = 0; y < FT; ++y) {
            if (colin && y < th) {
                const bool k = K[(size_t)(y0 + y) * W + cx] != 0;
                kn |= (uint64_t)k << y;
                unk |= (uint64_t)!k << y;
            }
        }
        const bool uabove = colin && y0 > 0 && K[(size_t)(y0 - 1) * W + cx] == 0;
        const bool ubelow = colin && y0 + FT < H && K[(size_t)(y0 + FT) * W + cx] == 0;
        const uint64_t lcol = __ballot(x0 > 0 && lane < th && K[(size_t)(y0 + lane) * W + x0 - 1] == 0);        // lane = row
        const uint64_t rcol = __ballot(x0 + FT < W && lane < th && K[(size_t)(y0 + lane) * W + x0 + FT] == 0);
        uint64_t lm = tl::shup64(unk), rm = tl::shdn64(unk);
        if (lane == 0) lm = lcol;
        if (lane == 63) rm = rcol;
        const uint64_t nb = (unk << 1) | (uint64_t)uabove | (unk >> 1) | ((uint64_t)ubelow << 63) | lm | rm;
        const uint64_t cand = kn & nb;
        uint64_t m = 0;
        if (__ballot(cand != 0ull) != 0ull) {
#pragma unroll
            for (int y = 0; y < FT; ++y) {
                if ((cand >> y) & 1ull) m |= (uint64_t)(D[(size_t)(y0 + y) * W + cx] >= a.thr) << y;
            }
        }
        if (__ballot(m != 0ull) == 0ull) {   // most tiles: no frontier cell
#pragma unroll 8
            for (int y = 0; y < FT; ++y) {
                if (colin && y < th) {
                    const size_t c = (size_t)(y0 + y) * W + cx;
                    L[c] = -1;
                    S[c] = 0;
                }
            }
            continue;
        }
        uint32_t lab[FT];
        tl::label_tile<true>(lab, m, lane);
        tl::count_runs(cnt, lab, m, lane);
        tl::store_forest(L, S, cnt, lab, W, x0, y0, th, colin, lane);
    }
}

// the cells on the near side of a tile edge: (TY - 1) * W above horizontal edges, then (TX - 1) * H left of vertical ones.
// Each is united with the cell facing it and the two diagonal ones across the edge, whichever tiles those lie in: every pair
// of cells of different tiles that touch, corners included, is met (some twice, which a union does not mind).  No pair is
// skipped on account of its predecessor along the edge: with diagonal links two facing pairs next to each other need not
// join the same local clusters on both sides only through each other, and frontier cells are few.
__global__ __launch_bounds__(256) void fr_border_kernel(int32_t* label, int G, int W, int H, int TX, int TY) {
    const size_t n = (size_t)W * H;
    const size_t ne_h = (size_t)(TY - 1) * W, ne = ne_h + (size_t)(TX - 1) * H;
    for (int gi = blockIdx.y; gi < G; gi += gridDim.y) {
        int32_t* L = label + (size_t)gi * n;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += (size_t)gridDim.x * blockDim.x) {
            const tl::edge e = tl::edge_decode(i, ne_h, W, H);
            const int32_t la = ld_agent(L + e.a);
            if (la < 0) continue;
            int32_t lb = ld_agent(L + e.b);
            if (lb >= 0) tl::unite(L, la, lb);
            // the diagonal partners, where they are inside the grid
            if (e.pos > 0 && (lb = ld_agent(L + e.b - e.step)) >= 0) tl::unite(L, la, lb);
            if (e.pos + 1 < e.len && (lb = ld_agent(L + e.b + e.step)) >= 0) tl::unite(L, la, lb);
        }
    }
}

// grid (ceil(n / 256), grids): grids strided.  ncl [G][2]: [1] counts the roots
__global__ __launch_bounds__(256) void fr_flatten_kernel(int32_t* label, int32_t* sz, int32_t* ncl, int G, int W, int H) {
    const size_t n = (size_t)W * H;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (int gi = blockIdx.y; gi < G; gi += gridDim.y) {
        const bool root = c < n && tl::flatten_cell(label + (size_t)gi * n, sz + (size_t)gi * n, c);
        const int k = __popcll(__ballot(root));
        if ((threadIdx.x & 63) == 0 && k) atomicAdd(ncl + 2 * gi + 1, k);
    }
}

__global__ void fr_init_kernel(int G, int Cmax, int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox, int64_t* csum) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)G * 2) ncl[i] = 0;
    if (i >= (size_t)G * Cmax) return;
    rep[i] = -1;
    csize[i] = 0;
    if (cbox) { cbox[4 * i] = 0; cbox[4 * i + 1] = 0; cbox[4 * i + 2] = 0; cbox[4 * i + 3] = 0; }
    if (csum) { csum[2 * i] = 0; csum[2 * i + 1] = 0; }
}

// the listed roots of every block of FR_BLOCK cells.  grid (NB, grids): grids strided; bc [G][NB]
__global__ __launch_bounds__(FR_BLOCK) void fr_count_kernel(const int32_t* label, const int32_t* sz, int G, int W, int H, int min_size,
                                                            int32_t* bc) {
    __shared__ int wsum[FR_BLOCK / 64];
    const size_t n = (size_t)W * H;
    const size_t c = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
    for (int gi = blockIdx.y; gi < G; gi += gridDim.y) {
        const bool listed = c < n && label[(size_t)gi * n + c] == (int32_t)c && sz[(size_t)gi * n + c] >= min_size;
        const int k = __popcll(__ballot(listed));
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = k;
        __syncthreads();
        if (threadIdx.x == 0) {
            int s = 0;
            for (int w = 0; w < FR_BLOCK / 64; ++w) s += wsum[w];
            bc[(size_t)gi * gridDim.x + blockIdx.x] = s;
        }
        __syncthreads();
    }
}

// bc [G][NB] -> its exclusive prefix sums in place; ncl[g][0] = the total.  One workgroup per grid (grids strided): thread t
// owns a contiguous stretch of blocks.
__global__ __launch_bounds__(FR_SCAN) void fr_scan_kernel(int32_t* bc, int NB, int G, int32_t* ncl) {
    __shared__ int part[FR_SCAN];
    const int t = threadIdx.x;
    const int per = (NB + FR_SCAN - 1) / FR_SCAN;
    const int b0 = min(t * per, NB), b1 = min(b0 + per, NB);
    for (int gi = blockIdx.x; gi < G; gi += gridDim.x) {
        int32_t* B = bc + (size_t)gi * NB;
        int s = 0;
        for (int b = b0; b < b1; ++b) s += B[b];
        part[t] = s;
        __syncthreads();
        for (int d = 1; d < FR_SCAN; d <<= 1) {
            const int o = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += o;
            __syncthreads();
        }
        int run = part[t] - s;
        if (t == FR_SCAN - 1) ncl[2 * gi] = part[t];
        for (int b = b0; b < b1; ++b) {
            const int v = B[b];
            B[b] = run;
            run += v;
        }
        __syncthreads();
    }
}

// the column of every root: rank among the listed roots in index order, -1 when not listed or past Cmax; written into sz at
// the root, whose size moves to csize
__global__ __launch_bounds__(FR_BLOCK) void fr_rank_kernel(const int32_t* label, int32_t* sz, int G, int W, int H, int min_size, int Cmax,
                                                           const int32_t* bc, int32_t* rep, int32_t* csize, int32_t* cbox) {
    __shared__ int wsum[FR_BLOCK / 64];
    const size_t n = (size_t)W * H;
    const size_t c = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int gi = blockIdx.y; gi < G; gi += gridDim.y) {
        int32_t* S = sz + (size_t)gi * n;
        const bool root = c < n && label[(size_t)gi * n + c] == (int32_t)c;
        const int32_t s = root ? S[c] : 0;
        const bool listed = root && s >= min_size;
        const uint64_t bal = __ballot(listed);
        if (lane == 0) wsum[wv] = __popcll(bal);
        __syncthreads();
        if (root) {
            int k = -1;
            if (listed) {
                k = bc[(size_t)gi * gridDim.x + blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
                for (int w = 0; w < wv; ++w) k += wsum[w];
                if (k < Cmax) {
                    const size_t o = (size_t)gi * Cmax + k;
                    rep[o] = (int32_t)c;
                    csize[o] = s;
                    if (cbox) {
                        const int x = (int)(c % W), y = (int)(c / W);
                        cbox[4 * o] = x; cbox[4 * o + 1] = y; cbox[4 * o + 2] = x; cbox[4 * o + 3] = y;
                    }
                } else k = -1;
            }
            S[c] = k;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void fr_slot_kernel(const int32_t* label, const int32_t* sz, int G, int W, int H, int Cmax, int32_t* slot,
                                                      int32_t* cbox, int64_t* csum) {
    const size_t n = (size_t)W * H;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    for (int gi = blockIdx.y; gi < G; gi += gridDim.y) {
        const int32_t l = label[(size_t)gi * n + c];
        const int32_t k = l >= 0 ? sz[(size_t)gi * n + l] : -1;
        if (slot) slot[(size_t)gi * n + c] = k;
        if (k < 0) continue;
        const size_t o = (size_t)gi * Cmax + k;
        const int x = (int)(c % W), y = (int)(c / W);
        if (cbox) {
            atomicMin(cbox + 4 * o, x); atomicMin(cbox + 4 * o + 1, y);
            atomicMax(cbox + 4 * o + 2, x); atomicMax(cbox + 4 * o + 3, y);
        }
        if (csum) {
            atomicAdd((unsigned long long*)csum + 2 * o, (unsigned long long)x);
            atomicAdd((unsigned long long*)csum + 2 * o + 1, (unsigned long long)y);
        }
    }
}

// ---- known space ----
__global__ __launch_bounds__(256) void known_discs_kernel(const uint8_t* base, const int32_t* discs, int R, int W, int H, uint8_t* known) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (size_t)W * H) return;
    const long long x = (long long)(c % W), y = (long long)(c / W);
    bool k = base && base[c] != 0;
    for (int r = 0; r < R && !k; ++r) {
        const long long dx = x - discs[3 * r], dy = y - discs[3 * r + 1], r2 = discs[3 * r + 2];
        k = r2 >= 0 && dx * dx + dy * dy <= r2;
    }
    known[c] = k ? 1 : 0;
}

__global__ __launch_bounds__(256) void d2_known_kernel(const int32_t* d2, const uint8_t* known, size_t cells, int32_t* d2k) {
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < cells; c += (size_t)gridDim.x * 256) d2k[c] = known[c] ? d2[c] : 0;
}

// ---- robots x clusters ----
struct fr_mat_args {
    const int32_t* g;       // [F][H][W]
    const int32_t* fgrid;   // [F] or NULL
    const int32_t* slot;    // [G][H][W]
    const int32_t* csize;   // [G][Cmax]
    int F, G, Cmax;
    size_t n;
    long long gain, size_cap;
    unsigned long long* key;   // [F][Cmax]
    int32_t *cost, *cell;      // [F][Cmax]
};

// one thread per cell of every grid; a cell of a listed cluster offers its value of every field of its grid to the field's
// key of the cluster's column: min over g << 32 | cell = the smallest g, then the smallest cell
__global__ __launch_bounds__(256) void fr_mat_min_kernel(fr_mat_args a) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.n) return;
    for (int gi = blockIdx.y; gi < a.G; gi += gridDim.y) {
        const int32_t k = a.slot[(size_t)gi * a.n + c];
        if (k < 0 || k >= a.Cmax) continue;
        for (int f = 0; f < a.F; ++f) {
            if ((a.fgrid ? a.fgrid[f] : 0) != gi) continue;
            const int32_t v = a.g[(size_t)f * a.n + c];
            if (v < 0 || v == SC_FIELD_INF) continue;
            atomicMin(a.key + (size_t)f * a.Cmax + k, ((unsigned long long)(uint32_t)v << 32) | (unsigned long long)c);
        }
    }
}

__global__ __launch_bounds__(256) void fr_mat_out_kernel(fr_mat_args a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.F * a.Cmax) return;
    const unsigned long long key = a.key[i];
    if (key == ~0ull) {
        a.cost[i] = SC_FIELD_INF;
        a.cell[i] = -1;
        return;
    }
    const int f = (int)(i / a.Cmax), k = (int)(i % a.Cmax);
    const int gi = a.fgrid ? a.fgrid[f] : 0;   // in range: a key was offered
    const long long s = a.csize[(size_t)gi * a.Cmax + k];
    const long long v = (long long)(key >> 32) + a.gain * (a.size_cap - (s < a.size_cap ? s : a.size_cap));
    a.cost[i] = (int32_t)(v < (long long)INT32_MAX - 1 ? v : (long long)INT32_MAX - 1);
    a.cell[i] = (int32_t)(uint32_t)key;
}

__global__ void fr_goal_kernel(const int32_t* g, size_t n, int F, int Cmax, const int32_t* cell, const int32_t* col_of, int32_t* goal,
                               int32_t* gcost) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= F) return;
    const int32_t k = col_of[r];
    const int32_t t = (k >= 0 && k < Cmax) ? cell[(size_t)r * Cmax + k] : -1;
    goal[r] = t;
    gcost[r] = (t >= 0 && (size_t)t < n) ? g[(size_t)r * n + t] : -1;
}

}  // namespace

static bool fr_dims_ok(int W, int H) { return W >= 1 && W <= SC_MAX_DIM && H >= 1 && H <= SC_MAX_DIM; }

static bool known_args_ok(const sc_ctx* ctx, const int32_t* discs, int R, int W, int H, const uint8_t* known) {
    return ctx && known && R >= 0 && (discs || R == 0) && fr_dims_ok(W, H);
}

static bool d2k_args_ok(const sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int G, int W, int H, const int32_t* d2k) {
    return ctx && d2 && known && d2k && G > 0 && fr_dims_ok(W, H);
}

static bool frontier_args_ok(const sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int G, int W, int H, int min_size, int Cmax,
                             const int32_t* ncl, const int32_t* rep, const int32_t* csize) {
    return ctx && d2 && known && ncl && rep && csize && G > 0 && fr_dims_ok(W, H) && min_size >= 1 && Cmax >= 1 && Cmax <= SC_FRONTIER_MAX_CLUSTERS;
}

static bool fr_matrix_args_ok(const sc_ctx* ctx, const int32_t* g, int F, const int32_t* fgrid, const int32_t* slot, const int32_t* csize,
                              int G, int W, int H, int Cmax, int32_t gain, int32_t size_cap, const int32_t* cost, const int32_t* cell) {
    return ctx && g && slot && csize && cost && cell && F >= 1 && G > 0 && (fgrid || G == 1) && fr_dims_ok(W, H) && Cmax >= 1 &&
           Cmax <= SC_FRONTIER_MAX_CLUSTERS && (long long)F * Cmax <= (1ll << 30) && gain >= 0 && size_cap >= 0 &&
           (long long)gain * size_cap <= (1ll << 30);
}

static int fr_launch_frontier(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int G, int W, int H, int32_t r2_clear, int min_size,
                              int Cmax, int32_t* label, int32_t* slot, int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox,
                              int64_t* csum) {
    const int TX = (W + FT - 1) / FT, TY = (H + FT - 1) / FT;
    const size_t n = (size_t)W * H;
    const int NB = (int)((n + FR_BLOCK - 1) / FR_BLOCK);
    // scratch: the sizes (later the columns) at the roots, the block counts, the labels when the caller keeps none
    const size_t o_bc = al256((size_t)G * n * 4), o_lab = o_bc + al256((size_t)G * NB * 4);
    int r = sc_scratch_reserve(ctx, &ctx->fr_state, o_lab + (label ? 0 : (size_t)G * n * 4));
    if (r != SC_OK) return r;
    int32_t* sz = (int32_t*)ctx->fr_state.p;
    int32_t* bc = (int32_t*)((char*)ctx->fr_state.p + o_bc);
    if (!label) label = (int32_t*)((char*)ctx->fr_state.p + o_lab);
    const unsigned gy = (unsigned)(G < 65535 ? G : 65535);
    const size_t rows = (size_t)G * (Cmax > 2 ? Cmax : 2);
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    hipLaunchKernelGGL(fr_init_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, G, Cmax, ncl, rep, csize, cbox, csum);
    fr_args a{d2, known, label, sz, G, W, H, TX, TY, r2_clear > 1 ? r2_clear : 1};
    hipLaunchKernelGGL(fr_tile_kernel, dim3((unsigned)(TX * TY), gy), dim3(64), 0, ctx->stream, a);
    if (TX > 1 || TY > 1) {
        const size_t ne = (size_t)(TY - 1) * W + (size_t)(TX - 1) * H;
        hipLaunchKernelGGL(fr_border_kernel, dim3((unsigned)((ne + 255) / 256), gy), dim3(256), 0, ctx->stream, label, G, W, H, TX, TY);
    }
    hipLaunchKernelGGL(fr_flatten_kernel, dim3((unsigned)((n + 255) / 256), gy), dim3(256), 0, ctx->stream, label, sz, ncl, G, W, H);
    hipLaunchKernelGGL(fr_count_kernel, dim3((unsigned)NB, gy), dim3(FR_BLOCK), 0, ctx->stream, (const int32_t*)label, (const int32_t*)sz, G, W,
                       H, min_size, bc);
    hipLaunchKernelGGL(fr_scan_kernel, dim3(gy), dim3(FR_SCAN), 0, ctx->stream, bc, NB, G, ncl);
    hipLaunchKernelGGL(fr_rank_kernel, dim3((unsigned)NB, gy), dim3(FR_BLOCK), 0, ctx->stream, (const int32_t*)label, sz, G, W, H, min_size,
                       Cmax, (const int32_t*)bc, rep, csize, cbox);
    if (slot || cbox || csum)
        hipLaunchKernelGGL(fr_slot_kernel, dim3((unsigned)((n + 255) / 256), gy), dim3(256), 0, ctx->stream, (const int32_t*)label,
                           (const int32_t*)sz, G, W, H, Cmax, slot, cbox, csum);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

static int fr_launch_matrix(sc_ctx* ctx, const int32_t* g, int F, const int32_t* fgrid, const int32_t* slot, const int32_t* csize, int G,
                            int W, int H, int Cmax, int32_t gain, int32_t size_cap, int32_t* cost, int32_t* cell) {
    const size_t n = (size_t)W * H, fc = (size_t)F * Cmax;
    int r = sc_scratch_reserve(ctx, &ctx->fr_key, al256(fc * 8));
    if (r != SC_OK) return r;
    fr_mat_args a{g, fgrid, slot, csize, F, G, Cmax, n, gain, size_cap, (unsigned long long*)ctx->fr_key.p, cost, cell};
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    SC_HIP(ctx, hipMemsetAsync(a.key, 0xFF, fc * 8, ctx->stream));
    hipLaunchKernelGGL(fr_mat_min_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)(G < 65535 ? G : 65535)), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(fr_mat_out_kernel, dim3((unsigned)((fc + 255) / 256)), dim3(256), 0, ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_known_from_discs(sc_ctx* ctx, const uint8_t* base, const int32_t* discs, int R, int W, int H, uint8_t* known) {
    if (!known_args_ok(ctx, discs, R, W, H, known)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    hipLaunchKernelGGL(known_discs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, base, discs, R, W, H, known);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_d2_known_i32(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int G, int W, int H, int32_t* d2k) {
    if (!d2k_args_ok(ctx, d2, known, G, W, H, d2k)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)G * W * H;
    const size_t blocks = (cells + 255) / 256;
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    hipLaunchKernelGGL(d2_known_kernel, dim3((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(256), 0, ctx->stream, d2, known, cells,
                       d2k);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_frontier_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int G, int W, int H, int32_t r2_clear, int min_size,
                                 int Cmax, int32_t* label, int32_t* slot, int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox,
                                 int64_t* csum) {
    if (!frontier_args_ok(ctx, d2, known, G, W, H, min_size, Cmax, ncl, rep, csize)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return fr_launch_frontier(ctx, d2, known, G, W, H, r2_clear, min_size, Cmax, label, slot, ncl, rep, csize, cbox, csum);
}

extern "C" int sc_frontier_cost_matrix(sc_ctx* ctx, const int32_t* g, int F, const int32_t* fgrid, const int32_t* slot, const int32_t* csize,
                                       int G, int W, int H, int Cmax, int32_t gain, int32_t size_cap, int32_t* cost, int32_t* cell) {
    if (!fr_matrix_args_ok(ctx, g, F, fgrid, slot, csize, G, W, H, Cmax, gain, size_cap, cost, cell)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return fr_launch_matrix(ctx, g, F, fgrid, slot, csize, G, W, H, Cmax, gain, size_cap, cost, cell);
}

static bool explore_args_ok(const sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int W, int H, int min_size, int Cmax, const int32_t* g,
                            int F, int32_t gain, int32_t size_cap, const int32_t* goal, const int32_t* gcost) {
    return ctx && d2 && known && g && goal && gcost && fr_dims_ok(W, H) && min_size >= 1 && Cmax >= 1 && Cmax <= SC_ASSIGN_MAX_DIM && F >= 1 &&
           F <= SC_ASSIGN_MAX_DIM && gain >= 0 && size_cap >= 0 && (long long)gain * size_cap <= (1ll << 30);
}

// the arrays of sc_fleet_explore_batch the caller may leave out, in one block of scratch
struct fr_fleet_layout {
    size_t slot, ncl, rep, csize, cost, cell, col_of, info, end;
    fr_fleet_layout(size_t n, int F, int Cmax) {
        size_t o = 0;
        auto take = [&o](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
        slot = take(n * 4); ncl = take(8); rep = take((size_t)Cmax * 4); csize = take((size_t)Cmax * 4);
        cost = take((size_t)F * Cmax * 4); cell = take((size_t)F * Cmax * 4); col_of = take((size_t)F * 4); info = take(32);
        end = o;
    }
};

static int fr_launch_explore(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size, int Cmax,
                             const int32_t* g, int F, int32_t gain, int32_t size_cap, int32_t* label, int32_t* slot, int32_t* ncl, int32_t* rep,
                             int32_t* csize, int32_t* cbox, int64_t* csum, int32_t* cost, int32_t* cell, int32_t* col_of, int32_t* row_of,
                             int64_t* info, int32_t* goal, int32_t* gcost) {
    const size_t n = (size_t)W * H;
    int r = fr_launch_frontier(ctx, d2, known, 1, W, H, r2_clear, min_size, Cmax, label, slot, ncl, rep, csize, cbox, csum);
    if (r == SC_OK) r = fr_launch_matrix(ctx, g, F, nullptr, slot, csize, 1, W, H, Cmax, gain, size_cap, cost, cell);
    if (r == SC_OK) r = sc_assign_batch(ctx, cost, 1, F, Cmax, col_of, row_of, nullptr, nullptr, info);
    if (r != SC_OK) return r;
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    hipLaunchKernelGGL(fr_goal_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, ctx->stream, g, n, F, Cmax, (const int32_t*)cell,
                       (const int32_t*)col_of, goal, gcost);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_fleet_explore_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size,
                                      int Cmax, const int32_t* g, int F, int32_t gain, int32_t size_cap, int32_t* label, int32_t* slot,
                                      int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox, int64_t* csum, int32_t* cost, int32_t* cell,
                                      int32_t* col_of, int32_t* row_of, int64_t* info, int32_t* goal, int32_t* gcost) {
    if (!explore_args_ok(ctx, d2, known, W, H, min_size, Cmax, g, F, gain, size_cap, goal, gcost)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const fr_fleet_layout lay((size_t)W * H, F, Cmax);
    if (!slot || !ncl || !rep || !csize || !cost || !cell || !col_of || !info) {
        int r = sc_scratch_reserve(ctx, &ctx->fr_fleet, lay.end);
        if (r != SC_OK) return r;
    }
    char* base = (char*)ctx->fr_fleet.p;
    if (!slot) slot = (int32_t*)(base + lay.slot);
    if (!ncl) ncl = (int32_t*)(base + lay.ncl);
    if (!rep) rep = (int32_t*)(base + lay.rep);
    if (!csize) csize = (int32_t*)(base + lay.csize);
    if (!cost) cost = (int32_t*)(base + lay.cost);
    if (!cell) cell = (int32_t*)(base + lay.cell);
    if (!col_of) col_of = (int32_t*)(base + lay.col_of);
    if (!info) info = (int64_t*)(base + lay.info);
    return fr_launch_explore(ctx, d2, known, W, H, r2_clear, min_size, Cmax, g, F, gain, size_cap, label, slot, ncl, rep, csize, cbox, csum, cost,
                             cell, col_of, row_of, info, goal, gcost);
}

// ---- host forms ----
extern "C" int sc_known_from_discs_host(sc_ctx* ctx, const uint8_t* base, const int32_t* discs, int R, int W, int H, uint8_t* known) {
    if (!known_args_ok(ctx, discs, R, W, H, known)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    sc_stage st(ctx);
    const int i_b = st.in(base, base ? n : 0), i_d = st.in(discs, (size_t)R * 12);
    const int o_k = st.out(known, n);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_known_from_discs(ctx, base ? st.dev<const uint8_t>(i_b) : nullptr, st.dev<const int32_t>(i_d), R, W, H, st.dev<uint8_t>(o_k));
    return st.finish(r);
}

extern "C" int sc_d2_known_i32_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int G, int W, int H, int32_t* d2k) {
    if (!d2k_args_ok(ctx, d2, known, G, W, H, d2k)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)G * W * H;
    sc_stage st(ctx);
    const int i_d = st.in(d2, cells * 4), i_k = st.in(known, cells);
    const int o_d = st.out(d2k, cells * 4);
    int r = st.upload();
    if (r == SC_OK) r = sc_d2_known_i32(ctx, st.dev<const int32_t>(i_d), st.dev<const uint8_t>(i_k), G, W, H, st.dev<int32_t>(o_d));
    return st.finish(r);
}

extern "C" int sc_frontier_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int G, int W, int H, int32_t r2_clear,
                                      int min_size, int Cmax, int32_t* label, int32_t* slot, int32_t* ncl, int32_t* rep, int32_t* csize,
                                      int32_t* cbox, int64_t* csum) {
    if (!frontier_args_ok(ctx, d2, known, G, W, H, min_size, Cmax, ncl, rep, csize)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)G * W * H, gc = (size_t)G * Cmax;
    sc_stage st(ctx);
    const int i_d = st.in(d2, cells * 4), i_k = st.in(known, cells);
    const int o_l = st.out(label, label ? cells * 4 : 0), o_s = st.out(slot, slot ? cells * 4 : 0), o_n = st.out(ncl, (size_t)G * 8),
              o_r = st.out(rep, gc * 4), o_c = st.out(csize, gc * 4), o_b = st.out(cbox, cbox ? gc * 16 : 0),
              o_m = st.out(csum, csum ? gc * 16 : 0);
    int r = st.upload();
    if (r == SC_OK)
        r = fr_launch_frontier(ctx, st.dev<const int32_t>(i_d), st.dev<const uint8_t>(i_k), G, W, H, r2_clear, min_size, Cmax,
                               label ? st.dev<int32_t>(o_l) : nullptr, slot ? st.dev<int32_t>(o_s) : nullptr, st.dev<int32_t>(o_n),
                               st.dev<int32_t>(o_r), st.dev<int32_t>(o_c), cbox ? st.dev<int32_t>(o_b) : nullptr,
                               csum ? st.dev<int64_t>(o_m) : nullptr);
    return st.finish(r);
}

// what the kernels cannot refuse: a field value below 0 (the contract of g in sc_field_paths_batch)
static bool fr_field_data_invalid(const int32_t* g, size_t cells) {
    for (size_t k = 0; k < cells; ++k)
        if (g[k] < 0) return true;
    return false;
}

extern "C" int sc_frontier_cost_matrix_host(sc_ctx* ctx, const int32_t* g, int F, const int32_t* fgrid, const int32_t* slot,
                                            const int32_t* csize, int G, int W, int H, int Cmax, int32_t gain, int32_t size_cap, int32_t* cost,
                                            int32_t* cell) {
    if (!fr_matrix_args_ok(ctx, g, F, fgrid, slot, csize, G, W, H, Cmax, gain, size_cap, cost, cell)) return SC_ERR_INVALID;
    const size_t n = (size_t)W * H;
    if (fr_field_data_invalid(g, (size_t)F * n)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_g = st.in(g, (size_t)F * n * 4), i_f = st.in(fgrid, fgrid ? (size_t)F * 4 : 0), i_s = st.in(slot, (size_t)G * n * 4),
              i_c = st.in(csize, (size_t)G * Cmax * 4);
    const int o_c = st.out(cost, (size_t)F * Cmax * 4), o_l = st.out(cell, (size_t)F * Cmax * 4);
    int r = st.upload();
    if (r == SC_OK)
        r = fr_launch_matrix(ctx, st.dev<const int32_t>(i_g), F, fgrid ? st.dev<const int32_t>(i_f) : nullptr, st.dev<const int32_t>(i_s),
                             st.dev<const int32_t>(i_c), G, W, H, Cmax, gain, size_cap, st.dev<int32_t>(o_c), st.dev<int32_t>(o_l));
    return st.finish(r);
}

extern "C" int sc_fleet_explore_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size,
                                           int Cmax, const int32_t* g, int F, int32_t gain, int32_t size_cap, int32_t* label, int32_t* slot,
                                           int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox, int64_t* csum, int32_t* cost,
                                           int32_t* cell, int32_t* col_of, int32_t* row_of, int64_t* info, int32_t* goal, int32_t* gcost) {
    if (!explore_args_ok(ctx, d2, known, W, H, min_size, Cmax, g, F, gain, size_cap, goal, gcost)) return SC_ERR_INVALID;
    const size_t n = (size_t)W * H, fc = (size_t)F * Cmax;
    if (fr_field_data_invalid(g, (size_t)F * n)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_d = st.in(d2, n * 4), i_k = st.in(known, n), i_g = st.in(g, (size_t)F * n * 4);
    // a slot for every intermediate array, copied back where the caller keeps it
    const int o_l = st.out(label, label ? n * 4 : 0), o_s = st.out(slot, n * 4), o_n = st.out(ncl, 8), o_r = st.out(rep, (size_t)Cmax * 4),
              o_c = st.out(csize, (size_t)Cmax * 4), o_b = st.out(cbox, cbox ? (size_t)Cmax * 16 : 0),
              o_m = st.out(csum, csum ? (size_t)Cmax * 16 : 0), o_co = st.out(cost, fc * 4), o_ce = st.out(cell, fc * 4),
              o_q = st.out(col_of, (size_t)F * 4), o_ro = st.out(row_of, row_of ? (size_t)Cmax * 4 : 0), o_i = st.out(info, 32),
              o_go = st.out(goal, (size_t)F * 4), o_gc = st.out(gcost, (size_t)F * 4);
    int r = st.upload();
    if (r == SC_OK)
        r = fr_launch_explore(ctx, st.dev<const int32_t>(i_d), st.dev<const uint8_t>(i_k), W, H, r2_clear, min_size, Cmax,
                              st.dev<const int32_t>(i_g), F, gain, size_cap, label ? st.dev<int32_t>(o_l) : nullptr, st.dev<int32_t>(o_s),
                              st.dev<int32_t>(o_n), st.dev<int32_t>(o_r), st.dev<int32_t>(o_c), cbox ? st.dev<int32_t>(o_b) : nullptr,
                              csum ? st.dev<int64_t>(o_m) : nullptr, st.dev<int32_t>(o_co), st.dev<int32_t>(o_ce), st.dev<int32_t>(o_q),
                              row_of ? st.dev<int32_t>(o_ro) : nullptr, st.dev<int64_t>(o_i), st.dev<int32_t>(o_go), st.dev<int32_t>(o_gc));
    return st.finish(r);
}
