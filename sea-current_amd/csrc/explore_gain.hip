// explore_gain.hip -- coordinated exploration goals: greedy (robot, candidate) picks by what each view reveals
// (sc_explore_gain_batch), a central cell per frontier cluster (sc_frontier_centres) and the chain frontiers -> centres ->
// picks on one stream (sc_fleet_explore_gain_batch).  DESIGN.md section 29; the definitions are in include/sea_current_hip.h.
//
// Definition.  kw = known.  Round t: among the free robots r and the alive, untaken candidates n with g[r][cand[n]] finite and
// gain[n] >= min_gain, take the pair of largest wg * gain[n] - wc * g[r][cand[n]] (int64; ties: smallest r, then smallest n),
// record it, apply its view to kw (sc_known_from_views / sc_known_from_sectors of that one row) and recompute every gain.
//
// Kernels.  The call enqueues min(rounds, R, N) rounds sized on the host; nothing is read back in between.
//   before the rounds: sc_views_from_cells, then sc_view_gain_batch or sc_view_gain_headings_batch (their launchers) give the
//     gains against kw; eg_cost_kernel gathers cost[r][n] = g[r][cand[n]] (SC_FIELD_INF for a dead candidate) once.
//   1. eg_sel1_kernel / eg_sel2_kernel: a two-stage reduction over the R * N pairs on the key (score, r, n), a total order, so
//      the pick does not depend on the order of execution.  Stage two writes the pick's outputs, marks robot and candidate,
//      and stores the chosen sector row (cx, cy, r2, a, b) in the state words; with no eligible pair it sets the done word,
//      and every kernel of the later rounds leaves on reading it.
//   2. eg_view_kernel: sectors.hip's ray kernel for the row in the state words; writes vis_new.
//   3. eg_delta_kernel: grid (tiles of the chosen box, candidates).  A candidate that is dead, or whose box does not meet the
//      chosen box, leaves at once; a tile outside the candidate's box is skipped.  A lane takes a cell c with vis_new[c] and
//      kw[c] == 0 inside the candidate's disc and walks the ray from the candidate to c (views_common.h); the wave subtracts
//      its count from gain[n] (one integer atomicSub), or with a table from hist[n][bin] and c0[n] through the workgroup's LDS
//      histogram, as vs_hist_kernel adds.  vis_n depends on occ only, so this is the whole change of gain[n]: the newly known
//      cells of surf are occupied and nobody's gain.
//   4. eg_best_kernel (table only): one wave per candidate re-derives (max window sum, smallest heading) from hist and c0.
//   5. eg_combine_kernel: kw |= vis_new | surf, one thread per cell, and clears the vis buffer of the next round (two buffers
//      take turns, so no round starts with a memset).
// No workgroup waits for another; integer atomics only; every loop is bounded by the data's size.
#include "sectors_common.h"

namespace {

enum { EG_DONE = 0, EG_NPICK = 1, EG_ROW = 2, EG_WORDS = 16 };   // state words: done, picks so far, the chosen row [7]
constexpr int EG_PARTS = 256;                                    // workgroups of stage one at most

struct eg_part {
    long long score;
    int r, n;   // r < 0: no eligible pair
};

// a precedes b: larger score, then smaller r, then smaller n; "none" comes last
__device__ __forceinline__ bool eg_before(const eg_part& a, const eg_part& b) {
    if (a.r < 0) return false;
    if (b.r < 0) return true;
    if (a.score != b.score) return a.score > b.score;
    if (a.r != b.r) return a.r < b.r;
    return a.n < b.n;
}

// the first of the workgroup's 256 entries, in every thread
__device__ __forceinline__ eg_part eg_block_first(eg_part p, eg_part* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        eg_part o;
        o.score = __shfl_xor(p.score, off);
        o.r = __shfl_xor(p.r, off);
        o.n = __shfl_xor(p.n, off);
        if (eg_before(o, p)) p = o;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = p;
    __syncthreads();
    p = lds[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (eg_before(lds[w], p)) p = lds[w];
    return p;
}

__global__ __launch_bounds__(256) void eg_init_kernel(int32_t* __restrict__ st, int R, int N, int32_t* goal, int32_t* gcost, int32_t* ggain,
                                                      int32_t* head, int32_t* cand_of, int32_t* pick, int32_t* __restrict__ assigned,
                                                      int32_t* __restrict__ taken) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < EG_WORDS) st[i] = i == EG_ROW + 2 ? -1 : 0;   // the row is an ignored view until a pick stores one
    if (i < R) {
        goal[i] = -1;
        gcost[i] = -1;
        if (ggain) ggain[i] = 0;
        if (head) head[i] = -1;
        if (cand_of) cand_of[i] = -1;
        if (pick) pick[i] = -1;
        assigned[i] = 0;
    }
    if (i < N) taken[i] = 0;
}

__global__ __launch_bounds__(256) void eg_cost_kernel(const uint8_t* __restrict__ occ, const int32_t* __restrict__ g, const int32_t* __restrict__ cand,
                                                      int R, int N, int cells, int32_t* __restrict__ cost) {
    const size_t pairs = (size_t)R * N;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < pairs; p += (size_t)gridDim.x * 256) {
        const int r = (int)(p / N), n = (int)(p - (size_t)r * N);
        const int c = cand[n];
        const bool alive = c >= 0 && c < cells && occ[c] == 0;
        cost[p] = alive ? g[(size_t)r * cells + c] : SC_FIELD_INF;
    }
}

struct eg_sel_args {
    const int32_t* cost;   // [R][N]
    const int32_t* gain;   // gain of candidate n at gain[n * gs]
    int gs, R, N;
    int32_t wg, wc, min_gain;
    int32_t *assigned, *taken;
};

__global__ __launch_bounds__(256) void eg_sel1_kernel(const int32_t* __restrict__ st, const eg_sel_args a, eg_part* __restrict__ part) {
    __shared__ eg_part lds[4];
    if (st[EG_DONE]) return;
    eg_part best{0, -1, -1};
    const size_t pairs = (size_t)a.R * a.N;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < pairs; p += (size_t)gridDim.x * 256) {
        const int32_t c = a.cost[p];
        if (c == SC_FIELD_INF) continue;
        const int r = (int)(p / a.N), n = (int)(p - (size_t)r * a.N);
        if (a.assigned[r] || a.taken[n]) continue;
        const int32_t gn = a.gain[(size_t)n * a.gs];
        if (gn < a.min_gain) continue;
        const eg_part q{(long long)a.wg * gn - (long long)a.wc * c, r, n};
        if (eg_before(q, best)) best = q;
    }
    best = eg_block_first(best, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = best;
}

struct eg_pick_args {
    const int32_t* cand;
    const int32_t* head_of;   // heading of candidate n at head_of[2 n + 1]; NULL: the full circle
    int W, B, span;
    int32_t r2;
    int32_t *goal, *gcost, *ggain, *head, *cand_of, *pick;
};

__global__ __launch_bounds__(256) void eg_sel2_kernel(int32_t* __restrict__ st, const eg_part* __restrict__ part, int P, int t, const eg_sel_args a,
                                                      const eg_pick_args o, const vs_dirs dirs) {
    __shared__ eg_part lds[4];
    if (st[EG_DONE]) return;
    eg_part best{0, -1, -1};
    for (int i = threadIdx.x; i < P; i += 256)
        if (eg_before(part[i], best)) best = part[i];
    best = eg_block_first(best, lds);
    if (threadIdx.x != 0) return;
    if (best.r < 0) {
        st[EG_DONE] = 1;
        st[EG_ROW + 2] = -1;
        return;
    }
    const int r = best.r, n = best.n, c = o.cand[n];
    const int h = o.head_of ? o.head_of[2 * (size_t)n + 1] : -1;
    o.goal[r] = c;
    o.gcost[r] = a.cost[(size_t)r * a.N + n];
    if (o.ggain) o.ggain[r] = a.gain[(size_t)n * a.gs];
    if (o.head) o.head[r] = h;
    if (o.cand_of) o.cand_of[r] = n;
    if (o.pick) o.pick[r] = t;
    a.assigned[r] = 1;
    a.taken[n] = 1;
    st[EG_NPICK] = t + 1;
    const int h1 = h < 0 ? 0 : (h + o.span) % o.B;
    st[EG_ROW] = c % o.W;
    st[EG_ROW + 1] = c / o.W;
    st[EG_ROW + 2] = o.r2;
    st[EG_ROW + 3] = h < 0 ? 0 : dirs.u[h][0];
    st[EG_ROW + 4] = h < 0 ? 0 : dirs.u[h][1];
    st[EG_ROW + 5] = h < 0 ? 0 : dirs.u[h1][0];
    st[EG_ROW + 6] = h < 0 ? 0 : dirs.u[h1][1];
}

__global__ __launch_bounds__(256) void eg_view_kernel(const int32_t* __restrict__ st, const uint8_t* __restrict__ occ, int W, int H,
                                                      uint8_t* __restrict__ vis) {
    if (st[EG_DONE]) return;
    const int32_t* row = st + EG_ROW;
    const vs_sector s = vs_load(row, 0);
    const vw_box b = vs_view_box(occ, row, 0, s, W, H);
    const int cells = W * H;
    for (int t = blockIdx.x; t < b.ntiles; t += gridDim.x) {
        if (vs_skip(b, s, t)) continue;
        int x, y;
        const int c = vw_target(b, t, W, H, x, y);
        if (c >= 0 && vs_in(s, x - b.cx, y - b.cy) && vw_clear(occ, W, cells, b, x, y)) vis[c] = 1;
    }
}

// the gains' change by the chosen view: candidate blockIdx.y of this launch against the cells vis_new newly marks
template <bool TABLE>
__global__ __launch_bounds__(256) void eg_delta_kernel(const int32_t* __restrict__ st, const uint8_t* __restrict__ occ, const uint8_t* __restrict__ kw,
                                                       const uint8_t* __restrict__ vis, const int32_t* __restrict__ views, int W, int H,
                                                       int32_t* __restrict__ gain, const vs_dirs dirs, int B, int32_t* __restrict__ hist,
                                                       int32_t* __restrict__ c0) {
    __shared__ int2 u[SC_VIEW_MAX_BINS];
    __shared__ int lh[SC_VIEW_MAX_BINS];
    if (st[EG_DONE]) return;
    const int32_t* row = st + EG_ROW;
    const vs_sector s = vs_load(row, 0);
    const vw_box cb = vs_view_box(occ, row, 0, s, W, H);
    const int n = blockIdx.y;
    const vw_box b = vw_view_box(occ, views, n, W, H);
    if (cb.ntiles == 0 || b.ntiles == 0) return;   // a dead candidate
    // both boxes span centre -+ floor(sqrt(r2)), clipped to the grid
    const int rc = vw_isqrt(cb.r2), rn = vw_isqrt(b.r2);
    const int cx1 = min(cb.cx + rc, W - 1), cy1 = min(cb.cy + rc, H - 1), bx1 = min(b.cx + rn, W - 1), by1 = min(b.cy + rn, H - 1);
    if (b.x0 > cx1 || bx1 < cb.x0 || b.y0 > cy1 || by1 < cb.y0) return;   // the boxes do not meet
    if (TABLE) {
        if (threadIdx.x < SC_VIEW_MAX_BINS) {
            lh[threadIdx.x] = 0;
            if ((int)threadIdx.x < B) u[threadIdx.x] = make_int2(dirs.u[threadIdx.x][0], dirs.u[threadIdx.x][1]);
        }
        __syncthreads();
    }
    const int cells = W * H;
    const int lane = threadIdx.x & 63;
    int cnt = 0;   // uniform across the wave
    for (int t = blockIdx.x; t < cb.ntiles; t += gridDim.x) {
        const int tx0 = cb.x0 + (t % cb.tx) * VW_TILE, ty0 = cb.y0 + (t / cb.tx) * VW_TILE;
        if (tx0 > bx1 || tx0 + VW_TILE - 1 < b.x0 || ty0 > by1 || ty0 + VW_TILE - 1 < b.y0) continue;   // outside the candidate's box
        if (vs_skip(cb, s, t)) continue;
        int x, y;
        const int c = vw_target(cb, t, W, H, x, y);
        const int dx = x - b.cx, dy = y - b.cy;
        const bool hit = c >= 0 && vis[c] != 0 && kw[c] == 0 && (long long)dx * dx + (long long)dy * dy <= b.r2 && vw_clear(occ, W, cells, b, x, y);
        if (!TABLE) {
            cnt += __popcll(__ballot(hit));
        } else {
            const bool centre = dx == 0 && dy == 0;
            if (hit && centre) atomicSub(c0 + n, 1);
            int lo = 0;
            if (hit && !centre) {   // d lies in one of the bins lo .. lo + k - 1; lo + k <= B throughout
                for (int k = B; k > 1;) {
                    const int j = k >> 1;
                    if (vs_in_cone(u[lo], u[lo + j], dx, dy)) k = j;
                    else { lo += j; k -= j; }
                }
            }
            unsigned long long left = __ballot(hit && !centre);
            while (left) {   // uniform across the wave
                const int bin = __shfl(lo, __ffsll((long long)left) - 1);
                const unsigned long long same = left & __ballot(lo == bin);
                if (lane == 0) atomicAdd(&lh[bin], __popcll(same));
                left &= ~same;
            }
        }
    }
    if (!TABLE) {
        if (lane == 0 && cnt) atomicSub(gain + n, cnt);
    } else {
        __syncthreads();
        if ((int)threadIdx.x < B && lh[threadIdx.x]) atomicSub(hist + (size_t)n * B + threadIdx.x, lh[threadIdx.x]);
    }
}

// one wave per candidate, four candidates per workgroup: best[n] = (the largest window sum, the smallest heading attaining it)
__global__ __launch_bounds__(256) void eg_best_kernel(const int32_t* __restrict__ st, const int32_t* __restrict__ hist, const int32_t* __restrict__ c0,
                                                      int N, int B, int span, int32_t* __restrict__ best) {
    __shared__ int row[4][SC_VIEW_MAX_BINS];
    if (st[EG_DONE]) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    if (i >= N) return;   // a whole wave; no workgroup barrier below
    if (lane < B) row[wv][lane] = hist[(size_t)i * B + lane];
    wave_lds_sync();
    int g = -1, h = lane;
    if (lane < B) {
        g = c0[i];
        int k = lane;
        for (int j = 0; j < span; ++j) {
            g += row[wv][k];
            k = k + 1 == B ? 0 : k + 1;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int og = __shfl_xor(g, off), oh = __shfl_xor(h, off);
        if (og > g || (og == g && oh < h)) { g = og; h = oh; }
    }
    if (lane == 0) {
        best[2 * (size_t)i] = g;
        best[2 * (size_t)i + 1] = h;
    }
}

// kw = kw | vis | surf of its own cell; clears the other vis buffer for the next round
__global__ __launch_bounds__(256) void eg_combine_kernel(const int32_t* __restrict__ st, const uint8_t* __restrict__ occ, const uint8_t* __restrict__ vis,
                                                         uint8_t* __restrict__ vis_next, int W, int H, uint8_t* __restrict__ kw) {
    if (st[EG_DONE]) return;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (size_t)W * H) return;
    const int x = (int)(c % W), y = (int)(c / W);
    bool k = kw[c] != 0 || vis[c] != 0;
    if (!k && occ[c] != 0)
        k = (x > 0 && vis[c - 1]) || (x + 1 < W && vis[c + 1]) || (y > 0 && vis[c - W]) || (y + 1 < H && vis[c + W]);
    kw[c] = k ? 1 : 0;
    vis_next[c] = 0;
}

// dst[n] = gain of candidate n (dst may be NULL); npick[0] = the picks so far (npick may be NULL)
__global__ __launch_bounds__(256) void eg_out_kernel(const int32_t* __restrict__ st, const int32_t* __restrict__ gain, int gs, int N,
                                                     int32_t* __restrict__ dst, int32_t* __restrict__ npick) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (dst && i < N) dst[i] = gain[(size_t)i * gs];
    if (npick && i == 0) npick[0] = st[EG_NPICK];
}

// ---- sc_frontier_centres ----
struct fc_args {
    const int32_t *slot, *csize;
    const int64_t* csum;
    int G, W, Cmax;
    size_t n;
    unsigned long long* key;
    int32_t* centre;
};

// pass 0: the smallest key of every cluster; pass 1: the smallest cell among those attaining it
template <int PASS>
__global__ __launch_bounds__(256) void fc_min_kernel(const fc_args a) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.n) return;
    const long long x = (long long)(c % a.W), y = (long long)(c / a.W);
    for (int g = blockIdx.y; g < a.G; g += gridDim.y) {
        const int k = a.slot[(size_t)g * a.n + c];
        if (k < 0 || k >= a.Cmax) continue;
        const size_t i = (size_t)g * a.Cmax + k;
        const long long s = a.csize[i], ex = s * x - a.csum[2 * i], ey = s * y - a.csum[2 * i + 1];
        const unsigned long long key = (unsigned long long)((ex < 0 ? -ex : ex) + (ey < 0 ? -ey : ey));
        if (PASS == 0) atomicMin(a.key + i, key);
        else if (a.key[i] == key) atomicMin(a.centre + i, (int32_t)c);
    }
}

__global__ __launch_bounds__(256) void fc_fix_kernel(int32_t* __restrict__ centre, size_t rows, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < rows && (centre[i] < 0 || (size_t)centre[i] >= n)) centre[i] = -1;
}

}  // namespace

// ---- argument checks ----
// everything but the candidates' pointer, which the chain makes itself
static bool eg_args_ok(const sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* g, int R, int N, int W, int H, int32_t r2,
                       const int32_t* dirs, int B, int span, int32_t wg, int32_t wc, int32_t min_gain, int rounds, const int32_t* goal,
                       const int32_t* gcost, const int32_t* npick, const uint8_t* known_out) {
    return ctx && occ && known && g && goal && gcost && npick && vw_dims_ok(W, H) && R >= 1 && R <= SC_ASSIGN_MAX_DIM && N >= 0 &&
           N <= SC_FRONTIER_MAX_CLUSTERS && (long long)R * N <= (1ll << 26) && r2 >= 0 && wg >= 0 && wg <= (1 << 20) &&
           wc >= 0 && wc <= (1 << 20) && min_gain >= 0 && rounds >= 0 && rounds <= SC_ASSIGN_MAX_DIM &&
           (!dirs || (vs_dirs_ok(dirs, B) && span >= 1 && span < B)) && known_out != occ;
}

static bool fc_args_ok(const sc_ctx* ctx, const int32_t* slot, const int32_t* csize, const int64_t* csum, int G, int W, int H, int Cmax,
                       const int32_t* centre) {
    return ctx && slot && csize && csum && centre && G > 0 && vw_dims_ok(W, H) && Cmax >= 1 && Cmax <= SC_FRONTIER_MAX_CLUSTERS;
}

static bool eg_fleet_args_ok(const sc_ctx* ctx, const int32_t* d2, int min_size, int Cmax) {
    return ctx && d2 && min_size >= 1 && Cmax >= 1 && Cmax <= SC_FRONTIER_MAX_CLUSTERS;
}

// what the kernels cannot refuse: a field value below 0 (the contract of g in sc_field_paths_batch)
static bool eg_field_data_invalid(const int32_t* g, size_t cells) {
    for (size_t k = 0; k < cells; ++k)
        if (g[k] < 0) return true;
    return false;
}

// the scratch of one sc_explore_gain_batch call
struct eg_layout {
    size_t st, kw, vis, views, best, hist, c0, assigned, taken, cost, part, end;
    eg_layout(size_t n, int R, int N, int B, bool own_kw) {
        size_t o = 0;
        auto take = [&o](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
        st = take(EG_WORDS * 4); kw = take(own_kw ? n : 0); vis = take(2 * al256(n)); views = take((size_t)N * 12); best = take((size_t)N * 8);
        hist = take((size_t)N * B * 4); c0 = take((size_t)N * 4); assigned = take((size_t)R * 4); taken = take((size_t)N * 4);
        cost = take((size_t)R * N * 4); part = take(EG_PARTS * sizeof(eg_part));
        end = o;
    }
};

// an upper bound of the tiles of a view's clipped box at this radius, VW_SLOTS at most: the workgroups of the view launch
static unsigned eg_view_slots(int W, int H, int32_t r2) {
    const long long side = 2 * ((long long)sqrt((double)r2) + 1) / VW_TILE + 2;
    const long long tiles = side * side, grid = vw_slots(W, H, VW_SLOTS);
    return (unsigned)(tiles < grid ? tiles : grid);
}

// workgroups per candidate of the delta launch: about 32768 in all (most leave at once: few boxes meet the chosen one), 64 per
// candidate at most
static unsigned eg_delta_slots(int W, int H, int32_t r2, int N) {
    const unsigned tiles = eg_view_slots(W, H, r2), per = 32768 / N < 1 ? 1 : (32768 / N > 64 ? 64 : 32768 / N);
    return tiles < per ? tiles : per;
}

extern "C" int sc_explore_gain_batch(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* g, int R, const int32_t* cand, int N,
                                     int W, int H, int32_t r2, const int32_t* dirs, int B, int span, int32_t wg, int32_t wc, int32_t min_gain,
                                     int rounds, int32_t* goal, int32_t* gcost, int32_t* ggain, int32_t* head, int32_t* cand_of, int32_t* pick,
                                     int32_t* npick, int32_t* gain0, int32_t* gain_end, uint8_t* known_out) {
    if (!(cand || N == 0) || !eg_args_ok(ctx, occ, known, g, R, N, W, H, r2, dirs, B, span, wg, wc, min_gain, rounds, goal, gcost, npick, known_out))
        return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const bool table = dirs != nullptr;
    if (!table) B = span = 0;
    const size_t n = (size_t)W * H;
    const eg_layout lay(n, R, N, B, known_out == nullptr);
    int r = sc_scratch_reserve(ctx, &ctx->eg_state, lay.end);
    if (r != SC_OK) return r;
    char* base = (char*)ctx->eg_state.p;
    int32_t* st = (int32_t*)(base + lay.st);
    uint8_t* kw = known_out ? known_out : (uint8_t*)(base + lay.kw);
    uint8_t* vis[2] = {(uint8_t*)(base + lay.vis), (uint8_t*)(base + lay.vis) + al256(n)};
    int32_t* views = (int32_t*)(base + lay.views);
    int32_t* best = (int32_t*)(base + lay.best);   // the full circle: gain [N]
    int32_t* hist = (int32_t*)(base + lay.hist);
    int32_t* c0 = (int32_t*)(base + lay.c0);
    int32_t* assigned = (int32_t*)(base + lay.assigned);
    int32_t* taken = (int32_t*)(base + lay.taken);
    int32_t* cost = (int32_t*)(base + lay.cost);
    eg_part* part = (eg_part*)(base + lay.part);
    const int gs = table ? 2 : 1;
    const int most = R > N ? R : N;

    int tk = sc_time_begin(ctx, SC_K_MOVES);
    hipLaunchKernelGGL(eg_init_kernel, dim3((unsigned)(((most > EG_WORDS ? most : EG_WORDS) + 255) / 256)), dim3(256), 0, ctx->stream, st, R, N, goal,
                       gcost, ggain, head, cand_of, pick, assigned, taken);
    if (kw != known) SC_HIP(ctx, hipMemcpyAsync(kw, known, n, hipMemcpyDeviceToDevice, ctx->stream));
    sc_time_end(ctx, tk);
    if (N == 0) {
        tk = sc_time_begin(ctx, SC_K_MOVES);
        hipLaunchKernelGGL(eg_out_kernel, dim3(1), dim3(256), 0, ctx->stream, (const int32_t*)st, (const int32_t*)best, gs, 0, (int32_t*)nullptr, npick);
        sc_time_end(ctx, tk);
        SC_HIP(ctx, hipGetLastError());
        return SC_OK;
    }
    // the gains against kw: the view calls' own kernels
    r = sc_views_from_cells(ctx, cand, N, W, H, r2, views);
    if (r == SC_OK && !table) r = sc_view_gain_batch(ctx, occ, kw, views, N, W, H, best);
    if (r == SC_OK && table) r = sc_view_gain_headings_batch(ctx, occ, kw, views, N, W, H, dirs, B, span, hist, nullptr, best);
    if (r != SC_OK) return r;
    vs_dirs tab;
    memset(&tab, 0, sizeof tab);
    if (table) memcpy(tab.u, dirs, (size_t)B * 8);
    const int fewest = R < N ? R : N, T = rounds < fewest ? rounds : fewest;
    const size_t pairs = (size_t)R * N;
    const unsigned P = (unsigned)((pairs + 255) / 256 < EG_PARTS ? (pairs + 255) / 256 : EG_PARTS);
    const unsigned nblk = (unsigned)((N + 255) / 256), cblk = (unsigned)((n + 255) / 256);
    const eg_sel_args sa{cost, best, gs, R, N, wg, wc, min_gain, assigned, taken};
    const eg_pick_args pa{cand, table ? best : nullptr, W, table ? B : 1, span, r2, goal, gcost, ggain, head, cand_of, pick};
    const unsigned dslots = eg_delta_slots(W, H, r2, N), vslots = eg_view_slots(W, H, r2);

    tk = sc_time_begin(ctx, SC_K_MOVES);
    // c0 of the headings call lies at the start of its scratch (sc_internal.h: vs_state)
    if (table) SC_HIP(ctx, hipMemcpyAsync(c0, ctx->vs_state.p, (size_t)N * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (T > 0) SC_HIP(ctx, hipMemsetAsync(vis[0], 0, 2 * al256(n), ctx->stream));
    hipLaunchKernelGGL(eg_cost_kernel, dim3((unsigned)((pairs + 255) / 256 < 4096 ? (pairs + 255) / 256 : 4096)), dim3(256), 0, ctx->stream, occ, g,
                       cand, R, N, (int)n, cost);
    hipLaunchKernelGGL(eg_out_kernel, dim3(nblk), dim3(256), 0, ctx->stream, (const int32_t*)st, (const int32_t*)best, gs, N, gain0, (int32_t*)nullptr);
    for (int t = 0; t < T; ++t) {
        uint8_t* v = vis[t & 1];
        hipLaunchKernelGGL(eg_sel1_kernel, dim3(P), dim3(256), 0, ctx->stream, (const int32_t*)st, sa, part);
        hipLaunchKernelGGL(eg_sel2_kernel, dim3(1), dim3(256), 0, ctx->stream, st, (const eg_part*)part, (int)P, t, sa, pa, tab);
        if (t == T - 1 && !gain_end && !known_out) break;   // nobody reads what the last pick's view changes
        hipLaunchKernelGGL(eg_view_kernel, dim3(vslots), dim3(256), 0, ctx->stream, (const int32_t*)st, occ, W, H, v);
        for (int v0 = 0; v0 < N; v0 += 65535) {   // gridDim.y <= 65535
            const int nv = N - v0 < 65535 ? N - v0 : 65535;
            if (table)
                hipLaunchKernelGGL(eg_delta_kernel<true>, dim3(dslots, (unsigned)nv), dim3(256), 0, ctx->stream, (const int32_t*)st, occ,
                                   (const uint8_t*)kw, (const uint8_t*)v, (const int32_t*)views + 3 * (size_t)v0, W, H, (int32_t*)nullptr, tab, B,
                                   hist + (size_t)v0 * B, c0 + v0);
            else
                hipLaunchKernelGGL(eg_delta_kernel<false>, dim3(dslots, (unsigned)nv), dim3(256), 0, ctx->stream, (const int32_t*)st, occ,
                                   (const uint8_t*)kw, (const uint8_t*)v, (const int32_t*)views + 3 * (size_t)v0, W, H, best + v0, tab, 0,
                                   (int32_t*)nullptr, (int32_t*)nullptr);
        }
        if (table)
            hipLaunchKernelGGL(eg_best_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, (const int32_t*)st, (const int32_t*)hist,
                               (const int32_t*)c0, N, B, span, best);
        hipLaunchKernelGGL(eg_combine_kernel, dim3(cblk), dim3(256), 0, ctx->stream, (const int32_t*)st, occ, (const uint8_t*)v, vis[(t + 1) & 1], W, H,
                           kw);
    }
    hipLaunchKernelGGL(eg_out_kernel, dim3(nblk), dim3(256), 0, ctx->stream, (const int32_t*)st, (const int32_t*)best, gs, N, gain_end, npick);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_frontier_centres(sc_ctx* ctx, const int32_t* slot, const int32_t* csize, const int64_t* csum, int G, int W, int H, int Cmax,
                                   int32_t* centre) {
    if (!fc_args_ok(ctx, slot, csize, csum, G, W, H, Cmax, centre)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H, rows = (size_t)G * Cmax;
    int r = sc_scratch_reserve(ctx, &ctx->eg_centre, al256(rows * 8));
    if (r != SC_OK) return r;
    const fc_args a{slot, csize, csum, G, W, Cmax, n, (unsigned long long*)ctx->eg_centre.p, centre};
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)(G < 65535 ? G : 65535));
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    SC_HIP(ctx, hipMemsetAsync(a.key, 0xFF, rows * 8, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(centre, 0x7F, rows * 4, ctx->stream));   // above every cell: W * H <= 2^26
    hipLaunchKernelGGL(fc_min_kernel<0>, grid, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(fc_min_kernel<1>, grid, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(fc_fix_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, centre, rows, n);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// the arrays of sc_fleet_explore_gain_batch the caller may leave out, in one block of scratch
struct eg_fleet_layout {
    size_t slot, ncl, rep, csize, csum, centre, end;
    eg_fleet_layout(size_t n, int Cmax) {
        size_t o = 0;
        auto take = [&o](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
        slot = take(n * 4); ncl = take(8); rep = take((size_t)Cmax * 4); csize = take((size_t)Cmax * 4); csum = take((size_t)Cmax * 16);
        centre = take((size_t)Cmax * 4);
        end = o;
    }
};

static int eg_launch_fleet(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size, int Cmax,
                           const uint8_t* occ, const int32_t* g, int R, int32_t r2, const int32_t* dirs, int B, int span, int32_t wg, int32_t wc,
                           int32_t min_gain, int rounds, int32_t* label, int32_t* slot, int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox,
                           int64_t* csum, int32_t* centre, int32_t* goal, int32_t* gcost, int32_t* ggain, int32_t* head, int32_t* cand_of,
                           int32_t* pick, int32_t* npick, int32_t* gain0, int32_t* gain_end, uint8_t* known_out) {
    int r = sc_frontier_batch(ctx, d2, known, 1, W, H, r2_clear, min_size, Cmax, label, slot, ncl, rep, csize, cbox, csum);
    if (r == SC_OK) r = sc_frontier_centres(ctx, slot, csize, csum, 1, W, H, Cmax, centre);
    if (r == SC_OK)
        r = sc_explore_gain_batch(ctx, occ, known, g, R, centre, Cmax, W, H, r2, dirs, B, span, wg, wc, min_gain, rounds, goal, gcost, ggain, head,
                                  cand_of, pick, npick, gain0, gain_end, known_out);
    return r;
}

extern "C" int sc_fleet_explore_gain_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size,
                                           int Cmax, const uint8_t* occ, const int32_t* g, int R, int32_t r2, const int32_t* dirs, int B, int span,
                                           int32_t wg, int32_t wc, int32_t min_gain, int rounds, int32_t* label, int32_t* slot, int32_t* ncl,
                                           int32_t* rep, int32_t* csize, int32_t* cbox, int64_t* csum, int32_t* centre, int32_t* goal,
                                           int32_t* gcost, int32_t* ggain, int32_t* head, int32_t* cand_of, int32_t* pick, int32_t* npick,
                                           int32_t* gain0, int32_t* gain_end, uint8_t* known_out) {
    if (!eg_fleet_args_ok(ctx, d2, min_size, Cmax) ||
        !eg_args_ok(ctx, occ, known, g, R, Cmax, W, H, r2, dirs, B, span, wg, wc, min_gain, rounds, goal, gcost, npick, known_out))
        return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const eg_fleet_layout lay((size_t)W * H, Cmax);
    if (!slot || !ncl || !rep || !csize || !csum || !centre) {
        int r = sc_scratch_reserve(ctx, &ctx->eg_fleet, lay.end);
        if (r != SC_OK) return r;
    }
    char* base = (char*)ctx->eg_fleet.p;
    if (!slot) slot = (int32_t*)(base + lay.slot);
    if (!ncl) ncl = (int32_t*)(base + lay.ncl);
    if (!rep) rep = (int32_t*)(base + lay.rep);
    if (!csize) csize = (int32_t*)(base + lay.csize);
    if (!csum) csum = (int64_t*)(base + lay.csum);
    if (!centre) centre = (int32_t*)(base + lay.centre);
    return eg_launch_fleet(ctx, d2, known, W, H, r2_clear, min_size, Cmax, occ, g, R, r2, dirs, B, span, wg, wc, min_gain, rounds, label, slot, ncl,
                           rep, csize, cbox, csum, centre, goal, gcost, ggain, head, cand_of, pick, npick, gain0, gain_end, known_out);
}

// ---- host forms ----
extern "C" int sc_explore_gain_batch_host(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* g, int R, const int32_t* cand,
                                          int N, int W, int H, int32_t r2, const int32_t* dirs, int B, int span, int32_t wg, int32_t wc,
                                          int32_t min_gain, int rounds, int32_t* goal, int32_t* gcost, int32_t* ggain, int32_t* head,
                                          int32_t* cand_of, int32_t* pick, int32_t* npick, int32_t* gain0, int32_t* gain_end, uint8_t* known_out) {
    if (!(cand || N == 0) || !eg_args_ok(ctx, occ, known, g, R, N, W, H, r2, dirs, B, span, wg, wc, min_gain, rounds, goal, gcost, npick, known_out))
        return SC_ERR_INVALID;
    const size_t n = (size_t)W * H;
    if (eg_field_data_invalid(g, (size_t)R * n)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_o = st.in(occ, n), i_k = st.in(known, n), i_g = st.in(g, (size_t)R * n * 4), i_c = st.in(cand, (size_t)N * 4);
    const size_t rb = (size_t)R * 4, nb = (size_t)N * 4;
    const int o_go = st.out(goal, rb), o_gc = st.out(gcost, rb), o_gg = st.out(ggain, ggain ? rb : 0), o_h = st.out(head, head ? rb : 0),
              o_co = st.out(cand_of, cand_of ? rb : 0), o_p = st.out(pick, pick ? rb : 0), o_n = st.out(npick, 4),
              o_g0 = st.out(gain0, gain0 ? nb : 0), o_ge = st.out(gain_end, gain_end ? nb : 0), o_k = st.out(known_out, known_out ? n : 0);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_explore_gain_batch(ctx, st.dev<const uint8_t>(i_o), st.dev<const uint8_t>(i_k), st.dev<const int32_t>(i_g), R,
                                  st.dev<const int32_t>(i_c), N, W, H, r2, dirs, B, span, wg, wc, min_gain, rounds, st.dev<int32_t>(o_go),
                                  st.dev<int32_t>(o_gc), ggain ? st.dev<int32_t>(o_gg) : nullptr, head ? st.dev<int32_t>(o_h) : nullptr,
                                  cand_of ? st.dev<int32_t>(o_co) : nullptr, pick ? st.dev<int32_t>(o_p) : nullptr, st.dev<int32_t>(o_n),
                                  gain0 ? st.dev<int32_t>(o_g0) : nullptr, gain_end ? st.dev<int32_t>(o_ge) : nullptr,
                                  known_out ? st.dev<uint8_t>(o_k) : nullptr);
    return st.finish(r);
}

extern "C" int sc_frontier_centres_host(sc_ctx* ctx, const int32_t* slot, const int32_t* csize, const int64_t* csum, int G, int W, int H, int Cmax,
                                        int32_t* centre) {
    if (!fc_args_ok(ctx, slot, csize, csum, G, W, H, Cmax, centre)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)G * W * H, gc = (size_t)G * Cmax;
    sc_stage st(ctx);
    const int i_s = st.in(slot, cells * 4), i_c = st.in(csize, gc * 4), i_m = st.in(csum, gc * 16);
    const int o_c = st.out(centre, gc * 4);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_frontier_centres(ctx, st.dev<const int32_t>(i_s), st.dev<const int32_t>(i_c), st.dev<const int64_t>(i_m), G, W, H, Cmax,
                                st.dev<int32_t>(o_c));
    return st.finish(r);
}

extern "C" int sc_fleet_explore_gain_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size,
                                                int Cmax, const uint8_t* occ, const int32_t* g, int R, int32_t r2, const int32_t* dirs, int B,
                                                int span, int32_t wg, int32_t wc, int32_t min_gain, int rounds, int32_t* label, int32_t* slot,
                                                int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox, int64_t* csum, int32_t* centre,
                                                int32_t* goal, int32_t* gcost, int32_t* ggain, int32_t* head, int32_t* cand_of, int32_t* pick,
                                                int32_t* npick, int32_t* gain0, int32_t* gain_end, uint8_t* known_out) {
    if (!eg_fleet_args_ok(ctx, d2, min_size, Cmax) ||
        !eg_args_ok(ctx, occ, known, g, R, Cmax, W, H, r2, dirs, B, span, wg, wc, min_gain, rounds, goal, gcost, npick, known_out))
        return SC_ERR_INVALID;
    const size_t n = (size_t)W * H;
    if (eg_field_data_invalid(g, (size_t)R * n)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_d = st.in(d2, n * 4), i_k = st.in(known, n), i_o = st.in(occ, n), i_g = st.in(g, (size_t)R * n * 4);
    const size_t rb = (size_t)R * 4, cb = (size_t)Cmax * 4;
    // a slot for every intermediate array, copied back where the caller keeps it
    const int o_l = st.out(label, label ? n * 4 : 0), o_s = st.out(slot, n * 4), o_nc = st.out(ncl, 8), o_r = st.out(rep, cb),
              o_cs = st.out(csize, cb), o_b = st.out(cbox, cbox ? cb * 4 : 0), o_m = st.out(csum, cb * 4), o_ce = st.out(centre, cb);
    const int o_go = st.out(goal, rb), o_gc = st.out(gcost, rb), o_gg = st.out(ggain, ggain ? rb : 0), o_h = st.out(head, head ? rb : 0),
              o_co = st.out(cand_of, cand_of ? rb : 0), o_p = st.out(pick, pick ? rb : 0), o_n = st.out(npick, 4),
              o_g0 = st.out(gain0, gain0 ? cb : 0), o_ge = st.out(gain_end, gain_end ? cb : 0), o_k = st.out(known_out, known_out ? n : 0);
    int r = st.upload();
    if (r == SC_OK)
        r = eg_launch_fleet(ctx, st.dev<const int32_t>(i_d), st.dev<const uint8_t>(i_k), W, H, r2_clear, min_size, Cmax, st.dev<const uint8_t>(i_o),
                            st.dev<const int32_t>(i_g), R, r2, dirs, B, span, wg, wc, min_gain, rounds, label ? st.dev<int32_t>(o_l) : nullptr,
                            st.dev<int32_t>(o_s), st.dev<int32_t>(o_nc), st.dev<int32_t>(o_r), st.dev<int32_t>(o_cs),
                            cbox ? st.dev<int32_t>(o_b) : nullptr, st.dev<int64_t>(o_m), st.dev<int32_t>(o_ce), st.dev<int32_t>(o_go),
                            st.dev<int32_t>(o_gc), ggain ? st.dev<int32_t>(o_gg) : nullptr, head ? st.dev<int32_t>(o_h) : nullptr,
                            cand_of ? st.dev<int32_t>(o_co) : nullptr, pick ? st.dev<int32_t>(o_p) : nullptr, st.dev<int32_t>(o_n),
                            gain0 ? st.dev<int32_t>(o_g0) : nullptr, gain_end ? st.dev<int32_t>(o_ge) : nullptr,
                            known_out ? st.dev<uint8_t>(o_k) : nullptr);
    return st.finish(r);
}
