// pose.hip -- planning in poses: the footprint mask (sc_footprint_mask_u8), cost fields over (cell, heading)
// (sc_pose_field_batch) and their read-out (sc_pose_paths_batch).  include/sea_current_hip.h has the definition, DESIGN.md
// section 28 the argument.
//
// Footprint mask.  At an axis heading the covered offsets are a box in (dx, dy); at a diagonal heading they are the points of
// a box in (P, Q) = (dx + dy, dy - dx) with P = Q mod 2, which is every point of that box that is a cell at all.  So one
// summed-area table of the blocked cells over (x, y) and one over (x + y, y - x + W - 1) answer every heading with four reads:
// bit k is set iff the box, clipped to the table, holds no blocked cell.  The boxes come from the definition itself: the host
// evaluates the two inequalities over every offset that can be covered and takes the extremes.  Per grid of the batch:
// sat_rows_kernel (the indicator and its prefix sums along a row, one wavefront per row), sat_cols_kernel (one lane per
// column) for each table, then footprint_kernel (one lane per cell).
//
// Field.  The grid is cut into 32 x 32 tiles.  A tile visit is one workgroup of 256 lanes with the eight layers of the tile and
// a one-cell halo in LDS (row stride 35 words, odd against bank conflicts) and, per cell, T and the eight pose-valid bits.  It
// alternates two phases until one round of both lowers nothing:
//   lines  within layer k, states connect only along the grid lines of direction h_k.  A lane takes one line (32 rows or
//          columns, 63 diagonals per layer; 380 in all) and walks it once in each direction, carrying the running minimum
//          plus the edge cost (w_k forwards, w_k + rev_cost backwards) across the legal edges.  Halo cells are read, never
//          written.
//   turns  a lane takes a cell and closes its eight headings: two laps each way round the circle with turn_cost across
//          neighbouring valid headings.
// Every value written is the cost of a legal path from a seed, and the visit ends only when no legal edge into one of its
// cells lowers a value against the halo it loaded.  Changed cells are stored; the up to 8 neighbour tiles whose halo holds a
// changed cell are queued.  Chip-wide rounds, stamps (atomicMax), the two lists and the finisher are those of field.hip: a
// visit may read a neighbour's border while that neighbour is rewritten, every value it sees is the cost of a legal path, and
// the neighbour queues this tile again.  No workgroup waits for another.  The finisher (one workgroup per field) visits the
// tiles still queued, one at a time from an LDS bitmap, until none is: values only fall and a tile is queued only when a
// value fell, so it terminates at the unique fixed point, for every `rounds`.
//   toward: the transposed graph is the graph with every heading vector negated (sgn = -1); the kernels keep the caller's
//   layer numbers, which is the header's renaming k -> k + 4 applied twice.
// Read-out: one wavefront per query; lanes 0..3 test the four candidates of a step at once, the first that matches is taken.
#include "sc_internal.h"

namespace {

constexpr int PT = 32;                      // tile edge
constexpr int PR = PT + 2;                  // with the halo
constexpr int PS = PR + 1;                  // LDS row stride (odd)
constexpr int PL = PR * PS;                 // LDS layer stride
constexpr int P_LINES = 4 * PT + 4 * (2 * PT - 1);   // lines of the eight layers
constexpr uint32_t PINF = 0x7FFFFFFFu;      // SC_FIELD_INF; INF + 14 + 255 still fits in uint32
constexpr int P_THREADS = 256;
constexpr int P_MAX_TILES = (SC_MAX_DIM / PT) * (SC_MAX_DIM / PT);
constexpr int PP_WAVES = 4;

__constant__ int P_HX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
__constant__ int P_HY[8] = {0, 1, 1, 1, 0, -1, -1, -1};

struct pose_args {
    const int32_t* d2;       // [G][H][W]
    const uint8_t* hmask;    // [G][H][W] or NULL
    const int32_t* fgrid;    // [F] or NULL (G == 1)
    const int32_t* root;     // [F]
    const int32_t* rhead;    // [F]
    int32_t* gp;             // [F][8][H][W]
    int32_t* ok;             // [F] 1: the field has a seed
    int32_t* stamp;          // [F][nt] round + 1 a tile is queued for (grows only)
    int32_t* list[2];        // [F * nt] each: f * nt + tile
    int32_t* ctr;            // [rounds + 1] list length of each round
    int G, W, H, F, TX, TY, nt;
    int32_t thr;
    uint32_t tc;             // turn_cost
    int rev;                 // rev_cost, -1: none
    int sgn;                 // +1: from the root, -1: toward it
};

__device__ __forceinline__ bool pose_valid(const int32_t* D, const uint8_t* M, size_t c, int k, int32_t thr) {
    return D[c] >= thr && (!M || ((M[c] >> k) & 1));
}

// gp = INF everywhere; grid (blocks, fields), fields strided.  Block 0 of a field writes "no seed" into its ok flag and status.
__global__ void pose_fill_kernel(pose_args a, int32_t* fstatus) {
    const size_t n = (size_t)8 * a.W * a.H;
    for (int f = blockIdx.y; f < a.F; f += gridDim.y) {
        int32_t* G = a.gp + (size_t)f * n;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) G[i] = (int32_t)PINF;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.ok[f] = 0;
            if (fstatus) fstatus[f] = SC_Q_BAD_ENDPOINT;
        }
    }
}

// one lane per field: the seeds at 0, the field ok, and queued for round 0 (stamp 1) the root's tile and every neighbour tile
// whose halo holds the root (a visit that changes nothing marks no neighbour, and the seed itself never changes)
__global__ void pose_seed_kernel(pose_args a, int32_t* fstatus) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.F) return;
    const long long n = (long long)a.W * a.H;
    const int gi = a.fgrid ? a.fgrid[f] : 0;
    const int c = a.root[f], rh = a.rhead[f];
    if (gi < 0 || gi >= a.G || c < 0 || c >= n || rh < -1 || rh > 7) return;
    const int32_t* D = a.d2 + (size_t)gi * n;
    const uint8_t* M = a.hmask ? a.hmask + (size_t)gi * n : nullptr;
    bool any = false;
    for (int k = 0; k < 8; ++k)
        if ((rh == k || rh == -1) && pose_valid(D, M, (size_t)c, k, a.thr)) {
            a.gp[((size_t)f * 8 + k) * n + c] = 0;
            any = true;
        }
    if (!any) return;
    a.ok[f] = 1;
    if (fstatus) fstatus[f] = SC_Q_OK;
    const int x = c % a.W, y = c / a.W, tx = x / PT, ty = y / PT, lx = x % PT, ly = y % PT;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int ux = tx + dx, uy = ty + dy;
            if (ux < 0 || uy < 0 || ux >= a.TX || uy >= a.TY) continue;
            if ((dx < 0 && lx != 0) || (dx > 0 && lx != PT - 1) || (dy < 0 && ly != 0) || (dy > 0 && ly != PT - 1)) continue;
            const int u = f * a.nt + uy * a.TX + ux;
            if (atomicMax(a.stamp + u, 1) < 1) a.list[0][atomicAdd(a.ctr, 1)] = u;
        }
}

// one line of layer k, walked from cell `at` in steps of `st` (LDS offsets): cells 1 .. len - 2 are the tile's, the two ends
// its halo.  c: the cost of an edge walked this way; diag: the side cells of the step lie at +sa and +sb of its first cell
__device__ __forceinline__ bool walk_line(uint32_t* g, const uint16_t* vm, int at, int st, int len, int k, uint32_t c, bool diag, int sa, int sb) {
    bool chg = false;
    uint32_t run = g[at];
    uint32_t vp = vm[at];
    for (int i = 1; i <= len - 2; ++i) {
        const int nx = at + st;
        const uint32_t vn = vm[nx];
        bool legal = ((vp & vn) >> k) & 1u;
        if (diag) legal = legal && (vm[at + sa] & 0x100u) && (vm[at + sb] & 0x100u);
        uint32_t v = g[nx];
        if (legal && run + c < v) {
            v = run + c;
            g[nx] = v;
            chg = true;
        }
        run = v;
        vp = vn;
        at = nx;
    }
    return chg;
}

// Visit tile (tx, ty) of field f with the workgroup; mark(tx', ty') queues a neighbour (called by lane 0).  g: 8 * PL words,
// vm: PL half-words, edge: one word, all LDS.
template <class Mark>
__device__ __forceinline__ void pose_visit(const pose_args& a, int f, int tx, int ty, uint32_t* g, uint16_t* vm, uint32_t* edge, Mark mark) {
    const int tid = threadIdx.x;
    const int W = a.W, H = a.H;
    const size_t n = (size_t)W * H;
    const int gi = a.fgrid ? a.fgrid[f] : 0;
    const int32_t* D = a.d2 + (size_t)gi * n;
    const uint8_t* M = a.hmask ? a.hmask + (size_t)gi * n : nullptr;
    int32_t* G = a.gp + (size_t)f * 8 * n;
    const int x0 = tx * PT - 1, y0 = ty * PT - 1;   // the grid cell of LDS cell (0, 0)
    __syncthreads();                                // the LDS of the visit before
    if (tid == 0) *edge = 0;
    for (int i = tid; i < PR * PR; i += P_THREADS) {
        const int lx = i % PR, ly = i / PR, x = x0 + lx, y = y0 + ly, o = ly * PS + lx;
        const bool in = x >= 0 && x < W && y >= 0 && y < H;
        const size_t c = in ? (size_t)y * W + x : 0;
        uint32_t m = 0;
        if (in && D[c] >= a.thr) m = 0x100u | (M ? (uint32_t)M[c] : 0xFFu);
        vm[o] = (uint16_t)m;
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k * PL + o] = in ? (uint32_t)G[(size_t)k * n + c] : PINF;
    }
    __syncthreads();
    for (;;) {
        int chg = 0;
        for (int li = tid; li < P_LINES; li += P_THREADS) {
            int k, at, st, len, sa = 0, sb = 0;
            bool diag;
            if (li < 4 * PT) {              // rows (k = 0, 4) and columns (k = 2, 6)
                k = 2 * (li / PT);
                const int j = li % PT + 1;
                diag = false;
                len = PR;
                if ((k & 3) == 0) { at = j * PS; st = 1; }
                else { at = j; st = PS; }
            } else {                        // diagonals (k = 1, 5) and anti-diagonals (k = 3, 7)
                const int e = li - 4 * PT, nd = 2 * PT - 1;
                k = 2 * (e / nd) + 1;
                const int d = e % nd - (PT - 1), sx = d > 0 ? d : 0, sy = d < 0 ? -d : 0;
                diag = true;
                len = PR - (d < 0 ? -d : d);
                if ((k & 3) == 1) { at = sy * PS + sx; st = PS + 1; sa = 1; sb = PS; }
                else { at = sy * PS + (PR - 1 - sx); st = PS - 1; sa = -1; sb = PS; }
            }
            // the base step of the line is h_(k & 3); a move of the layer runs along it iff k < 4 (from the root) / k >= 4 (toward)
            const bool along = (k < 4) == (a.sgn > 0);
            const uint32_t w = (k & 1) ? 14u : 10u;
            uint32_t* gk = g + k * PL;
            if (along || a.rev >= 0) chg |= walk_line(gk, vm, at, st, len, k, along ? w : w + (uint32_t)a.rev, diag, sa, sb);
            if (!along || a.rev >= 0) {
                const int end = at + (len - 1) * st;
                chg |= walk_line(gk, vm, end, -st, len, k, along ? w + (uint32_t)a.rev : w, diag, -sa, -sb);
            }
        }
        __syncthreads();
        for (int i = tid; i < PT * PT; i += P_THREADS) {
            const int o = (i / PT + 1) * PS + i % PT + 1;
            const uint32_t m = vm[o] & 0xFFu;
            if (m == 0) continue;
            uint32_t v[8], old[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) old[k] = v[k] = g[k * PL + o];
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int k = s & 7, kn = (k + 1) & 7;
                if (((m >> k) & (m >> kn) & 1u) && v[k] + a.tc < v[kn]) v[kn] = v[k] + a.tc;
            }
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int k = (16 - s) & 7, kn = (k + 7) & 7;
                if (((m >> k) & (m >> kn) & 1u) && v[k] + a.tc < v[kn]) v[kn] = v[k] + a.tc;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (v[k] < old[k]) {
                    g[k * PL + o] = v[k];
                    chg = 1;
                }
        }
        if (!__syncthreads_or(chg)) break;
    }
    // store what fell (a tile's cells are written by its own visits only, so what memory holds is what this visit loaded)
    uint32_t eb = 0;
    for (int i = tid; i < PT * PT; i += P_THREADS) {
        const int lx = i % PT + 1, ly = i / PT + 1, x = x0 + lx, y = y0 + ly, o = ly * PS + lx;
        if (x >= W || y >= H) continue;
        const size_t c = (size_t)y * W + x;
        bool fell = false;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t v = g[k * PL + o];
            if (v < (uint32_t)G[(size_t)k * n + c]) {
                G[(size_t)k * n + c] = (int32_t)v;
                fell = true;
            }
        }
        if (fell) {
            const uint32_t l = lx == 1, r = lx == PT, u = ly == 1, d = ly == PT;
            eb |= l | r << 1 | u << 2 | d << 3 | (l & u) << 4 | (r & u) << 5 | (l & d) << 6 | (r & d) << 7;
        }
    }
    if (eb) atomicOr(edge, eb);
    __syncthreads();
    if (tid == 0) {
        const uint32_t e = *edge;
        const bool hasL = tx > 0, hasR = tx + 1 < a.TX, hasU = ty > 0, hasD = ty + 1 < a.TY;
        if (hasL && (e & 1u)) mark(tx - 1, ty);
        if (hasR && (e & 2u)) mark(tx + 1, ty);
        if (hasU && (e & 4u)) mark(tx, ty - 1);
        if (hasD && (e & 8u)) mark(tx, ty + 1);
        if (hasL && hasU && (e & 16u)) mark(tx - 1, ty - 1);
        if (hasR && hasU && (e & 32u)) mark(tx + 1, ty - 1);
        if (hasL && hasD && (e & 64u)) mark(tx - 1, ty + 1);
        if (hasR && hasD && (e & 128u)) mark(tx + 1, ty + 1);
    }
}

// chip-wide round r: one workgroup per queued (field, tile), grid-stride over the list
__global__ __launch_bounds__(P_THREADS) void pose_round_kernel(pose_args a, int r) {
    __shared__ uint32_t g[8 * PL];
    __shared__ uint16_t vm[PL];
    __shared__ uint32_t edge;
    const int n = a.ctr[r];
    const int32_t* cur = a.list[r & 1];
    int32_t* nxt = a.list[(r + 1) & 1];
    int32_t* nctr = a.ctr + r + 1;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int e = cur[i];
        const int f = e / a.nt, t = e % a.nt;
        pose_visit(a, f, t % a.TX, t / a.TX, g, vm, &edge, [&](int ux, int uy) {
            const int u = f * a.nt + uy * a.TX + ux;
            if (atomicMax(a.stamp + u, r + 2) < r + 2) nxt[atomicAdd(nctr, 1)] = u;
        });
    }
}

// finisher: one workgroup per field completes the tiles still queued after `rounds` chip-wide rounds
__global__ __launch_bounds__(P_THREADS) void pose_finish_kernel(pose_args a, int rounds) {
    __shared__ uint32_t g[8 * PL];
    __shared__ uint16_t vm[PL];
    __shared__ uint32_t edge;
    __shared__ uint32_t dirty[P_MAX_TILES / 32];
    __shared__ int next;
    const int f = blockIdx.x;
    if (!a.ok[f]) return;
    const int nt = a.nt, nw = (nt + 31) / 32;
    const int tid = threadIdx.x;
    for (int w = tid; w < nw; w += P_THREADS) {
        uint32_t b = 0;
        for (int k = 0; k < 32 && w * 32 + k < nt; ++k) b |= (uint32_t)(a.stamp[(size_t)f * nt + w * 32 + k] == rounds + 1) << k;
        dirty[w] = b;
    }
    for (;;) {
        if (tid == 0) next = nt;
        __syncthreads();
        for (int w = tid; w < nw; w += P_THREADS)
            if (dirty[w]) {
                atomicMin(&next, w * 32 + __ffs(dirty[w]) - 1);
                break;
            }
        __syncthreads();
        const int t = next;
        if (t >= nt) break;
        if (tid == 0) dirty[t >> 5] &= ~(1u << (t & 31));
        pose_visit(a, f, t % a.TX, t / a.TX, g, vm, &edge, [&](int ux, int uy) {
            const int u = uy * a.TX + ux;
            dirty[u >> 5] |= 1u << (u & 31);
        });
        __syncthreads();
    }
}

// ---- read-out ------------------------------------------------------------------------------------------------------
struct pose_paths_args {
    const int32_t* d2;
    const uint8_t* hmask;
    const int32_t* fgrid;
    const int32_t* gp;
    const int32_t* root;
    const int32_t* rhead;
    const int32_t* qfield;
    const int32_t* target;
    const int32_t* thead;
    int G, W, H, F, Q, Lmax, to_root, cells_only;
    int32_t thr;
    uint32_t tc;
    int rev, sgn;
    int32_t* path;
    uint8_t* head;
    int32_t *len, *cost, *status;
};

__global__ __launch_bounds__(64 * PP_WAVES) void pose_paths_kernel(pose_paths_args a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * PP_WAVES + wave;
    if (q >= a.Q) return;
    const int W = a.W, H = a.H;
    const long long n = (long long)W * H;
    const int fq = a.qfield[q];
    const int gi = (fq >= 0 && fq < a.F) ? (a.fgrid ? a.fgrid[fq] : 0) : -1;
    const int r = gi >= 0 ? a.root[fq] : -1, rh = gi >= 0 ? a.rhead[fq] : -2;
    const int t = a.target[q], th = a.thead[q];
    bool ok = gi >= 0 && gi < a.G && r >= 0 && r < n && rh >= -1 && rh <= 7 && t >= 0 && t < n && th >= -1 && th <= 7;
    const int32_t* D = a.d2 + (size_t)(ok ? gi : 0) * n;
    const uint8_t* M = a.hmask ? a.hmask + (size_t)(ok ? gi : 0) * n : nullptr;
    if (ok) {
        bool rv = false;
        for (int k = 0; k < 8; ++k) rv = rv || ((rh == k || rh == -1) && pose_valid(D, M, (size_t)r, k, a.thr));
        ok = rv && (th >= 0 ? pose_valid(D, M, (size_t)t, th, a.thr) : D[t] >= a.thr);
    }
    if (!ok) {
        if (lane == 0) { a.len[q] = 0; a.cost[q] = -1; a.status[q] = SC_Q_BAD_ENDPOINT; }
        return;
    }
    const int32_t* G = a.gp + (size_t)fq * 8 * n;
    int k = th;
    uint32_t v;
    if (th >= 0) v = (uint32_t)G[(size_t)th * n + t];
    else {
        k = 0;
        v = PINF;
        for (int j = 0; j < 8; ++j) {
            const uint32_t u = (uint32_t)G[(size_t)j * n + t];
            if (u < v) { v = u; k = j; }
        }
    }
    if (v >= PINF) {
        if (lane == 0) { a.len[q] = 0; a.cost[q] = -1; a.status[q] = SC_Q_NO_PATH; }
        return;
    }
    const uint32_t vt = v;
    int32_t* P = a.path + (size_t)q * a.Lmax;
    uint8_t* Hd = a.head + (size_t)q * a.Lmax;
    int cx = t % W, cy = t / W;
    long long L = 0, steps = 0;
    int last = -1;
    bool fail = false;
    for (;;) {
        // the entry of state (c, k), in walk order (target first)
        const int c = cy * W + cx;
        if (a.cells_only && c == last) {
            if (!a.to_root && lane == 0 && L - 1 < a.Lmax) Hd[L - 1] = (uint8_t)k;   // root..target: the last of a cell in walk order is its first
        } else {
            if (lane == 0 && L < a.Lmax) { P[L] = c; Hd[L] = (uint8_t)k; }
            ++L;
            last = c;
        }
        if (v == 0) break;
        // lanes 0..3: the candidates in the order of the definition
        int px = cx, py = cy, pk = k;
        uint32_t ec = a.tc;
        bool legal = false;
        if (lane < 2) {
            const int s = lane == 0 ? -a.sgn : a.sgn;
            px = cx + s * P_HX[k]; py = cy + s * P_HY[k];
            ec = ((k & 1) ? 14u : 10u) + (lane == 1 ? (uint32_t)a.rev : 0u);
            legal = (lane == 0 || a.rev >= 0) && px >= 0 && px < W && py >= 0 && py < H;
            if (legal) legal = pose_valid(D, M, (size_t)py * W + px, k, a.thr);
            if (legal && (k & 1)) legal = D[(size_t)cy * W + px] >= a.thr && D[(size_t)py * W + cx] >= a.thr;
        } else if (lane < 4) {
            pk = (k + (lane == 2 ? 7 : 1)) & 7;
            legal = pose_valid(D, M, (size_t)c, pk, a.thr);
        }
        uint32_t pv = PINF;
        if (legal) pv = (uint32_t)G[(size_t)pk * n + (size_t)py * W + px];
        const uint64_t hit = __ballot(legal && pv < PINF && pv + ec == v) & 0xFull;
        if (hit == 0ull || ++steps > 8 * n) { fail = true; break; }
        const int j = __ffsll((long long)hit) - 1;
        cx = __shfl(px, j); cy = __shfl(py, j); k = __shfl(pk, j); v = (uint32_t)__shfl((int)pv, j);
    }
    if (fail) {
        if (lane == 0) { a.len[q] = 0; a.cost[q] = -1; a.status[q] = SC_Q_NO_PATH; }
        return;
    }
    const int Li = (int)(L < 0x7FFFFFFF ? L : 0x7FFFFFFF);
    if (L <= a.Lmax && !a.to_root) {
        __threadfence_block();   // lane 0 wrote the walk; every lane reverses it
        for (int i = lane; i < Li / 2; i += 64) {
            const int32_t u = P[i], w = P[Li - 1 - i];
            P[i] = w;
            P[Li - 1 - i] = u;
            const uint8_t hu = Hd[i], hw = Hd[Li - 1 - i];
            Hd[i] = hw;
            Hd[Li - 1 - i] = hu;
        }
    }
    if (lane == 0) { a.len[q] = Li; a.cost[q] = (int32_t)vt; a.status[q] = L <= a.Lmax ? SC_Q_OK : SC_Q_TRUNCATED; }
}

// ---- footprint mask ------------------------------------------------------------------------------------------------
struct fp_boxes {
    int lo_a[8], hi_a[8], lo_b[8], hi_b[8];   // axis headings: a = dx, b = dy; diagonal headings: a = dx + dy, b = dy - dx
};

// is table cell (i, j) a blocked grid cell?  DIAG: (i, j) = (x + y, y - x + W - 1)
template <bool DIAG>
__device__ __forceinline__ int fp_blocked(const int32_t* D, int W, int H, int32_t thr, int i, int j) {
    int x, y;
    if (DIAG) {
        const int q = j - (W - 1);
        if ((i + q) & 1) return 0;
        x = (i - q) / 2;
        y = (i + q) / 2;
        if (i - q < 0 || i + q < 0) return 0;
    } else {
        x = j;
        y = i;
    }
    if (x < 0 || y < 0 || x >= W || y >= H) return 0;
    return D[(size_t)y * W + x] < thr;
}

// S [PH + 1][PW + 1]: row 0 and column 0 are zero, S[i + 1][j + 1] = the blocked cells of row i up to column j.  One wavefront
// per row.
template <bool DIAG>
__global__ __launch_bounds__(64) void sat_rows_kernel(const int32_t* __restrict__ D, int W, int H, int32_t thr, int PH, int PW, int32_t* __restrict__ S) {
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i <= PH; i += gridDim.x) {
        int32_t* R = S + (size_t)i * (PW + 1);
        if (i == 0) {
            for (int j = lane; j <= PW; j += 64) R[j] = 0;
            continue;
        }
        if (lane == 0) R[0] = 0;
        int carry = 0;
        for (int j0 = 0; j0 < PW; j0 += 64) {
            const int j = j0 + lane;
            int v = j < PW ? fp_blocked<DIAG>(D, W, H, thr, i - 1, j) : 0;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const int o = __shfl_up(v, s, 64);
                if (lane >= s) v += o;
            }
            if (j < PW) R[j + 1] = carry + v;
            carry += __shfl(v, 63, 64);
        }
    }
}

// the prefix sums down every column, one lane per column
__global__ void sat_cols_kernel(int PH, int PW, int32_t* __restrict__ S) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > PW) return;
    int run = 0;
    for (int i = 1; i <= PH; ++i) {
        run += S[(size_t)i * (PW + 1) + j];
        S[(size_t)i * (PW + 1) + j] = run;
    }
}

// blocked cells of table rows i0..i1, columns j0..j1 (clipped by the caller)
__device__ __forceinline__ int sat_box(const int32_t* S, int PW, int i0, int i1, int j0, int j1) {
    const size_t st = (size_t)PW + 1;
    return S[(size_t)(i1 + 1) * st + j1 + 1] - S[(size_t)i0 * st + j1 + 1] - S[(size_t)(i1 + 1) * st + j0] + S[(size_t)i0 * st + j0];
}

__global__ void footprint_kernel(const int32_t* __restrict__ Sa, const int32_t* __restrict__ Sd, int W, int H, fp_boxes b, uint8_t* __restrict__ out) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (size_t)W * H) return;
    const int x = (int)(c % W), y = (int)(c / W);
    const int PD = W + H - 1, p = x + y, q = y - x + W - 1;
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int cnt;
        if (k & 1)
            cnt = sat_box(Sd, PD, max(p + b.lo_a[k], 0), min(p + b.hi_a[k], PD - 1), max(q + b.lo_b[k], 0), min(q + b.hi_b[k], PD - 1));
        else
            cnt = sat_box(Sa, W, max(y + b.lo_b[k], 0), min(y + b.hi_b[k], H - 1), max(x + b.lo_a[k], 0), min(x + b.hi_a[k], W - 1));
        m |= (uint32_t)(cnt == 0) << k;
    }
    out[c] = (uint8_t)m;
}

int pose_default_rounds(int TX, int TY) { return 4 * (TX + TY) + 16; }

}  // namespace

// ---- host side -----------------------------------------------------------------------------------------------------
// the map and cost side of a pose call
struct pose_map {
    const int32_t* d2;
    const uint8_t* hmask;
    int G;
    const int32_t* fgrid;
    int W, H;
    int32_t r2_clear;
    int turn_cost, rev_cost, toward;
    const int32_t* root;
    const int32_t* rhead;
    int F;
};

struct pose_query {
    const int32_t* qfield;
    const int32_t* target;
    const int32_t* thead;
    int Q, Lmax, to_root, cells_only;
    int32_t* path;
    uint8_t* head;
    int32_t *len, *cost, *status;
};

// the argument contract of the four pose entries; q NULL: a build
static bool pose_args_ok(const sc_ctx* ctx, const pose_map& m, const int32_t* gp, const pose_query* q) {
    if (!ctx || !m.d2 || !gp || !m.root || !m.rhead || m.G <= 0 || m.F <= 0 || m.W <= 0 || m.H <= 0) return false;
    if (!(m.W <= SC_MAX_DIM && m.H <= SC_MAX_DIM && (m.fgrid || m.G == 1))) return false;
    if (m.turn_cost < 0 || m.turn_cost > 255 || m.rev_cost < -1 || m.rev_cost > 255) return false;
    const long long step = 14 + (m.rev_cost > 0 ? m.rev_cost : 0), top = step > m.turn_cost ? step : m.turn_cost;
    if (top * (8ll * m.W * m.H - 1) > (long long)INT32_MAX - 1) return false;
    if (!q) return true;
    if (m.turn_cost < 1 || q->Q < 0 || q->Lmax <= 0) return false;
    return q->Q == 0 || (q->qfield && q->target && q->thead && q->path && q->head && q->len && q->cost && q->status);   // Q == 0: a no-op, its arrays may be empty
}

static int pose_build(sc_ctx* ctx, const pose_map& m, int rounds, int32_t* gp, int32_t* fstatus) {
    if (!pose_args_ok(ctx, m, gp, nullptr)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const int W = m.W, H = m.H, F = m.F;
    const int TX = (W + PT - 1) / PT, TY = (H + PT - 1) / PT, nt = TX * TY;
    if ((long long)F * nt > 0x7FFFFFFF / 2) return SC_ERR_INVALID;
    if (rounds < 0) rounds = pose_default_rounds(TX, TY);
    const size_t o_ok = 0, o_stamp = al256((size_t)F * 4), o_l0 = o_stamp + al256((size_t)F * nt * 4), o_l1 = o_l0 + al256((size_t)F * nt * 4),
                 o_ctr = o_l1 + al256((size_t)F * nt * 4), total = o_ctr + al256((size_t)(rounds + 1) * 4);
    int r = sc_scratch_reserve(ctx, &ctx->pose_state, total);
    if (r != SC_OK) return r;
    if (!ctx->cu_count) {
        int cu = 0;
        SC_HIP(ctx, hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
        ctx->cu_count = cu > 0 ? cu : 1;
    }
    char* b = (char*)ctx->pose_state.p;
    pose_args a;
    a.d2 = m.d2; a.hmask = m.hmask; a.fgrid = m.fgrid; a.root = m.root; a.rhead = m.rhead; a.gp = gp;
    a.ok = (int32_t*)(b + o_ok); a.stamp = (int32_t*)(b + o_stamp);
    a.list[0] = (int32_t*)(b + o_l0); a.list[1] = (int32_t*)(b + o_l1); a.ctr = (int32_t*)(b + o_ctr);
    a.G = m.G; a.W = W; a.H = H; a.F = F; a.TX = TX; a.TY = TY; a.nt = nt;
    a.thr = m.r2_clear > 1 ? m.r2_clear : 1;
    a.tc = (uint32_t)m.turn_cost; a.rev = m.rev_cost; a.sgn = m.toward ? -1 : 1;
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    SC_HIP(ctx, hipMemsetAsync(b + o_stamp, 0, o_l0 - o_stamp, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(b + o_ctr, 0, total - o_ctr, ctx->stream));
    {
        const size_t n = (size_t)8 * W * H;
        unsigned bx = (unsigned)((n + 1023) / 1024);
        if (bx > 1024) bx = 1024;
        hipLaunchKernelGGL(pose_fill_kernel, dim3(bx, F < 65535 ? F : 65535), dim3(1024), 0, ctx->stream, a, fstatus);
        hipLaunchKernelGGL(pose_seed_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, ctx->stream, a, fstatus);
    }
    if (rounds > 0) {
        const long long cap = (long long)ctx->cu_count * 4;
        const unsigned blocks = (unsigned)((long long)F * nt < cap ? (long long)F * nt : cap);
        for (int k = 0; k < rounds; ++k) hipLaunchKernelGGL(pose_round_kernel, dim3(blocks), dim3(P_THREADS), 0, ctx->stream, a, k);
    }
    hipLaunchKernelGGL(pose_finish_kernel, dim3(F), dim3(P_THREADS), 0, ctx->stream, a, rounds);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

static int pose_read(sc_ctx* ctx, const pose_map& m, const int32_t* gp, const pose_query& q) {
    if (!pose_args_ok(ctx, m, gp, &q)) return SC_ERR_INVALID;
    if (q.Q == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    pose_paths_args a{m.d2, m.hmask, m.fgrid, gp, m.root, m.rhead, q.qfield, q.target, q.thead, m.G, m.W, m.H, m.F, q.Q, q.Lmax,
                      q.to_root ? 1 : 0, q.cells_only ? 1 : 0, m.r2_clear > 1 ? m.r2_clear : 1, (uint32_t)m.turn_cost, m.rev_cost,
                      m.toward ? -1 : 1, q.path, q.head, q.len, q.cost, q.status};
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    hipLaunchKernelGGL(pose_paths_kernel, dim3((unsigned)((q.Q + PP_WAVES - 1) / PP_WAVES)), dim3(64 * PP_WAVES), 0, ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

template <class T> static T* pose_staged(const sc_stage& st, int i, T* host) { return host ? st.dev<T>(i) : nullptr; }

// the device copies of the map side of a _host call
struct pose_map_stage {
    int d2, hm, fg, rt, rh;
    pose_map_stage(sc_stage& st, const pose_map& m) {
        const size_t n = (size_t)m.W * m.H, fb = (size_t)m.F * 4;
        d2 = st.in(m.d2, (size_t)m.G * n * 4); hm = st.in(m.hmask, m.hmask ? (size_t)m.G * n : 0); fg = st.in(m.fgrid, m.fgrid ? fb : 0);
        rt = st.in(m.root, fb); rh = st.in(m.rhead, fb);
    }
    pose_map dev(const sc_stage& st, const pose_map& m) const {
        pose_map d = m;
        d.d2 = pose_staged(st, d2, m.d2); d.hmask = pose_staged(st, hm, m.hmask); d.fgrid = pose_staged(st, fg, m.fgrid);
        d.root = pose_staged(st, rt, m.root); d.rhead = pose_staged(st, rh, m.rhead);
        return d;
    }
};

static int pose_build_host(sc_ctx* ctx, const pose_map& m, int rounds, int32_t* gp, int32_t* fstatus) {
    if (!pose_args_ok(ctx, m, gp, nullptr)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const pose_map_stage ms(st, m);
    const int o_g = st.out(gp, (size_t)m.F * 8 * m.W * m.H * 4), o_st = st.out(fstatus, fstatus ? (size_t)m.F * 4 : 0);
    int r = st.upload();
    if (r == SC_OK) r = pose_build(ctx, ms.dev(st, m), rounds, st.dev<int32_t>(o_g), pose_staged(st, o_st, fstatus));
    return st.finish(r);
}

static int pose_read_host(sc_ctx* ctx, const pose_map& m, const int32_t* gp, const pose_query& q) {
    if (!pose_args_ok(ctx, m, gp, &q)) return SC_ERR_INVALID;
    if (q.Q == 0) return SC_OK;
    // data contract: every gp value is a cost or SC_FIELD_INF
    const size_t cells = (size_t)m.F * 8 * m.W * m.H;
    for (size_t i = 0; i < cells; ++i)
        if (gp[i] < 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t qb = (size_t)q.Q * 4;
    sc_stage st(ctx);
    const pose_map_stage ms(st, m);
    const int i_g = st.in(gp, cells * 4), i_qf = st.in(q.qfield, qb), i_t = st.in(q.target, qb), i_th = st.in(q.thead, qb);
    const int o_p = st.out(q.path, qb * q.Lmax), o_h = st.out(q.head, (size_t)q.Q * q.Lmax), o_len = st.out(q.len, qb), o_c = st.out(q.cost, qb),
              o_s = st.out(q.status, qb);
    int r = st.upload();
    if (r == SC_OK)
        r = pose_read(ctx, ms.dev(st, m), st.dev<const int32_t>(i_g),
                      {st.dev<const int32_t>(i_qf), st.dev<const int32_t>(i_t), st.dev<const int32_t>(i_th), q.Q, q.Lmax, q.to_root, q.cells_only,
                       st.dev<int32_t>(o_p), st.dev<uint8_t>(o_h), st.dev<int32_t>(o_len), st.dev<int32_t>(o_c), st.dev<int32_t>(o_s)});
    return st.finish(r);
}

// is offset (dx, dy) covered at heading k?  The definition, word for word.
static bool fp_covered(int k, int dx, int dy, int front, int back, int left, int right) {
    static const int hx[8] = {1, 1, 0, -1, -1, -1, 0, 1}, hy[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    const int n = hx[k] * hx[k] + hy[k] * hy[k], u = dx * hx[k] + dy * hy[k], v = -dx * hy[k] + dy * hx[k];
    return (u >= 0 ? u * u <= n * front * front : u * u <= n * back * back) && (v >= 0 ? v * v <= n * left * left : v * v <= n * right * right);
}

static bool fp_args_ok(const sc_ctx* ctx, const int32_t* d2, int W, int H, int batch, int front, int back, int left, int right,
                       const uint8_t* hmask) {
    const int M = SC_FOOTPRINT_MAX;
    return ctx && d2 && hmask && W >= 1 && W <= SC_MAX_DIM && H >= 1 && H <= SC_MAX_DIM && batch >= 1 && front >= 0 && front <= M && back >= 0 &&
           back <= M && left >= 0 && left <= M && right >= 0 && right <= M;
}

extern "C" int sc_footprint_mask_u8(sc_ctx* ctx, const int32_t* d2, int W, int H, int batch, int32_t r2_clear, int front, int back, int left,
                                    int right, uint8_t* hmask) {
    if (!fp_args_ok(ctx, d2, W, H, batch, front, back, left, right, hmask)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    // the extremes of the covered offsets, in (dx, dy) at the axis headings and in (dx + dy, dy - dx) at the diagonal ones
    fp_boxes bx;
    const int R = 2 * SC_FOOTPRINT_MAX;
    for (int k = 0; k < 8; ++k) {
        bx.lo_a[k] = bx.hi_a[k] = bx.lo_b[k] = bx.hi_b[k] = 0;
        for (int dy = -R; dy <= R; ++dy)
            for (int dx = -R; dx <= R; ++dx) {
                if (!fp_covered(k, dx, dy, front, back, left, right)) continue;
                const int ca = (k & 1) ? dx + dy : dx, cb = (k & 1) ? dy - dx : dy;
                if (ca < bx.lo_a[k]) bx.lo_a[k] = ca;
                if (ca > bx.hi_a[k]) bx.hi_a[k] = ca;
                if (cb < bx.lo_b[k]) bx.lo_b[k] = cb;
                if (cb > bx.hi_b[k]) bx.hi_b[k] = cb;
            }
    }
    const int PD = W + H - 1;
    const size_t ba = al256((size_t)(W + 1) * (H + 1) * 4), bd = (size_t)(PD + 1) * (PD + 1) * 4;
    int r = sc_scratch_reserve(ctx, &ctx->fp_sat, ba + bd);
    if (r != SC_OK) return r;
    int32_t* Sa = (int32_t*)ctx->fp_sat.p;
    int32_t* Sd = (int32_t*)((char*)ctx->fp_sat.p + ba);
    const int32_t thr = r2_clear > 1 ? r2_clear : 1;
    const size_t n = (size_t)W * H;
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    for (int g = 0; g < batch; ++g) {
        const int32_t* D = d2 + (size_t)g * n;
        hipLaunchKernelGGL(sat_rows_kernel<false>, dim3((unsigned)(H + 1)), dim3(64), 0, ctx->stream, D, W, H, thr, H, W, Sa);
        hipLaunchKernelGGL(sat_cols_kernel, dim3((unsigned)((W + 1 + 255) / 256)), dim3(256), 0, ctx->stream, H, W, Sa);
        hipLaunchKernelGGL(sat_rows_kernel<true>, dim3((unsigned)(PD + 1)), dim3(64), 0, ctx->stream, D, W, H, thr, PD, PD, Sd);
        hipLaunchKernelGGL(sat_cols_kernel, dim3((unsigned)((PD + 1 + 255) / 256)), dim3(256), 0, ctx->stream, PD, PD, Sd);
        hipLaunchKernelGGL(footprint_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, Sa, Sd, W, H, bx, hmask + (size_t)g * n);
    }
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_footprint_mask_u8_host(sc_ctx* ctx, const int32_t* d2, int W, int H, int batch, int32_t r2_clear, int front, int back,
                                         int left, int right, uint8_t* hmask) {
    if (!fp_args_ok(ctx, d2, W, H, batch, front, back, left, right, hmask)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)batch * W * H;
    sc_stage st(ctx);
    const int i_d2 = st.in(d2, n * 4), o_m = st.out(hmask, n);
    int r = st.upload();
    if (r == SC_OK) r = sc_footprint_mask_u8(ctx, st.dev<const int32_t>(i_d2), W, H, batch, r2_clear, front, back, left, right, st.dev<uint8_t>(o_m));
    return st.finish(r);
}

extern "C" int sc_pose_field_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int G, const int32_t* fgrid, int W, int H,
                                   int32_t r2_clear, int turn_cost, int rev_cost, int toward, const int32_t* root, const int32_t* rhead, int F,
                                   int rounds, int32_t* gp, int32_t* fstatus) {
    return pose_build(ctx, {d2, hmask, G, fgrid, W, H, r2_clear, turn_cost, rev_cost, toward, root, rhead, F}, rounds, gp, fstatus);
}

extern "C" int sc_pose_field_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int G, const int32_t* fgrid, int W, int H,
                                        int32_t r2_clear, int turn_cost, int rev_cost, int toward, const int32_t* root, const int32_t* rhead,
                                        int F, int rounds, int32_t* gp, int32_t* fstatus) {
    return pose_build_host(ctx, {d2, hmask, G, fgrid, W, H, r2_clear, turn_cost, rev_cost, toward, root, rhead, F}, rounds, gp, fstatus);
}

extern "C" int sc_pose_paths_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int G, const int32_t* fgrid, int W, int H,
                                   int32_t r2_clear, int turn_cost, int rev_cost, int toward, const int32_t* gp, const int32_t* root,
                                   const int32_t* rhead, int F, const int32_t* qfield, const int32_t* target, const int32_t* thead, int Q,
                                   int Lmax, int to_root, int cells_only, int32_t* path, uint8_t* head, int32_t* len, int32_t* cost,
                                   int32_t* status) {
    return pose_read(ctx, {d2, hmask, G, fgrid, W, H, r2_clear, turn_cost, rev_cost, toward, root, rhead, F}, gp,
                     {qfield, target, thead, Q, Lmax, to_root, cells_only, path, head, len, cost, status});
}

extern "C" int sc_pose_paths_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int G, const int32_t* fgrid, int W, int H,
                                        int32_t r2_clear, int turn_cost, int rev_cost, int toward, const int32_t* gp, const int32_t* root,
                                        const int32_t* rhead, int F, const int32_t* qfield, const int32_t* target, const int32_t* thead,
                                        int Q, int Lmax, int to_root, int cells_only, int32_t* path, uint8_t* head, int32_t* len,
                                        int32_t* cost, int32_t* status) {
    return pose_read_host(ctx, {d2, hmask, G, fgrid, W, H, r2_clear, turn_cost, rev_cost, toward, root, rhead, F}, gp,
                          {qfield, target, thead, Q, Lmax, to_root, cells_only, path, head, len, cost, status});
}
