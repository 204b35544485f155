// car.hip -- car-like pose planning: the arc mask (sc_arc_mask_u16), cost fields over (cell, heading) whose heading changes
// only along arcs (sc_car_field_batch) and their read-out (sc_car_paths_batch).  include/sea_current_hip_car.h has the
// definition, DESIGN.md section 32 the argument.  What this file shares with pose.hip (headings, pose validity, the line walk,
// rounds, stamps, lists and the finisher) it restates: pose.hip stays as it is.
//
// Arc mask.  One lane per cell.  Per heading it walks the first leg once (n steps) and, where that is legal, the second leg
// of either sense: at most 24 n step tests per cell, every one the definition's.
//
// Field.  The grid is cut into 32 x 32 tiles.  A tile visit is one workgroup of 256 lanes with the eight layers of the tile
// and a halo of 2 n cells in LDS (a window of 32 + 4 n cells a side, row stride odd against bank conflicts) and one word per
// cell: T, the eight pose-valid bits and the sixteen arc bits.  It alternates two phases until one round of both lowers
// nothing:
//   lines  pose.hip's: within layer k states connect along the grid lines of direction h_k; a lane walks one line of the
//          tile once each way, from the halo cell next to the tile.  Edges 1 and 2.
//   arcs   a lane takes a cell and, per heading, gathers over the at most four arc edges that end in the state (toward: that
//          leave it): two whose other end lies 2 n cells ahead (legality: the cell's own arc bits) and two whose other end
//          lies behind (legality: the arc bits of that cell).  Edges 3 .. 6.
// Every value written is the cost of a legal path from a seed, and the visit ends only when no legal edge into one of its
// cells lowers a value against the halo it loaded.  Changed cells are stored; a cell that fell within 2 n cells of a tile side
// queues every neighbour tile whose halo holds it, the diagonal ones included.  Chip-wide rounds, stamps (atomicMax), the two
// lists and the finisher are those of pose.hip: no workgroup waits for another, values only fall, a tile is queued only when
// a value fell, so the fixed point is the field for every `rounds`.
//   toward: the layers keep the caller's numbers.  The line walk negates the heading vectors (sgn = -1); the arc gather swaps
//   the costs of the edges ahead and behind.
// Read-out: one wavefront per query; lanes 0..5 test the six candidates of a step, a ballot takes the first, and the lanes
// write the 2 n - 1 intermediate cells of an arc.
#include "sc_internal.h"

#include "../../include/sea_current_hip_car.h"

namespace {

constexpr int CT = 32;                      // tile edge
constexpr int CS = CT + 2;                  // the lines' window: the tile and one cell round it
constexpr int C_LINES = 4 * CT + 4 * (2 * CT - 1);
constexpr uint32_t CINF = 0x7FFFFFFFu;      // SC_FIELD_INF; INF + the dearest edge still fits in uint32
constexpr int C_THREADS = 256;
constexpr int C_MAX_TILES = (SC_MAX_DIM / CT) * (SC_MAX_DIM / CT);
constexpr int CP_WAVES = 4;
constexpr int C_MAX_ROUNDS = 65536;

__constant__ int C_HX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
__constant__ int C_HY[8] = {0, 1, 1, 1, 0, -1, -1, -1};

// the LDS window of a tile visit for arc_n = N: halo 2 N, edge 32 + 4 N, row stride (odd), layer stride, bytes (g [8][PL] | cm [PL])
template <int N> struct car_win {
    static constexpr int hl = 2 * N, PR = CT + 2 * hl, PS = PR + 1, PL = PR * PS, bytes = 9 * PL * 4;
};

struct car_args {
    const int32_t* d2;       // [G][H][W]
    const uint8_t* hmask;    // [G][H][W] or NULL
    const uint16_t* amask;   // [G][H][W]
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
    int n;                   // arc_n
    int hl;                  // halo 2 n
    uint32_t ca, cr;         // the cost of a forward arc and of a reverse arc
    int rev;                 // rev_cost, -1: none
    int sgn;                 // +1: from the root, -1: toward it
};

__device__ __forceinline__ bool car_valid(const int32_t* D, const uint8_t* M, size_t c, int k, int32_t thr) {
    return D[c] >= thr && (!M || ((M[c] >> k) & 1));
}

// gp = INF everywhere; grid (blocks, fields), fields strided.  Block 0 of a field writes "no seed" into its ok flag and status.
__global__ void car_fill_kernel(car_args a, int32_t* fstatus) {
    const size_t n = (size_t)8 * a.W * a.H;
    for (int f = blockIdx.y; f < a.F; f += gridDim.y) {
        int32_t* G = a.gp + (size_t)f * n;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) G[i] = (int32_t)CINF;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.ok[f] = 0;
            if (fstatus) fstatus[f] = SC_Q_BAD_ENDPOINT;
        }
    }
}

// one lane per field: the seeds at 0, the field ok, and queued for round 0 (stamp 1) the root's tile and every neighbour tile
// whose halo holds the root
__global__ void car_seed_kernel(car_args a, int32_t* fstatus) {
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
        if ((rh == k || rh == -1) && car_valid(D, M, (size_t)c, k, a.thr)) {
            a.gp[((size_t)f * 8 + k) * n + c] = 0;
            any = true;
        }
    if (!any) return;
    a.ok[f] = 1;
    if (fstatus) fstatus[f] = SC_Q_OK;
    const int x = c % a.W, y = c / a.W, tx = x / CT, ty = y / CT, lx = x % CT, ly = y % CT;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int ux = tx + dx, uy = ty + dy;
            if (ux < 0 || uy < 0 || ux >= a.TX || uy >= a.TY) continue;
            if ((dx < 0 && lx >= a.hl) || (dx > 0 && lx < CT - a.hl) || (dy < 0 && ly >= a.hl) || (dy > 0 && ly < CT - a.hl)) continue;
            const int u = f * a.nt + uy * a.TX + ux;
            if (atomicMax(a.stamp + u, 1) < 1) a.list[0][atomicAdd(a.ctr, 1)] = u;
        }
}

// one line of layer k, walked from cell `at` in steps of `st` (LDS offsets): cells 1 .. len - 2 are the tile's, the two ends
// its halo.  c: the cost of an edge walked this way; diag: the side cells of the step lie at +sa and +sb of its first cell
__device__ __forceinline__ bool car_walk_line(uint32_t* g, const uint32_t* cm, int at, int st, int len, int k, uint32_t c, bool diag, int sa, int sb) {
    bool chg = false;
    uint32_t run = g[at];
    uint32_t vp = cm[at];
    for (int i = 1; i <= len - 2; ++i) {
        const int nx = at + st;
        const uint32_t vn = cm[nx];
        bool legal = ((vp & vn) >> k) & 1u;
        if (diag) legal = legal && (cm[at + sa] & 0x100u) && (cm[at + sb] & 0x100u);
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
// cm: PL words (bits 0..7 pose valid, bit 8 T, bits 16..31 the arc bits), edge: one word, all LDS.
template <int N, class Mark>
__device__ __forceinline__ void car_visit(const car_args& a, int f, int tx, int ty, uint32_t* g, uint32_t* cm, uint32_t* edge, Mark mark) {
    const int tid = threadIdx.x;
    constexpr int an = N, hl = car_win<N>::hl, PR = car_win<N>::PR, PS = car_win<N>::PS, PL = car_win<N>::PL;
    const int W = a.W, H = a.H;
    const size_t n = (size_t)W * H;
    const int gi = a.fgrid ? a.fgrid[f] : 0;
    const int32_t* D = a.d2 + (size_t)gi * n;
    const uint8_t* M = a.hmask ? a.hmask + (size_t)gi * n : nullptr;
    const uint16_t* AM = a.amask + (size_t)gi * n;
    int32_t* G = a.gp + (size_t)f * 8 * n;
    const int x0 = tx * CT - hl, y0 = ty * CT - hl;   // the grid cell of LDS cell (0, 0)
    __syncthreads();                                  // the LDS of the visit before
    if (tid == 0) *edge = 0;
    for (int i = tid; i < PR * PR; i += C_THREADS) {
        const int lx = i % PR, ly = i / PR, x = x0 + lx, y = y0 + ly, o = ly * PS + lx;
        const bool in = x >= 0 && x < W && y >= 0 && y < H;
        const size_t c = in ? (size_t)y * W + x : 0;
        uint32_t m = 0;
        if (in && D[c] >= a.thr) m = 0x100u | (M ? (uint32_t)M[c] : 0xFFu) | ((uint32_t)AM[c] << 16);
        cm[o] = m;
        const int32_t* gc = G + c;   // a running pointer: eight scalar layer bases would not fit the scalar registers
#pragma unroll
        for (int k = 0; k < 8; ++k, gc += n) g[k * PL + o] = in ? (uint32_t)*gc : CINF;
    }
    __syncthreads();
    const int lbase = (hl - 1) * PS + (hl - 1);       // LDS cell (0, 0) of the lines' window
    // the arc edges of a state: ahead costs what an out-edge costs when the field runs toward the root
    const bool toward = a.sgn < 0;
    const uint32_t c_ahead = toward ? a.ca : a.cr, c_behind = toward ? a.cr : a.ca;
    const bool do_ahead = toward || a.rev >= 0, do_behind = !toward || a.rev >= 0;
    for (;;) {
        int chg = 0;
        for (int li = tid; li < C_LINES; li += C_THREADS) {
            int k, at, st, len, sa = 0, sb = 0;
            bool diag;
            if (li < 4 * CT) {              // rows (k = 0, 4) and columns (k = 2, 6)
                k = 2 * (li / CT);
                const int j = li % CT + 1;
                diag = false;
                len = CS;
                if ((k & 3) == 0) { at = j * PS; st = 1; }
                else { at = j; st = PS; }
            } else {                        // diagonals (k = 1, 5) and anti-diagonals (k = 3, 7)
                const int e = li - 4 * CT, nd = 2 * CT - 1;
                k = 2 * (e / nd) + 1;
                const int d = e % nd - (CT - 1), sx = d > 0 ? d : 0, sy = d < 0 ? -d : 0;
                diag = true;
                len = CS - (d < 0 ? -d : d);
                if ((k & 3) == 1) { at = sy * PS + sx; st = PS + 1; sa = 1; sb = PS; }
                else { at = sy * PS + (CS - 1 - sx); st = PS - 1; sa = -1; sb = PS; }
            }
            at += lbase;
            // the base step of the line is h_(k & 3); a move of the layer runs along it iff k < 4 (from the root) / k >= 4 (toward)
            const bool along = (k < 4) == (a.sgn > 0);
            const uint32_t w = (k & 1) ? 14u : 10u;
            uint32_t* gk = g + k * PL;
            if (along || a.rev >= 0) chg |= car_walk_line(gk, cm, at, st, len, k, along ? w : w + (uint32_t)a.rev, diag, sa, sb);
            if (!along || a.rev >= 0) {
                const int end = at + (len - 1) * st;
                chg |= car_walk_line(gk, cm, end, -st, len, k, along ? w + (uint32_t)a.rev : w, diag, -sa, -sb);
            }
        }
        __syncthreads();
        // arcs: other lanes lower the values this gather reads; every one of them is the cost of a legal path, and a round in
        // which any lane wrote is followed by another
        for (int i = tid; i < CT * CT; i += C_THREADS) {
            const int o = (i / CT + hl) * PS + i % CT + hl;
            const uint32_t m = cm[o];
            if ((m & 0xFFu) == 0) continue;
#pragma unroll 1
            for (int k = 0; k < 8; ++k) {   // rolled: the 32 uniform offsets of an unrolled gather do not fit the scalar registers
                if (!((m >> k) & 1u)) continue;
                const uint32_t old = g[k * PL + o];
                uint32_t v = old;
#pragma unroll
                for (int si = 0; si < 2; ++si) {
                    const int kn = (k + (si ? 7 : 1)) & 7;      // the other heading of an arc of sense s = si ? -1 : +1 ahead
                    const int kp = (k + (si ? 1 : 7)) & 7;      // ... and of the arc of that sense that ends here
                    if (do_ahead && ((m >> (16 + 2 * k + si)) & 1u)) {
                        const int oy = o + an * (C_HX[k] + C_HX[kn]) + an * (C_HY[k] + C_HY[kn]) * PS;
                        const uint32_t pv = g[kn * PL + oy];
                        if (pv < CINF && pv + c_ahead < v) v = pv + c_ahead;
                    }
                    if (do_behind) {
                        const int oy = o - an * (C_HX[k] + C_HX[kp]) - an * (C_HY[k] + C_HY[kp]) * PS;
                        if ((cm[oy] >> (16 + 2 * kp + si)) & 1u) {
                            const uint32_t pv = g[kp * PL + oy];
                            if (pv < CINF && pv + c_behind < v) v = pv + c_behind;
                        }
                    }
                }
                if (v < old) {
                    g[k * PL + o] = v;
                    chg = 1;
                }
            }
        }
        if (!__syncthreads_or(chg)) break;
    }
    // store what fell (a tile's cells are written by its own visits only, so what memory holds is what this visit loaded)
    uint32_t eb = 0;
    for (int i = tid; i < CT * CT; i += C_THREADS) {
        const int lx = i % CT, ly = i / CT, x = tx * CT + lx, y = ty * CT + ly, o = (ly + hl) * PS + lx + hl;
        if (x >= W || y >= H) continue;
        const size_t c = (size_t)y * W + x;
        bool fell = false;
        int32_t* gc = G + c;
#pragma unroll
        for (int k = 0; k < 8; ++k, gc += n) {
            const uint32_t v = g[k * PL + o];
            if (v < (uint32_t)*gc) {
                *gc = (int32_t)v;
                fell = true;
            }
        }
        if (fell) {   // the neighbour tiles whose halo of 2 n cells holds the cell
            const uint32_t l = lx < hl, r = lx >= CT - hl, u = ly < hl, d = ly >= CT - hl;
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
template <int N>
__global__ __launch_bounds__(C_THREADS) void car_round_kernel(car_args a, int r) {
    extern __shared__ uint32_t car_lds[];   // g [8][PL] | cm [PL]
    __shared__ uint32_t edge;
    uint32_t* g = car_lds;
    uint32_t* cm = car_lds + 8 * car_win<N>::PL;
    for (int i = blockIdx.x; i < a.ctr[r]; i += gridDim.x) {   // the list's length is read anew: one scalar fewer kept across a visit
        const int e = a.list[r & 1][i];
        const int f = e / a.nt, t = e % a.nt;
        car_visit<N>(a, f, t % a.TX, t / a.TX, g, cm, &edge, [&](int ux, int uy) {
            const int u = e - t + uy * a.TX + ux;
            if (atomicMax(a.stamp + u, r + 2) < r + 2) a.list[(r + 1) & 1][atomicAdd(a.ctr + r + 1, 1)] = u;
        });
    }
}

// finisher: one workgroup per field completes the tiles still queued after `rounds` chip-wide rounds
template <int N>
__global__ __launch_bounds__(C_THREADS) void car_finish_kernel(car_args a, int rounds) {
    __shared__ uint32_t edge;
    __shared__ uint32_t dirty[C_MAX_TILES / 32];
    __shared__ int next;
    extern __shared__ uint32_t car_lds[];   // g [8][PL] | cm [PL]
    uint32_t* g = car_lds;
    uint32_t* cm = car_lds + 8 * car_win<N>::PL;
    const int f = blockIdx.x;
    if (!a.ok[f]) return;
    const int nt = a.nt, nw = (nt + 31) / 32;
    const int tid = threadIdx.x;
    for (int w = tid; w < nw; w += C_THREADS) {
        uint32_t b = 0;
        for (int k = 0; k < 32 && w * 32 + k < nt; ++k) b |= (uint32_t)(a.stamp[(size_t)f * nt + w * 32 + k] == rounds + 1) << k;
        dirty[w] = b;
    }
    for (;;) {
        if (tid == 0) next = nt;
        __syncthreads();
        for (int w = tid; w < nw; w += C_THREADS)
            if (dirty[w]) {
                atomicMin(&next, w * 32 + __ffs(dirty[w]) - 1);
                break;
            }
        __syncthreads();
        const int t = next;
        if (t >= nt) break;
        if (tid == 0) dirty[t >> 5] &= ~(1u << (t & 31));
        car_visit<N>(a, f, t % a.TX, t / a.TX, g, cm, &edge, [&](int ux, int uy) {
            const int u = uy * a.TX + ux;
            dirty[u >> 5] |= 1u << (u & 31);
        });
        __syncthreads();
    }
}

// ---- read-out ------------------------------------------------------------------------------------------------------
struct car_paths_args {
    const int32_t* d2;
    const uint8_t* hmask;
    const uint16_t* amask;
    const int32_t* fgrid;
    const int32_t* gp;
    const int32_t* root;
    const int32_t* rhead;
    const int32_t* qfield;
    const int32_t* target;
    const int32_t* thead;
    int G, W, H, F, Q, Lmax, to_root;
    int32_t thr;
    int n;
    uint32_t ca, cr;
    int rev, sgn;
    int32_t* path;
    uint8_t* head;
    int32_t *len, *cost, *status;
};

// candidate j (0 .. 5 = the definition's edges 1 .. 6) of a step from state (cx, cy, k)
struct car_cand {
    int px, py, pk;   // the far end
    int ka, kb;       // arcs: the headings of the forward arc's first and second leg
    bool ahead, fwd;  // arcs: the far end lies ahead of the state; the edge is driven forwards
};

__device__ __forceinline__ car_cand car_candidate(int j, int cx, int cy, int k, int n, int sgn) {
    car_cand r;
    r.ka = r.kb = r.pk = k;
    r.ahead = r.fwd = false;
    if (j < 2) {
        const int s = j == 0 ? -sgn : sgn;
        r.px = cx + s * C_HX[k];
        r.py = cy + s * C_HY[k];
        return r;
    }
    const int s = (j & 1) ? 7 : 1;   // j = 2, 4: sense +1; j = 3, 5: sense -1
    r.fwd = j < 4;
    r.ahead = r.fwd == (sgn < 0);
    if (r.ahead) {
        r.kb = (k + s) & 7;
        r.pk = r.kb;
        r.px = cx + n * (C_HX[k] + C_HX[r.kb]);
        r.py = cy + n * (C_HY[k] + C_HY[r.kb]);
    } else {
        r.ka = (k + 8 - s) & 7;
        r.pk = r.ka;
        r.px = cx - n * (C_HX[k] + C_HX[r.ka]);
        r.py = cy - n * (C_HY[k] + C_HY[r.ka]);
    }
    return r;
}

__global__ __launch_bounds__(64 * CP_WAVES) void car_paths_kernel(car_paths_args a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * CP_WAVES + wave;
    if (q >= a.Q) return;
    const int W = a.W, H = a.H, an = a.n;
    const long long n = (long long)W * H;
    const int fq = a.qfield[q];
    const int gi = (fq >= 0 && fq < a.F) ? (a.fgrid ? a.fgrid[fq] : 0) : -1;
    const int r = gi >= 0 ? a.root[fq] : -1, rh = gi >= 0 ? a.rhead[fq] : -2;
    const int t = a.target[q], th = a.thead[q];
    bool ok = gi >= 0 && gi < a.G && r >= 0 && r < n && rh >= -1 && rh <= 7 && t >= 0 && t < n && th >= -1 && th <= 7;
    const int32_t* D = a.d2 + (size_t)(ok ? gi : 0) * n;
    const uint8_t* M = a.hmask ? a.hmask + (size_t)(ok ? gi : 0) * n : nullptr;
    const uint16_t* AM = a.amask + (size_t)(ok ? gi : 0) * n;
    if (ok) {
        bool rv = false;
        for (int k = 0; k < 8; ++k) rv = rv || ((rh == k || rh == -1) && car_valid(D, M, (size_t)r, k, a.thr));
        ok = rv && (th >= 0 ? car_valid(D, M, (size_t)t, th, a.thr) : D[t] >= a.thr);
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
        v = CINF;
        for (int j = 0; j < 8; ++j) {
            const uint32_t u = (uint32_t)G[(size_t)j * n + t];
            if (u < v) { v = u; k = j; }
        }
    }
    if (v >= CINF) {
        if (lane == 0) { a.len[q] = 0; a.cost[q] = -1; a.status[q] = SC_Q_NO_PATH; }
        return;
    }
    const uint32_t vt = v;
    int32_t* P = a.path + (size_t)q * a.Lmax;
    uint8_t* Hd = a.head + (size_t)q * a.Lmax;
    int cx = t % W, cy = t / W;
    long long L = 0, steps = 0;
    bool fail = false;
    for (;;) {
        // the entry of state (c, k), in walk order (target first)
        if (lane == 0 && L < a.Lmax) { P[L] = cy * W + cx; Hd[L] = (uint8_t)k; }
        ++L;
        if (v == 0) break;
        // lanes 0..5: the candidates in the order of the definition
        bool legal = false;
        uint32_t ec = 0, pv = CINF;
        if (lane < 6) {
            const car_cand cd = car_candidate(lane, cx, cy, k, an, a.sgn);
            const bool in = cd.px >= 0 && cd.px < W && cd.py >= 0 && cd.py < H;
            if (lane < 2) {
                ec = ((k & 1) ? 14u : 10u) + (lane == 1 ? (uint32_t)a.rev : 0u);
                legal = (lane == 0 || a.rev >= 0) && in;
                if (legal) legal = car_valid(D, M, (size_t)cd.py * W + cd.px, k, a.thr);
                if (legal && (k & 1)) legal = D[(size_t)cy * W + cd.px] >= a.thr && D[(size_t)cd.py * W + cx] >= a.thr;
            } else {
                ec = cd.fwd ? a.ca : a.cr;
                legal = (cd.fwd || a.rev >= 0) && in;
                if (legal) {   // the arc starts at this state (ahead) or at the far end
                    const size_t mc = cd.ahead ? (size_t)cy * W + cx : (size_t)cd.py * W + cd.px;
                    legal = (AM[mc] >> (2 * cd.ka + (lane & 1))) & 1;
                }
            }
            if (legal) pv = (uint32_t)G[(size_t)cd.pk * n + (size_t)cd.py * W + cd.px];
        }
        const uint64_t hit = __ballot(legal && pv < CINF && pv + ec == v) & 0x3Full;
        if (hit == 0ull || ++steps > 8 * n) { fail = true; break; }
        const int j = __ffsll((long long)hit) - 1;
        const car_cand cd = car_candidate(j, cx, cy, k, an, a.sgn);
        if (j >= 2) {
            // the 2 n - 1 cells between the end poses, in walk order; cell i of the forward arc is reached by its first leg up to
            // the corner (i = n) when driven forwards, short of it when driven backwards
            const int m = lane + 1;
            if (m < 2 * an && L + lane < a.Lmax) {
                int x, y;
                if (cd.ahead) {
                    const int m1 = m < an ? m : an, m2 = m - m1;
                    x = cx + m1 * C_HX[cd.ka] + m2 * C_HX[cd.kb];
                    y = cy + m1 * C_HY[cd.ka] + m2 * C_HY[cd.kb];
                } else {
                    const int m1 = m < an ? m : an, m2 = m - m1;
                    x = cx - m1 * C_HX[cd.kb] - m2 * C_HX[cd.ka];
                    y = cy - m1 * C_HY[cd.kb] - m2 * C_HY[cd.ka];
                }
                const int i = cd.ahead ? m : 2 * an - m;
                const int hd = i < an ? cd.ka : i > an ? cd.kb : cd.fwd ? cd.ka : cd.kb;
                P[L + lane] = y * W + x;
                Hd[L + lane] = (uint8_t)hd;
            }
            L += 2 * an - 1;
        }
        v = (uint32_t)__shfl((int)pv, j);
        cx = cd.px; cy = cd.py; k = cd.pk;
    }
    if (fail) {
        if (lane == 0) { a.len[q] = 0; a.cost[q] = -1; a.status[q] = SC_Q_NO_PATH; }
        return;
    }
    const int Li = (int)(L < 0x7FFFFFFF ? L : 0x7FFFFFFF);
    if (L <= a.Lmax && !a.to_root) {
        __threadfence_block();   // several lanes wrote the walk; every lane reverses it
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

// ---- arc mask --------------------------------------------------------------------------------------------------------
// is the step (x, y) -> (x + dx, y + dy) a legal A* move that ends in a valid pose of heading k?  T(x, y) is known.
__device__ __forceinline__ bool arc_step(const int32_t* D, const uint8_t* M, int W, int H, int32_t thr, int x, int y, int dx, int dy, int k) {
    const int nx = x + dx, ny = y + dy;
    if (nx < 0 || ny < 0 || nx >= W || ny >= H) return false;
    if (!car_valid(D, M, (size_t)ny * W + nx, k, thr)) return false;
    return !(dx && dy) || (D[(size_t)y * W + nx] >= thr && D[(size_t)ny * W + x] >= thr);
}

__global__ void arc_mask_kernel(const int32_t* __restrict__ d2, const uint8_t* __restrict__ hmask, int W, int H, int32_t thr, int n,
                                uint16_t* __restrict__ amask) {
    const size_t cells = (size_t)W * H, c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cells) return;
    const int32_t* D = d2 + (size_t)blockIdx.y * cells;
    const uint8_t* M = hmask ? hmask + (size_t)blockIdx.y * cells : nullptr;
    const int x0 = (int)(c % W), y0 = (int)(c / W);
    uint32_t m = 0;
    if (D[c] >= thr) {
        for (int k = 0; k < 8; ++k) {
            bool ok = car_valid(D, M, c, k, thr);
            int x = x0, y = y0;
            for (int i = 0; i < n && ok; ++i) {
                ok = arc_step(D, M, W, H, thr, x, y, C_HX[k], C_HY[k], k);
                x += C_HX[k];
                y += C_HY[k];
            }
            if (!ok) continue;
            for (int si = 0; si < 2; ++si) {
                const int kb = (k + (si ? 7 : 1)) & 7;
                bool ok2 = car_valid(D, M, (size_t)y * W + x, kb, thr);   // the corner at the second heading
                int xx = x, yy = y;
                for (int j = 0; j < n && ok2; ++j) {
                    ok2 = arc_step(D, M, W, H, thr, xx, yy, C_HX[kb], C_HY[kb], kb);
                    xx += C_HX[kb];
                    yy += C_HY[kb];
                }
                m |= (uint32_t)ok2 << (2 * k + si);
            }
        }
    }
    amask[(size_t)blockIdx.y * cells + c] = (uint16_t)m;
}

int car_default_rounds(int TX, int TY) { return 4 * (TX + TY) + 16; }

}  // namespace

// ---- host side -----------------------------------------------------------------------------------------------------
// the map and cost side of a car call
struct car_map {
    const int32_t* d2;
    const uint8_t* hmask;
    const uint16_t* amask;
    int G;
    const int32_t* fgrid;
    int W, H;
    int32_t r2_clear;
    int arc_n, arc_cost, rev_cost, toward;
    const int32_t* root;
    const int32_t* rhead;
    int F;
};

struct car_query {
    const int32_t* qfield;
    const int32_t* target;
    const int32_t* thead;
    int Q, Lmax, to_root;
    int32_t* path;
    uint8_t* head;
    int32_t *len, *cost, *status;
};

static long long car_arc_cost(const car_map& m, bool reverse) {
    return 24ll * m.arc_n + m.arc_cost + (reverse ? 2ll * m.arc_n * (m.rev_cost > 0 ? m.rev_cost : 0) : 0);
}

// the argument contract of the four field and read-out entries; q NULL: a build
static bool car_args_ok(const sc_ctx* ctx, const car_map& m, const int32_t* gp, const car_query* q) {
    if (!ctx || !m.d2 || !m.amask || !gp || !m.root || !m.rhead || m.G <= 0 || m.F <= 0 || m.W <= 0 || m.H <= 0) return false;
    if (!(m.W <= SC_MAX_DIM && m.H <= SC_MAX_DIM && (m.fgrid || m.G == 1))) return false;
    if (m.arc_n < 1 || m.arc_n > SC_ARC_MAX || m.arc_cost < 0 || m.arc_cost > 255 || m.rev_cost < -1 || m.rev_cost > 255) return false;
    if (car_arc_cost(m, true) * (8ll * m.W * m.H - 1) > (long long)INT32_MAX - 1) return false;
    if (!q) return true;
    if (q->Q < 0 || q->Lmax <= 0) return false;
    return q->Q == 0 || (q->qfield && q->target && q->thead && q->path && q->head && q->len && q->cost && q->status);   // Q == 0: a no-op, its arrays may be empty
}

static int car_build(sc_ctx* ctx, const car_map& m, int rounds, int32_t* gp, int32_t* fstatus) {
    if (!car_args_ok(ctx, m, gp, nullptr)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const int W = m.W, H = m.H, F = m.F;
    const int TX = (W + CT - 1) / CT, TY = (H + CT - 1) / CT, nt = TX * TY;
    if ((long long)F * nt > 0x7FFFFFFF / 2) return SC_ERR_INVALID;
    if (rounds < 0) rounds = car_default_rounds(TX, TY);
    if (rounds > C_MAX_ROUNDS) rounds = C_MAX_ROUNDS;
    const size_t o_ok = 0, o_stamp = al256((size_t)F * 4), o_l0 = o_stamp + al256((size_t)F * nt * 4), o_l1 = o_l0 + al256((size_t)F * nt * 4),
                 o_ctr = o_l1 + al256((size_t)F * nt * 4), total = o_ctr + al256((size_t)(rounds + 1) * 4);
    int r = sc_scratch_reserve(ctx, &ctx->car_state, total);
    if (r != SC_OK) return r;
    if (!ctx->cu_count) {
        int cu = 0;
        SC_HIP(ctx, hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
        ctx->cu_count = cu > 0 ? cu : 1;
    }
    char* b = (char*)ctx->car_state.p;
    car_args a;
    a.d2 = m.d2; a.hmask = m.hmask; a.amask = m.amask; a.fgrid = m.fgrid; a.root = m.root; a.rhead = m.rhead; a.gp = gp;
    a.ok = (int32_t*)(b + o_ok); a.stamp = (int32_t*)(b + o_stamp);
    a.list[0] = (int32_t*)(b + o_l0); a.list[1] = (int32_t*)(b + o_l1); a.ctr = (int32_t*)(b + o_ctr);
    a.G = m.G; a.W = W; a.H = H; a.F = F; a.TX = TX; a.TY = TY; a.nt = nt;
    a.thr = m.r2_clear > 1 ? m.r2_clear : 1;
    a.n = m.arc_n; a.hl = 2 * m.arc_n;
    a.ca = (uint32_t)car_arc_cost(m, false); a.cr = (uint32_t)car_arc_cost(m, true);
    a.rev = m.rev_cost; a.sgn = m.toward ? -1 : 1;
    // the kernels of this arc_n and their LDS: 47952 B (n = 1), 59040 B (2), 71280 B (3), 84672 B (4)
    void (*round_k)(car_args, int) = car_round_kernel<1>;
    void (*finish_k)(car_args, int) = car_finish_kernel<1>;
    int lds = car_win<1>::bytes;
    if (m.arc_n == 2) { round_k = car_round_kernel<2>; finish_k = car_finish_kernel<2>; lds = car_win<2>::bytes; }
    if (m.arc_n == 3) { round_k = car_round_kernel<3>; finish_k = car_finish_kernel<3>; lds = car_win<3>::bytes; }
    if (m.arc_n == 4) { round_k = car_round_kernel<4>; finish_k = car_finish_kernel<4>; lds = car_win<4>::bytes; }
    if (lds + 9 * 1024 > 64 * 1024) {   // with the finisher's static 8.3 KB: arc_n >= 2
        r = sc_allow_big_lds(ctx, reinterpret_cast<const void*>(round_k), 96 * 1024);
        if (r == SC_OK) r = sc_allow_big_lds(ctx, reinterpret_cast<const void*>(finish_k), 96 * 1024);
        if (r != SC_OK) return r;
    }
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    SC_HIP(ctx, hipMemsetAsync(b + o_stamp, 0, o_l0 - o_stamp, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(b + o_ctr, 0, total - o_ctr, ctx->stream));
    {
        const size_t n = (size_t)8 * W * H;
        unsigned bx = (unsigned)((n + 1023) / 1024);
        if (bx > 1024) bx = 1024;
        hipLaunchKernelGGL(car_fill_kernel, dim3(bx, F < 65535 ? F : 65535), dim3(1024), 0, ctx->stream, a, fstatus);
        hipLaunchKernelGGL(car_seed_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, ctx->stream, a, fstatus);
    }
    if (rounds > 0) {
        const int per_cu = (160 * 1024) / (lds + 1024);   // workgroups of a compute unit that the LDS admits: 3, 2, 2, 1
        const long long cap = (long long)ctx->cu_count * per_cu;
        const unsigned blocks = (unsigned)((long long)F * nt < cap ? (long long)F * nt : cap);
        for (int k = 0; k < rounds; ++k) hipLaunchKernelGGL(round_k, dim3(blocks), dim3(C_THREADS), lds, ctx->stream, a, k);
    }
    hipLaunchKernelGGL(finish_k, dim3(F), dim3(C_THREADS), lds, ctx->stream, a, rounds);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

static int car_read(sc_ctx* ctx, const car_map& m, const int32_t* gp, const car_query& q) {
    if (!car_args_ok(ctx, m, gp, &q)) return SC_ERR_INVALID;
    if (q.Q == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    car_paths_args a{m.d2, m.hmask, m.amask, m.fgrid, gp, m.root, m.rhead, q.qfield, q.target, q.thead, m.G, m.W, m.H, m.F, q.Q, q.Lmax,
                     q.to_root ? 1 : 0, m.r2_clear > 1 ? m.r2_clear : 1, m.arc_n, (uint32_t)car_arc_cost(m, false),
                     (uint32_t)car_arc_cost(m, true), m.rev_cost, m.toward ? -1 : 1, q.path, q.head, q.len, q.cost, q.status};
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    hipLaunchKernelGGL(car_paths_kernel, dim3((unsigned)((q.Q + CP_WAVES - 1) / CP_WAVES)), dim3(64 * CP_WAVES), 0, ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

template <class T> static T* car_staged(const sc_stage& st, int i, T* host) { return host ? st.dev<T>(i) : nullptr; }

// the device copies of the map side of a _host call
struct car_map_stage {
    int d2, hm, am, fg, rt, rh;
    car_map_stage(sc_stage& st, const car_map& m) {
        const size_t n = (size_t)m.W * m.H, fb = (size_t)m.F * 4;
        d2 = st.in(m.d2, (size_t)m.G * n * 4); hm = st.in(m.hmask, m.hmask ? (size_t)m.G * n : 0); am = st.in(m.amask, (size_t)m.G * n * 2);
        fg = st.in(m.fgrid, m.fgrid ? fb : 0); rt = st.in(m.root, fb); rh = st.in(m.rhead, fb);
    }
    car_map dev(const sc_stage& st, const car_map& m) const {
        car_map d = m;
        d.d2 = car_staged(st, d2, m.d2); d.hmask = car_staged(st, hm, m.hmask); d.amask = car_staged(st, am, m.amask);
        d.fgrid = car_staged(st, fg, m.fgrid); d.root = car_staged(st, rt, m.root); d.rhead = car_staged(st, rh, m.rhead);
        return d;
    }
};

static int car_build_host(sc_ctx* ctx, const car_map& m, int rounds, int32_t* gp, int32_t* fstatus) {
    if (!car_args_ok(ctx, m, gp, nullptr)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const car_map_stage ms(st, m);
    const int o_g = st.out(gp, (size_t)m.F * 8 * m.W * m.H * 4), o_st = st.out(fstatus, fstatus ? (size_t)m.F * 4 : 0);
    int r = st.upload();
    if (r == SC_OK) r = car_build(ctx, ms.dev(st, m), rounds, st.dev<int32_t>(o_g), car_staged(st, o_st, fstatus));
    return st.finish(r);
}

static int car_read_host(sc_ctx* ctx, const car_map& m, const int32_t* gp, const car_query& q) {
    if (!car_args_ok(ctx, m, gp, &q)) return SC_ERR_INVALID;
    if (q.Q == 0) return SC_OK;
    // data contract: every gp value is a cost or SC_FIELD_INF
    const size_t cells = (size_t)m.F * 8 * m.W * m.H;
    for (size_t i = 0; i < cells; ++i)
        if (gp[i] < 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t qb = (size_t)q.Q * 4;
    sc_stage st(ctx);
    const car_map_stage ms(st, m);
    const int i_g = st.in(gp, cells * 4), i_qf = st.in(q.qfield, qb), i_t = st.in(q.target, qb), i_th = st.in(q.thead, qb);
    const int o_p = st.out(q.path, qb * q.Lmax), o_h = st.out(q.head, (size_t)q.Q * q.Lmax), o_len = st.out(q.len, qb), o_c = st.out(q.cost, qb),
              o_s = st.out(q.status, qb);
    int r = st.upload();
    if (r == SC_OK)
        r = car_read(ctx, ms.dev(st, m), st.dev<const int32_t>(i_g),
                     {st.dev<const int32_t>(i_qf), st.dev<const int32_t>(i_t), st.dev<const int32_t>(i_th), q.Q, q.Lmax, q.to_root,
                      st.dev<int32_t>(o_p), st.dev<uint8_t>(o_h), st.dev<int32_t>(o_len), st.dev<int32_t>(o_c), st.dev<int32_t>(o_s)});
    return st.finish(r);
}

static bool arc_args_ok(const sc_ctx* ctx, const int32_t* d2, int W, int H, int batch, int arc_n, const uint16_t* amask) {
    return ctx && d2 && amask && W >= 1 && W <= SC_MAX_DIM && H >= 1 && H <= SC_MAX_DIM && batch >= 1 && arc_n >= 1 && arc_n <= SC_ARC_MAX;
}

extern "C" int sc_arc_mask_u16(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int W, int H, int batch, int32_t r2_clear, int arc_n,
                               uint16_t* amask) {
    if (!arc_args_ok(ctx, d2, W, H, batch, arc_n, amask)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    for (int g0 = 0; g0 < batch; g0 += 65535) {   // the y dimension of a launch holds 65535 grids
        const int gb = batch - g0 < 65535 ? batch - g0 : 65535;
        hipLaunchKernelGGL(arc_mask_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)gb), dim3(256), 0, ctx->stream, d2 + (size_t)g0 * n,
                           hmask ? hmask + (size_t)g0 * n : nullptr, W, H, r2_clear > 1 ? r2_clear : 1, arc_n, amask + (size_t)g0 * n);
    }
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_arc_mask_u16_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int W, int H, int batch, int32_t r2_clear,
                                    int arc_n, uint16_t* amask) {
    if (!arc_args_ok(ctx, d2, W, H, batch, arc_n, amask)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)batch * W * H;
    sc_stage st(ctx);
    const int i_d2 = st.in(d2, n * 4), i_hm = st.in(hmask, hmask ? n : 0), o_m = st.out(amask, n * 2);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_arc_mask_u16(ctx, st.dev<const int32_t>(i_d2), car_staged(st, i_hm, hmask), W, H, batch, r2_clear, arc_n, st.dev<uint16_t>(o_m));
    return st.finish(r);
}

extern "C" int sc_car_field_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, const uint16_t* amask, int G, const int32_t* fgrid,
                                  int W, int H, int32_t r2_clear, int arc_n, int arc_cost, int rev_cost, int toward, const int32_t* root,
                                  const int32_t* rhead, int F, int rounds, int32_t* gp, int32_t* fstatus) {
    return car_build(ctx, {d2, hmask, amask, G, fgrid, W, H, r2_clear, arc_n, arc_cost, rev_cost, toward, root, rhead, F}, rounds, gp, fstatus);
}

extern "C" int sc_car_field_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, const uint16_t* amask, int G,
                                       const int32_t* fgrid, int W, int H, int32_t r2_clear, int arc_n, int arc_cost, int rev_cost, int toward,
                                       const int32_t* root, const int32_t* rhead, int F, int rounds, int32_t* gp, int32_t* fstatus) {
    return car_build_host(ctx, {d2, hmask, amask, G, fgrid, W, H, r2_clear, arc_n, arc_cost, rev_cost, toward, root, rhead, F}, rounds, gp,
                          fstatus);
}

extern "C" int sc_car_paths_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, const uint16_t* amask, int G, const int32_t* fgrid,
                                  int W, int H, int32_t r2_clear, int arc_n, int arc_cost, int rev_cost, int toward, const int32_t* gp,
                                  const int32_t* root, const int32_t* rhead, int F, const int32_t* qfield, const int32_t* target,
                                  const int32_t* thead, int Q, int Lmax, int to_root, int32_t* path, uint8_t* head, int32_t* len,
                                  int32_t* cost, int32_t* status) {
    return car_read(ctx, {d2, hmask, amask, G, fgrid, W, H, r2_clear, arc_n, arc_cost, rev_cost, toward, root, rhead, F}, gp,
                    {qfield, target, thead, Q, Lmax, to_root, path, head, len, cost, status});
}

extern "C" int sc_car_paths_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, const uint16_t* amask, int G,
                                       const int32_t* fgrid, int W, int H, int32_t r2_clear, int arc_n, int arc_cost, int rev_cost, int toward,
                                       const int32_t* gp, const int32_t* root, const int32_t* rhead, int F, const int32_t* qfield,
                                       const int32_t* target, const int32_t* thead, int Q, int Lmax, int to_root, int32_t* path,
                                       uint8_t* head, int32_t* len, int32_t* cost, int32_t* status) {
    return car_read_host(ctx, {d2, hmask, amask, G, fgrid, W, H, r2_clear, arc_n, arc_cost, rev_cost, toward, root, rhead, F}, gp,
                         {qfield, target, thead, Q, Lmax, to_root, path, head, len, cost, status});
}
