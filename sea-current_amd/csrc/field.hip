// field.hip -- cost-to-come fields over the A* graph (sc_cost_field_batch) and path read-out (sc_field_paths_batch).
//
// Graph (the one A* uses, oracle/sc_oracle.h): 8 moves, costs 10 / 14, T(c) <=> d2[c] >= max(r2_clear, 1), a diagonal
// needs both orthogonal side cells traversable, no move leaves the grid.  A field holds the exact optimal cost from its
// root to every cell, SC_FIELD_INF where there is none.  DESIGN.md section 12.
//
// Field kernels.  The grid is cut into 64 x 64 tiles.  A tile visit is one wavefront: lane x holds column x of the tile,
// its 64 g values in registers, and the column's traversability as a 64-bit mask (field_mask_kernel packs them once per
// call).  The visit relaxes the tile to its local fixed point against a one-cell halo with row sweeps, down and up in
// turn: every row takes the moves from the row before it, then a segmented min-plus scan across the lanes closes the row
// (g'[x] = min over its traversable run of g[k] + 10 |x - k|).  It stops after a sweep, not the first, that changed
// nothing.  Changed cells are stored; each of the up to 8 neighbour tiles whose halo holds a changed cell is queued.
//   Chip-wide rounds: `rounds` launches of field_round_kernel, each visiting the queued tiles of every field.  A tile is
//   queued for round r + 1 by raising its stamp to r + 2 (atomicMax: at most one entry per round); round r reads list
//   r % 2 and appends to list (r + 1) % 2.  A visit may read a neighbour's border while that neighbour is rewritten: every
//   value it sees is the cost of a legal path, and the neighbour queues this tile again.  No workgroup waits for another.
//   Finisher: one workgroup per field takes the tiles still queued (stamp == rounds + 1) and runs rounds of its own, its
//   8 wavefronts claiming tiles from an LDS bitmap between barriers, until no tile is queued.  Values only fall and a tile
//   is queued only when a value fell, so it terminates; what it returns is the unique fixed point.
// Read-out: one wavefront per query walks the parent rule from the target, 32 x 32 cells of g at a time in LDS.
//
// Weighted fields (sc_cost_field_weighted_batch, sc_field_paths_weighted_batch): the move into cell
// c costs w_d + min(pen[c], pen_cap).  The same kernels, built a second time with WEIGHTED = true: a visit also holds
// its column's 64 capped penalties, four to a register; every move it relaxes enters one of its own cells, so it needs
// no penalty of a halo cell.  The row closing becomes a min-scan over prefix sums of the entry costs (close_row).  The
// unweighted builds take the `if constexpr` branches they always had.
//
// Multi-source fields (sc_cost_field_multi_batch, sc_field_paths_multi_batch): field f starts from a
// list of seeds, each with a start cost; g[c] = min over its valid seeds s of seed_cost[s] + dist(seed[s], c).  The
// relaxation is the one above: only the init differs (field_fill_kernel + field_seed_kernel: INF, then atomicMin of the
// seed costs; it queues every seed's tile and the neighbour tiles whose halo holds the seed) and a visit's `force`, which
// reads a per-(field, tile) flag the init sets where a tile holds a seed.  The single-root entries are the case of one
// seed of cost 0 per field and run through the same init.
//   Owner pass: a cell is terminal iff a valid seed s sits on it with seed_cost[s] == g; its owner is the smallest such
//   s.  Every other finite cell's owner is that of its parent (the read-out's rule).  owner_claim_kernel: atomicMin of s
//   over the terminal seeds.  owner_parent_kernel: every unclaimed finite cell stores its parent p as -2 - p.
//   owner_jump_kernel, ceil(log2(W H)) launches: a cell that holds -2 - p reads owner[p] (up to OWN_HOPS times): a value
//   >= 0 is its owner, a value <= -2 a farther ancestor.  The stores are in place and unordered: whatever a cell reads is
//   an ancestor of it or its final owner, so the result does not depend on the order.  A launch counts the cells it left
//   unresolved for the next one, which returns at once when that count is 0.
//   Read-out: field_paths_kernel with the end cell seed[owner[target]] in place of the root.
//
// Repair after a map change (sc_cost_field_update_batch and the weighted form): the field of the old
// map becomes that of the new one, bit-equal to a build: a raise pass over the cells that lost their support, then the
// relaxation above seeded at the damage.  Its kernels stand together further down, before the host side.
#include <type_traits>

#include "tile_label.h"   // the wave shuffles
#include "../../include/sea_current_hip_update.h"

namespace {

constexpr int FT = 64;                     // tile edge (= wavefront width: lane = column)
constexpr uint32_t FINF = 0x7FFFFFFFu;     // SC_FIELD_INF; INF + 640 still fits in uint32, so sums need no saturation
constexpr int FIN_WAVES = 8;               // wavefronts of a finisher workgroup
constexpr int FIN_WAVES_W = 4;             // ... of the weighted finisher: its visit needs more than the 256 VGPRs 8 would leave
constexpr int FIN_MAX_TILES = (SC_MAX_DIM / FT) * (SC_MAX_DIM / FT);
constexpr int RP_WIN = 32;                 // read-out window edge
constexpr int RP_WAVES = 4;

struct field_args {
    const uint64_t* mask;    // [G][TY][W] bit y: T(x, ty*64 + y)
    const int32_t* d2;       // [G][H][W]
    const int32_t* fgrid;    // [F] or NULL (G == 1)
    int32_t* g;              // [F][H][W]
    int32_t* ok;             // [F] 1: the field has a valid seed
    int32_t* stamp;          // [F][nt] round + 1 a tile is queued for (grows only)
    int32_t* seeded;         // [F][nt] != 0: the tile holds a valid seed of the field
    int32_t* list[2];        // [F * nt] each: f * nt + tile
    int32_t* ctr;            // [rounds + 1] list length of each round
    int G, W, H, F, TX, TY, nt;
    int32_t thr;
};

struct field_args_w : field_args {
    const uint8_t* pen;      // [G][H][W] entry penalty of every cell
    uint32_t cap;            // pen_cap
};

using tl::shup, tl::shdn, tl::shup64, tl::shdn64;
__device__ __forceinline__ uint32_t rdl(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

// traversability of row y (-1 .. 64) of a column: m = rows 0..63, ex bit 0 = row -1, bit 1 = row 64
__device__ __forceinline__ bool tbit(uint64_t m, uint32_t ex, int y) {
    return y < 0 ? (ex & 1u) != 0 : (y >= FT ? (ex & 2u) != 0 : ((m >> y) & 1ull) != 0);
}

// close row values v across the lanes: segmented min-plus scans left-to-right then right-to-left over runs of traversable
// lanes (tmask = ballot of T in this row).
// WEIGHTED: c = the entry cost 10 + penalty of this lane's cell.  Going right from k to x costs c[k+1] + .. + c[x] =
// S[k] - S[x] with the suffix sums S[x] = c[x+1] + .. + c[63], so g'[x] = min over the run's k <= x of (g[k] + S[k]) - S[x];
// going left costs Q[k] - Q[x] with the prefix sums Q[x] = c[0] + .. + c[x-1].  Both are min-scans with the shuffles of
// the uniform form, and S, Q <= 63 * 265, so INF + S does not wrap.  k = x is in every minimum: a value never rises.
template <bool WEIGHTED>
__device__ __forceinline__ uint32_t close_row(uint32_t v, uint64_t tmask, bool tc, int lane, uint32_t c) {
    const uint64_t blocked = ~tmask;
    const uint64_t below = blocked & ((1ull << lane) - 1ull);
    const int rs = below ? 64 - __clzll((long long)below) : 0;
    const uint64_t above = lane == 63 ? 0ull : (blocked & (~0ull << (lane + 1)));
    const int re = above ? __ffsll((long long)above) - 2 : 63;
    if constexpr (WEIGHTED) {
        uint32_t P = c;                      // inclusive prefix sum of c over the 64 lanes
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t o = shup(P, s);
            if (lane >= s) P += o;
        }
        const uint32_t Q = P - c, S = rdl(P, 63) - P;
        uint32_t u = v + S;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t o = shup(u, s);
            if (tc && lane - s >= rs) u = min(u, o);
        }
        u = u - S + Q;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t o = shdn(u, s);
            if (tc && lane + s <= re) u = min(u, o);
        }
        return u - Q;
    } else {
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t o = shup(v, s) + 10u * s;
            if (tc && lane - s >= rs) v = min(v, o);
        }
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t o = shdn(v, s) + 10u * s;
            if (tc && lane + s <= re) v = min(v, o);
        }
        return v;
    }
}

template <bool WEIGHTED>
struct tile_state {
    uint32_t g[FT];          // column `lane`, rows 0..63
    uint32_t pc[WEIGHTED ? FT / 4 : 1];   // WEIGHTED: the column's capped penalties, row y in byte y % 4 of pc[y / 4]
    uint64_t m, mL, mR;      // T of this column and of the columns to the left / right, rows 0..63
    uint32_t ex, exL, exR;   // the same for rows -1 and 64
    uint32_t gu, gd;         // g of rows -1 and 64 in this column
    uint32_t hla, hlb, hra, hrb;   // g of the halo columns: lane l of *a = row l - 1, lanes 0, 1 of *b = rows 63, 64
    uint64_t chg;            // rows changed in this visit
};

template <bool WT> __device__ __forceinline__ uint32_t HL(const tile_state<WT>& s, int y) { return y + 1 < 64 ? rdl(s.hla, y + 1) : rdl(s.hlb, y - 63); }
template <bool WT> __device__ __forceinline__ uint32_t HR(const tile_state<WT>& s, int y) { return y + 1 < 64 ? rdl(s.hra, y + 1) : rdl(s.hrb, y - 63); }

// one row step of a sweep: row y takes the moves from row yp = y -/+ 1, then closes; returns whether it changed.  Called
// from fully unrolled loops only, so every g index is a constant and the column stays in registers.
// WEIGHTED: every move here enters cell (lane, y), so the cheapest of them pays that cell's penalty once.
template <bool WEIGHTED>
__device__ __forceinline__ bool row_step(tile_state<WEIGHTED>& s, int y, int yp, int lane, bool force) {
    const uint32_t pv = yp < 0 ? s.gu : (yp >= FT ? s.gd : s.g[yp]);
    uint32_t pl = shup(pv, 1), pr = shdn(pv, 1);
    if (lane == 0) pl = HL(s, yp);
    if (lane == 63) pr = HR(s, yp);
    const bool tc = tbit(s.m, s.ex, y), tcp = tbit(s.m, s.ex, yp);
    const bool tl = tbit(s.mL, s.exL, y), tr = tbit(s.mR, s.exR, y);
    const uint32_t old = s.g[y];
    uint32_t v = old;
    uint32_t c = 10u;
    if constexpr (WEIGHTED) {
        const uint32_t p = (s.pc[y >> 2] >> (8 * (y & 3))) & 0xFFu;
        c += p;
        if (tc) {
            uint32_t m = pv + 10u;
            if (tl && tcp) m = min(m, pl + 14u);
            if (tr && tcp) m = min(m, pr + 14u);
            if (lane == 0) m = min(m, HL(s, y) + 10u);
            if (lane == 63) m = min(m, HR(s, y) + 10u);
            v = min(v, m + p);
        }
    } else {
        if (tc) {
            v = min(v, pv + 10u);
            if (tl && tcp) v = min(v, pl + 14u);
            if (tr && tcp) v = min(v, pr + 14u);
            if (lane == 0) v = min(v, HL(s, y) + 10u);
            if (lane == 63) v = min(v, HR(s, y) + 10u);
        }
    }
    if ((__ballot(v < old) != 0ull || force) && __ballot(v < FINF) != 0ull) v = close_row<WEIGHTED>(v, __ballot(tc), tc, lane, c);
    s.g[y] = v;
    if (v < old) s.chg |= 1ull << y;
    return __ballot(v < old) != 0ull;
}

// the weighted row step is past the size at which `#pragma unroll` still unrolls 64 of them, and a loop left standing
// would index g dynamically and send it to scratch: its sweeps unroll by recursion instead
template <int Y, bool DOWN>
__device__ __forceinline__ void sweep_rows_w(tile_state<true>& s, int lane, bool force, bool& c) {
    c |= row_step(s, Y, DOWN ? Y - 1 : Y + 1, lane, force);
    if constexpr (DOWN ? Y + 1 < FT : Y > 0) sweep_rows_w<DOWN ? Y + 1 : Y - 1, DOWN>(s, lane, force, c);
}

template <bool WT>
__device__ __forceinline__ bool sweep(tile_state<WT>& s, bool down, int lane, bool force) {
    bool c = false;
    if constexpr (WT) {
        if (down) sweep_rows_w<0, true>(s, lane, force, c);
        else sweep_rows_w<FT - 1, false>(s, lane, force, c);
    } else if (down) {
#pragma unroll
        for (int y = 0; y < FT; ++y) c |= row_step(s, y, y - 1, lane, force);
    } else {
#pragma unroll
        for (int y = FT - 1; y >= 0; --y) c |= row_step(s, y, y + 1, lane, force);
    }
    return c;
}

// Visit tile (tx, ty) of field f with one wavefront; e = f * nt + ty * TX + tx, its index in stamp and seeded; mark(tx', ty')
// queues a neighbour (called by every lane, uniform).
template <bool WEIGHTED, class Args, class Mark>
__device__ __forceinline__ void visit_tile(const Args& a, int f, int tx, int ty, size_t e, Mark mark) {
    const int lane = threadIdx.x & 63;
    const int W = a.W, H = a.H;
    const int gi = a.fgrid ? a.fgrid[f] : 0;
    const uint64_t* M = a.mask + (size_t)gi * a.TY * W;
    int32_t* G = a.g + (size_t)f * W * H;
    const int x0 = tx * FT, y0 = ty * FT;
    const int tw = min(FT, W - x0), th = min(FT, H - y0);
    const int cx = x0 + lane;
    const bool colin = lane < tw;
    tile_state<WEIGHTED> s;
    s.m = colin ? M[(size_t)ty * W + cx] : 0ull;
    s.ex = 0;
    if (colin && ty > 0) s.ex |= (uint32_t)(M[(size_t)(ty - 1) * W + cx] >> 63);
    if (colin && ty + 1 < a.TY) s.ex |= (uint32_t)(M[(size_t)(ty + 1) * W + cx] & 1ull) << 1;
    // halo columns: lane 0 loads column x0 - 1, lane 63 column x0 + 64
    const int hc = lane == 0 ? x0 - 1 : x0 + FT;
    const bool hv = (lane == 0 || lane == 63) && hc >= 0 && hc < W;
    uint64_t hm = hv ? M[(size_t)ty * W + hc] : 0ull;
    uint32_t hex = 0;
    if (hv && ty > 0) hex |= (uint32_t)(M[(size_t)(ty - 1) * W + hc] >> 63);
    if (hv && ty + 1 < a.TY) hex |= (uint32_t)(M[(size_t)(ty + 1) * W + hc] & 1ull) << 1;
    s.mL = shup64(s.m); s.exL = shup(s.ex, 1);
    s.mR = shdn64(s.m); s.exR = shdn(s.ex, 1);
    if (lane == 0) { s.mL = hm; s.exL = hex; }
    if (lane == 63) { s.mR = hm; s.exR = hex; }
#pragma unroll
    for (int y = 0; y < FT; ++y) s.g[y] = (colin && y < th) ? (uint32_t)G[(size_t)(y0 + y) * W + cx] : FINF;
    s.gu = (colin && y0 > 0) ? (uint32_t)G[(size_t)(y0 - 1) * W + cx] : FINF;
    s.gd = (colin && y0 + FT < H) ? (uint32_t)G[(size_t)(y0 + FT) * W + cx] : FINF;
    {
        const int ra = y0 - 1 + lane, rb = y0 + 63 + lane;
        const bool va = ra >= 0 && ra < H, vb = lane < 2 && rb < H;
        s.hla = (va && x0 > 0) ? (uint32_t)G[(size_t)ra * W + x0 - 1] : FINF;
        s.hra = (va && x0 + FT < W) ? (uint32_t)G[(size_t)ra * W + x0 + FT] : FINF;
        s.hlb = (vb && x0 > 0) ? (uint32_t)G[(size_t)rb * W + x0 - 1] : FINF;
        s.hrb = (vb && x0 + FT < W) ? (uint32_t)G[(size_t)rb * W + x0 + FT] : FINF;
    }
    if constexpr (WEIGHTED) {
        const uint8_t* Pn = a.pen + (size_t)gi * W * H;
#pragma unroll
        for (int k = 0; k < FT / 4; ++k) {
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int y = 4 * k + j;
                const uint32_t b = (colin && y < th) ? min((uint32_t)Pn[(size_t)(y0 + y) * W + cx], a.cap) : 0u;
                w |= b << (8 * j);
            }
            s.pc[k] = w;
        }
    }
    s.chg = 0;
    // a tile that holds a seed starts with rows that are not closed (its cost at the seed, INF beside it): its first sweep
    // closes every row
    const bool force = a.seeded[e] != 0;
    bool down = true;
    for (int n = 0;; ++n) {
        const bool c = sweep(s, down, lane, force && n == 0);
        if (!c && n >= 1) break;
        down = !down;
    }
#pragma unroll
    for (int y = 0; y < FT; ++y)
        if ((s.chg >> y) & 1ull) G[(size_t)(y0 + y) * W + cx] = (int32_t)s.g[y];
    // neighbours whose halo holds a changed cell
    const uint64_t any = __ballot(s.chg != 0ull);
    if (any == 0ull) return;
    const bool top = __ballot(s.chg & 1ull) != 0ull, bot = __ballot((s.chg >> (th - 1)) & 1ull) != 0ull;
    const uint64_t cl = __builtin_amdgcn_readlane((int)(uint32_t)s.chg, 0) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(s.chg >> 32), 0) << 32);
    const uint64_t cr = __builtin_amdgcn_readlane((int)(uint32_t)s.chg, tw - 1) |
                        ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(s.chg >> 32), tw - 1) << 32);
    const bool hasL = tx > 0, hasR = tx + 1 < a.TX, hasU = ty > 0, hasD = ty + 1 < a.TY;
    if (hasU && top) mark(tx, ty - 1);
    if (hasD && bot) mark(tx, ty + 1);
    if (hasL && cl) mark(tx - 1, ty);
    if (hasR && cr) mark(tx + 1, ty);
    if (hasU && hasL && (cl & 1ull)) mark(tx - 1, ty - 1);
    if (hasU && hasR && (cr & 1ull)) mark(tx + 1, ty - 1);
    if (hasD && hasL && ((cl >> (th - 1)) & 1ull)) mark(tx - 1, ty + 1);
    if (hasD && hasR && ((cr >> (th - 1)) & 1ull)) mark(tx + 1, ty + 1);
}

// T of 64 rows per (grid, tile row, column)
__global__ void field_mask_kernel(const int32_t* __restrict__ d2, int G, int W, int H, int TY, int32_t thr, uint64_t* __restrict__ mask) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)G * TY * W) return;
    const int x = (int)(i % W);
    const size_t gt = i / W;
    const int ty = (int)(gt % TY), gi = (int)(gt / TY);
    const int32_t* D = d2 + (size_t)gi * W * H;
    uint64_t m = 0;
    const int y0 = ty * FT, th = min(FT, H - y0);
    for (int y = 0; y < th; ++y) m |= (uint64_t)(D[(size_t)(y0 + y) * W + x] >= thr) << y;
    mask[i] = m;
}

// the seed lists of a call: field f owns seeds off[f] .. off[f + 1] - 1 (off NULL: seed f alone), cost NULL: all 0
struct seed_args {
    const int32_t* seed;
    const int32_t* cost;
    const int32_t* off;
    int n_seed;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void seed_range(const seed_args& sa, int f, int& lo, int& hi) {
    lo = sa.off ? clampi(sa.off[f], 0, sa.n_seed) : clampi(f, 0, sa.n_seed);
    hi = sa.off ? clampi(sa.off[f + 1], 0, sa.n_seed) : clampi(f + 1, 0, sa.n_seed);
}

// seed s of a field on grid gi (in range) is valid; c = its cell, sc = its cost
__device__ __forceinline__ bool seed_ok(const seed_args& sa, const int32_t* d2, int gi, long long n, int32_t thr, int s, int& c, int32_t& sc) {
    c = sa.seed[s];
    sc = sa.cost ? sa.cost[s] : 0;
    return c >= 0 && c < n && sc >= 0 && sc <= SC_FIELD_SEED_COST_MAX && d2[(size_t)gi * n + c] >= thr;
}

// g = INF everywhere; grid (blocks, fields), fields strided.  Block 0 of a field writes "no valid seed" into its ok flag and status.
__global__ void field_fill_kernel(field_args a, int32_t* fstatus) {
    const size_t n = (size_t)a.W * a.H;
    for (int f = blockIdx.y; f < a.F; f += gridDim.y) {
        int32_t* G = a.g + (size_t)f * n;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) G[i] = (int32_t)FINF;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.ok[f] = 0;
            if (fstatus) fstatus[f] = SC_Q_BAD_ENDPOINT;
        }
    }
}

// One block per field (strided), one thread per seed (strided): a valid seed lowers g at its cell to its cost, marks the
// field ok and its tile seeded, and queues for round 0 (stamp 1, at most once per tile) its tile and every neighbour tile
// whose one-cell halo holds the seed.  The neighbours are needed: the seed's value does not change in its tile's first
// visit, so when nothing else in the tile changes, that visit marks no neighbour.
__global__ void field_seed_kernel(field_args a, seed_args sa, int32_t* fstatus) {
    const long long n = (long long)a.W * a.H;
    for (int f = blockIdx.x; f < a.F; f += gridDim.x) {
        const int gi = a.fgrid ? a.fgrid[f] : 0;
        if (gi < 0 || gi >= a.G) continue;
        int lo, hi;
        seed_range(sa, f, lo, hi);
        for (int s = lo + (int)threadIdx.x; s < hi; s += blockDim.x) {
            int c;
            int32_t sc;
            if (!seed_ok(sa, a.d2, gi, n, a.thr, s, c, sc)) continue;
            atomicMin(a.g + (size_t)f * n + c, sc);
            a.ok[f] = 1;
            if (fstatus) fstatus[f] = SC_Q_OK;
            const int x = c % a.W, y = c / a.W, tx = x / FT, ty = y / FT, lx = x % FT, ly = y % FT;
            a.seeded[(size_t)f * a.nt + ty * a.TX + tx] = 1;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int ux = tx + dx, uy = ty + dy;
                    if (ux < 0 || uy < 0 || ux >= a.TX || uy >= a.TY) continue;
                    if ((dx < 0 && lx != 0) || (dx > 0 && lx != FT - 1) || (dy < 0 && ly != 0) || (dy > 0 && ly != FT - 1)) continue;
                    const int u = f * a.nt + uy * a.TX + ux;
                    if (atomicMax(a.stamp + u, 1) < 1) a.list[0][atomicAdd(a.ctr, 1)] = u;
                }
        }
    }
}

// chip-wide round r: one wavefront per queued (field, tile), grid-stride over the list
template <bool WEIGHTED>
__global__ __launch_bounds__(64) void field_round_kernel(std::conditional_t<WEIGHTED, field_args_w, field_args> a, int r) {
    const int n = a.ctr[r];
    const int32_t* cur = a.list[r & 1];
    int32_t* nxt = a.list[(r + 1) & 1];
    int32_t* nctr = a.ctr + r + 1;
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int e = cur[i];
        const int f = e / a.nt, t = e % a.nt;
        visit_tile<WEIGHTED>(a, f, t % a.TX, t / a.TX, (size_t)e, [&](int ux, int uy) {
            if (lane == 0) {
                const int u = f * a.nt + uy * a.TX + ux;
                if (atomicMax(a.stamp + u, r + 2) < r + 2) nxt[atomicAdd(nctr, 1)] = u;
            }
        });
    }
}

// finisher: one workgroup per field completes the tiles still queued after `rounds` chip-wide rounds
template <bool WEIGHTED, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void field_finish_kernel(std::conditional_t<WEIGHTED, field_args_w, field_args> a, int rounds) {
    __shared__ uint32_t dirty[FIN_MAX_TILES / 32];
    __shared__ uint16_t work[FIN_MAX_TILES];
    __shared__ int count;
    const int f = blockIdx.x;
    if (!a.ok[f]) return;
    const int nt = a.nt, nw = (nt + 31) / 32;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int w = tid; w < nw; w += blockDim.x) {
        uint32_t b = 0;
        for (int k = 0; k < 32 && w * 32 + k < nt; ++k) b |= (uint32_t)(a.stamp[(size_t)f * nt + w * 32 + k] == rounds + 1) << k;
        dirty[w] = b;
    }
    __syncthreads();
    for (;;) {
        if (tid == 0) count = 0;
        __syncthreads();
        for (int w = tid; w < nw; w += blockDim.x) {
            uint32_t b = dirty[w];
            if (b) {
                dirty[w] = 0;
                int p = atomicAdd(&count, __popc(b));
                while (b) {
                    const int k = __ffs(b) - 1;
                    b &= b - 1;
                    work[p++] = (uint16_t)(w * 32 + k);
                }
            }
        }
        __syncthreads();
        const int n = count;
        if (n == 0) break;
        // the wave index and the tile are the same in every lane: said outright, the tile's addresses are scalar
        for (int i = __builtin_amdgcn_readfirstlane(wave); i < n; i += WAVES) {
            const int t = __builtin_amdgcn_readfirstlane((int)work[i]);
            visit_tile<WEIGHTED>(a, f, t % a.TX, t / a.TX, (size_t)f * nt + t, [&](int ux, int uy) {
                if (lane == 0) {
                    const int u = uy * a.TX + ux;
                    atomicOr(&dirty[u >> 5], 1u << (u & 31));
                }
            });
        }
        __syncthreads();
    }
}

// ---- owner pass ----------------------------------------------------------------------------------------------------
constexpr int OWN_HOPS = 4;                // ancestors a cell follows per jump launch
constexpr int32_t OWN_FREE = 0x7F7F7F7F;   // what the memset before owner_claim_kernel leaves: no seed has claimed the cell

__constant__ int RP_DX[8] = {1, -1, 0, 0, 1, -1, 1, -1};
__constant__ int RP_DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};

struct owner_args {
    const int32_t* d2;
    const uint8_t* pen;      // NULL: unweighted
    const int32_t* fgrid;
    const int32_t* g;
    int32_t* owner;          // [F][H][W]
    int32_t* left;           // [jumps + 1] cells without an owner before jump launch k
    int G, W, H, F;
    int32_t thr;
    uint32_t cap;
};

// terminal seeds claim their cell: the smallest valid s with seed_cost[s] == g[seed[s]]
__global__ void owner_claim_kernel(owner_args a, seed_args sa) {
    const long long n = (long long)a.W * a.H;
    for (int f = blockIdx.x; f < a.F; f += gridDim.x) {
        const int gi = a.fgrid ? a.fgrid[f] : 0;
        if (gi < 0 || gi >= a.G) continue;
        int lo, hi;
        seed_range(sa, f, lo, hi);
        for (int s = lo + (int)threadIdx.x; s < hi; s += blockDim.x) {
            int c;
            int32_t sc;
            if (seed_ok(sa, a.d2, gi, n, a.thr, s, c, sc) && a.g[(size_t)f * n + c] == sc) atomicMin(a.owner + (size_t)f * n + c, s);
        }
    }
}

// every cell no seed claimed: -1 where g is INF, else -2 - p with p its parent by the read-out's rule, decided from g alone
// (the side cells of a diagonal: reachable <=> traversable next to a reachable cell)
__global__ void owner_parent_kernel(owner_args a) {
    const int W = a.W, H = a.H;
    const size_t n = (size_t)W * H, total = n * a.F;
    int open = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        if (a.owner[i] != OWN_FREE) continue;
        const int f = (int)(i / n), c = (int)(i % n);
        const int32_t* G = a.g + (size_t)f * n;
        const uint32_t gc = (uint32_t)G[c];
        int32_t o = -1;
        const int gi = a.fgrid ? a.fgrid[f] : 0;
        if (gc < FINF && gi >= 0 && gi < a.G) {
            const uint32_t pc = a.pen ? min((uint32_t)a.pen[(size_t)gi * n + c], a.cap) : 0u;
            const int cx = c % W, cy = c / W;
            for (int d = 0; d < 8; ++d) {
                const int px = cx - RP_DX[d], py = cy - RP_DY[d];
                if (px < 0 || py < 0 || px >= W || py >= H) continue;
                const uint32_t gp = (uint32_t)G[(size_t)py * W + px];
                if (gp >= FINF || gp + (d < 4 ? 10u : 14u) + pc != gc) continue;
                if (d >= 4 && ((uint32_t)G[(size_t)cy * W + px] >= FINF || (uint32_t)G[(size_t)py * W + cx] >= FINF)) continue;
                o = -2 - (py * W + px);
                break;
            }
        }
        a.owner[i] = o;
        open |= o <= -2;
    }
    if (__syncthreads_or(open) && threadIdx.x == 0) atomicAdd(a.left, 1);
}

// jump launch k: a cell that holds -2 - p takes what its ancestor p holds, up to OWN_HOPS times
__global__ void owner_jump_kernel(owner_args a, int k) {
    if (a.left[k] == 0) return;
    const size_t n = (size_t)a.W * a.H, total = n * a.F;
    int open = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        int32_t v = a.owner[i];
        if (v > -2) continue;
        int32_t* O = a.owner + (i / n) * n;
        for (int h = 0; h < OWN_HOPS && v <= -2; ++h) {
            const long long p = -2ll - v;
            v = p < (long long)n ? __hip_atomic_load(O + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1;
        }
        if (v >= OWN_FREE) v = -1;
        __hip_atomic_store(a.owner + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        open |= v <= -2;
    }
    if (__syncthreads_or(open) && threadIdx.x == 0) atomicAdd(a.left + k + 1, 1);
}

// ---- read-out ------------------------------------------------------------------------------------------------------
struct paths_args {
    const int32_t* d2;
    const int32_t* fgrid;
    const int32_t* g;
    const int32_t* root;     // [F] the end cell of field f; NULL: multi-source, the end cell of a query is seed[owner[target]]
    const int32_t* qfield;
    const int32_t* target;
    int G, W, H, F, Q, Lmax, to_root;
    int32_t thr;
    int32_t *path, *len, *cost, *status;
    const int32_t* owner = nullptr;   // multi-source: [F][H][W]
    const int32_t* seed = nullptr;    // [n_seed]
    int32_t* which = nullptr;         // [Q] or NULL
    int n_seed = 0;
};

struct paths_args_w : paths_args {
    const uint8_t* pen;
    uint32_t cap;
};

// WEIGHTED: a second window holds the capped penalties.  The step into the current cell c cost w_d + penalty(c), so the
// parent test and the cost walked back both add the penalty of c.
template <bool WEIGHTED>
__global__ __launch_bounds__(64 * RP_WAVES) void field_paths_kernel(std::conditional_t<WEIGHTED, paths_args_w, paths_args> a) {
    __shared__ uint32_t win_all[RP_WAVES][RP_WIN * RP_WIN];
    __shared__ uint8_t winp_all[WEIGHTED ? RP_WAVES : 1][WEIGHTED ? RP_WIN * RP_WIN : 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * RP_WAVES + wave;
    if (q >= a.Q) return;
    uint32_t* win = win_all[wave];
    [[maybe_unused]] uint8_t* winp = winp_all[WEIGHTED ? wave : 0];
    const int W = a.W, H = a.H;
    const long long n = (long long)W * H;
    const int fq = a.qfield[q];
    const int gi = (fq >= 0 && fq < a.F) ? (a.fgrid ? a.fgrid[fq] : 0) : -1;
    const bool multi = a.root == nullptr;
    int r = !multi && fq >= 0 && fq < a.F ? a.root[fq] : -1;
    const int t = a.target[q];
    if (lane == 0 && a.which) a.which[q] = -1;
    const bool ok = gi >= 0 && gi < a.G && t >= 0 && t < n && a.d2[(size_t)gi * n + t] >= a.thr &&
                    (multi || (r >= 0 && r < n && a.d2[(size_t)gi * n + r] >= a.thr));
    if (!ok) {
        if (lane == 0) { a.len[q] = 0; a.cost[q] = -1; a.status[q] = SC_Q_BAD_ENDPOINT; }
        return;
    }
    const int32_t* G = a.g + (size_t)fq * n;
    const uint32_t gt = (uint32_t)G[t];
    int own = -1;
    if (multi && gt < FINF) {
        own = a.owner[(size_t)fq * n + t];
        r = own >= 0 && own < a.n_seed ? a.seed[own] : -1;
    }
    if (gt >= FINF || r < 0 || r >= n) {
        if (lane == 0) { a.len[q] = 0; a.cost[q] = -1; a.status[q] = SC_Q_NO_PATH; }
        return;
    }
    int32_t* P = a.path + (size_t)q * a.Lmax;
    const int rx = r % W, ry = r / W;
    int cx = t % W, cy = t / W;
    uint32_t gc = gt;
    long long L = 1;
    if (lane == 0) P[0] = t;
    bool fail = false;
    while (!(cx == rx && cy == ry)) {
        // window placed so that the walk, which heads for the root, has room in the root's direction
        const int ox = cx - (rx < cx ? RP_WIN - 3 : (rx > cx ? 2 : RP_WIN / 2));
        const int oy = cy - (ry < cy ? RP_WIN - 3 : (ry > cy ? 2 : RP_WIN / 2));
#pragma unroll
        for (int k = 0; k < RP_WIN * RP_WIN / 64; ++k) {
            const int i = k * 64 + lane, wx = ox + (i % RP_WIN), wy = oy + (i / RP_WIN);
            win[i] = (wx >= 0 && wx < W && wy >= 0 && wy < H) ? (uint32_t)G[(size_t)wy * W + wx] : FINF;
            if constexpr (WEIGHTED)
                winp[i] = (wx >= 0 && wx < W && wy >= 0 && wy < H)
                              ? (uint8_t)min((uint32_t)a.pen[(size_t)gi * n + (size_t)wy * W + wx], a.cap) : (uint8_t)0;
        }
        wave_lds_sync();
        // parent rule inside the window (c and its 8 neighbours must lie in it)
        while (!(cx == rx && cy == ry) && cx - ox >= 1 && cx - ox <= RP_WIN - 2 && cy - oy >= 1 && cy - oy <= RP_WIN - 2) {
            const int lx = cx - ox, ly = cy - oy;
            [[maybe_unused]] uint32_t pc = 0;
            if constexpr (WEIGHTED) pc = winp[ly * RP_WIN + lx];
            int d = 0;
            for (; d < 8; ++d) {
                const int px = cx - RP_DX[d], py = cy - RP_DY[d];
                if (px < 0 || py < 0 || px >= W || py >= H) continue;
                const uint32_t gp = win[(ly - RP_DY[d]) * RP_WIN + lx - RP_DX[d]];
                if constexpr (WEIGHTED) {
                    if (gp >= FINF || gp + (d < 4 ? 10u : 14u) + pc != gc) continue;
                } else {
                    if (gp >= FINF || gp + (d < 4 ? 10u : 14u) != gc) continue;
                }
                // side cells of a diagonal: reachable <=> traversable next to a reachable cell
                if (d >= 4 && (win[ly * RP_WIN + lx - RP_DX[d]] >= FINF || win[(ly - RP_DY[d]) * RP_WIN + lx] >= FINF)) continue;
                break;
            }
            if (d == 8 || L >= n) { fail = true; break; }
            cx -= RP_DX[d]; cy -= RP_DY[d];
            gc -= d < 4 ? 10u : 14u;
            if constexpr (WEIGHTED) gc -= pc;
            if (lane == 0 && L < a.Lmax) P[L] = cy * W + cx;
            ++L;
        }
        wave_lds_sync();
        if (fail) break;
    }
    if (fail) {
        if (lane == 0) { a.len[q] = 0; a.cost[q] = -1; a.status[q] = SC_Q_NO_PATH; }
        return;
    }
    const int Li = (int)L;
    if (Li <= a.Lmax && !a.to_root) {
        __threadfence_block();   // lane 0 wrote the walk; every lane reverses it
        for (int i = lane; i < Li / 2; i += 64) {
            const int32_t u = P[i], v = P[Li - 1 - i];
            P[i] = v;
            P[Li - 1 - i] = u;
        }
    }
    if (lane == 0) {
        a.len[q] = Li; a.cost[q] = (int32_t)gt; a.status[q] = Li <= a.Lmax ? SC_Q_OK : SC_Q_TRUNCATED;
        if (a.which) a.which[q] = own;
    }
}

int field_default_rounds(int TX, int TY) { return 2 * (TX + TY) + 16; }

// ---- repair after a map change (sc_cost_field_update_batch) -----------------------------------
// g holds the field of the old map.  Phases, all on the stream, none reads on the host:
//   masks of both maps; update_diff_kernel: changed cells per grid (count and the tiles whose 66 x 66 window holds one);
//   update_prep_kernel: which fields are alive (grid and root in range, T'(root)), g[root] = 0, fstatus, stats;
//   update_dead_kernel: a field that is not alive becomes all INF (its finite cells are its U);
//   update_queue_kernel: every (alive field, flagged tile) is queued for the raise and marked for the relaxation;
//   raise: raise_tile visits under the stamp / two-list / rounds / finisher scheme of the relaxation, with lists of its own;
//   update_seed_kernel: the marked tiles become list 0 of the relaxation, which then runs as in a build.
// raise_tile: one wavefront, the tile and its one-cell halo in a 66 x 66 LDS window of g with bit 31 set where the cell is
// not traversable in the new map (so `w < FINF` reads "finite and traversable").  A finite cell with no tight legal
// finite predecessor becomes INF.  Sweeps in four directions in turn -- rows downwards and upwards (lane = column), columns
// rightwards and leftwards (lane = row) -- each testing every cell once, so an invalidation that runs through the tile
// in any direction is carried across it by one sweep; the visit ends with the first sweep that raises nothing (every
// cell was then tested against the final state).  In place this is sound: a cell is raised only when every tight
// predecessor already is, and a value it reads from a neighbour tile is the old one or INF.  Values only rise: it
// terminates.  Rows of the window are RS = 67 words apart: a row and a column of it each fall into 64 different banks.
constexpr int RW = FT + 2;                 // window edge
constexpr int RS = RW + 1;                 // words between its rows
constexpr uint32_t RBLK = 0x80000000u;     // window word: not traversable in the new map, or off the grid
constexpr int RAISE_FIN_WAVES = 4;         // wavefronts of the raise finisher: 4 windows of 17 KiB (+ 4 KiB penalties) beside its tile lists

struct update_args {
    const uint64_t* mask_old;  // [G][TY][W] of the old map (a.mask: the new one)
    const uint8_t* pen_old;    // weighted: [G][H][W] (a.pen: the new one)
    const int32_t* root;       // [F]
    int32_t* stats;            // [F][2] or NULL
    int32_t* gflag;            // [G][nt] != 0: the tile's window holds a changed cell
    int32_t* gcount;           // [G] changed cells
    int32_t* rstamp;           // [F][nt] raise round + 1 a tile is queued for
    int32_t* rlist[2];         // [F * nt] each
    int32_t* rctr;             // [raise rounds + 1]
};

// one lane per (grid, tile row, column) word
template <bool WEIGHTED>
__global__ void update_diff_kernel(field_args_w a, update_args u) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)a.G * a.TY * a.W) return;
    const int W = a.W, H = a.H;
    const int x = (int)(i % W);
    const size_t gt = i / W;
    const int ty = (int)(gt % a.TY), gi = (int)(gt / a.TY);
    const uint64_t m0 = u.mask_old[i], m1 = a.mask[i];
    uint64_t chg = m0 ^ m1;
    if constexpr (WEIGHTED) {
        if (u.pen_old != a.pen) {
            const uint8_t* P0 = u.pen_old + (size_t)gi * W * H;
            const uint8_t* P1 = a.pen + (size_t)gi * W * H;
            const int y0 = ty * FT, th = min(FT, H - y0);
            const uint64_t both = m0 & m1;
            for (int y = 0; y < th; ++y) {
                const size_t c = (size_t)(y0 + y) * W + x;
                if (((both >> y) & 1ull) && min((uint32_t)P0[c], a.cap) != min((uint32_t)P1[c], a.cap)) chg |= 1ull << y;
            }
        }
    }
    if (chg == 0ull) return;
    atomicAdd(u.gcount + gi, __popcll(chg));
    const int th = min(FT, H - ty * FT);
    const int txa = max(x - 1, 0) / FT, txb = min(x + 1, W - 1) / FT;
    const int tya = (ty > 0 && (chg & 1ull)) ? ty - 1 : ty, tyb = (ty + 1 < a.TY && ((chg >> (th - 1)) & 1ull)) ? ty + 1 : ty;
    for (int vy = tya; vy <= tyb; ++vy)
        for (int vx = txa; vx <= txb; ++vx) u.gflag[(size_t)gi * a.nt + vy * a.TX + vx] = 1;
}

// one thread per field
__global__ void update_prep_kernel(field_args a, update_args u, int32_t* fstatus) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.F) return;
    const long long n = (long long)a.W * a.H;
    const int gi = a.fgrid ? a.fgrid[f] : 0;
    const bool gok = gi >= 0 && gi < a.G;
    const int r = u.root[f];
    const bool alive = gok && r >= 0 && r < n && a.d2[(size_t)gi * n + r] >= a.thr;
    a.ok[f] = alive;
    if (fstatus) fstatus[f] = alive ? SC_Q_OK : SC_Q_BAD_ENDPOINT;
    if (alive) a.g[(size_t)f * n + r] = 0;
    if (u.stats) {
        u.stats[2 * f] = gok ? u.gcount[gi] : 0;
        u.stats[2 * f + 1] = 0;
    }
}

// a field that is not alive: all INF; on a grid in range its finite cells are its U.  Grid (blocks, fields), fields strided.
__global__ void update_dead_kernel(field_args a, update_args u) {
    const size_t n = (size_t)a.W * a.H;
    for (int f = blockIdx.y; f < a.F; f += gridDim.y) {
        if (a.ok[f]) continue;
        const int gi = a.fgrid ? a.fgrid[f] : 0;
        const bool count = u.stats && gi >= 0 && gi < a.G;
        int32_t* G = a.g + (size_t)f * n;
        int c = 0;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
            c += (uint32_t)G[i] < FINF;
            G[i] = (int32_t)FINF;
        }
        if (count && c) atomicAdd(u.stats + 2 * f + 1, c);
    }
}

// one thread per (field, tile)
__global__ void update_queue_kernel(field_args a, update_args u) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)a.F * a.nt) return;
    const int f = (int)(e / a.nt), t = (int)(e % a.nt);
    if (!a.ok[f]) return;
    const int gi = a.fgrid ? a.fgrid[f] : 0;
    if (!u.gflag[(size_t)gi * a.nt + t]) return;
    a.seeded[e] = 1;
    u.rstamp[e] = 1;
    u.rlist[0][atomicAdd(u.rctr, 1)] = (int32_t)e;
}

// after the raise: every marked tile of an alive field is list 0 of the relaxation
__global__ void update_seed_kernel(field_args a) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)a.F * a.nt) return;
    if (!a.ok[e / a.nt] || !a.seeded[e]) return;
    a.stamp[e] = 1;
    a.list[0][atomicAdd(a.ctr, 1)] = (int32_t)e;
}

// Raise visit of tile (tx, ty) of alive field f with one wavefront; win [RW * RS], pw [FT * FT] (WEIGHTED) are the
// wavefront's own LDS.  mark(tx', ty') is called, by every lane, for the tile itself when it raised a cell and for every
// neighbour whose halo holds a raised cell.
template <bool WEIGHTED, class Mark>
__device__ __forceinline__ void raise_tile(const field_args_w& a, const update_args& u, uint32_t* win, uint8_t* pw, int f, int tx, int ty,
                                           Mark mark) {
    const int lane = threadIdx.x & 63;
    const int W = a.W, H = a.H;
    const size_t n = (size_t)W * H;
    const int gi = a.fgrid ? a.fgrid[f] : 0;
    const int32_t* D = a.d2 + (size_t)gi * n;
    int32_t* G = a.g + (size_t)f * n;
    const int x0 = tx * FT, y0 = ty * FT;
    const int tw = min(FT, W - x0), th = min(FT, H - y0);
    const int r = u.root[f];
    const int rlx = r % W - x0, rly = r / W - y0;
    // row by row: lane l loads window column l, lanes 0 and 1 also columns 64 and 65
    for (int ry = 0; ry < RW; ++ry) {
        const int wy = y0 - 1 + ry;
        for (int rx = lane; rx < RW; rx += 64) {
            const int wx = x0 - 1 + rx;
            uint32_t w = FINF | RBLK;
            if (wx >= 0 && wx < W && wy >= 0 && wy < H) {
                const size_t c = (size_t)wy * W + wx;
                w = min((uint32_t)G[c], FINF);
                if (D[c] < a.thr) w |= RBLK;
            }
            win[ry * RS + rx] = w;
        }
    }
    if constexpr (WEIGHTED) {
        const uint8_t* Pn = a.pen + (size_t)gi * n;
        for (int i = lane; i < FT * FT; i += 64) {
            const int lx = i % FT, ly = i / FT;
            pw[i] = (lx < tw && ly < th) ? (uint8_t)min((uint32_t)Pn[(size_t)(y0 + ly) * W + x0 + lx], a.cap) : (uint8_t)0;
        }
    }
    wave_lds_sync();
    const bool colin = lane < tw;
    bool some = false;   // a cell of the tile has been raised (uniform)
    // the cells that lost traversability
    for (int y = 0; y < th; ++y) {
        const int idx = (y + 1) * RS + lane + 1;
        const uint32_t w = win[idx];
        const bool rz = colin && (w & RBLK) && (w & ~RBLK) < FINF;
        if (rz) win[idx] = FINF | RBLK;
        some |= __ballot(rz) != 0ull;
    }
    wave_lds_sync();
    for (int dir = 0;; dir = (dir + 1) & 3) {
        // dir 0, 1: row s of the tile, downwards / upwards, lane = column; dir 2, 3: column s, rightwards / leftwards, lane = row
        const bool rows = dir < 2;
        const int steps = rows ? th : tw;
        const bool in = lane < (rows ? tw : th);
        bool any = false;
        for (int k = 0; k < steps; ++k) {
            const int s = (dir & 1) ? steps - 1 - k : k;
            const int lx = rows ? lane : s, ly = rows ? s : lane;
            const int idx = (ly + 1) * RS + lx + 1;
            const uint32_t* c = win + idx;
            const uint32_t w = c[0];
            bool rz = false;
            if (in && w < FINF && !(lx == rlx && ly == rly)) {
                uint32_t p = 0;
                if constexpr (WEIGHTED) p = pw[ly * FT + lx];
                const uint32_t t10 = w - 10u - p, t14 = w - 14u - p;   // what a tight predecessor holds (used only where they do not wrap)
                const uint32_t wl = c[-1], wr = c[1], wu = c[-RS], wd = c[RS];
                const bool fl = !(wl & RBLK), fr = !(wr & RBLK), fu = !(wu & RBLK), fd = !(wd & RBLK);
                bool sup = (w >= 10u + p) && (wl == t10 || wr == t10 || wu == t10 || wd == t10);
                if (w >= 14u + p) {
                    sup |= fl && fu && c[-RS - 1] == t14;
                    sup |= fr && fu && c[-RS + 1] == t14;
                    sup |= fl && fd && c[RS - 1] == t14;
                    sup |= fr && fd && c[RS + 1] == t14;
                }
                rz = !sup;
            }
            wave_lds_sync();   // every lane has read before any writes
            if (rz) win[idx] = FINF;
            wave_lds_sync();
            any |= __ballot(rz) != 0ull;
        }
        if (!any) break;
        some = true;
    }
    if (!some) return;
    // the raised cells of this lane's column: finite in g, INF in the window
    uint64_t raised = 0;
    for (int y = 0; y < th; ++y) {
        const size_t c = (size_t)(y0 + y) * W + x0 + lane;
        if (colin && (uint32_t)G[c] < FINF && (win[(y + 1) * RS + lane + 1] & ~RBLK) >= FINF) {
            raised |= 1ull << y;
            G[c] = (int32_t)FINF;
        }
    }
    if (u.stats) {
        int cnt = __popcll(raised);
        for (int s = 32; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
        if (lane == 0) atomicAdd(u.stats + 2 * f + 1, cnt);
    }
    mark(tx, ty);
    const bool top = __ballot(raised & 1ull) != 0ull, bot = __ballot((raised >> (th - 1)) & 1ull) != 0ull;
    const uint64_t cl = __builtin_amdgcn_readlane((int)(uint32_t)raised, 0) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(raised >> 32), 0) << 32);
    const uint64_t cr = __builtin_amdgcn_readlane((int)(uint32_t)raised, tw - 1) |
                        ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(raised >> 32), tw - 1) << 32);
    const bool hasL = tx > 0, hasR = tx + 1 < a.TX, hasU = ty > 0, hasD = ty + 1 < a.TY;
    if (hasU && top) mark(tx, ty - 1);
    if (hasD && bot) mark(tx, ty + 1);
    if (hasL && cl) mark(tx - 1, ty);
    if (hasR && cr) mark(tx + 1, ty);
    if (hasU && hasL && (cl & 1ull)) mark(tx - 1, ty - 1);
    if (hasU && hasR && (cr & 1ull)) mark(tx + 1, ty - 1);
    if (hasD && hasL && ((cl >> (th - 1)) & 1ull)) mark(tx - 1, ty + 1);
    if (hasD && hasR && ((cr >> (th - 1)) & 1ull)) mark(tx + 1, ty + 1);
}

// chip-wide raise round r: one wavefront per queued (field, tile)
template <bool WEIGHTED>
__global__ __launch_bounds__(64) void raise_round_kernel(field_args_w a, update_args u, int r) {
    __shared__ uint32_t win[RW * RS];
    __shared__ uint8_t pw[WEIGHTED ? FT * FT : 1];
    const int n = u.rctr[r];
    const int32_t* cur = u.rlist[r & 1];
    int32_t* nxt = u.rlist[(r + 1) & 1];
    int32_t* nctr = u.rctr + r + 1;
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int e = cur[i];
        const int f = e / a.nt, t = e % a.nt, tx = t % a.TX, ty = t / a.TX;
        raise_tile<WEIGHTED>(a, u, win, pw, f, tx, ty, [&](int ux, int uy) {
            if (lane == 0) {
                const int v = f * a.nt + uy * a.TX + ux;
                a.seeded[v] = 1;
                if ((ux != tx || uy != ty) && atomicMax(u.rstamp + v, r + 2) < r + 2) nxt[atomicAdd(nctr, 1)] = v;
            }
        });
        wave_lds_sync();
    }
}

// raise finisher: one workgroup per field completes the tiles still queued after `rounds` chip-wide raise rounds
template <bool WEIGHTED>
__global__ __launch_bounds__(64 * RAISE_FIN_WAVES) void raise_finish_kernel(field_args_w a, update_args u, int rounds) {
    __shared__ uint32_t win_all[RAISE_FIN_WAVES][RW * RS];
    __shared__ uint8_t pw_all[WEIGHTED ? RAISE_FIN_WAVES : 1][WEIGHTED ? FT * FT : 1];
    __shared__ uint32_t dirty[FIN_MAX_TILES / 32];
    __shared__ uint16_t work[FIN_MAX_TILES];
    __shared__ int count;
    const int f = blockIdx.x;
    if (!a.ok[f]) return;
    const int nt = a.nt, nw = (nt + 31) / 32;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int w = tid; w < nw; w += blockDim.x) {
        uint32_t b = 0;
        for (int k = 0; k < 32 && w * 32 + k < nt; ++k) b |= (uint32_t)(u.rstamp[(size_t)f * nt + w * 32 + k] == rounds + 1) << k;
        dirty[w] = b;
    }
    __syncthreads();
    for (;;) {
        if (tid == 0) count = 0;
        __syncthreads();
        for (int w = tid; w < nw; w += blockDim.x) {
            uint32_t b = dirty[w];
            if (b) {
                dirty[w] = 0;
                int p = atomicAdd(&count, __popc(b));
                while (b) {
                    const int k = __ffs(b) - 1;
                    b &= b - 1;
                    work[p++] = (uint16_t)(w * 32 + k);
                }
            }
        }
        __syncthreads();
        const int n = count;
        if (n == 0) break;
        for (int i = __builtin_amdgcn_readfirstlane(wave); i < n; i += RAISE_FIN_WAVES) {
            const int t = __builtin_amdgcn_readfirstlane((int)work[i]);
            const int tx = t % a.TX, ty = t / a.TX;
            raise_tile<WEIGHTED>(a, u, win_all[wave], pw_all[WEIGHTED ? wave : 0], f, tx, ty, [&](int ux, int uy) {
                if (lane == 0) {
                    const int v = uy * a.TX + ux;
                    a.seeded[(size_t)f * nt + v] = 1;
                    if (ux != tx || uy != ty) atomicOr(&dirty[v >> 5], 1u << (v & 31));
                }
            });
            wave_lds_sync();
        }
        __syncthreads();
    }
}

int raise_default_rounds(int TX, int TY) { return TX + TY + 8; }
constexpr int UPDATE_MAX_ROUNDS = 1 << 16;   // chip-wide launches per phase a repair enqueues at most

}  // namespace

// ---- host side -----------------------------------------------------------------------------------------------------
// The twelve entries (three contracts x build / read-out x device / _host form) pack their arguments and call one of four
// functions: field_build, field_read and their _host stagers.  field_args_ok is the argument contract of all of them.
// The four repair entries (include/sea_current_hip_update.h) go through field_update and its _host stager in the same
// way; field_relax is the round loop a build and a repair share.
enum field_contract { FC_ROOTS, FC_ROOTS_WEIGHTED, FC_MULTI };

// the map side of a call; pen NULL: unweighted (the FC_ROOTS entries pass none)
struct field_map {
    const int32_t* d2;
    const uint8_t* pen;
    int pen_cap, G;
    const int32_t* fgrid;
    int W, H;
    int32_t r2_clear;
    int F;
};

// the query side of a read-out; to_end: write target..end cell; which [Q] or NULL (FC_MULTI)
struct field_query {
    const int32_t* qfield;
    const int32_t* target;
    int Q, Lmax, to_end;
    int32_t *path, *len, *cost, *status, *which;
};

// Where the paths of a field end is a seed_args in every contract: the seed lists (FC_MULTI), or {root, NULL, NULL, F} --
// one seed of cost 0 per field.  q NULL: the call is a build (FC_MULTI: seed_off required), else a read-out (FC_MULTI: owner
// required).  Overflow contract: a simple path enters each of the other W*H - 1 cells at most once, on top of a seed cost
// (FC_MULTI); unweighted it holds at every size up to SC_MAX_DIM^2, so FC_ROOTS has no bound of its own.
static bool field_args_ok(const sc_ctx* ctx, field_contract c, const field_map& m, const seed_args& sa, const int32_t* g,
                          const int32_t* owner, const field_query* q) {
    if (!ctx || !m.d2 || !g || m.G <= 0 || m.F <= 0 || m.W <= 0 || m.H <= 0) return false;
    if (!(m.W <= SC_MAX_DIM && m.H <= SC_MAX_DIM && (m.fgrid || m.G == 1))) return false;
    if (sa.n_seed < 0 || (!sa.seed && sa.n_seed > 0)) return false;
    if (c == FC_ROOTS_WEIGHTED && !m.pen) return false;
    if (m.pen && (m.pen_cap < 0 || m.pen_cap > 255)) return false;
    const long long cap = m.pen ? m.pen_cap : 0, top = c == FC_MULTI ? SC_FIELD_SEED_COST_MAX : 0;
    if ((14 + cap) * ((long long)m.W * m.H - 1) + top > (long long)INT32_MAX - 1) return false;
    if (!q) return c != FC_MULTI || sa.off;
    return (c != FC_MULTI || owner) && q->qfield && q->target && q->path && q->len && q->cost && q->status && q->Q >= 0 && q->Lmax > 0;
}

// the compute units of the context's device, asked once
static int field_cu_count(sc_ctx* ctx) {
    if (ctx->cu_count) return SC_OK;
    int cu = 0;
    SC_HIP(ctx, hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
    ctx->cu_count = cu > 0 ? cu : 1;
    return SC_OK;
}

// the jump launches of the owner pass: ceil(log2(W H))
static int owner_jumps(int W, int H) {
    int k = 0;
    while ((1ll << k) < (long long)W * H) ++k;
    return k;
}

// the relaxation of a build or a repair: `rounds` chip-wide launches over the queued tiles (list 0 is filled), then the
// finisher; a.pen NULL: the unweighted kernels
static void field_relax(sc_ctx* ctx, const field_args_w& a, int rounds) {
    if (rounds > 0) {
        const long long cap = (long long)ctx->cu_count * 8;
        const unsigned blocks = (unsigned)((long long)a.F * a.nt < cap ? (long long)a.F * a.nt : cap);
        for (int k = 0; k < rounds; ++k) {
            if (a.pen) hipLaunchKernelGGL(field_round_kernel<true>, dim3(blocks), dim3(64), 0, ctx->stream, a, k);
            else hipLaunchKernelGGL(field_round_kernel<false>, dim3(blocks), dim3(64), 0, ctx->stream, (field_args)a, k);
        }
    }
    if (a.pen) hipLaunchKernelGGL((field_finish_kernel<true, FIN_WAVES_W>), dim3(a.F), dim3(64 * FIN_WAVES_W), 0, ctx->stream, a, rounds);
    else hipLaunchKernelGGL((field_finish_kernel<false, FIN_WAVES>), dim3(a.F), dim3(64 * FIN_WAVES), 0, ctx->stream, (field_args)a, rounds);
}

// every build; m.pen NULL: the unweighted kernels.  owner != NULL: the owner pass follows.
static int field_build(sc_ctx* ctx, field_contract c, const field_map& m, const seed_args& sa, int rounds, int32_t* g, int32_t* owner,
                       int32_t* fstatus) {
    if (!field_args_ok(ctx, c, m, sa, g, owner, nullptr)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const int G = m.G, W = m.W, H = m.H, F = m.F;
    const int TX = (W + FT - 1) / FT, TY = (H + FT - 1) / FT, nt = TX * TY;
    if ((long long)F * nt > 0x7FFFFFFF / 2) return SC_ERR_INVALID;
    if (rounds < 0) rounds = field_default_rounds(TX, TY);
    const int jumps = owner_jumps(W, H);
    const size_t mask_b = (size_t)G * TY * W * 8;
    // stamp and seeded lie next to each other: one memset clears both
    const size_t o_ok = 0, o_stamp = al256((size_t)F * 4), o_seeded = o_stamp + al256((size_t)F * nt * 4),
                 o_l0 = o_seeded + al256((size_t)F * nt * 4), o_l1 = o_l0 + al256((size_t)F * nt * 4), o_ctr = o_l1 + al256((size_t)F * nt * 4),
                 o_left = o_ctr + al256((size_t)(rounds + 1) * 4), total = o_left + al256((size_t)(jumps + 1) * 4);
    int r = sc_scratch_reserve(ctx, &ctx->fld_mask, mask_b);
    if (r == SC_OK) r = sc_scratch_reserve(ctx, &ctx->fld_state, total);
    if (r == SC_OK) r = field_cu_count(ctx);
    if (r != SC_OK) return r;
    char* b = (char*)ctx->fld_state.p;
    field_args_w a;
    a.pen = m.pen; a.cap = (uint32_t)m.pen_cap;
    a.mask = (const uint64_t*)ctx->fld_mask.p; a.d2 = m.d2; a.fgrid = m.fgrid; a.g = g;
    a.ok = (int32_t*)(b + o_ok); a.stamp = (int32_t*)(b + o_stamp); a.seeded = (int32_t*)(b + o_seeded);
    a.list[0] = (int32_t*)(b + o_l0); a.list[1] = (int32_t*)(b + o_l1); a.ctr = (int32_t*)(b + o_ctr);
    a.G = G; a.W = W; a.H = H; a.F = F; a.TX = TX; a.TY = TY; a.nt = nt;
    a.thr = m.r2_clear > 1 ? m.r2_clear : 1;
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    SC_HIP(ctx, hipMemsetAsync(b + o_stamp, 0, o_l0 - o_stamp, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(b + o_ctr, 0, total - o_ctr, ctx->stream));
    {
        const size_t nm = (size_t)G * TY * W;
        hipLaunchKernelGGL(field_mask_kernel, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, ctx->stream, m.d2, G, W, H, TY, a.thr,
                           (uint64_t*)ctx->fld_mask.p);
    }
    {
        const size_t n = (size_t)W * H;
        unsigned bx = (unsigned)((n + 1023) / 1024);
        if (bx > 1024) bx = 1024;
        hipLaunchKernelGGL(field_fill_kernel, dim3(bx, F < 65535 ? F : 65535), dim3(1024), 0, ctx->stream, (field_args)a, fstatus);
        hipLaunchKernelGGL(field_seed_kernel, dim3(F < 65535 ? F : 65535), dim3(64), 0, ctx->stream, (field_args)a, sa, fstatus);
    }
    field_relax(ctx, a, rounds);
    if (owner) {
        const size_t cells = (size_t)F * W * H;
        owner_args oa{m.d2, m.pen, m.fgrid, g, owner, (int32_t*)(b + o_left), G, W, H, F, a.thr, (uint32_t)m.pen_cap};
        const size_t cap = (size_t)ctx->cu_count * 8, need = (cells + 255) / 256;
        const unsigned blocks = (unsigned)(need < cap ? need : cap);
        SC_HIP(ctx, hipMemsetAsync(owner, 0x7F, cells * 4, ctx->stream));
        hipLaunchKernelGGL(owner_claim_kernel, dim3(F < 65535 ? F : 65535), dim3(64), 0, ctx->stream, oa, sa);
        hipLaunchKernelGGL(owner_parent_kernel, dim3(blocks), dim3(256), 0, ctx->stream, oa);
        for (int k = 0; k < jumps; ++k) hipLaunchKernelGGL(owner_jump_kernel, dim3(blocks), dim3(256), 0, ctx->stream, oa, k);
    }
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// every read-out: the end cell of a query is sa.seed[qfield] (the roots), FC_MULTI: sa.seed[owner[target]]
static int field_read(sc_ctx* ctx, field_contract c, const field_map& m, const seed_args& sa, const int32_t* g, const int32_t* owner,
                      const field_query& q) {
    if (!field_args_ok(ctx, c, m, sa, g, owner, &q)) return SC_ERR_INVALID;
    if (q.Q == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const bool multi = c == FC_MULTI;
    paths_args_w a;
    (paths_args&)a = paths_args{m.d2, m.fgrid, g, multi ? nullptr : sa.seed, q.qfield, q.target, m.G, m.W, m.H, m.F, q.Q, q.Lmax,
                                q.to_end ? 1 : 0, m.r2_clear > 1 ? m.r2_clear : 1, q.path, q.len, q.cost, q.status, owner,
                                multi ? sa.seed : nullptr, q.which, multi ? sa.n_seed : 0};
    a.pen = m.pen; a.cap = (uint32_t)m.pen_cap;
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    const dim3 grid((unsigned)((q.Q + RP_WAVES - 1) / RP_WAVES)), block(64 * RP_WAVES);
    if (!m.pen) hipLaunchKernelGGL(field_paths_kernel<false>, grid, block, 0, ctx->stream, (paths_args)a);
    else hipLaunchKernelGGL(field_paths_kernel<true>, grid, block, 0, ctx->stream, a);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// the device copy of a staged array, NULL where the caller passed none
template <class T> static T* staged(const sc_stage& st, int i, T* host) { return host ? st.dev<T>(i) : nullptr; }

// the _host form of every build: the data contract, then field_build on device copies (an absent array: an empty slot)
static int field_build_host(sc_ctx* ctx, field_contract c, const field_map& m, const seed_args& sa, int rounds, int32_t* g,
                            int32_t* owner, int32_t* fstatus) {
    if (!field_args_ok(ctx, c, m, sa, g, owner, nullptr)) return SC_ERR_INVALID;
    // data contract: seed_off non-decreasing within 0 .. n_seed, every seed cost within 0 .. SC_FIELD_SEED_COST_MAX
    for (int f = 0; sa.off && f <= m.F; ++f)
        if (sa.off[f] < 0 || sa.off[f] > sa.n_seed || (f > 0 && sa.off[f] < sa.off[f - 1])) return SC_ERR_INVALID;
    for (int s = 0; sa.cost && s < sa.n_seed; ++s)
        if (sa.cost[s] < 0 || sa.cost[s] > SC_FIELD_SEED_COST_MAX) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)m.W * m.H, fb = (size_t)m.F * 4, sb = (size_t)sa.n_seed * 4;
    sc_stage st(ctx);
    const int i_d2 = st.in(m.d2, (size_t)m.G * n * 4), i_pen = st.in(m.pen, m.pen ? (size_t)m.G * n : 0), i_fg = st.in(m.fgrid, fb),
              i_sd = st.in(sa.seed, sb), i_sc = st.in(sa.cost, sa.cost ? sb : 0), i_so = st.in(sa.off, sa.off ? fb + 4 : 0);
    const int o_g = st.out(g, fb * n), o_ow = st.out(owner, owner ? fb * n : 0), o_st = st.out(fstatus, fb);
    int r = st.upload();
    if (r == SC_OK)
        r = field_build(ctx, c, {staged(st, i_d2, m.d2), staged(st, i_pen, m.pen), m.pen_cap, m.G, staged(st, i_fg, m.fgrid), m.W, m.H, m.r2_clear, m.F},
                        {staged(st, i_sd, sa.seed), staged(st, i_sc, sa.cost), staged(st, i_so, sa.off), sa.n_seed}, rounds, staged(st, o_g, g),
                        staged(st, o_ow, owner), staged(st, o_st, fstatus));
    return st.finish(r);
}

// the repair of single-root fields after a map change: m is the new map, d2_old / pen_old the old one (pen_old with m.pen)
static int field_update(sc_ctx* ctx, field_contract c, const int32_t* d2_old, const uint8_t* pen_old, const field_map& m,
                        const int32_t* root, int rounds, int32_t* g, int32_t* fstatus, int32_t* stats) {
    if (!field_args_ok(ctx, c, m, {root, nullptr, nullptr, m.F}, g, nullptr, nullptr) || !d2_old || (m.pen && !pen_old)) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const int G = m.G, W = m.W, H = m.H, F = m.F;
    const int TX = (W + FT - 1) / FT, TY = (H + FT - 1) / FT, nt = TX * TY;
    if ((long long)F * nt > 0x7FFFFFFF / 2 || (long long)G * nt > 0x7FFFFFFF / 2) return SC_ERR_INVALID;
    if (rounds > UPDATE_MAX_ROUNDS) rounds = UPDATE_MAX_ROUNDS;   // the result does not depend on it; the counters are sized by it
    const int rrounds = rounds < 0 ? raise_default_rounds(TX, TY) : rounds;
    if (rounds < 0) rounds = field_default_rounds(TX, TY);
    const size_t mask_b = (size_t)G * TY * W * 8, ft = al256((size_t)F * nt * 4);
    // stamp | seeded and rstamp .. gcount lie next to each other: one memset clears each run
    const size_t o_ok = 0, o_stamp = al256((size_t)F * 4), o_seeded = o_stamp + ft, o_l0 = o_seeded + ft, o_l1 = o_l0 + ft, o_ctr = o_l1 + ft,
                 o_rstamp = o_ctr + al256((size_t)(rounds + 1) * 4), o_rctr = o_rstamp + ft, o_gflag = o_rctr + al256((size_t)(rrounds + 1) * 4),
                 o_gcount = o_gflag + al256((size_t)G * nt * 4), o_rl0 = o_gcount + al256((size_t)G * 4), o_rl1 = o_rl0 + ft, total = o_rl1 + ft;
    int r = sc_scratch_reserve(ctx, &ctx->fld_mask, mask_b);
    if (r == SC_OK) r = sc_scratch_reserve(ctx, &ctx->fld_mask_old, mask_b);
    if (r == SC_OK) r = sc_scratch_reserve(ctx, &ctx->fld_state, total);
    if (r == SC_OK) r = field_cu_count(ctx);
    if (r != SC_OK) return r;
    char* b = (char*)ctx->fld_state.p;
    field_args_w a;
    a.pen = m.pen; a.cap = (uint32_t)m.pen_cap;
    a.mask = (const uint64_t*)ctx->fld_mask.p; a.d2 = m.d2; a.fgrid = m.fgrid; a.g = g;
    a.ok = (int32_t*)(b + o_ok); a.stamp = (int32_t*)(b + o_stamp); a.seeded = (int32_t*)(b + o_seeded);
    a.list[0] = (int32_t*)(b + o_l0); a.list[1] = (int32_t*)(b + o_l1); a.ctr = (int32_t*)(b + o_ctr);
    a.G = G; a.W = W; a.H = H; a.F = F; a.TX = TX; a.TY = TY; a.nt = nt;
    a.thr = m.r2_clear > 1 ? m.r2_clear : 1;
    update_args u;
    u.mask_old = (const uint64_t*)ctx->fld_mask_old.p; u.pen_old = pen_old; u.root = root; u.stats = stats;
    u.gflag = (int32_t*)(b + o_gflag); u.gcount = (int32_t*)(b + o_gcount); u.rstamp = (int32_t*)(b + o_rstamp);
    u.rlist[0] = (int32_t*)(b + o_rl0); u.rlist[1] = (int32_t*)(b + o_rl1); u.rctr = (int32_t*)(b + o_rctr);
    int tk = sc_time_begin(ctx, SC_K_ASTAR);
    SC_HIP(ctx, hipMemsetAsync(b + o_stamp, 0, o_l0 - o_stamp, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(b + o_ctr, 0, o_rl0 - o_ctr, ctx->stream));
    const size_t nm = (size_t)G * TY * W, ne = (size_t)F * nt;
    const dim3 gm((unsigned)((nm + 255) / 256)), ge((unsigned)((ne + 255) / 256));
    hipLaunchKernelGGL(field_mask_kernel, gm, dim3(256), 0, ctx->stream, m.d2, G, W, H, TY, a.thr, (uint64_t*)ctx->fld_mask.p);
    hipLaunchKernelGGL(field_mask_kernel, gm, dim3(256), 0, ctx->stream, d2_old, G, W, H, TY, a.thr, (uint64_t*)ctx->fld_mask_old.p);
    if (m.pen) hipLaunchKernelGGL(update_diff_kernel<true>, gm, dim3(256), 0, ctx->stream, a, u);
    else hipLaunchKernelGGL(update_diff_kernel<false>, gm, dim3(256), 0, ctx->stream, a, u);
    hipLaunchKernelGGL(update_prep_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, ctx->stream, (field_args)a, u, fstatus);
    {
        const size_t n = (size_t)W * H;
        unsigned bx = (unsigned)((n + 1023) / 1024);
        if (bx > 64) bx = 64;   // rarely more than an early exit per block
        hipLaunchKernelGGL(update_dead_kernel, dim3(bx, F < 65535 ? F : 65535), dim3(1024), 0, ctx->stream, (field_args)a, u);
    }
    hipLaunchKernelGGL(update_queue_kernel, ge, dim3(256), 0, ctx->stream, (field_args)a, u);
    {
        const long long cap = (long long)ctx->cu_count * 8;
        const unsigned blocks = (unsigned)((long long)ne < cap ? (long long)ne : cap);
        for (int k = 0; k < rrounds; ++k) {
            if (m.pen) hipLaunchKernelGGL(raise_round_kernel<true>, dim3(blocks), dim3(64), 0, ctx->stream, a, u, k);
            else hipLaunchKernelGGL(raise_round_kernel<false>, dim3(blocks), dim3(64), 0, ctx->stream, a, u, k);
        }
        if (m.pen) hipLaunchKernelGGL(raise_finish_kernel<true>, dim3(F), dim3(64 * RAISE_FIN_WAVES), 0, ctx->stream, a, u, rrounds);
        else hipLaunchKernelGGL(raise_finish_kernel<false>, dim3(F), dim3(64 * RAISE_FIN_WAVES), 0, ctx->stream, a, u, rrounds);
    }
    hipLaunchKernelGGL(update_seed_kernel, ge, dim3(256), 0, ctx->stream, (field_args)a);
    field_relax(ctx, a, rounds);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// the _host form of the repair: a negative g value is refused, g goes up and comes back
static int field_update_host(sc_ctx* ctx, field_contract c, const int32_t* d2_old, const uint8_t* pen_old, const field_map& m,
                             const int32_t* root, int rounds, int32_t* g, int32_t* fstatus, int32_t* stats) {
    if (!field_args_ok(ctx, c, m, {root, nullptr, nullptr, m.F}, g, nullptr, nullptr) || !d2_old || (m.pen && !pen_old)) return SC_ERR_INVALID;
    const size_t n = (size_t)m.W * m.H, fb = (size_t)m.F * 4;
    for (size_t i = 0; i < (size_t)m.F * n; ++i)
        if (g[i] < 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    sc_stage st(ctx);
    const int i_d0 = st.in(d2_old, (size_t)m.G * n * 4), i_d1 = st.in(m.d2, (size_t)m.G * n * 4), i_p0 = st.in(pen_old, m.pen ? (size_t)m.G * n : 0),
              i_p1 = st.in(m.pen, m.pen ? (size_t)m.G * n : 0), i_fg = st.in(m.fgrid, fb), i_rt = st.in(root, fb), i_g = st.in(g, fb * n);
    st.back(i_g, g, fb * n);
    const int o_st = st.out(fstatus, fb), o_ss = st.out(stats, fb * 2);
    int r = st.upload();
    if (r == SC_OK)
        r = field_update(ctx, c, st.dev<const int32_t>(i_d0), staged(st, i_p0, pen_old),
                         {st.dev<const int32_t>(i_d1), staged(st, i_p1, m.pen), m.pen_cap, m.G, staged(st, i_fg, m.fgrid), m.W, m.H, m.r2_clear, m.F},
                         st.dev<const int32_t>(i_rt), rounds, st.dev<int32_t>(i_g), staged(st, o_st, fstatus), staged(st, o_ss, stats));
    return st.finish(r);
}

// the _host form of every read-out
static int field_read_host(sc_ctx* ctx, field_contract c, const field_map& m, const seed_args& sa, const int32_t* g, const int32_t* owner,
                           const field_query& q) {
    if (!field_args_ok(ctx, c, m, sa, g, owner, &q)) return SC_ERR_INVALID;
    if (q.Q == 0) return SC_OK;
    // data contract: every g value is a cost or SC_FIELD_INF
    const size_t n = (size_t)m.W * m.H;
    for (size_t i = 0; i < (size_t)m.F * n; ++i)
        if (g[i] < 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t fb = (size_t)m.F * 4, qb = (size_t)q.Q * 4;
    sc_stage st(ctx);
    const int i_d2 = st.in(m.d2, (size_t)m.G * n * 4), i_pen = st.in(m.pen, m.pen ? (size_t)m.G * n : 0), i_fg = st.in(m.fgrid, fb),
              i_g = st.in(g, fb * n), i_ow = st.in(owner, owner ? fb * n : 0), i_sd = st.in(sa.seed, (size_t)sa.n_seed * 4),
              i_qf = st.in(q.qfield, qb), i_t = st.in(q.target, qb);
    const int o_p = st.out(q.path, qb * q.Lmax), o_len = st.out(q.len, qb), o_c = st.out(q.cost, qb), o_s = st.out(q.status, qb),
              o_w = st.out(q.which, qb);
    int r = st.upload();
    if (r == SC_OK)
        r = field_read(ctx, c, {staged(st, i_d2, m.d2), staged(st, i_pen, m.pen), m.pen_cap, m.G, staged(st, i_fg, m.fgrid), m.W, m.H, m.r2_clear, m.F},
                       {staged(st, i_sd, sa.seed), nullptr, nullptr, sa.n_seed}, staged(st, i_g, g), staged(st, i_ow, owner),
                       {staged(st, i_qf, q.qfield), staged(st, i_t, q.target), q.Q, q.Lmax, q.to_end, staged(st, o_p, q.path),
                        staged(st, o_len, q.len), staged(st, o_c, q.cost), staged(st, o_s, q.status), staged(st, o_w, q.which)});
    return st.finish(r);
}

// ---- the C ABI: each entry packs {map}, {ends}, [{query}] for its contract
extern "C" int sc_cost_field_batch(sc_ctx* ctx, const int32_t* d2, int G, const int32_t* fgrid, int W, int H, int32_t r2_clear,
                                   const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus) {
    return field_build(ctx, FC_ROOTS, {d2, nullptr, 0, G, fgrid, W, H, r2_clear, F}, {root, nullptr, nullptr, F}, rounds, g, nullptr, fstatus);
}

extern "C" int sc_cost_field_batch_host(sc_ctx* ctx, const int32_t* d2, int G, const int32_t* fgrid, int W, int H, int32_t r2_clear,
                                        const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus) {
    return field_build_host(ctx, FC_ROOTS, {d2, nullptr, 0, G, fgrid, W, H, r2_clear, F}, {root, nullptr, nullptr, F}, rounds, g, nullptr,
                            fstatus);
}

extern "C" int sc_cost_field_weighted_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid,
                                            int W, int H, int32_t r2_clear, const int32_t* root, int F, int rounds, int32_t* g,
                                            int32_t* fstatus) {
    return field_build(ctx, FC_ROOTS_WEIGHTED, {d2, pen, pen_cap, G, fgrid, W, H, r2_clear, F}, {root, nullptr, nullptr, F}, rounds, g, nullptr,
                       fstatus);
}

extern "C" int sc_cost_field_weighted_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid,
                                                 int W, int H, int32_t r2_clear, const int32_t* root, int F, int rounds, int32_t* g,
                                                 int32_t* fstatus) {
    return field_build_host(ctx, FC_ROOTS_WEIGHTED, {d2, pen, pen_cap, G, fgrid, W, H, r2_clear, F}, {root, nullptr, nullptr, F}, rounds, g,
                            nullptr, fstatus);
}

extern "C" int sc_cost_field_multi_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid, int W,
                                         int H, int32_t r2_clear, const int32_t* seed, const int32_t* seed_cost, const int32_t* seed_off,
                                         int n_seed, int F, int rounds, int32_t* g, int32_t* owner, int32_t* fstatus) {
    return field_build(ctx, FC_MULTI, {d2, pen, pen_cap, G, fgrid, W, H, r2_clear, F}, {seed, seed_cost, seed_off, n_seed}, rounds, g, owner,
                       fstatus);
}

extern "C" int sc_cost_field_multi_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid,
                                              int W, int H, int32_t r2_clear, const int32_t* seed, const int32_t* seed_cost,
                                              const int32_t* seed_off, int n_seed, int F, int rounds, int32_t* g, int32_t* owner,
                                              int32_t* fstatus) {
    return field_build_host(ctx, FC_MULTI, {d2, pen, pen_cap, G, fgrid, W, H, r2_clear, F}, {seed, seed_cost, seed_off, n_seed}, rounds, g,
                            owner, fstatus);
}

extern "C" int sc_field_paths_batch(sc_ctx* ctx, const int32_t* d2, int G, const int32_t* fgrid, int W, int H, int32_t r2_clear,
                                    const int32_t* g, const int32_t* root, int F, const int32_t* qfield, const int32_t* target, int Q,
                                    int Lmax, int to_root, int32_t* path, int32_t* len, int32_t* cost, int32_t* status) {
    return field_read(ctx, FC_ROOTS, {d2, nullptr, 0, G, fgrid, W, H, r2_clear, F}, {root, nullptr, nullptr, F}, g, nullptr,
                      {qfield, target, Q, Lmax, to_root, path, len, cost, status, nullptr});
}

extern "C" int sc_field_paths_batch_host(sc_ctx* ctx, const int32_t* d2, int G, const int32_t* fgrid, int W, int H, int32_t r2_clear,
                                         const int32_t* g, const int32_t* root, int F, const int32_t* qfield, const int32_t* target, int Q,
                                         int Lmax, int to_root, int32_t* path, int32_t* len, int32_t* cost, int32_t* status) {
    return field_read_host(ctx, FC_ROOTS, {d2, nullptr, 0, G, fgrid, W, H, r2_clear, F}, {root, nullptr, nullptr, F}, g, nullptr,
                           {qfield, target, Q, Lmax, to_root, path, len, cost, status, nullptr});
}

extern "C" int sc_field_paths_weighted_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid,
                                             int W, int H, int32_t r2_clear, const int32_t* g, const int32_t* root, int F,
                                             const int32_t* qfield, const int32_t* target, int Q, int Lmax, int to_root, int32_t* path,
                                             int32_t* len, int32_t* cost, int32_t* status) {
    return field_read(ctx, FC_ROOTS_WEIGHTED, {d2, pen, pen_cap, G, fgrid, W, H, r2_clear, F}, {root, nullptr, nullptr, F}, g, nullptr,
                      {qfield, target, Q, Lmax, to_root, path, len, cost, status, nullptr});
}

extern "C" int sc_field_paths_weighted_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G,
                                                  const int32_t* fgrid, int W, int H, int32_t r2_clear, const int32_t* g, const int32_t* root,
                                                  int F, const int32_t* qfield, const int32_t* target, int Q, int Lmax, int to_root,
                                                  int32_t* path, int32_t* len, int32_t* cost, int32_t* status) {
    return field_read_host(ctx, FC_ROOTS_WEIGHTED, {d2, pen, pen_cap, G, fgrid, W, H, r2_clear, F}, {root, nullptr, nullptr, F}, g, nullptr,
                           {qfield, target, Q, Lmax, to_root, path, len, cost, status, nullptr});
}

extern "C" int sc_field_paths_multi_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid, int W,
                                          int H, int32_t r2_clear, const int32_t* g, const int32_t* owner, const int32_t* seed, int n_seed,
                                          int F, const int32_t* qfield, const int32_t* target, int Q, int Lmax, int to_seed, int32_t* path,
                                          int32_t* len, int32_t* cost, int32_t* status, int32_t* which) {
    return field_read(ctx, FC_MULTI, {d2, pen, pen_cap, G, fgrid, W, H, r2_clear, F}, {seed, nullptr, nullptr, n_seed}, g, owner,
                      {qfield, target, Q, Lmax, to_seed, path, len, cost, status, which});
}

extern "C" int sc_field_paths_multi_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid,
                                               int W, int H, int32_t r2_clear, const int32_t* g, const int32_t* owner, const int32_t* seed,
                                               int n_seed, int F, const int32_t* qfield, const int32_t* target, int Q, int Lmax, int to_seed,
                                               int32_t* path, int32_t* len, int32_t* cost, int32_t* status, int32_t* which) {
    return field_read_host(ctx, FC_MULTI, {d2, pen, pen_cap, G, fgrid, W, H, r2_clear, F}, {seed, nullptr, nullptr, n_seed}, g, owner,
                           {qfield, target, Q, Lmax, to_seed, path, len, cost, status, which});
}

// ---- repair after a map change (include/sea_current_hip_update.h)
extern "C" int sc_cost_field_update_batch(sc_ctx* ctx, const int32_t* d2_old, const int32_t* d2_new, int G, const int32_t* fgrid, int W, int H,
                                          int32_t r2_clear, const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus,
                                          int32_t* stats) {
    return field_update(ctx, FC_ROOTS, d2_old, nullptr, {d2_new, nullptr, 0, G, fgrid, W, H, r2_clear, F}, root, rounds, g, fstatus, stats);
}

extern "C" int sc_cost_field_update_batch_host(sc_ctx* ctx, const int32_t* d2_old, const int32_t* d2_new, int G, const int32_t* fgrid, int W,
                                               int H, int32_t r2_clear, const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus,
                                               int32_t* stats) {
    return field_update_host(ctx, FC_ROOTS, d2_old, nullptr, {d2_new, nullptr, 0, G, fgrid, W, H, r2_clear, F}, root, rounds, g, fstatus, stats);
}

extern "C" int sc_cost_field_weighted_update_batch(sc_ctx* ctx, const int32_t* d2_old, const uint8_t* pen_old, const int32_t* d2_new,
                                                   const uint8_t* pen_new, int pen_cap, int G, const int32_t* fgrid, int W, int H,
                                                   int32_t r2_clear, const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus,
                                                   int32_t* stats) {
    return field_update(ctx, FC_ROOTS_WEIGHTED, d2_old, pen_old, {d2_new, pen_new, pen_cap, G, fgrid, W, H, r2_clear, F}, root, rounds, g,
                        fstatus, stats);
}

extern "C" int sc_cost_field_weighted_update_batch_host(sc_ctx* ctx, const int32_t* d2_old, const uint8_t* pen_old, const int32_t* d2_new,
                                                        const uint8_t* pen_new, int pen_cap, int G, const int32_t* fgrid, int W, int H,
                                                        int32_t r2_clear, const int32_t* root, int F, int rounds, int32_t* g,
                                                        int32_t* fstatus, int32_t* stats) {
    return field_update_host(ctx, FC_ROOTS_WEIGHTED, d2_old, pen_old, {d2_new, pen_new, pen_cap, G, fgrid, W, H, r2_clear, F}, root, rounds, g,
                             fstatus, stats);
}
