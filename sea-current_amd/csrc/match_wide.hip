// match_wide.hip -- wide-window scan matching: an exact pruned search over a min-pooled pyramid of the cost map
// (sc_scan_match_wide_batch).  DESIGN.md section 26; the definition is in include/sea_current_hip.h.
//
// The search runs level by level on the device; the host only enqueues a fixed sequence of launches (it never learns a list's
// length), all on one stream.  Per call:
//   1. mt_cost_kernel (match_common.h): level 0, the padded cost map of the dense matcher.
//   2. mw_pool_kernel, twice per level: P_2h = the minimum of four cells of P_h at distance h.  Level 4^j is a uint16 map at
//      full resolution over x in -m .. W, y in -m .. H; a coordinate clamped to that range reads the right value.
//   3. mw_init_kernel, one workgroup per (scan, rotation): score(r, 0, 0) into U, the present points, and the first list.
//   4. per level, from the top: mw_bound_kernel, mw_dive_kernel, mw_expand_kernel (the last level: bound only).
//   5. mw_pick_kernel, one workgroup per scan: best, ties and stats.
// A list holds PARENTS: a node of size 4m that survived, with the offset at which the bounds of its (up to 16) children of
// size m lie.  The bound kernel gives a wave four parents, a lane one child: the points of a parent are read once per 16
// lanes (the same address), the 16 pooled cells are 4 rows of 4 cells m apart.  The nodes of the top level are the children
// of parents of size 4 * 4^top that the init kernel lays over the window.  The order of a list is whatever the atomics
// gave; nothing reads it but through minima of keys and sums of counts.
#include "match_common.h"

namespace {

constexpr int MW_LEVELS = SC_MATCH_WIDE_MAX_TOP + 1;
constexpr int MW_CNT = 16;       // int32 per scan: [0..5] nodes of level j, [6..11] parents whose children they are, [12] n_dive, [13] present points
constexpr int MW_NPAR = 6, MW_NDIVE = 12, MW_NPRES = 13;
constexpr int MW_U = 8;          // int32 per scan: [j] = U at the start of level j
constexpr int MW_MAX_BLOCKS = 2048, MW_MAX_G = 256;   // workgroups of a list kernel, and of one scan in it
constexpr unsigned long long MW_NONE = ~0ull;

struct mw_pyr { const uint16_t* lv[MW_LEVELS]; };

// a parent: off << 34 | r << 26 | dyi << 13 | dxi, (dxi, dyi) = its origin + (wx, wy) in 0 .. 4096, off < 2^27
__device__ __forceinline__ unsigned long long mw_pack(unsigned off, int r, int dyi, int dxi) {
    return (unsigned long long)off << 34 | (unsigned long long)r << 26 | (unsigned)dyi << 13 | (unsigned)dxi;
}
// children of size q a node at index i (origin + half window) has along one axis: those that begin inside the window 2w
__device__ __forceinline__ int mw_kids(int i, int q, int w2) { return min(4, (w2 - i) / q + 1); }
// a node's key among its rotation's: B << 26 | dyi << 13 | dxi, the order (B, dy0, dx0)
__device__ __forceinline__ unsigned long long mw_nkey(uint32_t B, int dyi, int dxi) {
    return (unsigned long long)B << 26 | (unsigned)dyi << 13 | (unsigned)dxi;
}

// one cell of P_m at (x, y), clamped to the level's range
__device__ __forceinline__ uint32_t mw_cell(const uint16_t* __restrict__ lv, int x, int y, int m, int W, int H) {
    const int xi = min(max(x, -m), W) + m, yi = min(max(y, -m), H) + m;   // [0, W + m], [0, H + m]
    return lv[yi * (W + m + 1) + xi];                                       // (8192 + 1025)^2 < 2^27
}

// dst = P_2h over x, y in -dm .. W / H from src = P_h over -sm ..: one thread per cell, a row per blockIdx.y
__global__ __launch_bounds__(256) void mw_pool_kernel(const uint16_t* __restrict__ src, int sm, uint16_t* __restrict__ dst, int dm, int h, int W,
                                                      int H) {
    const int xi = blockIdx.x * 256 + threadIdx.x, yi = blockIdx.y, Wd = W + dm + 1;
    if (xi >= Wd) return;
    const int x = xi - dm, y = yi - dm;
    const uint32_t a = mw_cell(src, x, y, sm, W, H), b = mw_cell(src, x + h, y, sm, W, H), c = mw_cell(src, x, y + h, sm, W, H),
                   d = mw_cell(src, x + h, y + h, sm, W, H);
    dst[yi * Wd + xi] = (uint16_t)min(min(a, b), min(c, d));
}

__device__ __forceinline__ bool mw_live(const int32_t* __restrict__ centre, const int32_t* __restrict__ cnt, int s) {
    return mt_centre_ok(centre[2 * s]) && mt_centre_ok(centre[2 * s + 1]) && cnt[s * MW_CNT + MW_NPRES] > 0;
}

__global__ __launch_bounds__(256) void mw_init_kernel(const uint16_t* __restrict__ cost, const int32_t* __restrict__ pts,
                                                      const int32_t* __restrict__ centre, int R, int N, int W, int H, int wx, int wy, int top,
                                                      int max_nodes, int32_t* __restrict__ cnt, int32_t* __restrict__ U,
                                                      unsigned long long* __restrict__ list) {
    __shared__ uint32_t red[2][4];
    const int s = blockIdx.x / R, r = blockIdx.x % R, tid = threadIdx.x;
    const int cx = centre[2 * s], cy = centre[2 * s + 1];
    if (!mt_centre_ok(cx) || !mt_centre_ok(cy)) return;
    const int32_t* __restrict__ p = pts + ((size_t)s * R + r) * (size_t)N * 2;
    uint32_t sum = 0, present = 0;   // a sum is at most 32767 * 65536 < 2^31
    for (int k = tid; k < N; k += 256) {
        const int px = p[2 * k], py = p[2 * k + 1];
        if (mt_absent(px) || mt_absent(py)) continue;
        sum += mw_cell(cost, cx + px, cy + py, 1, W, H);
        ++present;
    }
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d);
        present += __shfl_xor(present, d);
    }
    if ((tid & 63) == 0) red[0][tid >> 6] = sum, red[1][tid >> 6] = present;
    __syncthreads();
    if (tid == 0) {
        atomicMin(&U[s * MW_U + top], (int32_t)(red[0][0] + red[0][1] + red[0][2] + red[0][3]));
        atomicAdd(&cnt[s * MW_CNT + MW_NPRES], (int32_t)(red[1][0] + red[1][1] + red[1][2] + red[1][3]));
    }
    // the parents of size 4m whose children are the top nodes: nx * ny nodes per rotation, nX * nY parents
    const int m = 1 << (2 * top), nx = 2 * wx / m + 1, ny = 2 * wy / m + 1, nX = (nx + 3) / 4, nY = (ny + 3) / 4;
    unsigned long long* __restrict__ mine = list + (size_t)s * max_nodes + (size_t)r * nX * nY;   // R nX nY <= R nx ny <= max_nodes
    for (int i = tid; i < nX * nY; i += 256) {
        const int I = i % nX, J = i / nX, ky = min(4, ny - 4 * J);
        mine[i] = mw_pack((unsigned)(r * nx * ny + 4 * J * nx + ky * 4 * I), r, J * 4 * m, I * 4 * m);
    }
    if (r == 0 && tid == 0) {
        cnt[s * MW_CNT + top] = R * nx * ny;
        cnt[s * MW_CNT + MW_NPAR + top] = R * nX * nY;
    }
}

// The nodes of level j (size m = 4^j): a wave takes four parents of list, a lane one child.
__global__ __launch_bounds__(256) void mw_bound_kernel(const uint16_t* __restrict__ lv, const int32_t* __restrict__ pts,
                                                       const int32_t* __restrict__ centre, int R, int N, int W, int H, int wx, int wy, int j,
                                                       int max_nodes, int G, const int32_t* __restrict__ cnt, int32_t* __restrict__ U,
                                                       const unsigned long long* __restrict__ list, int32_t* __restrict__ bnd,
                                                       unsigned long long* __restrict__ keys) {
    const int s = blockIdx.x / G, g = blockIdx.x % G, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (j > 0 && g == 0 && tid == 0) U[s * MW_U + j - 1] = U[s * MW_U + j];   // the dives of this level lower the copy
    if (!mw_live(centre, cnt, s) || cnt[s * MW_CNT + j] > max_nodes) return;
    const int np = cnt[s * MW_CNT + MW_NPAR + j], m = 1 << (2 * j), a = lane & 3, b = (lane >> 2) & 3;
    const int cx = centre[2 * s], cy = centre[2 * s + 1];
    const unsigned long long* __restrict__ ls = list + (size_t)s * max_nodes;
    int32_t* __restrict__ bs = bnd + (size_t)s * max_nodes;
    for (int base = (g * 4 + wave) * 4; base < np; base += G * 16) {
        const int pi = base + (lane >> 4);
        const bool has = pi < np;
        const unsigned long long e = has ? ls[pi] : 0;
        const int pdx = (int)(e & 0x1fff), pdy = (int)(e >> 13) & 0x1fff, r = (int)(e >> 26) & 0xff;
        const unsigned off = (unsigned)(e >> 34);
        const int kx = mw_kids(pdx, m, 2 * wx), ky = mw_kids(pdy, m, 2 * wy);
        const bool valid = has && a < kx && b < ky;
        const int dxi = pdx + a * m, dyi = pdy + b * m;
        // |cx + dx0 + px| <= 8192 + 2 * 16384 + 2 * 2048 + 3 * 1024: far inside int32
        const int bx = cx + dxi - wx, by = cy + dyi - wy;
        const int32_t* __restrict__ p = pts + ((size_t)s * R + r) * (size_t)N * 2;
        uint32_t sum = 0;
        for (int k0 = 0; k0 < N; k0 += 4) {
            uint32_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = min(k0 + u, N - 1);
                const int px = p[2 * k], py = p[2 * k + 1];
                const bool present = k0 + u < N && !mt_absent(px) && !mt_absent(py);
                v[u] = mw_cell(lv, present ? bx + px : 0, present ? by + py : 0, m, W, H);   // always a load inside the level
                v[u] = present ? v[u] : 0;
            }
            sum += v[0] + v[1] + v[2] + v[3];
        }
        if (valid) bs[off + b * kx + a] = (int32_t)sum;   // off + kx ky <= the level's nodes <= max_nodes
        unsigned long long key = valid ? mw_nkey(sum, dyi, dxi) : MW_NONE;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) key = min(key, (unsigned long long)__shfl_xor((long long)key, d));
        if (keys && has && (lane & 15) == 0) atomicMin(&keys[(size_t)s * R + r], key);   // level 0 has no dives
    }
}

// One dive per (scan, rotation) from the rotation's smallest node of level j down to a candidate: 16 children a round, the
// workgroup's 16 slices of 16 lanes share the points.
__global__ __launch_bounds__(256) void mw_dive_kernel(mw_pyr pyr, const int32_t* __restrict__ pts, const int32_t* __restrict__ centre, int R,
                                                      int N, int W, int H, int wx, int wy, int j, int max_nodes, int32_t* __restrict__ cnt,
                                                      int32_t* __restrict__ U, unsigned long long* __restrict__ keys) {
    __shared__ uint32_t sums[16][16];
    __shared__ unsigned long long ckey[16], first;
    const int s = blockIdx.x / R, r = blockIdx.x % R, tid = threadIdx.x;
    if (!mw_live(centre, cnt, s) || cnt[s * MW_CNT + j] > max_nodes) return;   // then no bound kernel touched the key
    if (tid == 0) {
        first = keys[(size_t)s * R + r];
        keys[(size_t)s * R + r] = MW_NONE;   // for the next level
    }
    __syncthreads();
    unsigned long long cur = first;
    if (cur == MW_NONE || (int32_t)(cur >> 26) > U[s * MW_U + j]) return;   // no node, or none worth a dive: U of the start of the level
    const int cx = centre[2 * s], cy = centre[2 * s + 1], c = tid & 15, a = c & 3, b = c >> 2, slice = tid >> 4;
    const int32_t* __restrict__ p = pts + ((size_t)s * R + r) * (size_t)N * 2;
    int n_dive = 0;
    for (int jj = j - 1; jj >= 0; --jj) {
        const int q = 1 << (2 * jj), pdx = (int)(cur & 0x1fff), pdy = (int)(cur >> 13) & 0x1fff;
        const int kx = mw_kids(pdx, q, 2 * wx), ky = mw_kids(pdy, q, 2 * wy);
        const int dxi = pdx + a * q, dyi = pdy + b * q, bx = cx + dxi - wx, by = cy + dyi - wy;
        const uint16_t* __restrict__ lv = pyr.lv[jj];
        uint32_t sum = 0;
        for (int k = slice; k < N; k += 16) {
            const int px = p[2 * k], py = p[2 * k + 1];
            if (!mt_absent(px) && !mt_absent(py)) sum += mw_cell(lv, bx + px, by + py, q, W, H);
        }
        sums[slice][c] = sum;
        __syncthreads();
        if (tid < 16) {
            uint32_t t = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) t += sums[i][tid];
            ckey[tid] = a < kx && b < ky ? mw_nkey(t, dyi, dxi) : MW_NONE;
        }
        __syncthreads();
        cur = ckey[0];   // child (0, 0) always exists
#pragma unroll
        for (int i = 1; i < 16; ++i) cur = min(cur, ckey[i]);
        n_dive += kx * ky;
        __syncthreads();
    }
    if (tid == 0) {
        atomicMin(&U[s * MW_U + j - 1], (int32_t)(cur >> 26));
        atomicAdd(&cnt[s * MW_CNT + MW_NDIVE], n_dive);
    }
}

// The nodes of level j with B <= U become the parents of level j - 1: appended with one pair of atomics per wave.
__global__ __launch_bounds__(256) void mw_expand_kernel(const int32_t* __restrict__ centre, int R, int wx, int wy, int j, int max_nodes, int G,
                                                        int32_t* __restrict__ cnt, const int32_t* __restrict__ U,
                                                        const unsigned long long* __restrict__ list, const int32_t* __restrict__ bnd,
                                                        unsigned long long* __restrict__ next) {
    const int s = blockIdx.x / G, g = blockIdx.x % G, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!mw_live(centre, cnt, s) || cnt[s * MW_CNT + j] > max_nodes) return;
    const int np = cnt[s * MW_CNT + MW_NPAR + j], m = 1 << (2 * j), q = m >> 2, a = lane & 3, b = (lane >> 2) & 3;
    const int32_t Us = U[s * MW_U + j - 1];
    const unsigned long long* __restrict__ ls = list + (size_t)s * max_nodes;
    const int32_t* __restrict__ bs = bnd + (size_t)s * max_nodes;
    unsigned long long* __restrict__ ns = next + (size_t)s * max_nodes;
    for (int base = (g * 4 + wave) * 4; base < np; base += G * 16) {
        const int pi = base + (lane >> 4);
        const bool has = pi < np;
        const unsigned long long e = has ? ls[pi] : 0;
        const int pdx = (int)(e & 0x1fff), pdy = (int)(e >> 13) & 0x1fff, r = (int)(e >> 26) & 0xff;
        const unsigned off = (unsigned)(e >> 34);
        const int kx = mw_kids(pdx, m, 2 * wx), ky = mw_kids(pdy, m, 2 * wy);
        const bool valid = has && a < kx && b < ky;
        const int dxi = pdx + a * m, dyi = pdy + b * m;
        const bool surv = valid && bs[off + b * kx + a] <= Us;
        const int kids = surv ? mw_kids(dxi, q, 2 * wx) * mw_kids(dyi, q, 2 * wy) : 0;
        int incl = kids;   // inclusive prefix sum over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const unsigned long long mask = __ballot(surv);
        const int total = __shfl(incl, 63), n_surv = __popcll(mask);
        int obase = 0, pbase = 0;
        if (lane == 0 && n_surv) {
            obase = atomicAdd(&cnt[s * MW_CNT + j - 1], total);           // at most 16 * 2^22 over the level
            pbase = atomicAdd(&cnt[s * MW_CNT + MW_NPAR + j - 1], n_surv);   // survivors <= this level's nodes <= max_nodes
        }
        obase = __shfl(obase, 0), pbase = __shfl(pbase, 0);
        if (surv) ns[pbase + __popcll(mask & ((1ull << lane) - 1))] = mw_pack((unsigned)(obase + incl - kids), r, dyi, dxi);
    }
}

__global__ __launch_bounds__(256) void mw_pick_kernel(const int32_t* __restrict__ pts, const int32_t* __restrict__ centre, int R, int N, int wx,
                                                      int wy, int top, int max_nodes, const int32_t* __restrict__ cnt,
                                                      const int32_t* __restrict__ U, const unsigned long long* __restrict__ list,
                                                      const int32_t* __restrict__ bnd, int32_t* __restrict__ best, int32_t* __restrict__ stats) {
    __shared__ mt_key keys[256];
    __shared__ int acc[2][256];
    const int s = blockIdx.x, tid = threadIdx.x;
    int32_t* out = best + (size_t)s * 6;
    const int32_t* __restrict__ cs = cnt + s * MW_CNT;
    const bool ignored = !mt_centre_ok(centre[2 * s]) || !mt_centre_ok(centre[2 * s + 1]);
    if (ignored || cs[MW_NPRES] == 0) {   // cnt is all zero for an ignored scan
        if (tid < 6) out[tid] = ignored ? (tid == 0 ? SC_MATCH_IGNORED : 0) : (tid == 5 ? R * (2 * wx + 1) * (2 * wy + 1) : 0);
        if (stats && tid < 8) stats[(size_t)s * 8 + tid] = 0;
        return;
    }
    bool over = false;
    for (int l = 0; l <= top; ++l) over |= cs[l] > max_nodes;
    if (stats && tid < 8)
        stats[(size_t)s * 8 + tid] = tid < MW_LEVELS ? (cs[tid] > max_nodes ? 0 : cs[tid]) : tid == 6 ? cs[MW_NDIVE] : U[s * MW_U];
    if (over) {
        if (tid < 6) out[tid] = tid == 0 ? SC_MATCH_OVERFLOW : 0;
        return;
    }
    const unsigned long long* __restrict__ ls = list + (size_t)s * max_nodes;
    const int32_t* __restrict__ bs = bnd + (size_t)s * max_nodes;
    const int slots = cs[MW_NPAR] * 16;   // at most 2^26
    mt_key mk = {~0ull, ~0u};
    for (int i = tid; i < slots; i += 256) {
        const unsigned long long e = ls[i >> 4];
        const int a = i & 3, b = (i >> 2) & 3, pdx = (int)(e & 0x1fff), pdy = (int)(e >> 13) & 0x1fff;
        const int kx = mw_kids(pdx, 1, 2 * wx), ky = mw_kids(pdy, 1, 2 * wy);
        if (a >= kx || b >= ky) continue;
        const int dx = pdx + a - wx, dy = pdy + b - wy;
        const mt_key k = {(unsigned long long)(uint32_t)bs[(unsigned)(e >> 34) + b * kx + a] << 32 | (unsigned long long)(dx * dx + dy * dy) << 8 |
                              ((unsigned)(e >> 26) & 0xff),
                          (uint32_t)(pdy + b) << 13 | (uint32_t)(pdx + a)};
        if (mt_less(k, mk)) mk = k;
    }
    keys[tid] = mk;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h && mt_less(keys[tid + h], keys[tid])) keys[tid] = keys[tid + h];
        __syncthreads();
    }
    const mt_key bk = keys[0];
    const int32_t smin = (int32_t)(bk.k1 >> 32);
    const int r = (int)(bk.k1 & 0xffu);
    int ties = 0, present = 0;   // ties against the final minimum only
    for (int i = tid; i < slots; i += 256) {
        const unsigned long long e = ls[i >> 4];
        const int a = i & 3, b = (i >> 2) & 3;
        const int kx = mw_kids((int)(e & 0x1fff), 1, 2 * wx), ky = mw_kids((int)(e >> 13) & 0x1fff, 1, 2 * wy);
        ties += a < kx && b < ky && bs[(unsigned)(e >> 34) + b * kx + a] == smin;
    }
    const int32_t* __restrict__ p = pts + ((size_t)s * R + r) * (size_t)N * 2;
    for (int k = tid; k < N; k += 256) present += !mt_absent(p[2 * k]) && !mt_absent(p[2 * k + 1]);
    acc[0][tid] = ties, acc[1][tid] = present;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) acc[0][tid] += acc[0][tid + h], acc[1][tid] += acc[1][tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = r;
        out[1] = (int)(bk.k2 & 0x1fff) - wx;
        out[2] = (int)(bk.k2 >> 13) - wy;
        out[3] = smin;
        out[4] = acc[1][0];
        out[5] = acc[0][0];
    }
}

}  // namespace

static bool match_wide_args_ok(const sc_ctx* ctx, const int32_t* d2, const int32_t* pts, const int32_t* centre, int S, int R, int N, int W,
                               int H, int wx, int wy, int32_t d2_cap, int32_t unk, int top, int max_nodes, const int32_t* best,
                               const int32_t* stats) {
    if (!ctx || !d2 || !pts || !centre || !best || S < 0) return false;
    if (R < 1 || R > SC_MATCH_MAX_ROT || N < 1 || N > SC_MATCH_MAX_POINTS || W < 1 || W > SC_MAX_DIM || H < 1 || H > SC_MAX_DIM) return false;
    if (wx < 0 || wx > SC_MATCH_WIDE_MAX_HALF || wy < 0 || wy > SC_MATCH_WIDE_MAX_HALF || d2_cap < 1 || d2_cap > 32767 || unk < 0 ||
        unk > d2_cap || top < 0 || top > SC_MATCH_WIDE_MAX_TOP)
        return false;
    if (max_nodes < SC_MATCH_WIDE_MIN_NODES || max_nodes > SC_MATCH_WIDE_MAX_NODES || (int64_t)S * max_nodes > SC_MATCH_WIDE_MAX_TOTAL)
        return false;
    const int64_t m = (int64_t)1 << (2 * top);
    if (R * (2 * wx / m + 1) * (2 * wy / m + 1) > max_nodes) return false;          // the nodes of the top level
    if ((int64_t)R * (2 * wx + 1) * (2 * wy + 1) > INT32_MAX) return false;          // n_ties of a scan without points
    return stats != best;
}

extern "C" int sc_scan_match_wide_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre, int S,
                                        int R, int N, int W, int H, int wx, int wy, int32_t d2_cap, int32_t unk, int top, int max_nodes,
                                        int32_t* best, int32_t* stats) {
    if (!match_wide_args_ok(ctx, d2, pts, centre, S, R, N, W, H, wx, wy, d2_cap, unk, top, max_nodes, best, stats)) return SC_ERR_INVALID;
    if (S == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    // scratch.  Level 0 is the dense matcher's cost map; levels 1 .. top and the half-way map of a level share one buffer.
    const int cells0 = (W + 2) * (H + 2) + 1;
    size_t lv_off[MW_LEVELS + 1] = {0}, pyr_bytes = 0;
    for (int j = 1; j <= top; ++j) {
        const size_t m = (size_t)1 << (2 * j);
        lv_off[j] = pyr_bytes;
        pyr_bytes += al256((W + m + 1) * (H + m + 1) * 2);
    }
    const size_t half = (size_t)1 << (2 * top) >> 1, tmp_off = pyr_bytes;
    if (top > 0) pyr_bytes += al256((W + half + 1) * (H + half + 1) * 2);
    const size_t per = (size_t)S * max_nodes;   // <= 2^26
    const size_t o_bnd = 2 * per * 8, o_keys = o_bnd + al256(per * 4), o_cnt = o_keys + al256((size_t)S * R * 8),
                 o_u = o_cnt + al256((size_t)S * MW_CNT * 4), state_bytes = o_u + al256((size_t)S * MW_U * 4);
    int r = sc_scratch_reserve(ctx, &ctx->mt_cost, (size_t)cells0 * 2);
    if (r == SC_OK) r = sc_scratch_reserve(ctx, &ctx->mw_pyr, pyr_bytes ? pyr_bytes : 256);
    if (r == SC_OK) r = sc_scratch_reserve(ctx, &ctx->mw_state, state_bytes);
    if (r != SC_OK) return r;
    uint16_t* cost = (uint16_t*)ctx->mt_cost.p;
    char* pb = (char*)ctx->mw_pyr.p;
    char* sb = (char*)ctx->mw_state.p;
    unsigned long long* lists[2] = {(unsigned long long*)sb, (unsigned long long*)sb + per};
    int32_t* bnd = (int32_t*)(sb + o_bnd);
    unsigned long long* keys = (unsigned long long*)(sb + o_keys);
    int32_t* cnt = (int32_t*)(sb + o_cnt);
    int32_t* U = (int32_t*)(sb + o_u);
    hipStream_t st = ctx->stream;
    int tk = sc_time_begin(ctx, SC_K_MOVES);
    SC_HIP(ctx, hipMemsetAsync(keys, 0xff, (size_t)S * R * 8, st));
    SC_HIP(ctx, hipMemsetAsync(cnt, 0, (size_t)S * MW_CNT * 4, st));
    SC_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)U, INT32_MAX, (size_t)S * MW_U, st));
    hipLaunchKernelGGL(mt_cost_kernel, dim3((unsigned)((cells0 + 255) / 256)), dim3(256), 0, st, d2, known, W, H, d2_cap, unk, cost);
    mw_pyr pyr;
    for (int j = 0; j < MW_LEVELS; ++j) pyr.lv[j] = j == 0 || j > top ? cost : (const uint16_t*)(pb + lv_off[j]);
    for (int j = 1; j <= top; ++j) {   // two doublings: h = m / 4 into the half-way map, h = m / 2 into the level
        const int m = 1 << (2 * j), q = m / 4, hm = m / 2;
        uint16_t* tmp = (uint16_t*)(pb + tmp_off);
        hipLaunchKernelGGL(mw_pool_kernel, dim3((unsigned)((W + hm + 1 + 255) / 256), (unsigned)(H + hm + 1)), dim3(256), 0, st, pyr.lv[j - 1], q, tmp,
                           hm, q, W, H);
        hipLaunchKernelGGL(mw_pool_kernel, dim3((unsigned)((W + m + 1 + 255) / 256), (unsigned)(H + m + 1)), dim3(256), 0, st, tmp, hm,
                           (uint16_t*)(pb + lv_off[j]), m, hm, W, H);
    }
    hipLaunchKernelGGL(mw_init_kernel, dim3((unsigned)S * R), dim3(256), 0, st, cost, pts, centre, R, N, W, H, wx, wy, top, max_nodes, cnt, U,
                       lists[top & 1]);
    // workgroups per scan of the list kernels: each sweep of one takes 16 parents
    int G = MW_MAX_BLOCKS / S;
    G = G < 1 ? 1 : G > MW_MAX_G ? MW_MAX_G : G;
    if (G > (max_nodes + 15) / 16) G = (max_nodes + 15) / 16;
    for (int j = top; j >= 0; --j) {
        unsigned long long *cur = lists[j & 1], *next = lists[(j & 1) ^ 1];
        hipLaunchKernelGGL(mw_bound_kernel, dim3((unsigned)S * G), dim3(256), 0, st, pyr.lv[j], pts, centre, R, N, W, H, wx, wy, j, max_nodes, G, cnt,
                           U, cur, bnd, j > 0 ? keys : nullptr);
        if (j == 0) break;
        hipLaunchKernelGGL(mw_dive_kernel, dim3((unsigned)S * R), dim3(256), 0, st, pyr, pts, centre, R, N, W, H, wx, wy, j, max_nodes, cnt, U,
                           keys);
        hipLaunchKernelGGL(mw_expand_kernel, dim3((unsigned)S * G), dim3(256), 0, st, centre, R, wx, wy, j, max_nodes, G, cnt, U, cur, bnd, next);
    }
    hipLaunchKernelGGL(mw_pick_kernel, dim3((unsigned)S), dim3(256), 0, st, pts, centre, R, N, wx, wy, top, max_nodes, cnt, U, lists[0], bnd, best,
                       stats);
    sc_time_end(ctx, tk);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

extern "C" int sc_scan_match_wide_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre,
                                             int S, int R, int N, int W, int H, int wx, int wy, int32_t d2_cap, int32_t unk, int top,
                                             int max_nodes, int32_t* best, int32_t* stats) {
    if (!match_wide_args_ok(ctx, d2, pts, centre, S, R, N, W, H, wx, wy, d2_cap, unk, top, max_nodes, best, stats)) return SC_ERR_INVALID;
    if (S == 0) return SC_OK;
    for (int s = 0; s < S; ++s)
        if (!mt_centre_ok(centre[2 * s]) || !mt_centre_ok(centre[2 * s + 1])) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    sc_stage st(ctx);
    const int i_d = st.in(d2, n * 4), i_k = st.in(known, known ? n : 0), i_p = st.in(pts, (size_t)S * R * N * 8), i_c = st.in(centre, (size_t)S * 8);
    const int o_b = st.out(best, (size_t)S * 24), o_s = st.out(stats, stats ? (size_t)S * 32 : 0);
    int r = st.upload();
    if (r == SC_OK)
        r = sc_scan_match_wide_batch(ctx, st.dev<const int32_t>(i_d), known ? st.dev<const uint8_t>(i_k) : nullptr, st.dev<const int32_t>(i_p),
                                     st.dev<const int32_t>(i_c), S, R, N, W, H, wx, wy, d2_cap, unk, top, max_nodes, st.dev<int32_t>(o_b),
                                     stats ? st.dev<int32_t>(o_s) : nullptr);
    return st.finish(r);
}
