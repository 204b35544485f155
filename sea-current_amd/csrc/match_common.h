// match_common.h -- what the two scan matchers share (match.hip: the dense window, match_wide.hip: the pruned search): the
// tests for absent points and ignored centres, the cost pass and the key that orders candidates.
#pragma once
#include "sc_internal.h"

namespace {

__device__ __host__ __forceinline__ bool mt_absent(int p) { return p < -SC_SCAN_MAX_REACH || p > SC_SCAN_MAX_REACH; }
__device__ __host__ __forceinline__ bool mt_centre_ok(int c) { return c >= -SC_SCAN_MAX_REACH && c <= SC_MAX_DIM + SC_SCAN_MAX_REACH; }

__global__ __launch_bounds__(256) void mt_cost_kernel(const int32_t* __restrict__ d2, const uint8_t* __restrict__ known, int W, int H,
                                                      int32_t d2_cap, int32_t unk, uint16_t* __restrict__ cost) {
    const int Wp = W + 2, total = Wp * (H + 2) + 1;   // (SC_MAX_DIM + 2)^2 + 1 < 2^27
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int v = 0;   // the last entry: what an absent point reads
    if (i < total - 1) {
        const int x = i % Wp - 1, y = i / Wp - 1;
        v = unk;
        if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) {
            const int c = y * W + x;
            if (!known || known[c] != 0) v = min(d2[c], d2_cap);
        }
    }
    cost[i] = (uint16_t)v;
}

// lexicographic (score, displacement, r, dy, dx): k1 = score << 32 | disp << 8 | r (disp < 2^24), k2 = dyi << b | dxi with
// b = 8 in the dense matcher and 13 in the wide one
struct mt_key { unsigned long long k1; uint32_t k2; };
__device__ __forceinline__ bool mt_less(const mt_key& a, const mt_key& b) { return a.k1 < b.k1 || (a.k1 == b.k1 && a.k2 < b.k2); }

}  // namespace
