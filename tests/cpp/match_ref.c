/* match_ref.c -- the C statement of scan matching (sc_scan_match_batch), plain loops straight from the definition in
 * include/sea_current_hip.h.  Checker only: the library never links it. */
#include <stdint.h>
#include <stddef.h>

#define MX_MAX_REACH 16384
#define MX_MAX_DIM 8192
#define MX_IGNORED (-1)

static int mx_absent(int32_t p) { return p < -MX_MAX_REACH || p > MX_MAX_REACH; }
static int mx_centre_ok(int32_t c) { return c >= -MX_MAX_REACH && c <= MX_MAX_DIM + MX_MAX_REACH; }

static int64_t mx_cost(const int32_t* d2, const uint8_t* known, int W, int H, int x, int y, int32_t d2_cap, int32_t unk) {
    if (x < 0 || x >= W || y < 0 || y >= H) return unk;
    size_t c = (size_t)y * W + x;
    if (known && known[c] == 0) return unk;
    return d2[c] < d2_cap ? d2[c] : d2_cap;
}

/* 0, or 1 for arguments outside the contract.  score may be NULL. */
int mx_match(const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre, int S, int R, int N, int W, int H, int wx,
             int wy, int32_t d2_cap, int32_t unk, int32_t* best, int32_t* score) {
    if (!d2 || !pts || !centre || !best || S < 0 || R < 1 || R > 256 || N < 1 || N > 65536 || W < 1 || W > MX_MAX_DIM || H < 1 ||
        H > MX_MAX_DIM || wx < 0 || wx > 64 || wy < 0 || wy > 64 || d2_cap < 1 || d2_cap > 32767 || unk < 0 || unk > d2_cap || score == best)
        return 1;
    const int ndx = 2 * wx + 1, ndy = 2 * wy + 1;
    for (int s = 0; s < S; ++s) {
        int32_t* b = best + (size_t)s * 6;
        const int cx = centre[2 * s], cy = centre[2 * s + 1];
        if (!mx_centre_ok(cx) || !mx_centre_ok(cy)) {
            b[0] = MX_IGNORED;
            b[1] = b[2] = b[3] = b[4] = b[5] = 0;
            if (score)
                for (size_t i = 0; i < (size_t)R * ndy * ndx; ++i) score[(size_t)s * R * ndy * ndx + i] = 0;
            continue;
        }
        int have = 0;
        int64_t bs = 0, bd = 0, ties = 0;
        int br = 0, bdy = 0, bdx = 0;
        for (int r = 0; r < R; ++r) {
            const int32_t* p = pts + ((size_t)s * R + r) * (size_t)N * 2;
            for (int dy = -wy; dy <= wy; ++dy)
                for (int dx = -wx; dx <= wx; ++dx) {
                    int64_t sum = 0;   /* at most 32767 * 65536 < 2^31 */
                    for (int k = 0; k < N; ++k) {
                        if (mx_absent(p[2 * k]) || mx_absent(p[2 * k + 1])) continue;
                        sum += mx_cost(d2, known, W, H, cx + dx + p[2 * k], cy + dy + p[2 * k + 1], d2_cap, unk);
                    }
                    if (score) score[(((size_t)s * R + r) * ndy + (dy + wy)) * ndx + (dx + wx)] = (int32_t)sum;
                    const int64_t d = (int64_t)dx * dx + (int64_t)dy * dy;
                    if (have && sum == bs) ++ties;
                    /* the loops run r, dy, dx ascending, so among equal (score, displacement) the first met stays */
                    if (!have || sum < bs || (sum == bs && d < bd)) {
                        if (!have || sum < bs) ties = 1;
                        have = 1, bs = sum, bd = d, br = r, bdy = dy, bdx = dx;
                    }
                }
        }
        int np = 0;
        const int32_t* p = pts + ((size_t)s * R + br) * (size_t)N * 2;
        for (int k = 0; k < N; ++k) np += !mx_absent(p[2 * k]) && !mx_absent(p[2 * k + 1]);
        b[0] = br, b[1] = bdx, b[2] = bdy, b[3] = (int32_t)bs, b[4] = np, b[5] = (int32_t)ties;
    }
    return 0;
}
