/* Plain C restatement of the space-time re-planning (sc_traj_reserve_batch, sc_tplan_batch, sc_fleet_replan_batch; the definition
 * is in include/sea_current_hip.h): single-threaded, no tiles, no tricks.  Compared with tests/tplan_twin.py bit for bit by
 * tests/test_tplan_ref.py and timed against the GPU by tools/tplan_time.py.  Compile with -ffp-contract=off.
 * Bitmaps are uint32 [H][Wq], Wq = ceil(W / 32): cell x is bit x & 31 of word x >> 5. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { TP_OK = 0, TP_NO_PATH = 1, TP_BAD_ENDPOINT = 2, TP_START_BLOCKED = 3 };
static const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1}, DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};

static float centre(int i, float o, float r) {
    const float a = (float)i + 0.5f;
    const float b = a * r;
    return o + b;
}

static int bit(const uint32_t* layer, int Wq, int x, int y) { return (int)(layer[(size_t)y * Wq + (x >> 5)] >> (x & 31) & 1u); }
static void set(uint32_t* layer, int Wq, int x, int y) { layer[(size_t)y * Wq + (x >> 5)] |= 1u << (x & 31); }

static double clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

/* m2 of the path conflicts: the squared closest approach on one interval */
static double m2_of(double d0x, double d0y, double d1x, double d1y) {
    const double ex = d1x - d0x, ey = d1y - d0y;
    const double a = ex * ex + ey * ey;
    const double b = d0x * ex + d0y * ey;
    const double lam = a > 0.0 ? clampd(-b / a, 0.0, 1.0) : 0.0;
    const double px = d0x + lam * ex, py = d0y + lam * ey;
    return px * px + py * py;
}

/* every cell against every interval of every path */
void tp_reserve(const double* knots, int32_t* tstatus, int P, int K, const double* radius, const int32_t* select, double pad, int W, int H,
                float x_min, float y_min, float res_x, float res_y, uint32_t* res) {
    const int Wq = (W + 31) / 32;
    const size_t layer = (size_t)H * Wq;
    for (int q = 0; q < P; ++q) {
        const double r = radius[q];
        const int r_ok = isfinite(r) && r >= 0.0;
        if (tstatus && tstatus[q] == 0 && !r_ok) tstatus[q] = 2;
        if ((tstatus && tstatus[q] != 0) || !r_ok || (select && select[q] == 0)) continue;
        const double R = r + pad, RR = R * R;
        for (int k = 0; k < K; ++k) {
            const double* kn = knots + ((size_t)q * (K + 1) + k) * 2;
            if (isnan(kn[0]) || isnan(kn[1]) || isnan(kn[2]) || isnan(kn[3])) continue;
            for (int y = 0; y < H; ++y) {
                const double cy = (double)centre(y, y_min, res_y);
                for (int x = 0; x < W; ++x) {
                    const double cx = (double)centre(x, x_min, res_x);
                    if (m2_of(kn[0] - cx, kn[1] - cy, kn[2] - cx, kn[3] - cy) < RR) {
                        set(res + (size_t)k * layer, Wq, x, y);
                        set(res + (size_t)(k + 1) * layer, Wq, x, y);
                    }
                }
            }
        }
    }
}

/* sc_moves_i32_u8 */
void tp_moves(const int32_t* d2, int W, int H, int32_t r2_clear, uint8_t* moves) {
    const int32_t rmin = r2_clear > 1 ? r2_clear : 1;
#define FREE(x, y) ((x) >= 0 && (x) < W && (y) >= 0 && (y) < H && d2[(size_t)(y) * W + (x)] >= rmin)
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            unsigned m = 0;
            if (FREE(x, y))
                for (int d = 0; d < 8; ++d) {
                    int ok = FREE(x + DX[d], y + DY[d]);
                    if (DX[d] && DY[d]) ok = ok && FREE(x + DX[d], y) && FREE(x, y + DY[d]);
                    m |= (unsigned)ok << d;
                }
            moves[(size_t)y * W + x] = (uint8_t)m;
        }
#undef FREE
}

/* reach must hold B * L layers; layers outside t_start .. arrive (or L-1) of a query are zero */
void tp_plan(const int32_t* d2, int W, int H, int32_t r2_clear, const uint32_t* res, int L, const int32_t* start, const int32_t* goal,
             const int32_t* t_start, int B, int hold, int32_t* path, int32_t* len, int32_t* arrive, int32_t* status, double* knots_out,
             float x_min, float y_min, float res_x, float res_y, uint32_t* reach) {
    const int Wq = (W + 31) / 32, cells = W * H;
    const size_t layer = (size_t)H * Wq;
    const int32_t rmin = r2_clear > 1 ? r2_clear : 1;
    uint8_t* mv = (uint8_t*)malloc((size_t)cells);
    tp_moves(d2, W, H, r2_clear, mv);
    memset(reach, 0, (size_t)B * L * layer * 4);
    for (int b = 0; b < B; ++b) {
        uint32_t* rq = reach + (size_t)b * L * layer;
        const int s = start[b], g = goal[b], ts = t_start ? t_start[b] : 0;
        int st = TP_NO_PATH, arr = -1;
        if (s < 0 || s >= cells || g < 0 || g >= cells || ts < 0 || ts >= L || d2[s] < rmin || d2[g] < rmin) st = TP_BAD_ENDPOINT;
        else if (res && bit(res + (size_t)ts * layer, Wq, s % W, s / W)) st = TP_START_BLOCKED;
        else {
            const int gx = g % W, gy = g / W;
            int t_hold = 0;
            if (hold && res)
                for (int t = 0; t < L; ++t)
                    if (bit(res + (size_t)t * layer, Wq, gx, gy)) t_hold = t + 1;
            const int t_min = ts > t_hold ? ts : t_hold;
            set(rq + (size_t)ts * layer, Wq, s % W, s / W);
            for (int t = ts;; ++t) {
                const uint32_t* cur = rq + (size_t)t * layer;
                if (t >= t_min && bit(cur, Wq, gx, gy)) { arr = t; st = TP_OK; break; }
                if (t == L - 1) break;
                uint32_t* nxt = rq + (size_t)(t + 1) * layer;
                const uint32_t* rs = res ? res + (size_t)(t + 1) * layer : NULL;
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        if (!bit(cur, Wq, x, y)) continue;
                        if (!(rs && bit(rs, Wq, x, y))) set(nxt, Wq, x, y);   /* a wait */
                        for (int d = 0; d < 8; ++d)
                            if (mv[(size_t)y * W + x] >> d & 1) {
                                const int nx = x + DX[d], ny = y + DY[d];
                                if (!(rs && bit(rs, Wq, nx, ny))) set(nxt, Wq, nx, ny);
                            }
                    }
            }
        }
        status[b] = st;
        if (arrive) arrive[b] = arr;
        if (len) len[b] = st == TP_OK ? arr - ts + 1 : 0;
        if (knots_out)
            for (int t = 0; t < 2 * L; ++t) knots_out[(size_t)b * L * 2 + t] = NAN;
        if (st != TP_OK) continue;
        int x = g % W, y = g / W;
        for (int t = arr;; --t) {
            if (path) path[(size_t)b * L + t - ts] = y * W + x;
            if (knots_out) {
                knots_out[((size_t)b * L + t) * 2] = (double)centre(x, x_min, res_x);
                knots_out[((size_t)b * L + t) * 2 + 1] = (double)centre(y, y_min, res_y);
            }
            if (t == ts) break;
            const uint32_t* prev = rq + (size_t)(t - 1) * layer;
            if (bit(prev, Wq, x, y)) continue;   /* waits come first */
            for (int d = 0; d < 8; ++d) {
                const int px = x - DX[d], py = y - DY[d];
                if (px < 0 || px >= W || py < 0 || py >= H) continue;
                if (bit(prev, Wq, px, py) && (mv[(size_t)py * W + px] >> d & 1)) { x = px; y = py; break; }
            }
        }
        if (knots_out && hold)
            for (int t = arr + 1; t < L; ++t) {
                knots_out[((size_t)b * L + t) * 2] = (double)centre(g % W, x_min, res_x);
                knots_out[((size_t)b * L + t) * 2 + 1] = (double)centre(g / W, y_min, res_y);
            }
    }
    free(mv);
}

/* reach: B * L layers, or L layers with sequential (one robot at a time; it then holds the last robot's) */
void tp_fleet_replan(const double* knots, int32_t* tstatus, int P, int K, const double* radius, const int32_t* select, double pad, int W, int H,
                     float x_min, float y_min, float res_x, float res_y, uint32_t* res, const int32_t* d2, int32_t r2_clear, const int32_t* start,
                     const int32_t* goal, const int32_t* t_start, int B, int hold, int32_t* path, int32_t* len, int32_t* arrive, int32_t* status,
                     double* knots_out, uint32_t* reach, const double* r_new, int sequential) {
    const int L = K + 1;
    tp_reserve(knots, tstatus, P, K, radius, select, pad, W, H, x_min, y_min, res_x, res_y, res);
    if (!sequential) {
        tp_plan(d2, W, H, r2_clear, res, L, start, goal, t_start, B, hold, path, len, arrive, status, knots_out, x_min, y_min, res_x, res_y, reach);
        return;
    }
    for (int i = 0; i < B; ++i) {
        double* row = knots_out + (size_t)i * L * 2;
        tp_plan(d2, W, H, r2_clear, res, L, start + i, goal + i, t_start ? t_start + i : NULL, 1, hold, path ? path + (size_t)i * L : NULL,
                len ? len + i : NULL, arrive ? arrive + i : NULL, status + i, row, x_min, y_min, res_x, res_y, reach);
        tp_reserve(row, NULL, 1, K, r_new + i, NULL, pad, W, H, x_min, y_min, res_x, res_y, res);
    }
}
