// occupancy_grid::scan_match_wide and logodds_grid::relocalise through sea-current_amd/sea_current.hpp, on the two-room world of
// test_scan.cpp: bounding_rect {5, -5, 5, -5}, 100 cells, a wall along x = 0 with a door of one unit at y = 0, the robot in the
// left room.
//   occupancy_grid::scan_match_wide: best against a restatement on the host (a plain dense search over rotations, the window
//     and the points), two scans whose priors are off by tens of cells and four quarter-turn rotations, with and without known,
//     for top 0 .. 3; the stats obey what the definition fixes (the count of the top level, no level above it, no more leaves
//     than candidates); a window too wide for max_nodes at the top level throws; an overflowing scan reads SC_MATCH_OVERFLOW;
//   logodds_grid::relocalise: a map built from one scan, a second scan from two cells away with a prior that is 21 and 17
//     cells off: the row equals the restatement on (EDT of occ_est, known), and the pose is recovered.
// Exit code 0 and "match_wide OK" = all passed.
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

using row6 = std::array<int32_t, 6>;
using row8 = std::array<int32_t, 8>;

static bool absent(int32_t v) { return v < -SC_SCAN_MAX_REACH || v > SC_SCAN_MAX_REACH; }

// the dense search of include/sea_current_hip.h for one scan: pts [R][N]
static row6 match_naive(int W, int H, const std::vector<int32_t>& d2, const std::vector<uint8_t>& known, const scan_points& pts, int R,
                        std::array<int32_t, 2> c, const wide_match_params& p) {
    const size_t N = pts.size() / R;
    long long bs = -1, bd = 0, ties = 0;
    int br = 0, bdx = 0, bdy = 0;
    for (int r = 0; r < R; ++r)
        for (int dy = -p.wy; dy <= p.wy; ++dy)
            for (int dx = -p.wx; dx <= p.wx; ++dx) {
                long long sum = 0;
                for (size_t k = 0; k < N; ++k) {
                    const auto& q = pts[r * N + k];
                    if (absent(q[0]) || absent(q[1])) continue;
                    const int x = c[0] + dx + q[0], y = c[1] + dy + q[1];
                    const bool in = x >= 0 && y >= 0 && x < W && y < H;
                    sum += !in || (!known.empty() && !known[(size_t)y * W + x]) ? p.unk : std::min(d2[(size_t)y * W + x], p.d2_cap);
                }
                const long long d = (long long)dx * dx + (long long)dy * dy;
                if (sum == bs) ++ties;
                if (bs < 0 || sum < bs || (sum == bs && d < bd)) {
                    if (bs < 0 || sum < bs) ties = 1;
                    bs = sum; bd = d; br = r; bdx = dx; bdy = dy;
                }
            }
    int np = 0;
    for (size_t k = 0; k < N; ++k) np += !absent(pts[br * N + k][0]) && !absent(pts[br * N + k][1]);
    return {br, bdx, bdy, (int32_t)bs, np, (int32_t)ties};
}

int main() {
    const bounding_rect br{5.0f, -5.0f, 5.0f, -5.0f};
    planning_space space(br);
    obstacle lower({Vector2f(0.0f, -5.0f), Vector2f(0.0f, -0.5f)}, {{0, 1}}), upper({Vector2f(0.0f, 0.5f), Vector2f(0.0f, 5.0f)}, {{0, 1}});
    lower.closed = upper.closed = false;
    space.obstacles = {lower, upper};
    space.grid_cells = 100;
    occupancy_grid g = space.make_grid();
    CHECK(g.W == 100 && g.H == 100);
    for (int32_t c : {30 * 100 + 20, 61 * 100 + 33, 44 * 100 + 12, 70 * 100 + 40}) g.occ[c] = 1;
    g.edt();
    const int W = g.W, H = g.H;
    const int ax = 25, ay = 50;
    const auto rays = square_fan(ax, ay, 30);
    const auto hit = g.scan_cast(rays);
    const scan_points p0 = points_from_hits(rays, hit, W);
    int returns = 0;
    for (int32_t h : hit) returns += h >= 0;
    CHECK(returns > 20);

    // ---- occupancy_grid::scan_match_wide against the restatement ----
    const double quarter = std::acos(-1.0) / 2;
    const scan_points rot0 = rotate_points(p0, {0.0, quarter, 2 * quarter, 3 * quarter});
    const scan_points rot1 = rotate_points(rotate_points(p0, {-quarter}), {0.0, quarter, 2 * quarter, 3 * quarter});
    scan_points both = rot0;
    both.insert(both.end(), rot1.begin(), rot1.end());
    const std::vector<std::array<int32_t, 2>> centres = {{ax + 32, ay - 21}, {ax - 35, ay + 26}};   // the second prior lies outside the grid
    std::vector<uint8_t> known((size_t)W * H, 1);
    for (size_t c = 0; c < known.size(); c += 7) known[c] = 0;
    const std::vector<uint8_t> all_known;
    const std::vector<uint8_t>* masks_to_try[2] = {&all_known, &known};
    wide_match_params wp;
    wp.wx = 40; wp.wy = 30; wp.rotations = 4; wp.max_nodes = 1 << 15;
    for (const std::vector<uint8_t>* kn : masks_to_try) {
        const row6 want[2] = {match_naive(W, H, g.d2, *kn, rot0, 4, centres[0], wp), match_naive(W, H, g.d2, *kn, rot1, 4, centres[1], wp)};
        for (int top = 0; top <= 3; ++top) {
            wp.top = top;
            std::vector<row8> stats;
            const auto best = g.scan_match_wide(both, centres, wp, default_context(), *kn, &stats);
            CHECK(best.size() == 2 && stats.size() == 2);
            const int m = 1 << (2 * top);
            for (int s = 0; s < 2; ++s) {
                CHECK(best[s] == want[s]);
                CHECK(stats[s][top] == 4 * (2 * wp.wx / m + 1) * (2 * wp.wy / m + 1));
                for (int j = top + 1; j < 6; ++j) CHECK(stats[s][j] == 0);
                CHECK(stats[s][0] >= 1 && stats[s][0] <= 4 * 81 * 61 && stats[s][7] >= want[s][3] && (top > 0 || stats[s][6] == 0));
            }
            CHECK(g.scan_match_wide(both, centres, wp, default_context(), *kn) == best);
        }
        if (kn->empty()) {
            CHECK((want[0] == row6{0, -32, 21, 0, returns, 1}));
            CHECK((want[1] == row6{1, 35, -26, 0, returns, 1}));
        }
    }
    bool threw = false;
    wide_match_params bad = wp;
    bad.top = 0; bad.max_nodes = 4096;                                                  // 4 * 81 * 61 nodes at the top level
    try { g.scan_match_wide(both, centres, bad); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    threw = false;
    bad = wp;
    bad.rotations = 7;
    try { g.scan_match_wide(both, centres, bad); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { g.scan_match_wide(rot0, {{-SC_SCAN_MAX_REACH - 1, 0}}, wp); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);                                                                       // the host form refuses an ignored centre
    CHECK(g.scan_match_wide({}, {}, wp).empty());
    {   // a grid nobody knows: every candidate ties, and 64 nodes do not hold them
        const std::vector<uint8_t> nothing((size_t)W * H, 0);
        wide_match_params small;
        small.wx = small.wy = 20; small.top = 2; small.max_nodes = 64;
        const scan_points one(p0.begin(), p0.end());
        const auto over = g.scan_match_wide(one, {{ax, ay}}, small, default_context(), nothing);
        CHECK((over[0] == row6{SC_MATCH_OVERFLOW, 0, 0, 0, 0, 0}));
        small.max_nodes = 2048;
        const auto all = g.scan_match_wide(one, {{ax, ay}}, small, default_context(), nothing);
        CHECK((all[0] == row6{0, 0, 0, returns, returns, 41 * 41}));
    }

    // ---- logodds_grid::relocalise ----
    logodds_grid map(W, H);
    map.update(rays, hit);
    const int bx = ax + 2, by = ay - 1;
    CHECK(g.occ[(size_t)by * W + bx] == 0);
    const auto rays2 = square_fan(bx, by, 30);
    const scan_points p2 = points_from_hits(rays2, g.scan_cast(rays2), W);
    wide_match_params lm;
    lm.wx = lm.wy = 24; lm.d2_cap = 16; lm.top = 2; lm.max_nodes = 1 << 14;
    const row6 got = map.relocalise(p2, {bx - 21, by + 17}, lm);
    auto masks = map.masks();
    occupancy_grid est;
    est.W = W; est.H = H; est.occ = masks.occ_est;
    est.edt();
    CHECK(got == match_naive(W, H, est.d2, masks.known, p2, 1, {bx - 21, by + 17}, lm));
    CHECK(got[0] == 0 && got[1] == 21 && got[2] == -17 && got[5] == 1);

    std::printf("match_wide OK\n");
    return 0;
}
