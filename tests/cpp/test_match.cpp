// occupancy_grid::scan_match, logodds_grid::match, points_from_hits and rotate_points through sea-current_amd/sea_current.hpp, on
// the two-room world of test_scan.cpp: bounding_rect {5, -5, 5, -5}, 100 cells, a wall along x = 0 with a door of one unit at
// y = 0, the robot in the left room.
//   points_from_hits: hit = origin + offset for every beam with a return, SC_MATCH_ABSENT for the others;
//   rotate_points: at multiples of a quarter turn the integer rotation (x, y) -> (-y, x), absent points stay absent;
//   occupancy_grid::scan_match: best and the volume against a restatement on the host (plain loops over rotations, the
//     window and the points), two scans with different priors and four quarter-turn rotations, with and without known; the
//     scan of a sensor turned by a quarter turn is found at the rotation that undoes it;
//   logodds_grid::match: a map built from one scan, a second scan from two cells away with a prior that is off: the row
//     equals the restatement on (EDT of occ_est, known), and the pose is recovered.
// Exit code 0 and "match OK" = all passed.
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

using row6 = std::array<int32_t, 6>;

static bool absent(int32_t v) { return v < -SC_SCAN_MAX_REACH || v > SC_SCAN_MAX_REACH; }

// the definition of include/sea_current_hip.h for one scan: pts [R][N]
static row6 match_naive(int W, int H, const std::vector<int32_t>& d2, const std::vector<uint8_t>& known, const scan_points& pts, int R,
                        std::array<int32_t, 2> c, const match_params& p, std::vector<int32_t>& score) {
    const size_t N = pts.size() / R;
    long long bs = -1, bd = 0, ties = 0;
    int br = 0, bdx = 0, bdy = 0;
    score.clear();
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
                score.push_back((int32_t)sum);
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
    // a few free-standing cells, so that a pose is pinned along the wall too
    for (int32_t c : {30 * 100 + 20, 61 * 100 + 33, 44 * 100 + 12, 70 * 100 + 40}) g.occ[c] = 1;
    g.edt();
    const int W = g.W, H = g.H;

    // ---- points_from_hits ----
    const int ax = 25, ay = 50;
    const auto rays = square_fan(ax, ay, 30);
    const auto hit = g.scan_cast(rays);
    const scan_points p0 = points_from_hits(rays, hit, W);
    CHECK(p0.size() == rays.size());
    int returns = 0;
    for (size_t k = 0; k < rays.size(); ++k) {
        if (hit[k] >= 0) { CHECK((ay + p0[k][1]) * W + ax + p0[k][0] == hit[k]); ++returns; }
        else CHECK(p0[k][0] == SC_MATCH_ABSENT && p0[k][1] == SC_MATCH_ABSENT);
    }
    CHECK(returns > 20 && returns < (int)rays.size());

    // ---- rotate_points at quarter turns ----
    const double quarter = std::acos(-1.0) / 2;
    scan_points odd = p0;
    odd.push_back({SC_SCAN_MAX_REACH, -SC_SCAN_MAX_REACH});
    odd.push_back({3, SC_MATCH_ABSENT});
    const scan_points turned = rotate_points(odd, {0.0, quarter, 2 * quarter, 3 * quarter, -quarter, 4 * quarter});
    CHECK(turned.size() == 6 * odd.size());
    const int turns[6] = {0, 1, 2, 3, 3, 0};
    for (int r = 0; r < 6; ++r)
        for (size_t k = 0; k < odd.size(); ++k) {
            const auto& q = turned[r * odd.size() + k];
            if (absent(odd[k][0]) || absent(odd[k][1])) { CHECK(q[0] == SC_MATCH_ABSENT && q[1] == SC_MATCH_ABSENT); continue; }
            int32_t x = odd[k][0], y = odd[k][1];
            for (int t = 0; t < turns[r]; ++t) { const int32_t nx = -y; y = x; x = nx; }
            CHECK(q[0] == x && q[1] == y);
        }

    // ---- occupancy_grid::scan_match against the restatement ----
    match_params mp;
    mp.wx = 4; mp.wy = 3; mp.rotations = 4;
    // scan 0: seen as it is, the prior off by (+2, -1); scan 1: the sensor was turned by a quarter turn, so the points
    // arrive turned back by one and rotation 1 undoes it; the prior off by (-3, +2)
    const scan_points rot0 = rotate_points(p0, {0.0, quarter, 2 * quarter, 3 * quarter});
    const scan_points rot1 = rotate_points(rotate_points(p0, {-quarter}), {0.0, quarter, 2 * quarter, 3 * quarter});
    scan_points both = rot0;
    both.insert(both.end(), rot1.begin(), rot1.end());
    const std::vector<std::array<int32_t, 2>> centres = {{ax + 2, ay - 1}, {ax - 3, ay + 2}};
    std::vector<uint8_t> known((size_t)W * H, 1);
    for (size_t c = 0; c < known.size(); c += 7) known[c] = 0;
    const std::vector<uint8_t> all_known;                                               // empty: every cell
    const std::vector<uint8_t>* masks_to_try[2] = {&all_known, &known};
    for (const std::vector<uint8_t>* kn : masks_to_try) {
        std::vector<int32_t> vol, want_vol;
        const auto best = g.scan_match(both, centres, mp, default_context(), *kn, &vol);
        CHECK(best.size() == 2 && vol.size() == (size_t)2 * 4 * 7 * 9);
        for (int s = 0; s < 2; ++s) {
            const row6 want = match_naive(W, H, g.d2, *kn, s ? rot1 : rot0, 4, centres[s], mp, want_vol);
            CHECK(best[s] == want);
            CHECK(std::equal(want_vol.begin(), want_vol.end(), vol.begin() + (size_t)s * want_vol.size()));
        }
        if (kn->empty()) {
            CHECK((best[0] == row6{0, -2, 1, 0, returns, 1}));
            CHECK((best[1] == row6{1, 3, -2, 0, returns, 1}));
        }
        CHECK(g.scan_match(both, centres, mp, default_context(), *kn) == best);
    }
    bool threw = false;
    match_params seven = mp;
    seven.rotations = 7;
    try { g.scan_match(both, centres, seven); } catch (const std::invalid_argument&) { threw = true; }   // 480 points a scan are not 7 rotations
    CHECK(threw);
    threw = false;
    try { g.scan_match(rot0, {{-SC_SCAN_MAX_REACH - 1, 0}}, mp); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);                                                                       // the host form refuses an ignored centre
    CHECK(g.scan_match({}, {}, mp).empty());

    // ---- logodds_grid::match ----
    logodds_grid map(W, H);
    map.update(rays, hit);
    const int bx = ax + 2, by = ay - 1;
    CHECK(g.occ[(size_t)by * W + bx] == 0);
    const auto rays2 = square_fan(bx, by, 30);
    const scan_points p2 = points_from_hits(rays2, g.scan_cast(rays2), W);
    match_params lm;
    lm.wx = lm.wy = 3; lm.d2_cap = 16;
    const row6 got = map.match(p2, {bx - 2, by + 3}, lm);
    auto masks = map.masks();
    occupancy_grid est;
    est.W = W; est.H = H; est.occ = masks.occ_est;
    est.edt();
    std::vector<int32_t> unused;
    CHECK(got == match_naive(W, H, est.d2, masks.known, p2, 1, {bx - 2, by + 3}, lm, unused));
    CHECK(got[0] == 0 && got[1] == 2 && got[2] == -3 && got[5] == 1);

    std::printf("match OK\n");
    return 0;
}
