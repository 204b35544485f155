// occupancy_grid::scan_cast, logodds_grid, beams_from_ranges and planner::range_scan through sea-current_amd/sea_current.hpp, on
// the two-room world of test_views.cpp: bounding_rect {5, -5, 5, -5}, 100 cells, a wall along x = 0 with a door of one unit at
// y = 0, the robot in the left room at (-2.5, 0).
//   scan_cast: against a restatement on the host -- the cells whose unit square meets the segment (the four-corner sign test
//     over the bounding box, no column walk), sorted by column of the major axis and then away from the origin, cut at the
//     first cell outside the grid; the hit is the first occupied one.  A fan of half-side 30, rays that leave the grid, and
//     every ignored kind;
//   logodds_grid::update: the misses and the hit of every beam from the same restatement, hit wins, one update per call; a
//     second scan from the door on top of the first; masks() is the call with no beams;
//   beams_from_ranges: axis-aligned beams of whole-cell length, a return outside the grid, no return, ends beyond int32;
//   planner with range_scan and a closed wall: no goal and no known cell lies in the right room, the estimate never
//     contradicts the true grid, and the loop ends with the whole left room known;
//   planner with both flags off: the result of test_frontier.cpp's scenario, the disc allocated as before, map untouched.
// Exit code 0 and "scan OK" = all passed.
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

using ray = std::array<int32_t, 4>;

// Walk(a, b) by the definition: the cells of the bounding box whose closed unit square meets the closed segment (doubled
// coordinates; the square is clipped to the box of the two centres, where the segment is its whole line), in sequence order,
// up to the first one outside the grid.  Returns cell indices.
static std::vector<int32_t> walk_naive(int W, int H, const ray& r) {
    const int ax = r[0], ay = r[1], bx = r[2], by = r[3];
    const long long ux = 2LL * (bx - ax), uy = 2LL * (by - ay);
    const int X0 = 2 * std::min(ax, bx), X1 = 2 * std::max(ax, bx), Y0 = 2 * std::min(ay, by), Y1 = 2 * std::max(ay, by);
    const bool xmajor = std::abs(bx - ax) >= std::abs(by - ay);
    std::vector<std::array<int, 4>> cells;   // (major distance, minor distance, x, y)
    for (int y = std::min(ay, by); y <= std::max(ay, by); ++y)
        for (int x = std::min(ax, bx); x <= std::max(ax, bx); ++x) {
            const int xs[2] = {std::max(2 * x - 1, X0), std::min(2 * x + 1, X1)}, ys[2] = {std::max(2 * y - 1, Y0), std::min(2 * y + 1, Y1)};
            long long lo = 1, hi = -1;
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) {
                    const long long s = ux * (ys[j] - 2 * ay) - uy * (xs[i] - 2 * ax);
                    if (i + j == 0) lo = hi = s;
                    lo = std::min(lo, s); hi = std::max(hi, s);
                }
            if (lo <= 0 && hi >= 0) cells.push_back({xmajor ? std::abs(x - ax) : std::abs(y - ay), xmajor ? std::abs(y - ay) : std::abs(x - ax), x, y});
        }
    std::sort(cells.begin(), cells.end());
    std::vector<int32_t> out;
    for (const auto& c : cells) {
        if (c[2] < 0 || c[3] < 0 || c[2] >= W || c[3] >= H) break;
        out.push_back(c[3] * W + c[2]);
    }
    return out;
}

static bool ray_ok(int W, int H, const ray& r) {
    return r[0] >= 0 && r[1] >= 0 && r[0] < W && r[1] < H && std::llabs((long long)r[2] - r[0]) <= SC_SCAN_MAX_REACH &&
           std::llabs((long long)r[3] - r[1]) <= SC_SCAN_MAX_REACH;
}

static std::vector<int32_t> cast_naive(const occupancy_grid& g, const std::vector<ray>& rays) {
    std::vector<int32_t> hit(rays.size(), SC_SCAN_IGNORED);
    for (size_t k = 0; k < rays.size(); ++k) {
        if (!ray_ok(g.W, g.H, rays[k]) || g.occ[(size_t)rays[k][1] * g.W + rays[k][0]]) continue;
        hit[k] = SC_SCAN_NO_RETURN;
        for (int32_t c : walk_naive(g.W, g.H, rays[k]))
            if (g.occ[c]) { hit[k] = c; break; }
    }
    return hit;
}

// L after one call, and the two masks
static void update_naive(int W, int H, std::vector<int32_t>& L, const std::vector<ray>& rays, const std::vector<int32_t>& hit,
                         const logodds_params& p, std::vector<uint8_t>& occ_est, std::vector<uint8_t>& known) {
    std::vector<uint8_t> miss(L.size(), 0), struck(L.size(), 0);
    for (size_t k = 0; k < rays.size(); ++k) {
        if (!ray_ok(W, H, rays[k]) || hit[k] < SC_SCAN_NO_RETURN || hit[k] >= W * H) continue;
        if (hit[k] >= 0) struck[hit[k]] = 1;
        for (int32_t c : walk_naive(W, H, rays[k])) {
            if (c == hit[k]) break;
            miss[c] = 1;
        }
    }
    occ_est.assign(L.size(), 0); known.assign(L.size(), 0);
    for (size_t c = 0; c < L.size(); ++c) {
        L[c] = std::clamp(L[c] + (struck[c] ? p.l_hit : miss[c] ? -p.l_miss : 0), -p.l_clamp, p.l_clamp);
        occ_est[c] = L[c] >= p.t_occ;
        known[c] = L[c] >= p.t_occ || L[c] <= -p.t_free;
    }
}

int main() {
    const bounding_rect br{5.0f, -5.0f, 5.0f, -5.0f};
    planning_space space(br);
    obstacle lower({Vector2f(0.0f, -5.0f), Vector2f(0.0f, -0.5f)}, {{0, 1}}), upper({Vector2f(0.0f, 0.5f), Vector2f(0.0f, 5.0f)}, {{0, 1}});
    lower.closed = upper.closed = false;
    space.obstacles = {lower, upper};
    space.grid_cells = 100;
    const Vector2f start(-2.5f, 0.0f);
    const float radius = 3.0f;

    // ---- scan_cast and logodds_grid against a host restatement ----
    const occupancy_grid g = space.make_grid();
    CHECK(g.W == 100 && g.H == 100);
    const int32_t sc0 = g.cell_of(start), door = g.cell_of(Vector2f(-0.25f, 0.0f));
    CHECK(!g.occ[sc0] && !g.occ[door]);
    int in_wall = -1;
    for (int x = 0; x < g.W; ++x)
        if (g.occ[20 * g.W + x]) in_wall = x;
    CHECK(in_wall >= 49 && in_wall <= 51);
    const int ax = sc0 % g.W, ay = sc0 / g.W;
    std::vector<ray> first = square_fan(ax, ay, 30);
    CHECK(first.size() == 240);
    const std::vector<ray> odd{{ax, ay, ax, ay}, {ax, ay, -7, ay + 3}, {ax, ay, 130, 140}, {ax, ay, ax + 2, -9}, {ax, ay, 99, 99}, {0, 0, 99, 99},
                               {-1, 50, 20, 50}, {50, 100, 50, 20}, {ax, ay, ax + SC_SCAN_MAX_REACH + 1, ay}, {in_wall, 20, 0, 20},
                               {ax, ay, ax + 300, ay - 290}};
    first.insert(first.end(), odd.begin(), odd.end());
    const auto hit = g.scan_cast(first);
    const auto want_hit = cast_naive(g, first);
    int hits = 0, none = 0, ignored = 0, through = 0;
    for (size_t k = 0; k < first.size(); ++k) {
        CHECK(hit[k] == want_hit[k]);
        hits += hit[k] >= 0; none += hit[k] == SC_SCAN_NO_RETURN; ignored += hit[k] == SC_SCAN_IGNORED;
        if (hit[k] >= 0) CHECK(g.occ[hit[k]]);
    }
    CHECK(hits > 20 && none > 100 && ignored == 4);
    CHECK(g.scan_cast({}).empty());
    const logodds_params p{5, 3, 8, 5, 3};
    logodds_grid map(g.W, g.H);
    std::vector<int32_t> want_L(map.L.size(), 0);
    std::vector<uint8_t> want_est, want_known;
    auto m = map.update(first, hit, p);
    update_naive(g.W, g.H, want_L, first, hit, p, want_est, want_known);
    CHECK(map.L == want_L && m.occ_est == want_est && m.known == want_known);
    for (int32_t c = 0; c < g.W * g.H; ++c) {
        if (map.L[c] > 0) CHECK(g.occ[c]);                                              // soundness
        if (map.L[c] < 0) CHECK(!g.occ[c]);
        through += map.L[c] < 0 && c % g.W > in_wall;
    }
    CHECK(through > 0);                                                                 // beyond the wall: through the door
    // a second scan from the door on top of the first, then the same scan again: the cells count once per call
    const std::vector<ray> second = square_fan(door % g.W, door / g.W, 20);
    const auto hit2 = g.scan_cast(second);
    CHECK(hit2 == cast_naive(g, second));
    for (int rep = 0; rep < 2; ++rep) {
        m = map.update(second, hit2, p);
        update_naive(g.W, g.H, want_L, second, hit2, p, want_est, want_known);
        CHECK(map.L == want_L && m.occ_est == want_est && m.known == want_known);
    }
    const auto stored = map.masks(p);
    CHECK(stored.occ_est == m.occ_est && stored.known == m.known && map.L == want_L);
    // hit wins over the misses of the same call; a recorded hit off the walk
    logodds_grid small(8, 2);
    const auto sm = small.update({{0, 0, 7, 0}, {0, 0, 5, 0}, {0, 0, 7, 0}, {1, 0, 3, 0}, {0, 1, 3, 1}}, {-1, 3, 3, SC_SCAN_IGNORED, 5}, p);
    CHECK((small.L == std::vector<int32_t>{-3, -3, -3, 5, -3, 5, -3, -3, -3, -3, -3, -3, 0, 0, 0, 0}));
    CHECK(sm.occ_est[3] && sm.occ_est[5] && !sm.occ_est[0] && sm.known[0] && !sm.known[12]);

    // ---- beams_from_ranges: axis-aligned beams of whole-cell length ----
    {
        const Vector2f o = g.centre_of(50 * g.W + 25);
        const float pi = 3.14159265358979f, res = g.resolution;
        const auto b = beams_from_ranges(g, o, {0.0f, 0.5f * pi, pi, -0.5f * pi, 0.0f, -0.5f * pi, 0.0f}, {10 * res, 7 * res, 25 * res, 3 * res, std::numeric_limits<float>::infinity(), 70 * res, 200 * res},
                                         120 * res);
        const std::vector<ray> want{{25, 50, 35, 50}, {25, 50, 25, 57}, {25, 50, 0, 50}, {25, 50, 25, 47}, {25, 50, 145, 50}, {25, 50, 25, -20}, {25, 50, 145, 50}};
        CHECK(b.rays == want);
        CHECK((b.hit == std::vector<int32_t>{50 * 100 + 35, 57 * 100 + 25, 50 * 100, 47 * 100 + 25, SC_SCAN_NO_RETURN, SC_SCAN_NO_RETURN, SC_SCAN_NO_RETURN}));
        // ends beyond any int32 are held at a distance at which the beam is ignored
        const int32_t far = SC_MAX_DIM + SC_SCAN_MAX_REACH + 1;
        const auto huge = beams_from_ranges(g, o, {0.0f, pi}, {3.0e30f, std::numeric_limits<float>::infinity()}, 3.0e38f);
        CHECK((huge.rays[0] == ray{25, 50, far, 50}) && huge.rays[1][2] == -far && huge.hit[0] == SC_SCAN_NO_RETURN && huge.hit[1] == SC_SCAN_NO_RETURN);
        logodds_grid rec(g.W, g.H);
        rec.update(huge.rays, huge.hit);
        CHECK(rec.L == std::vector<int32_t>(rec.L.size(), 0));
        rec.update(b.rays, b.hit);
        CHECK(rec.L[50 * 100 + 35] == 2 && rec.L[50 * 100 + 34] == -1 && rec.L[50 * 100 + 99] == -1 && rec.L[25] == -1 && rec.L[50 * 100] == 2);
    }

    // ---- planner, range scans, a closed wall ----
    planning_space closed(br);
    obstacle wall({Vector2f(0.0f, -5.0f), Vector2f(0.0f, 5.0f)}, {{0, 1}});
    wall.closed = false;
    closed.obstacles = {wall};
    closed.grid_cells = 50;                                                             // 50 x 50 cells: a fan of half-side 15
    const occupancy_grid cg = closed.make_grid();
    int wall_col = -1;
    CHECK(cg.W == 50 && cg.H == 50);
    for (int x = 0; x < cg.W; ++x)
        if (cg.occ[25 * cg.W + x]) wall_col = x;
    CHECK(wall_col >= 24 && wall_col <= 26);
    for (int y = 0; y < cg.H; ++y) CHECK(cg.occ[(size_t)y * cg.W + wall_col]);          // no gap
    planner pl(closed);
    pl.range_scan = true;
    Vector2f pos = start;
    std::vector<uint8_t> before;
    int steps = 0, wall_known = 0;
    bool ended = false;
    for (; steps < 200 && !ended; ++steps) {
        try {
            pos = pl.pick_next_goal_point(pos, 16, radius);                            // the nearest frontier
        } catch (const std::runtime_error&) {
            ended = true;
        }
        CHECK(pl.ps.free_space_allocations.empty());                                    // no disc is allocated
        while (!pl.goal_point_cache.empty()) pl.goal_point_cache.pop();                 // no fall-back: the loop ends with the frontier
        CHECK(pl.seen.size() == cg.occ.size() && pl.map.L.size() == cg.occ.size());
        for (int32_t c = 0; c < cg.W * cg.H; ++c) {
            if (!before.empty()) CHECK(pl.seen[c] >= before[c]);                        // on a static map known only grows
            if (c % cg.W > wall_col) CHECK(!pl.seen[c] && pl.map.L[c] == 0);            // nothing behind the wall
            if (pl.map.L[c] > 0) CHECK(cg.occ[c]);                                      // the estimate never contradicts the grid
            if (pl.map.L[c] < 0) CHECK(!cg.occ[c]);
        }
        before = pl.seen;
        if (!ended) CHECK(cg.cell_of(pos) % cg.W < wall_col && !cg.occ[cg.cell_of(pos)]);   // the goal lies in the robot's room
    }
    CHECK(ended && steps >= 2);
    for (int32_t c = 0; c < cg.W * cg.H; ++c) {
        if (c % cg.W < wall_col) CHECK(pl.seen[c] && pl.map.L[c] < 0);                  // the left room
        wall_known += c % cg.W == wall_col && pl.seen[c];
    }
    CHECK(wall_known > 0);
    planner both(closed);
    both.range_scan = both.line_of_sight = true;
    bool threw = false;
    try { both.pick_next_goal_point(start, 16, radius); } catch (const std::logic_error&) { threw = true; }
    CHECK(threw);

    // ---- planner, both flags off: the disc, as before ----
    planning_space seen_space = space;
    seen_space.free_space_allocations.push_back([start, radius](Vector2f p) { return pt_dist(p, start) <= radius; });
    occupancy_grid dg = seen_space.make_grid();
    const std::vector<uint8_t> known = seen_space.known_grid(dg.W, dg.H);
    dg.edt();
    const auto solo = dg.explore_goals(known, {dg.cell_of(start)}, 0, 1, 16);
    planner plain(space);
    CHECK(!plain.line_of_sight && !plain.range_scan);
    const Vector2f next = plain.pick_next_goal_point(start, 16, radius);
    CHECK(plain.ps.free_space_allocations.size() == 1 && plain.seen.empty() && plain.map.L.empty());
    CHECK(solo.goal[0] >= 0 && dg.cell_of(next) == solo.goal[0]);
    int reachable = 0;
    for (int k = 0; k < 16; ++k) reachable += solo.cost[k] != SC_FIELD_INF;
    CHECK((int)plain.goal_point_cache.size() == reachable - 1);
    std::printf("scan: %d hits, %d no-returns, %d ignored of %zu beams, %d cells missed beyond the wall, %d planner steps, %d of %d wall cells known\nscan OK\n",
                hits, none, ignored, first.size(), through, steps, wall_known, cg.H);
    return 0;
}
