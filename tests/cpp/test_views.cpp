// occupancy_grid::known_from_views / view_gain and planner::line_of_sight through sea-current_amd/sea_current.hpp, on the
// two-room world of test_frontier.cpp: bounding_rect {5, -5, 5, -5}, 100 cells, a wall along x = 0 with a door of one unit at
// y = 0, the robot in the left room at (-2.5, 0) with a sensing radius of 3.
//   known_from_views: against a restatement on the host -- a free cell is seen iff it lies in the disc and no cell whose unit
//     square meets the segment from the centre is occupied (the four-corner sign test over the bounding box, no column walk);
//     an occupied cell is known iff it borders a seen one; occ_seen = occ where known; a second call with the first as base
//     only adds; views that are ignored add nothing;
//   view_gain: for every candidate the count of unknown cells the restatement sees, and the identity with known_from_views;
//   planner with line_of_sight and a closed wall: no goal and no seen cell lies in the right room, seen only grows, and the
//     loop ends with the whole left room seen;
//   planner without it: the result of test_frontier.cpp's scenario, the disc allocated as before, seen untouched.
// Exit code 0 and "views OK" = all passed.
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

using view = std::array<int32_t, 3>;

// Clear(a, b) by the definition: every cell of the bounding box whose closed unit square meets the closed segment is free.
// Doubled coordinates; the square is clipped to the box of the two centres, where the segment is its whole line.
static bool clear_naive(const occupancy_grid& g, int ax, int ay, int bx, int by) {
    const long long ux = 2 * (bx - ax), uy = 2 * (by - ay);
    const int X0 = 2 * std::min(ax, bx), X1 = 2 * std::max(ax, bx), Y0 = 2 * std::min(ay, by), Y1 = 2 * std::max(ay, by);
    for (int y = std::min(ay, by); y <= std::max(ay, by); ++y)
        for (int x = std::min(ax, bx); x <= std::max(ax, bx); ++x) {
            if (!g.occ[(size_t)y * g.W + x]) continue;
            const int xs[2] = {std::max(2 * x - 1, X0), std::min(2 * x + 1, X1)}, ys[2] = {std::max(2 * y - 1, Y0), std::min(2 * y + 1, Y1)};
            long long lo = 1, hi = -1;
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) {
                    const long long s = ux * (ys[j] - 2 * ay) - uy * (xs[i] - 2 * ax);
                    if (i + j == 0) lo = hi = s;
                    lo = std::min(lo, s); hi = std::max(hi, s);
                }
            if (lo <= 0 && hi >= 0) return false;
        }
    return true;
}

static std::vector<uint8_t> seen_naive(const occupancy_grid& g, const view& v) {
    std::vector<uint8_t> vis(g.occ.size(), 0);
    const int cx = v[0], cy = v[1];
    if (v[2] < 0 || cx < 0 || cy < 0 || cx >= g.W || cy >= g.H || g.occ[(size_t)cy * g.W + cx]) return vis;
    for (int y = 0; y < g.H; ++y)
        for (int x = 0; x < g.W; ++x)
            if ((long long)(x - cx) * (x - cx) + (long long)(y - cy) * (y - cy) <= v[2] && clear_naive(g, cx, cy, x, y)) vis[(size_t)y * g.W + x] = 1;
    return vis;
}

static std::vector<uint8_t> known_naive(const occupancy_grid& g, const std::vector<view>& views, const std::vector<uint8_t>& base) {
    std::vector<uint8_t> vis(g.occ.size(), 0), known(g.occ.size(), 0);
    for (const auto& v : views) {
        const auto one = seen_naive(g, v);
        for (size_t c = 0; c < vis.size(); ++c) vis[c] |= one[c];
    }
    for (int y = 0; y < g.H; ++y)
        for (int x = 0; x < g.W; ++x) {
            const size_t c = (size_t)y * g.W + x;
            const bool nb = (x > 0 && vis[c - 1]) || (x + 1 < g.W && vis[c + 1]) || (y > 0 && vis[c - g.W]) || (y + 1 < g.H && vis[c + g.W]);
            known[c] = ((!base.empty() && base[c]) || vis[c] || (g.occ[c] && nb)) ? 1 : 0;
        }
    return known;
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

    // ---- the header calls against a host restatement ----
    const occupancy_grid g = space.make_grid();
    CHECK(g.W == 100 && g.H == 100);
    const int32_t sc0 = g.cell_of(start);
    const int r2 = (int)((radius / g.resolution) * (radius / g.resolution));
    CHECK(r2 >= 899 && r2 <= 900);
    const std::vector<view> first{{sc0 % g.W, sc0 / g.W, r2}};
    const auto a = g.known_from_views(first);
    const auto want_a = known_naive(g, first, {});
    int n_known = 0, beyond = 0, disc_beyond = 0, walls = 0;
    for (int32_t c = 0; c < g.W * g.H; ++c) {
        CHECK(a.known[c] == want_a[c] && a.occ_seen[c] == (a.known[c] ? g.occ[c] : 0));
        n_known += a.known[c];
        walls += a.occ_seen[c] != 0;
        const Vector2f p = g.centre_of(c);
        beyond += a.known[c] && p.x() > 0.2f;
        disc_beyond += pt_dist(p, start) <= radius && p.x() > 0.2f;
    }
    CHECK(n_known > 1000 && walls > 10 && beyond > 0 && beyond < disc_beyond);          // beyond the wall: through the door only
    // a second look from the door, on top of the first; ignored views add nothing
    const int32_t door = g.cell_of(Vector2f(-0.25f, 0.0f));
    CHECK(!g.occ[door]);
    int in_wall = -1;
    for (int x = 0; x < g.W; ++x)
        if (g.occ[20 * g.W + x]) in_wall = x;
    CHECK(in_wall >= 49 && in_wall <= 51);
    const std::vector<view> second{{door % g.W, door / g.W, 400}, {-1, 50, 400}, {50, 100, 400}, {10, 10, -1}, {in_wall, 20, 400}};   // the last one stands in the wall
    const auto b = g.known_from_views(second, a.known);
    const auto want_b = known_naive(g, second, a.known);
    int more = 0;
    for (int32_t c = 0; c < g.W * g.H; ++c) {
        CHECK(b.known[c] == want_b[c] && b.known[c] >= a.known[c] && b.occ_seen[c] == (b.known[c] ? g.occ[c] : 0));
        more += b.known[c] - a.known[c];
    }
    CHECK(more > 100);
    const auto none = g.known_from_views({}, a.known);
    CHECK(none.known == a.known);
    // view_gain: a recount, and what known_from_views newly marks
    const auto gain = g.view_gain(a.known, second);
    CHECK(gain.size() == second.size() && gain[0] > 0 && gain[1] == 0 && gain[2] == 0 && gain[3] == 0 && gain[4] == 0);
    const std::vector<view> cands{{20, 50, 225}, {49, 50, 900}, {51, 50, 900}, {80, 80, 100}, {sc0 % g.W, sc0 / g.W, r2}};
    const auto gc = g.view_gain(a.known, cands);
    for (size_t i = 0; i < cands.size(); ++i) {
        const auto vis = seen_naive(g, cands[i]);
        const auto one = g.known_from_views({cands[i]}, a.known);
        int count = 0, fresh = 0;
        for (int32_t c = 0; c < g.W * g.H; ++c) {
            count += vis[c] && !a.known[c];
            fresh += one.known[c] && !a.known[c] && !g.occ[c];
        }
        CHECK(gc[i] == count && gc[i] == fresh);
    }
    CHECK(gc[4] == 0 && gc[2] > gc[0]);
    CHECK(g.view_gain(a.known, {}).empty());

    // ---- planner, line of sight, a closed wall ----
    planning_space closed(br);
    obstacle wall({Vector2f(0.0f, -5.0f), Vector2f(0.0f, 5.0f)}, {{0, 1}});
    wall.closed = false;
    closed.obstacles = {wall};
    closed.grid_cells = 50;                                                             // 50 x 50 cells: a radius of 15
    const occupancy_grid cg = closed.make_grid();
    int wall_col = -1;
    CHECK(cg.W == 50 && cg.H == 50);
    for (int x = 0; x < cg.W; ++x)
        if (cg.occ[25 * cg.W + x]) wall_col = x;
    CHECK(wall_col >= 24 && wall_col <= 26);
    for (int y = 0; y < cg.H; ++y) CHECK(cg.occ[(size_t)y * cg.W + wall_col]);          // no gap
    planner pl(closed);
    pl.line_of_sight = true;
    Vector2f pos = start;
    std::vector<uint8_t> before;
    int steps = 0;
    bool ended = false;
    for (; steps < 200 && !ended; ++steps) {
        try {
            pos = pl.pick_next_goal_point(pos, 16, radius);                            // the nearest frontier
        } catch (const std::runtime_error&) {
            ended = true;
        }
        CHECK(pl.ps.free_space_allocations.empty());                                    // no disc is allocated
        while (!pl.goal_point_cache.empty()) pl.goal_point_cache.pop();                 // no fall-back: the loop ends with the frontier
        CHECK(pl.seen.size() == cg.occ.size());
        for (int32_t c = 0; c < cg.W * cg.H; ++c) {
            if (!before.empty()) CHECK(pl.seen[c] >= before[c]);                        // seen only grows
            if (c % cg.W > wall_col) CHECK(!pl.seen[c]);                                // nothing behind the wall
        }
        before = pl.seen;
        if (!ended) CHECK(cg.cell_of(pos) % cg.W < wall_col && !cg.occ[cg.cell_of(pos)]);   // the goal lies in the robot's room
    }
    CHECK(ended && steps >= 2);
    for (int32_t c = 0; c < cg.W * cg.H; ++c)
        if (c % cg.W <= wall_col) CHECK(pl.seen[c]);                                    // the left room and the wall's face

    // ---- planner, flag off: the disc, as before ----
    planning_space seen_space = space;
    seen_space.free_space_allocations.push_back([start, radius](Vector2f p) { return pt_dist(p, start) <= radius; });
    occupancy_grid dg = seen_space.make_grid();
    const std::vector<uint8_t> known = seen_space.known_grid(dg.W, dg.H);
    dg.edt();
    const auto solo = dg.explore_goals(known, {dg.cell_of(start)}, 0, 1, 16);
    planner plain(space);
    CHECK(!plain.line_of_sight);
    const Vector2f next = plain.pick_next_goal_point(start, 16, radius);
    CHECK(plain.ps.free_space_allocations.size() == 1 && plain.seen.empty());
    CHECK(solo.goal[0] >= 0 && dg.cell_of(next) == solo.goal[0]);
    int reachable = 0;
    for (int k = 0; k < 16; ++k) reachable += solo.cost[k] != SC_FIELD_INF;
    CHECK((int)plain.goal_point_cache.size() == reachable - 1);
    std::printf("views: %d known cells through the door (%d beyond the wall, the disc has %d), %d more from the door, %d planner steps\nviews OK\n",
                n_known, beyond, disc_beyond, more, steps);
    return 0;
}
