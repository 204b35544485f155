// heading_dirs, occupancy_grid::known_from_sectors / sector_gain / view_gain_headings and planner::fov_span through
// sea-current_amd/sea_current.hpp, on the two-room world of test_views.cpp: bounding_rect {5, -5, 5, -5}, 100 cells, a wall
// along x = 0 with a door of one unit at y = 0, the robot in the left room at (-2.5, 0) with a sensing radius of 3.
//   the three header calls against a restatement on the host: In(d; a, b) from the definition in 64-bit integers, Clear by the
//     four-corner sign test over the bounding box, the bin of an offset by trying every bin; the identities (a), (b), (c);
//   planner with fov_span = 4 of 16 headings behind a closed wall: seen only grows, nothing behind the wall is seen, heading
//     and goal_heading stay in range, the loop ends with the robot's room seen; std::logic_error without line_of_sight;
//   planner with fov_span = 0: the results of test_views.cpp's scenario.
// Exit code 0 and "sectors OK" = all passed.
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

using view = std::array<int32_t, 3>;
using sview = std::array<int32_t, 7>;

static long long cross(long long px, long long py, long long qx, long long qy) { return px * qy - py * qx; }
static long long dot(long long px, long long py, long long qx, long long qy) { return px * qx + py * qy; }

// In(d; a, b) for a pair that is not ignored
static bool in_naive(long long dx, long long dy, long long ax, long long ay, long long bx, long long by) {
    if ((dx == 0 && dy == 0) || (ax == 0 && ay == 0 && bx == 0 && by == 0)) return true;
    const long long s = cross(ax, ay, bx, by);
    if (s > 0) return cross(ax, ay, dx, dy) >= 0 && cross(dx, dy, bx, by) > 0;
    if (s < 0) return !(cross(bx, by, dx, dy) >= 0 && cross(dx, dy, ax, ay) > 0);
    return cross(ax, ay, dx, dy) > 0 || (cross(ax, ay, dx, dy) == 0 && dot(ax, ay, dx, dy) > 0);
}

// Clear(a, b) by the definition (test_views.cpp's)
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

// the pairs (a, b) that make an ignored view
static bool ignored_naive(long long ax, long long ay, long long bx, long long by) {
    if (ax == 0 && ay == 0 && bx == 0 && by == 0) return false;
    for (long long v : {ax, ay, bx, by})
        if (v < -32767 || v > 32767) return true;
    if ((ax == 0 && ay == 0) != (bx == 0 && by == 0)) return true;
    return cross(ax, ay, bx, by) == 0 && dot(ax, ay, bx, by) > 0;
}

static std::vector<uint8_t> seen_naive(const occupancy_grid& g, const sview& v) {
    std::vector<uint8_t> vis(g.occ.size(), 0);
    const int cx = v[0], cy = v[1];
    if (ignored_naive(v[3], v[4], v[5], v[6])) return vis;
    if (v[2] < 0 || cx < 0 || cy < 0 || cx >= g.W || cy >= g.H || g.occ[(size_t)cy * g.W + cx]) return vis;
    for (int y = 0; y < g.H; ++y)
        for (int x = 0; x < g.W; ++x)
            if ((long long)(x - cx) * (x - cx) + (long long)(y - cy) * (y - cy) <= v[2] && in_naive(x - cx, y - cy, v[3], v[4], v[5], v[6]) &&
                clear_naive(g, cx, cy, x, y))
                vis[(size_t)y * g.W + x] = 1;
    return vis;
}

static std::vector<uint8_t> known_naive(const occupancy_grid& g, const std::vector<sview>& rows, const std::vector<uint8_t>& base) {
    std::vector<uint8_t> vis(g.occ.size(), 0), known(g.occ.size(), 0);
    for (const auto& v : rows) {
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

    // ---- the table ----
    const heading_table dirs = heading_dirs(16), odd = heading_dirs(5, 0.5);
    CHECK(dirs.size() == 16 && dirs[0][0] == 32767 && dirs[0][1] == 0 && dirs[4][0] == 0 && dirs[4][1] == 32767 && dirs[8][0] == -32767);
    for (size_t b = 0; b < odd.size(); ++b) CHECK(cross(odd[b][0], odd[b][1], odd[(b + 1) % 5][0], odd[(b + 1) % 5][1]) > 0);
    bool threw = false;
    try { heading_dirs(2); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);

    // ---- the header calls against a host restatement ----
    const occupancy_grid g = space.make_grid();
    CHECK(g.W == 100 && g.H == 100);
    const int32_t sc0 = g.cell_of(start), door = g.cell_of(Vector2f(-0.25f, 0.0f));
    const int r2 = (int)((radius / g.resolution) * (radius / g.resolution));
    const view here{sc0 % g.W, sc0 / g.W, r2}, at_door{door % g.W, door / g.W, 400};
    CHECK(!g.occ[door]);
    // a quarter towards the door, half a turn, a reflex sector, and rows that are ignored
    const std::vector<sview> rows{sector_view(here, dirs, 14, 4), sector_view(at_door, dirs, 4, 8), sector_view(at_door, dirs, 2, 13),
                                  {50, 50, 400, 1, 0, 2, 0}, {50, 50, 400, 1, 0, 0, 0}, {10, 10, -1, 1, 0, 0, 1}};
    const auto a = g.known_from_sectors({rows[0]});
    const auto want_a = known_naive(g, {rows[0]}, {});
    int n_known = 0;
    for (int32_t c = 0; c < g.W * g.H; ++c) {
        CHECK(a.known[c] == want_a[c] && a.occ_seen[c] == (a.known[c] ? g.occ[c] : 0));
        n_known += a.known[c];
    }
    CHECK(n_known > 200);
    const auto b = g.known_from_sectors(rows, a.known);
    const auto want_b = known_naive(g, rows, a.known);
    int more = 0;
    for (int32_t c = 0; c < g.W * g.H; ++c) {
        CHECK(b.known[c] == want_b[c] && b.known[c] >= a.known[c] && b.occ_seen[c] == (b.known[c] ? g.occ[c] : 0));
        more += b.known[c] - a.known[c];
    }
    CHECK(more > 100);
    CHECK(g.known_from_sectors({}, a.known).known == a.known);
    // (c): full-circle rows are the views
    const auto full_rows = g.known_from_sectors({sector_view(here, dirs, 3, 16), sector_view(at_door, dirs, 0, 16)}, a.known);
    const auto full_views = g.known_from_views({here, at_door}, a.known);
    CHECK(full_rows.known == full_views.known && full_rows.occ_seen == full_views.occ_seen);
    // sector_gain: a recount
    const auto sg = g.sector_gain(a.known, rows);
    CHECK(sg.size() == rows.size() && sg[0] == 0 && sg[1] > 0 && sg[3] == 0 && sg[4] == 0 && sg[5] == 0);
    for (size_t i = 0; i < 3; ++i) {
        const auto vis = seen_naive(g, rows[i]);
        int count = 0;
        for (int32_t c = 0; c < g.W * g.H; ++c) count += vis[c] && !a.known[c];
        CHECK(sg[i] == count);
    }
    CHECK(g.sector_gain(a.known, {}).empty());
    // view_gain_headings: the histogram by trying every bin, the windows, the first maximum; identities (a) and (b)
    const std::vector<view> cands{here, at_door, {20, 50, 225}, {51, 50, 900}, {-1, 50, 400}, {80, 80, 100}};
    const auto full_gain = g.view_gain(a.known, cands);
    for (int span : {1, 4, 8, 15, 16}) {
        const auto hr = g.view_gain_headings(a.known, cands, dirs, span);
        CHECK(hr.B == 16 && hr.best.size() == cands.size() && hr.hist.size() == cands.size() * 16 && hr.gainh.size() == hr.hist.size());
        for (size_t i = 0; i < cands.size(); ++i) {
            const auto vis = seen_naive(g, {cands[i][0], cands[i][1], cands[i][2], 0, 0, 0, 0});
            std::vector<int32_t> hist(16, 0);
            int c0 = 0;
            for (int32_t c = 0; c < g.W * g.H; ++c) {
                if (!vis[c] || a.known[c]) continue;
                const int dx = c % g.W - cands[i][0], dy = c / g.W - cands[i][1];
                if (dx == 0 && dy == 0) { c0 = 1; continue; }
                int bins = 0;
                for (int k = 0; k < 16; ++k)
                    if (in_naive(dx, dy, dirs[k][0], dirs[k][1], dirs[(k + 1) % 16][0], dirs[(k + 1) % 16][1])) { ++bins; hist[k] += 1; }
                CHECK(bins == 1);
            }
            int sum = c0, first = 0;
            for (int k = 0; k < 16; ++k) { CHECK(hr.hist[i * 16 + k] == hist[k]); sum += hist[k]; }
            CHECK(sum == full_gain[i]);                                                 // (a)
            for (int h = 0; h < 16; ++h) {
                int w = c0;
                for (int j = 0; j < span; ++j) w += hist[(h + j) % 16];
                CHECK(hr.gainh[i * 16 + h] == w);
                if (w > hr.gainh[i * 16 + first]) first = h;
            }
            CHECK(hr.best[i][0] == hr.gainh[i * 16 + first] && hr.best[i][1] == first);
        }
        for (int h = 0; h < 16; h += 5) {                                               // (b)
            std::vector<sview> sr;
            for (const auto& v : cands) sr.push_back(sector_view(v, dirs, h, span));
            const auto gs = g.sector_gain(a.known, sr);
            for (size_t i = 0; i < cands.size(); ++i) CHECK(gs[i] == hr.gainh[i * 16 + h] && (span < 16 || gs[i] == full_gain[i]));
        }
    }
    CHECK(g.view_gain_headings(a.known, {}, dirs, 4).best.empty());
    threw = false;
    try { g.view_gain_headings(a.known, cands, dirs, 17); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);

    // ---- planner, a quarter-circle sensor, a closed wall ----
    planning_space closed(br);
    obstacle wall({Vector2f(0.0f, -5.0f), Vector2f(0.0f, 5.0f)}, {{0, 1}});
    wall.closed = false;
    closed.obstacles = {wall};
    closed.grid_cells = 50;                                                             // 50 x 50 cells: a radius of 15
    const occupancy_grid cg = closed.make_grid();
    int wall_col = -1;
    for (int x = 0; x < cg.W; ++x)
        if (cg.occ[25 * cg.W + x]) wall_col = x;
    CHECK(wall_col >= 24 && wall_col <= 26);
    planner pl(closed);
    pl.line_of_sight = true;
    pl.fov_span = 4;
    CHECK(pl.headings == 16 && pl.heading == -1 && pl.goal_heading == -1);
    Vector2f pos = start;
    std::vector<uint8_t> before;
    int steps = 0;
    bool ended = false;
    for (; steps < 400 && !ended; ++steps) {
        try {
            pos = pl.pick_next_goal_point(pos, 16, radius);
        } catch (const std::runtime_error&) {
            ended = true;
        }
        CHECK(pl.ps.free_space_allocations.empty());
        while (!pl.goal_point_cache.empty()) pl.goal_point_cache.pop();
        CHECK(pl.seen.size() == cg.occ.size() && pl.heading >= 0 && pl.heading < 16);
        size_t grown = 0;
        for (int32_t c = 0; c < cg.W * cg.H; ++c) {
            if (!before.empty()) { CHECK(pl.seen[c] >= before[c]); grown += pl.seen[c] > before[c]; }
            if (c % cg.W > wall_col) CHECK(!pl.seen[c]);
        }
        if (!before.empty()) CHECK(grown > 0);                                          // every look adds a known cell
        before = pl.seen;
        if (!ended) {
            CHECK(cg.cell_of(pos) % cg.W < wall_col && !cg.occ[cg.cell_of(pos)]);
            CHECK(pl.goal_heading >= 0 && pl.goal_heading < 16);
            pl.heading = pl.goal_heading;                                               // arrive looking where most is to be seen
        } else {
            CHECK(pl.goal_heading == -1);
        }
    }
    CHECK(ended && steps >= 3);
    for (int32_t c = 0; c < cg.W * cg.H; ++c)
        if (c % cg.W <= wall_col) CHECK(pl.seen[c]);
    // fov_span without line_of_sight
    planner wrong(closed);
    wrong.fov_span = 4;
    threw = false;
    try { wrong.pick_next_goal_point(start, 16, radius); } catch (const std::logic_error&) { threw = true; }
    CHECK(threw && wrong.ps.free_space_allocations.empty());

    // ---- planner, fov_span = 0: test_views.cpp's scenarios ----
    planner los(closed);
    los.line_of_sight = true;
    const Vector2f los_next = los.pick_next_goal_point(start, 16, radius);
    const int32_t s50 = cg.cell_of(start);
    const float rc = radius / cg.resolution;
    const auto one = cg.known_from_views({{s50 % cg.W, s50 / cg.W, (int32_t)(rc * rc)}});
    CHECK(los.seen == one.known && los.heading == -1 && los.goal_heading == -1 && cg.cell_of(los_next) % cg.W < wall_col);
    planning_space seen_space = space;
    seen_space.free_space_allocations.push_back([start, radius](Vector2f p) { return pt_dist(p, start) <= radius; });
    occupancy_grid dg = seen_space.make_grid();
    const std::vector<uint8_t> known = seen_space.known_grid(dg.W, dg.H);
    dg.edt();
    const auto solo = dg.explore_goals(known, {dg.cell_of(start)}, 0, 1, 16);
    planner plain(space);
    CHECK(!plain.line_of_sight && plain.fov_span == 0);
    const Vector2f next = plain.pick_next_goal_point(start, 16, radius);
    CHECK(plain.ps.free_space_allocations.size() == 1 && plain.seen.empty() && plain.heading == -1 && plain.goal_heading == -1);
    CHECK(solo.goal[0] >= 0 && dg.cell_of(next) == solo.goal[0]);
    int reachable = 0;
    for (int k = 0; k < 16; ++k) reachable += solo.cost[k] != SC_FIELD_INF;
    CHECK((int)plain.goal_point_cache.size() == reachable - 1);
    std::printf("sectors: %d known cells in the first quarter, %d more from the door, %d planner steps with a quarter-circle sensor\nsectors OK\n",
                n_known, more, steps);
    return 0;
}
