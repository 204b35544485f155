// occupancy_grid::frontiers / explore_goals, planning_space::known_grid and planner::pick_next_goal_point through
// sea-current_amd/sea_current.hpp, on a two-room world: bounding_rect {5, -5, 5, -5}, 100 cells, a wall along x = 0 with a
// door of one unit at y = 0, the robot in the left room at (-2.5, 0) with a sensing radius of 3 (the disc crosses the wall, the
// door and the left border, so its frontier ring falls into several clusters).
//   frontiers: against a restatement on the host -- a label is >= 0 exactly on the known, free cells that touch an unknown
//     one, canonical (label[label[c]] == label[c] <= c), equal on cells that touch (diagonals included); the listed rows
//     ascend, their sizes are recounts and add up to the frontier; slot is the row of the cell's cluster;
//   explore_goals: every goal is a frontier cell, goal = cell[r][col_of[r]], gcost = cost[r][col_of[r]] with gain 0, two
//     robots get different clusters, a robot inside an obstacle gets none;
//   planner::pick_next_goal_point: returns the centre of a frontier cell of the disc, the cheapest one; the cache fills with
//     the other clusters' cells, cheapest on top; falls back to the cache when everything is known; throws when that is empty.
// Exit code 0 and "frontier OK" = all passed.
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static bool is_frontier(const occupancy_grid& g, const std::vector<uint8_t>& known, int32_t c) {
    const int W = g.W, H = g.H, x = c % W, y = c / W;
    if (!known[c] || g.d2[c] < 1) return false;
    return (x > 0 && !known[c - 1]) || (x + 1 < W && !known[c + 1]) || (y > 0 && !known[c - W]) || (y + 1 < H && !known[c + W]);
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
    planning_space seen = space;
    seen.free_space_allocations.push_back([start, radius](Vector2f p) { return pt_dist(p, start) <= radius; });
    occupancy_grid g = seen.make_grid();
    CHECK(g.W == 100 && g.H == 100);
    const std::vector<uint8_t> known = seen.known_grid(g.W, g.H);
    int n_known = 0;
    for (int32_t c = 0; c < g.W * g.H; ++c) {
        CHECK(known[c] == (pt_dist(g.centre_of(c), start) <= radius ? 1 : 0));
        n_known += known[c];
    }
    CHECK(n_known > 2000 && n_known < 2900);                         // a disc of radius 30 cells, clipped by the left border
    g.edt();
    const auto fr = g.frontiers(known, 0, 1, 64);
    int n_frontier = 0, roots = 0;
    for (int32_t c = 0; c < g.W * g.H; ++c) {
        const int32_t l = fr.label[c];
        CHECK((l >= 0) == is_frontier(g, known, c));
        if (l < 0) { CHECK(fr.slot[c] == -1); continue; }
        ++n_frontier;
        CHECK(l <= c && fr.label[l] == l);
        roots += l == c;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int x = c % g.W + dx, y = c / g.W + dy;
                if (x < 0 || y < 0 || x >= g.W || y >= g.H) continue;
                if (fr.label[y * g.W + x] >= 0) CHECK(fr.label[y * g.W + x] == l);
            }
        CHECK(fr.slot[c] >= 0 && fr.slot[c] < fr.listed && fr.rep[fr.slot[c]] == l);
    }
    CHECK(fr.total == roots && fr.listed == roots && roots >= 3 && roots <= 64);
    int sum = 0;
    for (int k = 0; k < fr.Cmax; ++k) {
        if (k >= fr.listed) { CHECK(fr.rep[k] == -1 && fr.csize[k] == 0); continue; }
        CHECK(k == 0 || fr.rep[k] > fr.rep[k - 1]);
        int size = 0;
        int64_t sx = 0, sy = 0;
        for (int32_t c = 0; c < g.W * g.H; ++c)
            if (fr.label[c] == fr.rep[k]) {
                ++size; sx += c % g.W; sy += c / g.W;
                CHECK(c % g.W >= fr.cbox[4 * k] && c % g.W <= fr.cbox[4 * k + 2] && c / g.W >= fr.cbox[4 * k + 1] && c / g.W <= fr.cbox[4 * k + 3]);
            }
        CHECK(size == fr.csize[k] && sx == fr.csum[2 * k] && sy == fr.csum[2 * k + 1]);
        sum += size;
    }
    CHECK(sum == n_frontier);
    const auto big = g.frontiers(known, 0, 1000, 64);                // no cluster is that large
    CHECK(big.listed == 0 && big.total == roots && big.rep[0] == -1);

    // two robots in the left room, one inside the wall
    const std::vector<int32_t> robots{g.cell_of(start), g.cell_of(Vector2f(-1.0f, 1.5f)), g.cell_of(Vector2f(0.0f, 2.0f))};
    CHECK(g.d2[robots[2]] == 0);
    const auto ex = g.explore_goals(known, robots, 0, 1, 64);
    CHECK(ex.fr.listed == fr.listed && ex.fr.label == fr.label && ex.fr.rep == fr.rep);
    for (int r = 0; r < 2; ++r) {
        CHECK(ex.goal[r] >= 0 && fr.label[ex.goal[r]] >= 0 && ex.col_of[r] == fr.slot[ex.goal[r]]);
        CHECK(ex.goal[r] == ex.cell[(size_t)r * 64 + ex.col_of[r]] && ex.gcost[r] == ex.cost[(size_t)r * 64 + ex.col_of[r]] && ex.gcost[r] > 0);
    }
    CHECK(ex.col_of[0] != ex.col_of[1]);
    CHECK(ex.goal[2] == -1 && ex.gcost[2] == -1 && ex.col_of[2] == -1);
    for (int k = 0; k < 64; ++k) CHECK(ex.cost[2 * 64 + k] == SC_FIELD_INF && ex.cell[2 * 64 + k] == -1);

    // ---- planner ----
    planner pl(space);
    const Vector2f next = pl.pick_next_goal_point(start, 16, radius);
    CHECK(pl.ps.free_space_allocations.size() == 1);
    const int32_t nc = g.cell_of(next);
    CHECK(fr.label[nc] >= 0 && next.x() == g.centre_of(nc).x() && next.y() == g.centre_of(nc).y());
    // the nearest reachable frontier: robot 0 alone, gain 0
    const auto solo = g.explore_goals(known, {robots[0]}, 0, 1, 16);
    CHECK(solo.goal[0] == nc);
    int reachable = 0;
    for (int k = 0; k < 16; ++k) reachable += solo.cost[k] != SC_FIELD_INF;
    CHECK(reachable >= 3 && (int)pl.goal_point_cache.size() == reachable - 1);
    int32_t last = solo.gcost[0];
    const size_t cached = pl.goal_point_cache.size();
    while (!pl.goal_point_cache.empty()) {                           // cheapest on top, none of the chosen cluster
        const int32_t c = g.cell_of(pl.goal_point_cache.top());
        pl.goal_point_cache.pop();
        const int32_t k = fr.slot[c];
        CHECK(k >= 0 && k != solo.col_of[0] && solo.cell[k] == c && solo.cost[k] >= last);
        last = solo.cost[k];
    }
    // everything known: the cache is the fallback, and the end of it is an error
    planning_space all = space;
    all.free_space_allocations.push_back([](Vector2f) { return true; });
    planner done(all);
    done.goal_point_cache.push(Vector2f(1.0f, 2.0f));
    const Vector2f fb = done.pick_next_goal_point(start, 16, radius);
    CHECK(fb.x() == 1.0f && fb.y() == 2.0f && done.goal_point_cache.empty());
    bool threw = false;
    try {
        done.pick_next_goal_point(start, 16, radius);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    CHECK(threw);
    std::printf("frontier: %d known cells, %d frontier cells in %d clusters, %zu cached goals\nfrontier OK\n", n_known, n_frontier, roots, cached);
    return 0;
}
