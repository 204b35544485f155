// planning_space::plan_to_nearest and occupancy_grid::cost_fields_multi / field_paths_multi through
// sea-current_amd/sea_current.hpp, on the non-dyadic world of test_fields.cpp (bounding_rect {4.4, -3.3, 4.4, -3.3}, 300
// cells, clearance 2 cells, the examples' polygons scaled by 3 and an open two-vertex wall):
//   plan_to_nearest(starts, goals, costs).paths[q] == plan_to(starts, goals[goal[q]])[q]
// for both settings of simplify_paths, without and with goal costs, and once with the soft-clearance knobs on; a start
// inside an obstacle has no path, goal -1 and cost -1.  On the grid: field_paths_multi against astar_batch from the
// owning seed, and the chosen goal is a cheapest one.  Exit code 0 and "multi fields OK" = all passed.
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

using plans = std::vector<std::optional<std::vector<Vector2f>>>;

static bool same(const std::optional<std::vector<Vector2f>>& a, const std::optional<std::vector<Vector2f>>& b) {
    if (a.has_value() != b.has_value()) return false;
    return !a || *a == *b;
}

int main() {
    const bounding_rect br{4.4f, -3.3f, 4.4f, -3.3f};
    planning_space space(br);
    const float s = 3.0f;
    space.obstacles = {obstacle({Vector2f(-0.5f * s, 0), Vector2f(1 * s, 0), Vector2f(1 * s, 1 * s), Vector2f(0, 1 * s)}),
                       obstacle({Vector2f(0, -0.5f * s), Vector2f(1 * s, 0), Vector2f(1 * s, 1 * s), Vector2f(0, 1 * s)}),
                       obstacle({Vector2f(-0.6f * s, 0.148f * s), Vector2f(-1 * s, 0.148f * s), Vector2f(-1 * s, 0),
                                 Vector2f(-0.6f * s, 0)})};
    obstacle wall({Vector2f(-2.5f, -2.0f), Vector2f(-0.5f, -2.8f)}, {{0, 1}});
    wall.closed = false;
    space.obstacles.push_back(wall);
    space.grid_cells = 300;
    space.clearance = 2.0f * (br.x_max - br.x_min) / 300.0f;
    std::vector<Vector2f> pts;
    halton_state hx, hy;
    while (pts.size() < 37) {
        const float u = halton(2, 1, hx)[0], v = halton(3, 1, hy)[0];
        const Vector2f p(br.x_min + (br.x_max - br.x_min) * u, br.y_min + (br.y_max - br.y_min) * v);
        if (!std::get<0>(space.is_obstacle(p))) pts.push_back(p);
    }
    const std::vector<Vector2f> goals(pts.begin(), pts.begin() + 5);
    std::vector<Vector2f> starts(pts.begin() + 5, pts.end());
    starts.push_back(Vector2f(1.5f, 1.5f));   // inside an obstacle: no path
    const std::vector<int32_t> costs = {0, 350, 120, 900, 40};
    int found = 0;
    for (int mode = 0; mode < 5; ++mode) {
        // simplify off / on, without / with goal costs; then the soft knobs on
        space.simplify_paths = (mode & 1) != 0;
        const bool with_costs = (mode & 2) != 0 || mode == 4;
        space.soft_clearance = mode == 4 ? 6.0f * (br.x_max - br.x_min) / 300.0f : 0.0f;
        space.soft_penalty = mode == 4 ? 40 : 0;
        const auto nr = space.plan_to_nearest(starts, goals, with_costs ? costs : std::vector<int32_t>{});
        CHECK(nr.paths.size() == starts.size() && nr.goal.size() == starts.size() && nr.cost.size() == starts.size());
        std::vector<plans> ref;
        for (const auto& gl : goals) ref.push_back(space.plan_to(starts, gl));
        for (size_t q = 0; q < starts.size(); ++q) {
            if (nr.goal[q] < 0) {
                CHECK(!nr.paths[q] && nr.cost[q] == -1);
                for (const auto& r : ref) CHECK(!r[q]);
                continue;
            }
            CHECK(nr.goal[q] < (int32_t)goals.size() && nr.cost[q] >= 0);
            CHECK(same(nr.paths[q], ref[(size_t)nr.goal[q]][q]));
            CHECK(nr.paths[q]->front() == starts[q] && nr.paths[q]->back() == goals[(size_t)nr.goal[q]]);
            ++found;
        }
        CHECK(nr.goal.back() == -1);
    }
    CHECK(found >= 5 * 21);   // two thirds of the free starts, the share test_fields.cpp asks of the same world
    {   // on the grid: the read-out against A* from the owning seed; the owner is a cheapest seed
        occupancy_grid g = space.make_grid();
        g.edt();
        const float cc = space.clearance / g.resolution;
        const int32_t r2 = (int32_t)std::ceil(cc * cc);
        std::vector<int32_t> seeds, tg, qf(starts.size(), 0);
        for (const auto& p : goals) seeds.push_back(g.cell_of(p));
        for (const auto& p : starts) tg.push_back(g.cell_of(p));
        auto fr = g.cost_fields_multi(seeds, {0, 5}, costs, r2);
        CHECK(fr.status[0] == SC_Q_OK);
        auto single = g.cost_fields(seeds, r2);
        auto mp = g.field_paths_multi(fr, qf, tg);
        std::vector<int32_t> from(tg.size());
        for (size_t q = 0; q < tg.size(); ++q) from[q] = seeds[(size_t)std::max(mp.which[q], 0)];
        auto ab = g.astar_batch(from, tg, r2);
        const size_t n = (size_t)g.W * g.H;
        for (size_t q = 0; q < tg.size(); ++q) {
            if (mp.which[q] < 0) { CHECK(mp.status[q] != SC_Q_OK && mp.len[q] == 0 && mp.cost[q] == -1); continue; }
            CHECK(mp.status[q] == ab.status[q] && mp.len[q] == ab.len[q] && mp.cost[q] - costs[(size_t)mp.which[q]] == ab.cost[q]);
            CHECK(mp.which[q] == fr.owner[(size_t)tg[q]]);
            for (int i = 0; i < mp.len[q]; ++i) CHECK(mp.path[q * mp.Lmax + i] == ab.path[q * ab.Lmax + i]);
            for (size_t k = 0; k < 5; ++k) {
                const int32_t gk = single.g[k * n + (size_t)tg[q]];
                CHECK(gk == SC_FIELD_INF || (int64_t)gk + costs[k] >= mp.cost[q]);
            }
        }
    }
    std::printf("plan_to_nearest: %d paths\nmulti fields OK\n", found);
    return 0;
}
