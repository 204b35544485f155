// planning_space::plan_assigned through sea-current_amd/sea_current.hpp, on a small version of the world of test_fields.cpp
// (bounding_rect {4.4, -3.3, 4.4, -3.3}, 150 cells, clearance 2 cells, the examples' polygons scaled by 3):
//   plan_assigned(starts, goals, costs).paths[q] == plan_to(starts, goals[goal[q]])[q]
// with more starts than goals and more goals than starts, simplify_paths off and on, without and with goal costs, and once
// with the soft-clearance knobs on.  Every goal is used at most once, as many starts have one as the largest matching over the
// pairs plan_to finds a path for (a start inside an obstacle has none: nullopt, goal -1, cost -1), and the costs add up to total.
// Exit code 0 and "assign OK" = all passed.
#include <cstdio>
#include <set>

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

// Kuhn's augmenting paths: the most (start, goal) pairs over the pairs with a path
static bool augment(const std::vector<plans>& ref, size_t q, std::vector<int>& owner, std::vector<char>& seen) {
    for (size_t k = 0; k < ref.size(); ++k) {
        if (!ref[k][q] || seen[k]) continue;
        seen[k] = 1;
        if (owner[k] < 0 || augment(ref, (size_t)owner[k], owner, seen)) { owner[k] = (int)q; return true; }
    }
    return false;
}

int main() {
    const bounding_rect br{4.4f, -3.3f, 4.4f, -3.3f};
    planning_space space(br);
    const float s = 3.0f;
    space.obstacles = {obstacle({Vector2f(-0.5f * s, 0), Vector2f(1 * s, 0), Vector2f(1 * s, 1 * s), Vector2f(0, 1 * s)}),
                       obstacle({Vector2f(0, -0.5f * s), Vector2f(1 * s, 0), Vector2f(1 * s, 1 * s), Vector2f(0, 1 * s)}),
                       obstacle({Vector2f(-0.6f * s, 0.148f * s), Vector2f(-1 * s, 0.148f * s), Vector2f(-1 * s, 0),
                                 Vector2f(-0.6f * s, 0)})};
    space.grid_cells = 150;
    space.clearance = 2.0f * (br.x_max - br.x_min) / 150.0f;
    std::vector<Vector2f> pts;
    halton_state hx, hy;
    while (pts.size() < 13) {
        const float u = halton(2, 1, hx)[0], v = halton(3, 1, hy)[0];
        const Vector2f p(br.x_min + (br.x_max - br.x_min) * u, br.y_min + (br.y_max - br.y_min) * v);
        if (!std::get<0>(space.is_obstacle(p))) pts.push_back(p);
    }
    const std::vector<int32_t> all_costs = {0, 350, 120, 900, 40, 10, 0};
    int found = 0;
    for (int mode = 0; mode < 6; ++mode) {
        // modes 0 .. 3: 5 goals and 7 starts, simplify off / on, without / with goal costs; 4: 7 goals and 5 starts; 5: soft knobs on
        const size_t n_goal = mode == 4 ? 7 : 5, n_start = mode == 4 ? 4 : 7;
        space.simplify_paths = (mode & 1) != 0;
        const bool with_costs = (mode & 2) != 0 || mode >= 4;
        space.soft_clearance = mode == 5 ? 6.0f * (br.x_max - br.x_min) / 150.0f : 0.0f;
        space.soft_penalty = mode == 5 ? 40 : 0;
        const std::vector<Vector2f> goals(pts.begin(), pts.begin() + n_goal);
        std::vector<Vector2f> starts(pts.begin() + 7, pts.begin() + 7 + std::min(n_start, (size_t)6));
        starts.push_back(Vector2f(1.5f, 1.5f));   // inside an obstacle: no goal
        const std::vector<int32_t> costs = with_costs ? std::vector<int32_t>(all_costs.begin(), all_costs.begin() + n_goal) : std::vector<int32_t>{};
        const auto ar = space.plan_assigned(starts, goals, costs);
        CHECK(ar.paths.size() == starts.size() && ar.goal.size() == starts.size() && ar.cost.size() == starts.size());
        std::vector<plans> ref;
        for (const auto& gl : goals) ref.push_back(space.plan_to(starts, gl));
        std::set<int32_t> taken;
        int64_t sum = 0, with_goal = 0;
        for (size_t q = 0; q < starts.size(); ++q) {
            if (ar.goal[q] < 0) { CHECK(!ar.paths[q] && ar.cost[q] == -1); continue; }
            CHECK(ar.goal[q] < (int32_t)goals.size() && ar.cost[q] >= 0 && taken.insert(ar.goal[q]).second);
            CHECK(same(ar.paths[q], ref[(size_t)ar.goal[q]][q]));
            CHECK(ar.paths[q]->front() == starts[q] && ar.paths[q]->back() == goals[(size_t)ar.goal[q]]);
            sum += ar.cost[q];
            ++with_goal;
            ++found;
        }
        CHECK(ar.goal.back() == -1);
        std::vector<int> owner(goals.size(), -1);
        int64_t most = 0;
        for (size_t q = 0; q < starts.size(); ++q) {
            std::vector<char> seen(goals.size(), 0);
            most += augment(ref, q, owner, seen);
        }
        CHECK(most >= 3 && with_goal == most && ar.matched == with_goal && ar.total == sum);
    }
    CHECK(space.plan_assigned({}, {Vector2f(0, -2)}).paths.empty());
    CHECK(space.plan_assigned({Vector2f(0, -2)}, {}).goal == std::vector<int32_t>({-1}));
    int threw = 0;
    try { space.plan_assigned({Vector2f(0, -2)}, {Vector2f(0, -2.5f)}, {1, 2}); } catch (const std::invalid_argument&) { ++threw; }
    try { space.plan_assigned({Vector2f(0, -2)}, {Vector2f(0, -2.5f)}, {-1}); } catch (const std::runtime_error&) { ++threw; }
    CHECK(threw == 2);
    std::printf("plan_assigned: %d paths\nassign OK\n", found);
    return 0;
}
