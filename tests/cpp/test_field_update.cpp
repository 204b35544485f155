// occupancy_grid::cost_fields_update through sea-current_amd/sea_current.hpp, on a two-room world: a wall across the middle
// with one door that closes and opens again.  Per frame the repaired fields equal cost_fields of the new grid, in g and
// status: plain, with a costmap from the soft knobs (computed again per grid) and with a caller's own costmap (kept).
// The stats say what a frame cost: a closed door raises the whole far room, an opened one raises nothing.
// Exit code 0 and "field update OK" = all passed.
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

int main() {
    const bounding_rect br{5.0f, -5.0f, 5.0f, -5.0f};
    planning_space open_space(br), closed_space(br);
    // the wall x in [-0.2, 0.2] with a door y in [-0.6, 0.6]
    open_space.obstacles = {obstacle({Vector2f(-0.2f, 0.6f), Vector2f(0.2f, 0.6f), Vector2f(0.2f, 5.0f), Vector2f(-0.2f, 5.0f)}),
                            obstacle({Vector2f(-0.2f, -5.0f), Vector2f(0.2f, -5.0f), Vector2f(0.2f, -0.6f), Vector2f(-0.2f, -0.6f)})};
    closed_space.obstacles = open_space.obstacles;
    closed_space.obstacles.push_back(obstacle({Vector2f(-0.2f, -0.6f), Vector2f(0.2f, -0.6f), Vector2f(0.2f, 0.6f), Vector2f(-0.2f, 0.6f)}));
    open_space.grid_cells = closed_space.grid_cells = 120;
    occupancy_grid open_grid = open_space.make_grid(), closed_grid = closed_space.make_grid();
    open_grid.edt();
    closed_grid.edt();
    CHECK(open_grid.W == closed_grid.W && open_grid.occ != closed_grid.occ);
    const int32_t r2 = 4, r2_soft = 64;
    const int pen_max = 60;
    const std::vector<int32_t> roots{open_grid.cell_of(Vector2f(-4.0f, 3.0f)), open_grid.cell_of(Vector2f(3.0f, -2.0f))};
    const int32_t far_cell = open_grid.cell_of(Vector2f(4.0f, 4.0f));
    std::vector<std::array<int32_t, 2>> stats;

    for (int mode = 0; mode < 3; ++mode) {   // 0: plain, 1: the soft knobs' costmap, 2: a caller's own costmap
        auto build = [&](occupancy_grid& g, const std::vector<uint8_t>& own) {
            if (mode == 0) return g.cost_fields(roots, r2);
            if (mode == 2) return g.cost_fields(roots, own, 200, r2);
            auto f = g.cost_fields(roots, g.clearance_penalty(r2, r2_soft, pen_max), pen_max, r2);
            f.r2_soft = r2_soft;
            f.pen_max = pen_max;
            return f;
        };
        std::vector<uint8_t> own(open_grid.occ.size());
        for (size_t c = 0; c < own.size(); ++c) own[c] = (uint8_t)((c * 2654435761u) >> 24);
        auto fields = build(open_grid, own);
        CHECK(fields.status[0] == SC_Q_OK && fields.status[1] == SC_Q_OK && fields.g[far_cell] != SC_FIELD_INF);
        const size_t n = open_grid.occ.size();
        long long finite_far = 0;   // what field 0 reaches beyond the wall
        for (size_t c = 0; c < n; ++c) finite_far += fields.g[c] != SC_FIELD_INF && (int)(c % open_grid.W) > open_grid.W / 2 + 4;
        CHECK(finite_far > 1000);

        // the door closes
        auto& same = closed_grid.cost_fields_update(open_grid, fields, default_context(), &stats);
        CHECK(&same == &fields);
        auto want = build(closed_grid, own);
        CHECK(fields.g == want.g && fields.status == want.status && fields.pen == want.pen);
        CHECK(fields.g[far_cell] == SC_FIELD_INF && fields.g[n + far_cell] != SC_FIELD_INF);
        CHECK(stats.size() == 2 && stats[0][0] > 0 && stats[0][0] == stats[1][0] && stats[0][1] >= finite_far && stats[1][1] > 1000);
        // nothing changes
        closed_grid.cost_fields_update(closed_grid, fields, default_context(), &stats);
        CHECK(fields.g == want.g && stats[0][0] == 0 && stats[0][1] == 0 && stats[1][1] == 0);
        // the door opens again
        open_grid.cost_fields_update(closed_grid, fields, default_context(), &stats);
        want = build(open_grid, own);
        CHECK(fields.g == want.g && fields.status == want.status && fields.pen == want.pen);
        CHECK(fields.g[far_cell] != SC_FIELD_INF && stats[0][0] > 0);
        if (mode == 0) CHECK(stats[0][1] == 0 && stats[1][1] == 0);   // unweighted: opening a door takes no cell's support
    }
    {   // without stats
        auto fields = open_grid.cost_fields(roots, r2);
        closed_grid.cost_fields_update(open_grid, fields);
        CHECK(fields.g == closed_grid.cost_fields(roots, r2).g);
    }
    // argument errors
    planning_space small_space(br);
    small_space.grid_cells = 50;
    occupancy_grid small = small_space.make_grid();
    auto f = open_grid.cost_fields(roots, r2);
    bool threw = false;
    try { small.cost_fields_update(open_grid, f); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    std::printf("field update OK\n");
    return 0;
}
