// Re-planning in space-time through sea-current_amd/sea_current.hpp: fleet_schedule, then fleet_replan, on the corridor with a
// pocket of tests/test_tplan_twin.py.  A corridor one cell wide along row 2 of an 11 x 4 grid of unit cells, a pocket two cells
// deep above column 3; one robot drives from x = 10 to x = 0 at one cell a second and parks there, radius 0.3; the other wants
// to go from x = 0 to x = 10.  Head-on in a corridor no start delay helps: fleet_schedule leaves the second path unresolved at
// every slot.  fleet_replan then finds the exact answer of the twin: in at (3, 2) at tick 3, up the pocket, wait at (3, 0) through
// tick 8, back down, arrival at tick 17 (10 in free space).  Without the pocket there is no path.
// Exit code 0 and "replan OK" = all passed.
#include <cmath>
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

// 11 samples 1 s apart along row 2, from the centre of column x0 to that of column x1
static smooth_result drive(int x0, int x1) {
    smooth_result r;
    r.status = SC_SMOOTH_OK;
    r.spline.pts = points_matrix::Zero(11, 2);
    toppra_compat::Vector t(11);
    for (int i = 0; i < 11; ++i) {
        r.spline.pts(i, 0) = (float)x0 + 0.5f + (float)(x1 - x0) * (float)i / 10.0f;
        r.spline.pts(i, 1) = 2.5f;
        t(i) = (double)i;
    }
    r.profile.time = t;
    return r;
}

static occupancy_grid corridor(bool pocket) {
    occupancy_grid g(bounding_rect(11.f, 0.f, 4.f, 0.f), 11, 4);
    for (int y = 0; y < 4; ++y)
        for (int x = 0; x < 11; ++x) g.occ[(size_t)y * 11 + x] = !(y == 2 || (pocket && x == 3 && y < 2));
    g.edt();
    return g;
}

int main() {
    typedef std::vector<int> ints;
    const int W = 11;
    const std::vector<smooth_result> paths{drive(10, 0), drive(0, 10)};
    const std::vector<double> radius{0.3, 0.3};
    const ints start{2 * W + 10, 2 * W}, goal{2 * W, 2 * W + 10};
    for (int D : {1, 8, 32}) {
        const schedule_result s = fleet_schedule(paths, radius, {}, {3, 3}, {}, 1.0, D);
        CHECK(s.slot == ints({0, SC_SLOT_UNRESOLVED}));
    }
    const schedule_result s = fleet_schedule(paths, radius, {}, {3, 3}, {}, 1.0, 8);
    const occupancy_grid with = corridor(true), without = corridor(false);
    for (bool sequential : {true, false}) {
        replan_result r = fleet_replan(paths, radius, s, with, start, goal, 0.3, {}, {3, 3}, 1.0, 1, sequential);
        CHECK(r.status == ints({-1, SC_TP_OK}) && r.arrive == ints({-1, 17}) && r.t_start == ints({0, 0}) && r.path[0].empty());
        CHECK(r.path[1] == ints({2 * W, 2 * W + 1, 2 * W + 2, 2 * W + 3, W + 3, 3, 3, 3, 3, W + 3, 2 * W + 3, 2 * W + 4, 2 * W + 5, 2 * W + 6, 2 * W + 7,
                                 2 * W + 8, 2 * W + 9, 2 * W + 10}));
        CHECK(r.K == 10 + 2 * (11 + 4));   // the end of the last path, no slot > 0, the default extra ticks
        r = fleet_replan(paths, radius, s, without, start, goal, 0.3, {}, {3, 3}, 1.0, 1, sequential);
        CHECK(r.status == ints({-1, SC_TP_NO_PATH}) && r.arrive == ints({-1, -1}) && r.path[1].empty());
    }
    // a start delay: the robot appears at tick 12, when the other one is parked at x = 0 and the corridor is free from x = 2 on
    replan_result r = fleet_replan(paths, radius, s, with, {0, 2 * W + 2}, goal, 0.3, {0.0, 11.5}, {3, 3}, 1.0);
    CHECK(r.status[1] == SC_TP_OK && r.t_start[1] == 12 && r.arrive[1] == 20 && (int)r.path[1].size() == 9);
    // nothing unresolved: nothing to plan
    schedule_result none = s;
    none.slot = {0, 0};
    r = fleet_replan(paths, radius, none, with, start, goal, 0.3, {}, {3, 3}, 1.0);
    CHECK(r.status == ints({-1, -1}) && r.path[1].empty());
    int threw = 0;
    try { fleet_replan(paths, radius, s, with, {0}, goal, 0.3); } catch (const std::invalid_argument&) { ++threw; }
    try { fleet_replan(paths, radius, s, with, start, goal, -0.3); } catch (const std::invalid_argument&) { ++threw; }
    try { fleet_replan(paths, radius, s, with, start, goal, 0.3, {}, {}, 1.0, 0); } catch (const std::invalid_argument&) { ++threw; }
    occupancy_grid raw(bounding_rect(11.f, 0.f, 4.f, 0.f), 11, 4);
    try { fleet_replan(paths, radius, s, raw, start, goal, 0.3); } catch (const std::invalid_argument&) { ++threw; }
    CHECK(threw == 4);
    std::printf("replan OK\n");
    return 0;
}
