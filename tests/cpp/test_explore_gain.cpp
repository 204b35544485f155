// occupancy_grid::frontier_centres / explore_goals_by_gain and planner::gain_weight through sea-current_amd/sea_current.hpp, on
// the two-room world of test_views.cpp: bounding_rect {5, -5, 5, -5}, 100 cells, a wall along x = 0 with a door of one unit at
// y = 0, the robot in the left room at (-2.5, 0) with a sensing radius of 3.
//   the two header calls against the C statement (explore_gain_ref.c, linked in): the centres of the frontier clusters of
//     what one look reveals; the picks of two robots for the full circle and for a sensor of 4 of 16 headings, on the fields
//     the header call returns; the identity sum(ggain) = free cells newly known;
//   planner with gain_weight = 0: the goals of a planner that never heard of the member; with gain_weight > 0: the goal and
//     goal_heading are explore_goals_by_gain's on the observed map, which are the C statement's; std::logic_error without
//     line_of_sight.
// Exit code 0 and "explore_gain OK" = all passed.
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

extern "C" int ex_explore_gain(const uint8_t* occ, const uint8_t* known, const int32_t* g, int R, const int32_t* cand, int N, int W, int H,
                               int32_t r2, const int32_t* dirs, int B, int span, int32_t wg, int32_t wc, int32_t min_gain, int rounds,
                               int32_t* goal, int32_t* gcost, int32_t* ggain, int32_t* head, int32_t* cand_of, int32_t* pick, int32_t* npick,
                               int32_t* gain0, int32_t* gain_end, uint8_t* known_out);
extern "C" void ex_frontier_centres(const int32_t* slot, const int32_t* csize, const int64_t* csum, int W, int H, int Cmax, int32_t* centre);

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

using view = std::array<int32_t, 3>;

// the header call's result against the C statement on the same fields and centres; 0 when every output is equal
static int equals_statement(const occupancy_grid& og, const std::vector<uint8_t>& known, const occupancy_grid::gain_result& r, int32_t r2,
                            const heading_table& dirs, int span, int32_t wg) {
    const int R = (int)r.goal.size(), N = (int)r.centre.size();
    std::vector<int32_t> goal(R), gcost(R), ggain(R), head(R), cand_of(R), pick(R), gain0(N), gain_end(N);
    std::vector<uint8_t> kout(known.size());
    int32_t npick = -7;
    CHECK(ex_explore_gain(og.occ.data(), known.data(), r.g.data(), R, r.centre.data(), N, og.W, og.H, r2, dirs.empty() ? nullptr : dirs[0].data(),
                          (int)dirs.size(), span, wg, 1, 1, R, goal.data(), gcost.data(), ggain.data(), head.data(), cand_of.data(), pick.data(),
                          &npick, gain0.data(), gain_end.data(), kout.data()) == 0);
    CHECK(goal == r.goal && gcost == r.gcost && ggain == r.ggain && head == r.head && cand_of == r.cand_of && pick == r.pick);
    CHECK(npick == r.npick && gain0 == r.gain0 && gain_end == r.gain_end && kout == r.known_out);
    long sum = 0, fresh = 0;
    for (int32_t v : r.ggain) sum += v;
    for (size_t c = 0; c < known.size(); ++c) fresh += !og.occ[c] && r.known_out[c] && !known[c];
    CHECK(sum == fresh);
    return 0;
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

    // ---- the header calls against the C statement ----
    const occupancy_grid g = space.make_grid();
    CHECK(g.W == 100 && g.H == 100);
    const int32_t sc0 = g.cell_of(start);
    const int r2 = (int)((radius / g.resolution) * (radius / g.resolution));
    const auto look = g.known_from_views({view{sc0 % g.W, sc0 / g.W, r2}});
    occupancy_grid og = g;                                                              // the observed map
    og.occ = look.occ_seen;
    og.edt();
    const int Cmax = 32;
    const auto fr = og.frontiers(look.known, 0, 2, Cmax);
    CHECK(fr.listed >= 2);
    const std::vector<int32_t> centres = og.frontier_centres(fr);
    std::vector<int32_t> want(Cmax, -7);
    ex_frontier_centres(fr.slot.data(), fr.csize.data(), fr.csum.data(), og.W, og.H, Cmax, want.data());
    CHECK(centres == want);
    for (int k = 0; k < Cmax; ++k) CHECK(k < std::min(fr.listed, Cmax) ? (centres[k] >= 0 && fr.slot[centres[k]] == k) : centres[k] == -1);
    const std::vector<int32_t> robots{sc0, g.cell_of(Vector2f(-3.5f, 2.0f))};
    CHECK(look.known[robots[1]] && !og.occ[robots[1]]);
    const auto full = og.explore_goals_by_gain(look.known, robots, r2, {}, 0, 2, 1, 1, 0, 2, Cmax);
    CHECK(full.centre == centres && full.npick == 2 && full.goal[0] >= 0 && full.goal[1] >= 0 && full.goal[0] != full.goal[1]);
    CHECK(full.head[0] == -1 && full.head[1] == -1 && full.fr.listed == fr.listed && full.fr.slot == fr.slot);
    if (equals_statement(og, look.known, full, r2, {}, 0, 2)) return 1;
    const heading_table dirs = heading_dirs(16);
    const auto fov = og.explore_goals_by_gain(look.known, robots, r2, dirs, 4, 2, 1, 1, 0, 2, Cmax);
    CHECK(fov.npick == 2 && fov.head[0] >= 0 && fov.head[0] < 16 && fov.head[1] >= 0 && fov.head[1] < 16);
    if (equals_statement(og, look.known, fov, r2, dirs, 4, 2)) return 1;
    CHECK(og.explore_goals_by_gain(look.known, {}, r2).goal.empty());
    bool threw = false;
    try { og.explore_goals_by_gain(look.known, robots, r2, dirs, 16); } catch (const std::exception&) { threw = true; }   // span == B
    CHECK(threw);

    // ---- planner ----
    planner plain(space), zero(space);
    plain.line_of_sight = zero.line_of_sight = true;
    zero.gain_weight = 0;
    CHECK(plain.gain_weight == 0);
    Vector2f pa = start, pb = start;
    for (int step = 0; step < 3; ++step) {
        pa = plain.pick_next_goal_point(pa, 16, radius);
        pb = zero.pick_next_goal_point(pb, 16, radius);
        CHECK(g.cell_of(pa) == g.cell_of(pb) && plain.seen == zero.seen && plain.goal_point_cache.size() == zero.goal_point_cache.size());
    }
    for (int span : {0, 4}) {
        planner pl(space);
        pl.line_of_sight = true;
        pl.gain_weight = 2;
        pl.fov_span = span;
        pl.heading = 0;                                                                 // a fixed first look for the sector sensor
        const Vector2f next = pl.pick_next_goal_point(start, Cmax, radius);
        // the same by hand: the planner's look, the observed map, the header call (equal to the C statement above)
        occupancy_grid seen_g = g;
        seen_g.occ = look.occ_seen;
        std::vector<uint8_t> known = look.known;
        if (span) {
            auto first = g.known_from_sectors({sector_view(view{sc0 % g.W, sc0 / g.W, r2}, dirs, 0, span)});
            size_t cells = 0;
            for (uint8_t k : first.known) cells += k != 0;
            CHECK(cells > 0);                                                           // else the planner would have turned on the spot
            known = first.known;
            seen_g.occ = first.occ_seen;
        }
        CHECK(pl.seen == known);
        seen_g.edt();
        const float cc = space.clearance / g.resolution;                                // the planner's clearance in cells, squared
        const auto by_hand = seen_g.explore_goals_by_gain(known, {sc0}, r2, span ? dirs : heading_table{}, span, 2, 1, 1,
                                                          (int32_t)std::ceil(cc * cc), 1, Cmax);
        CHECK(by_hand.goal[0] >= 0 && g.cell_of(next) == by_hand.goal[0] && pl.goal_heading == by_hand.head[0]);
        CHECK(span ? (pl.goal_heading >= 0 && pl.goal_heading < 16) : pl.goal_heading == -1);
        if (equals_statement(seen_g, known, by_hand, r2, span ? dirs : heading_table{}, span, 2)) return 1;
        CHECK(pl.goal_point_cache.empty() && pl.ps.free_space_allocations.empty());
    }
    planner wrong(space);
    wrong.gain_weight = 1;
    threw = false;
    try { wrong.pick_next_goal_point(start, 16, radius); } catch (const std::logic_error&) { threw = true; }
    CHECK(threw && wrong.ps.free_space_allocations.empty());
    std::printf("explore_gain: %d clusters listed, gains of the two picks %d + %d (full circle), %d + %d (4 of 16 headings)\nexplore_gain OK\n",
                fr.listed, full.ggain[0], full.ggain[1], fov.ggain[0], fov.ggain[1]);
    return 0;
}
