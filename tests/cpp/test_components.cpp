// occupancy_grid::components, planning_space::reachable and plan_batch(..., screen = true) through
// sea-current_amd/sea_current.hpp, on the non-dyadic world of test_fields.cpp (bounding_rect {4.4, -3.3, 4.4, -3.3}, 300
// cells, clearance 2 cells, the examples' polygons scaled by 3 and an open two-vertex wall) plus one walled-off room:
//   reachable(a, b) is true between points of the open space, false into the room, into an obstacle and out of the room;
//   plan_batch(starts, goals, ctx, true) == plan_batch(starts, goals), with nullopt for every query into the room;
//   the labels are canonical (label[label[c]] == label[c] <= c) and the sizes add up to the traversable cells.
// Exit code 0 and "components OK" = all passed.
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
    // a room of 1 x 1 around (3.5, -2.5): four walls, no door
    obstacle room({Vector2f(3.0f, -3.0f), Vector2f(4.0f, -3.0f), Vector2f(4.0f, -2.0f), Vector2f(3.0f, -2.0f)}, {{0, 1}, {1, 2}, {2, 3}, {3, 0}});
    room.closed = false;
    space.obstacles.push_back(room);
    space.grid_cells = 300;
    space.clearance = 2.0f * (br.x_max - br.x_min) / 300.0f;
    const Vector2f inside(3.5f, -2.5f), centre(-3.9f, 3.9f), in_obstacle(1.5f, 1.5f);

    CHECK(space.reachable(centre, Vector2f(3.9f, 3.9f)));
    CHECK(space.reachable(centre, centre));
    CHECK(space.reachable(inside, Vector2f(3.52f, -2.48f)));
    CHECK(!space.reachable(centre, inside));
    CHECK(!space.reachable(inside, centre));
    CHECK(!space.reachable(centre, in_obstacle));

    std::vector<Vector2f> pts;
    halton_state hx, hy;
    while (pts.size() < 40) {
        const float u = halton(2, 1, hx)[0], v = halton(3, 1, hy)[0];
        const Vector2f p(br.x_min + (br.x_max - br.x_min) * u, br.y_min + (br.y_max - br.y_min) * v);
        if (!std::get<0>(space.is_obstacle(p))) pts.push_back(p);
    }
    pts.push_back(inside);
    pts.push_back(in_obstacle);
    int found = 0, none = 0;
    for (bool simp : {false, true}) {
        space.simplify_paths = simp;
        const std::vector<Vector2f> starts(pts.size(), centre);
        const plans ref = space.plan_batch(starts, pts);
        const plans scr = space.plan_batch(starts, pts, default_context(), true);
        CHECK(ref.size() == pts.size() && scr.size() == pts.size());
        for (size_t q = 0; q < pts.size(); ++q) {
            CHECK(same(scr[q], ref[q]));
            CHECK(scr[q].has_value() == space.reachable(centre, pts[q]));
            (scr[q] ? found : none) += 1;
        }
        CHECK(!scr[pts.size() - 2].has_value() && !scr[pts.size() - 1].has_value());
        // out of the room: hopeless, but for the query that stays inside
        const plans out = space.plan_batch(std::vector<Vector2f>(pts.size(), inside), pts, default_context(), true);
        const plans out_ref = space.plan_batch(std::vector<Vector2f>(pts.size(), inside), pts);
        int left = 0;
        for (size_t q = 0; q < pts.size(); ++q) {
            CHECK(same(out[q], out_ref[q]) && out[q].has_value() == space.reachable(inside, pts[q]));
            left += out[q].has_value();
        }
        CHECK(out[pts.size() - 2].has_value() && left <= 4);
    }
    CHECK(found >= 40 && none >= 4);

    occupancy_grid g = space.make_grid();
    g.edt();
    const float cc = space.clearance / g.resolution;
    const int32_t r2 = (int32_t)std::ceil(cc * cc);
    const auto cr = g.components(r2);
    CHECK(cr.ncomp >= 2 && cr.largest >= 0);
    long long cells = 0, trav = 0;
    int32_t roots = 0;
    for (int32_t c = 0; c < g.W * g.H; ++c) {
        const int32_t l = cr.label[c];
        CHECK((l >= 0) == (g.d2[c] >= std::max(r2, (int32_t)1)));
        if (l < 0) { CHECK(cr.size[c] == 0); continue; }
        ++trav;
        CHECK(l <= c && cr.label[l] == l);
        if (l == c) { ++roots; CHECK(cr.size[c] >= 1 && cr.size[c] <= cr.size[cr.largest]); }
        else CHECK(cr.size[c] == 0);
        cells += cr.size[c];
    }
    CHECK(cells == trav && roots == cr.ncomp);
    CHECK(cr.label[g.cell_of(inside)] != cr.label[g.cell_of(centre)]);
    const auto st = g.reachable(cr, {g.cell_of(centre), g.cell_of(centre), -1}, {g.cell_of(inside), g.cell_of(Vector2f(3.9f, 3.9f)), 0});
    CHECK(st[0] == SC_Q_NO_PATH && st[1] == SC_Q_OK && st[2] == SC_Q_BAD_ENDPOINT);
    std::printf("plan_batch screened: %d paths, %d without; %d components\ncomponents OK\n", found, none, cr.ncomp);
    return 0;
}
