// planning_space::plan_from / plan_to through sea-current_amd/sea_current.hpp, on a non-dyadic world (bounding_rect
// {4.4, -3.3, 4.4, -3.3}, 300 cells, clearance 2 cells) with the examples' polygons scaled by 3 and an open two-vertex wall:
//   plan_from(start, goals) == plan_batch(std::vector(goals.size(), start), goals), and
//   plan_to(starts, goal)   == plan_batch({goal}, {starts[q]})[0] reversed (simplify_paths off), or the waypoints of the
//                              start..goal cell path with the exact ends (simplify_paths on),
// for both settings of simplify_paths, with goals and starts from the Halton sequence plus one inside an obstacle.  Also
// occupancy_grid::field_paths against astar_batch on the same grid.  Exit code 0 and "fields OK" = all passed.
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
    while (pts.size() < 48) {
        const float u = halton(2, 1, hx)[0], v = halton(3, 1, hy)[0];
        const Vector2f p(br.x_min + (br.x_max - br.x_min) * u, br.y_min + (br.y_max - br.y_min) * v);
        if (!std::get<0>(space.is_obstacle(p))) pts.push_back(p);
    }
    pts.push_back(Vector2f(1.5f, 1.5f));   // inside an obstacle: no path either way
    const Vector2f centre(-3.9f, 3.9f);
    int found = 0;
    for (bool simp : {false, true}) {
        space.simplify_paths = simp;
        const plans from = space.plan_from(centre, pts);
        const plans ref_from = space.plan_batch(std::vector<Vector2f>(pts.size(), centre), pts);
        CHECK(from.size() == pts.size() && ref_from.size() == pts.size());
        for (size_t q = 0; q < pts.size(); ++q) CHECK(same(from[q], ref_from[q]));
        CHECK(!from.back().has_value());
        const plans to = space.plan_to(pts, centre);
        CHECK(to.size() == pts.size());
        for (size_t q = 0; q < pts.size(); ++q) {
            const plans back = space.plan_batch({centre}, {pts[q]});
            CHECK(to[q].has_value() == back[0].has_value());
            if (!to[q]) continue;
            ++found;
            CHECK(to[q]->front() == pts[q] && to[q]->back() == centre);
            if (!simp) {
                std::vector<Vector2f> rev(back[0]->rbegin(), back[0]->rend());
                CHECK(*to[q] == rev);
            }
        }
        if (simp) {
            // the waypoints of the start..goal cell paths
            occupancy_grid g = space.make_grid();
            g.edt();
            const float cc = space.clearance / g.resolution;
            const int32_t r2 = (int32_t)std::ceil(cc * cc);
            std::vector<int32_t> st(pts.size()), qf(pts.size(), 0);
            for (size_t q = 0; q < pts.size(); ++q) st[q] = g.cell_of(pts[q]);
            auto fr = g.cost_fields({g.cell_of(centre)}, r2);
            CHECK(fr.status[0] == SC_Q_OK);
            auto bp = g.field_paths(fr, qf, st, 0, true);
            auto wr = g.waypoints_batch(bp, r2);
            auto ab = g.astar_batch(std::vector<int32_t>(pts.size(), g.cell_of(centre)), st, r2);
            for (size_t q = 0; q < pts.size(); ++q) {
                CHECK(bp.status[q] == ab.status[q] && bp.len[q] == ab.len[q] && bp.cost[q] == ab.cost[q]);
                if (bp.status[q] != SC_Q_OK) continue;
                for (int i = 0; i < bp.len[q]; ++i) CHECK(bp.path[q * bp.Lmax + i] == ab.path[q * ab.Lmax + bp.len[q] - 1 - i]);
                CHECK(wr.status[q] == SC_Q_OK);
                const auto& w = *to[q];
                CHECK((int)w.size() == std::max(wr.n[q], 2));
                for (int i = 1; i + 1 < wr.n[q]; ++i) CHECK(w[i] == g.centre_of(wr.wp[q * wr.Wmax + i]));
            }
        }
    }
    CHECK(found >= 64);
    std::printf("plan_from / plan_to: %d paths\nfields OK\n", found);
    return 0;
}
