// Polygon obstacles rasterised on the GPU through the successor header:
//   (a) planning_space::make_grid(ctx).occ == make_grid().occ (the host rasteriser) on the examples' world, the non-dyadic
//       world of test_waypoints.cpp at 300 and 1024 cells, a 2000-gon, a comb, a bow-tie, an edge-list obstacle whose
//       vertex 0 no edge uses, and obstacles past the frame;
//   (b) plan_batch (which now rasterises on the GPU) on 64 Halton queries of the non-dyadic world equals the old route:
//       the host make_grid(), then the same EDT and A* calls;
//   (c) a world whose left 60 % is one filled polygon, on a context of its own: the second EDT (the open-space build)
//       equals the first.
#include <cfloat>
#include <cmath>
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("CHECK failed: %s (line %d)\n", #c, __LINE__); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static std::vector<obstacle> examples_obstacles(float s) {
    return {obstacle({Vector2f(-0.5f * s, 0), Vector2f(1 * s, 0), Vector2f(1 * s, 1 * s), Vector2f(0, 1 * s)}),
            obstacle({Vector2f(0, -0.5f * s), Vector2f(1 * s, 0), Vector2f(1 * s, 1 * s), Vector2f(0, 1 * s)}),
            obstacle({Vector2f(-0.6f * s, 0.148f * s), Vector2f(-1 * s, 0.148f * s), Vector2f(-1 * s, 0), Vector2f(-0.6f * s, 0)})};
}

static planning_space nondyadic(int cells) {
    planning_space space(bounding_rect{4.4f, -3.3f, 4.4f, -3.3f});
    space.obstacles = examples_obstacles(3.0f);
    obstacle wall({Vector2f(-2.5f, -2.0f), Vector2f(-0.5f, -2.8f)}, {{0, 1}});
    wall.closed = false;
    space.obstacles.push_back(wall);
    space.grid_cells = cells;
    return space;
}

static int same_grid(const planning_space& space, gpu_context& ctx, const char* name) {
    const occupancy_grid h = space.make_grid(), d = space.make_grid(ctx);
    CHECK(h.W == d.W && h.H == d.H && h.occ == d.occ);
    size_t set = 0;
    for (uint8_t v : h.occ) set += v;
    CHECK(set > 0 && set < h.occ.size());
    std::printf("  %-22s %5d x %-5d %8zu cells set\n", name, h.W, h.H, set);
    return 0;
}

int main() {
    gpu_context ctx(0);
    // (a)
    {
        planning_space ex(bounding_rect{1, -1, 1, -1});
        ex.obstacles = examples_obstacles(1.0f);
        if (same_grid(ex, ctx, "examples")) return 1;
        if (same_grid(nondyadic(300), ctx, "non-dyadic 300")) return 1;
        if (same_grid(nondyadic(1024), ctx, "non-dyadic 1024")) return 1;
        planning_space w(bounding_rect{5, -5, 5, -5});
        w.grid_cells = 1024;
        std::vector<Vector2f> ngon, comb;
        for (int i = 0; i < 2000; ++i) {
            const float a = (float)i * (2.0f * 3.14159265f / 2000.0f), r = 3.0f + 0.8f * std::sin(7.0f * a);
            ngon.push_back(Vector2f(r * std::cos(a), r * std::sin(a)));
        }
        comb.push_back(Vector2f(-4.5f, -4.5f));
        for (int i = 0; i < 200; ++i) {
            const float x0 = -4.5f + 9.0f * (float)(2 * i) / 400.0f, x1 = -4.5f + 9.0f * (float)(2 * i + 1) / 400.0f,
                        x2 = -4.5f + 9.0f * (float)(2 * i + 2) / 400.0f;
            comb.push_back(Vector2f(x0, 4.0f)); comb.push_back(Vector2f(x1, 4.0f));
            comb.push_back(Vector2f(x1, -4.0f)); comb.push_back(Vector2f(x2, i == 199 ? -4.5f : -4.0f));
        }
        w.obstacles = {obstacle(ngon)};
        if (same_grid(w, ctx, "2000-gon")) return 1;
        w.obstacles = {obstacle(comb)};
        if (same_grid(w, ctx, "comb")) return 1;
        w.obstacles = {obstacle({Vector2f(-4, -3.5f), Vector2f(4, 3.5f), Vector2f(4, -3.5f), Vector2f(-4, 3.5f)}),
                       obstacle({Vector2f(-4.9f, 4.9f), Vector2f(-2, -2), Vector2f(2, -1), Vector2f(0.5f, 2.5f)}, {{1, 2}, {2, 3}, {3, 1}}),
                       obstacle({Vector2f(-7, 0.3f), Vector2f(-3, 0.4f), Vector2f(-4, 1.6f)}),
                       obstacle({Vector2f(6, 6), Vector2f(8, 6), Vector2f(8, 8)})};
        w.grid_cells = 333;
        if (same_grid(w, ctx, "bow-tie, edge list, out")) return 1;
    }
    // (b)
    {
        planning_space space = nondyadic(300);
        space.clearance = 2.0f * (8.8f / 300.0f);
        const bounding_rect& br = space.bound_rect;
        std::vector<Vector2f> starts, goals;
        halton_state hx, hy;
        while (starts.size() < 64 || goals.size() < 64) {
            const float u = halton(2, 1, hx)[0], v = halton(3, 1, hy)[0];
            const Vector2f p(br.x_min + (br.x_max - br.x_min) * u, br.y_min + (br.y_max - br.y_min) * v);
            if (std::get<0>(space.is_obstacle(p))) continue;
            (starts.size() <= goals.size() ? starts : goals).push_back(p);
        }
        const auto got = space.plan_batch(starts, goals, ctx);
        occupancy_grid g = space.make_grid();   // the old route: host grid, then the same EDT and A* calls
        g.edt(ctx);
        std::vector<int32_t> s(64), t(64);
        for (int q = 0; q < 64; ++q) { s[q] = g.cell_of(starts[q]); t[q] = g.cell_of(goals[q]); }
        const float cc = space.clearance / g.resolution;
        const auto br2 = g.astar_batch(s, t, (int32_t)std::ceil(cc * cc), 0, ctx);
        int found = 0;
        CHECK(got.size() == 64);
        for (int q = 0; q < 64; ++q) {
            CHECK(got[q].has_value() == (br2.status[q] == SC_Q_OK));
            if (!got[q]) continue;
            ++found;
            const auto& w = *got[q];
            CHECK((int)w.size() == std::max(2, br2.len[q]));
            CHECK(w.front() == starts[q] && w.back() == goals[q]);
            for (int i = 1; i + 1 < br2.len[q]; ++i) CHECK(w[i] == g.centre_of(br2.path[(size_t)q * br2.Lmax + i]));
        }
        CHECK(found >= 32);
        std::printf("  plan_batch: %d of 64 paths equal the host-grid route\n", found);
    }
    // (c)
    {
        gpu_context own(0);
        planning_space space(bounding_rect{5, -5, 5, -5});
        space.grid_cells = 1024;
        space.obstacles = {obstacle({Vector2f(-5.1f, -5.1f), Vector2f(1.0f, -5.1f), Vector2f(1.0f, 5.1f), Vector2f(-5.1f, 5.1f)})};
        occupancy_grid g = space.make_grid(own);
        g.edt(own);
        const std::vector<int32_t> first = g.d2;
        g.edt(own);
        CHECK(g.d2 == first);
        CHECK(first[(size_t)512 * g.W + g.W - 1] > 175 * 175);
        std::printf("  left 60 %%: second EDT equals the first (max d2 %d)\n", first[(size_t)512 * g.W + g.W - 1]);
    }
    std::printf("polygons OK\n");
    return 0;
}
