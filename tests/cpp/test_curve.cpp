// Curves clear of the grid through sea-current_amd/sea_current.hpp, on the world of test_speed_limits.cpp (bounding_rect
// {4.4, -3.3, 4.4, -3.3}, 300 cells, clearance 2 cells): 24 Halton start/goal pairs planned with plan_batch and
// simplify_paths, then
//   (0) the new members default to "off": clear_r2 = -1, clear_levels = 6, empty tangent_level and leg_min_d2, rounds 0
//       (checked before the GPU is touched);
//   (1) requests that do not ask, smoothed with the grid overload, come back without levels, as before;
//   (2) requests with clear_r2 = 1: every result has a level per waypoint and a minimum per leg; an OK path has no leg over
//       a cell with d2 < 1 and none of its returned points lies in such a cell; a path whose levels are all 0 equals the
//       result of (1) field by field; a path that is not OK reads SC_SMOOTH_COLLIDES with levels at clear_levels;
//   (3) clear_levels outside 1 .. SC_CURVE_MAX_LEVEL throws.
// Exit code 0 and "curve clear OK" = all passed.
#include <cmath>
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static std::vector<obstacle> examples_obstacles(float s) {
    return {obstacle({Vector2f(-0.5f * s, 0), Vector2f(1 * s, 0), Vector2f(1 * s, 1 * s), Vector2f(0, 1 * s)}),
            obstacle({Vector2f(0, -0.5f * s), Vector2f(1 * s, 0), Vector2f(1 * s, 1 * s), Vector2f(0, 1 * s)}),
            obstacle({Vector2f(-0.6f * s, 0.148f * s), Vector2f(-1 * s, 0.148f * s), Vector2f(-1 * s, 0), Vector2f(-0.6f * s, 0)})};
}

static int same_result(const smooth_result& a, const smooth_result& b) {
    CHECK(a.status == b.status && a.arclength.arclength == b.arclength.arclength);
    CHECK(a.spline.n_segments() == b.spline.n_segments() && a.spline.n_pts() == b.spline.n_pts());
    for (int i = 0; i < a.spline.n_segments(); ++i)
        for (int k = 0; k < 4; ++k) CHECK(a.spline.ctrl_pts[i][k] == b.spline.ctrl_pts[i][k]);
    const int L = a.spline.n_pts();
    for (int j = 0; j < L; ++j) {
        CHECK(a.spline.pts(j, 0) == b.spline.pts(j, 0) && a.spline.pts(j, 1) == b.spline.pts(j, 1));
        CHECK(a.profile.vel[0](j) == b.profile.vel[0](j) && a.profile.time(j) == b.profile.time(j));
        CHECK(a.ang_vel[j] == b.ang_vel[j]);
    }
    return 0;
}

int main() {
    // (0)
    {
        smooth_request r{{}, -1.0, 1.0, -0.5, 0.5};
        smooth_result s;
        CHECK(r.clear_r2 == -1 && r.clear_levels == 6);
        CHECK(s.tangent_level.empty() && s.leg_min_d2.empty() && s.rounds == 0);
        CHECK(SC_SMOOTH_COLLIDES == 6 && SC_CURVE_MAX_LEVEL == 30 && SC_CURVE_MAX_LEGS >= 64);
    }
    const bounding_rect br{4.4f, -3.3f, 4.4f, -3.3f};
    planning_space space(br);
    space.obstacles = examples_obstacles(3.0f);
    space.grid_cells = 300;
    space.clearance = 2.0f * (br.x_max - br.x_min) / 300.0f;
    space.simplify_paths = true;
    std::vector<Vector2f> starts, goals;
    halton_state hx, hy;
    while (starts.size() < 24 || goals.size() < 24) {
        const float u = halton(2, 1, hx)[0], v = halton(3, 1, hy)[0];
        const Vector2f p(br.x_min + (br.x_max - br.x_min) * u, br.y_min + (br.y_max - br.y_min) * v);
        if (std::get<0>(space.is_obstacle(p))) continue;
        (starts.size() <= goals.size() ? starts : goals).push_back(p);
    }
    const auto plans = space.plan_batch(starts, goals);
    occupancy_grid grid(br, 300, 300);
    grid.rasterize(space.obstacles);
    grid.edt();

    std::vector<smooth_request> off, on;
    for (int q = 0; q < 24; ++q) {
        if (!plans[q]) continue;
        off.push_back(smooth_request{*plans[q], -1.0, 1.0, -0.5, 0.5});
        smooth_request r{*plans[q], -1.0, 1.0, -0.5, 0.5};
        r.clear_r2 = 1;
        on.push_back(r);
    }
    CHECK(off.size() >= 12);
    // (1)
    const auto plain = smooth_paths_batch(off, space, grid);
    for (const auto& r : plain) CHECK(r.status == SC_SMOOTH_OK && r.tangent_level.empty() && r.leg_min_d2.empty() && r.rounds == 0);
    // (2)
    const auto clr = smooth_paths_batch(on, space, grid);
    CHECK(clr.size() == on.size());
    const float res_y = (br.y_max - br.y_min) / 300.0f;
    size_t ok = 0, shrunk = 0, collides = 0;
    for (size_t i = 0; i < on.size(); ++i) {
        const smooth_result& b = clr[i];
        CHECK(b.tangent_level.size() == on[i].path.size() && b.leg_min_d2.size() + 1 == on[i].path.size());
        int top = 0;
        for (uint8_t l : b.tangent_level) top = std::max(top, (int)l);
        CHECK((top == 0) == (b.rounds == 0) || b.status != SC_SMOOTH_OK);
        if (b.status == SC_SMOOTH_COLLIDES) { CHECK(top == on[i].clear_levels && b.spline.n_pts() == 0); ++collides; continue; }
        CHECK(b.status == SC_SMOOTH_OK);
        ++ok;
        for (int32_t m : b.leg_min_d2) CHECK(m >= 1);
        for (int j = 0; j < b.spline.n_pts(); ++j) {
            const int ix = (int)std::floor(((double)b.spline.pts(j, 0) - (double)br.x_min) / (double)grid.resolution);
            const int iy = (int)std::floor(((double)b.spline.pts(j, 1) - (double)br.y_min) / (double)res_y);
            CHECK(ix >= 0 && ix < grid.W && iy >= 0 && iy < grid.H && grid.d2[(size_t)iy * grid.W + ix] >= 1);
        }
        if (top == 0) { if (same_result(plain[i], b)) { std::printf("  request %zu\n", i); return 1; } }
        else ++shrunk;
    }
    CHECK(ok >= on.size() / 2);
    // (3)
    for (int lv : {0, SC_CURVE_MAX_LEVEL + 1}) {
        std::vector<smooth_request> bad(1, on[0]);
        bad[0].clear_levels = lv;
        bool threw = false;
        try { smooth_paths_batch(bad, space, grid); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw);
    }
    std::printf("%zu paths: %zu OK (%zu with shrunk tangents), %zu collide\ncurve clear OK\n", on.size(), ok, shrunk, collides);
    return 0;
}
