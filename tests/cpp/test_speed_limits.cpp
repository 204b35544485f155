// Per-stage speed limits through sea-current_amd/sea_current.hpp, on the non-dyadic world of test_smooth.cpp (bounding_rect
// {4.4, -3.3, 4.4, -3.3}, 300 cells, clearance 2 cells): 24 Halton start/goal pairs planned with plan_batch and
// simplify_paths, then
//   (1) requests with every term off, smoothed with the grid overload (the limited C entry), equal smooth_paths_batch of
//       the same requests field by field, and report vmax_stage = vel_max;
//   (2) requests with omega_max, alat_max and a clearance term: the batched result's profile is bit-equal to
//       gen_vel_prof<1> fed with speed_limit_func on the one-path chain from_path -> arclength, its points to resample
//       of that profile, and its vmax_stage is what speed_limit_func answers at every stage;
//   (3) a request that breaks the contract of the terms throws.
// Exit code 0 and "speed limits OK" = all passed.
#include <cfloat>
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
    CHECK((int)a.ang_vel.size() == L && (int)b.ang_vel.size() == L);
    for (int j = 0; j < L; ++j) {
        CHECK(a.spline.pts(j, 0) == b.spline.pts(j, 0) && a.spline.pts(j, 1) == b.spline.pts(j, 1));
        CHECK(a.profile.pos[0](j) == b.profile.pos[0](j) && a.profile.vel[0](j) == b.profile.vel[0](j));
        CHECK(a.profile.acc[0](j) == b.profile.acc[0](j) && a.profile.time(j) == b.profile.time(j));
        CHECK(a.ang_vel[j] == b.ang_vel[j]);
    }
    return 0;
}

int main() {
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
        off.push_back(smooth_request{*plans[q], -1.0, 1.0, -0.5, 0.5});   // the aggregate form of callers written before the terms
        smooth_request r{*plans[q], -1.0, 1.0, -0.5, 0.5};
        r.omega_max = 0.8; r.alat_max = 0.4; r.clear_floor = 0.1; r.clear_gain = 1.5;
        on.push_back(r);
    }
    CHECK(off.size() >= 12);
    // (1)
    const auto plain = smooth_paths_batch(off, space);
    const auto gated = smooth_paths_batch(off, space, grid);
    CHECK(plain.size() == off.size() && gated.size() == off.size());
    for (size_t i = 0; i < off.size(); ++i) {
        CHECK(plain[i].status == SC_SMOOTH_OK && plain[i].vmax_stage.empty());
        if (same_result(plain[i], gated[i])) { std::printf("  request %zu\n", i); return 1; }
        CHECK((int)gated[i].vmax_stage.size() == SC_TOPPRA_GRID + 1 && std::isinf(gated[i].min_clear));
        for (double v : gated[i].vmax_stage) CHECK(v == 1.0);
    }
    // (2)
    const auto lim = smooth_paths_batch(on, space, grid);
    size_t slower = 0, samples = 0;
    for (size_t i = 0; i < on.size(); ++i) {
        const smooth_result& b = lim[i];
        CHECK(b.status == SC_SMOOTH_OK && (int)b.vmax_stage.size() == SC_TOPPRA_GRID + 1 && std::isfinite(b.min_clear) && b.min_clear >= 0.f);
        bezier_spline pad = bezier_spline::from_path(on[i].path, space);
        const arclength_data ad = pad.arclength();
        CHECK(ad.arclength == b.arclength.arclength);
        const vel_lim_func f = speed_limit_func(pad, ad, on[i], &grid);
        for (int k = 0; k <= SC_TOPPRA_GRID; ++k) {
            const auto [lo, hi] = f((double)k / SC_TOPPRA_GRID);
            CHECK(lo(0) == on[i].vel_min && hi(0) == b.vmax_stage[k] && hi(0) > 0.0 && hi(0) <= on[i].vel_max);
        }
        velocity_profile prof = gen_vel_prof<1>(VectorNd<1>{ad.arclength}, VectorNd<1>{0}, VectorNd<1>{0}, VectorNd<1>{0}, f,
                                                VectorNd<1>{on[i].acc_min}, VectorNd<1>{on[i].acc_max});
        bezier_spline re = pad.resample(prof.pos[0], ad, true);
        const int L = re.n_pts();
        CHECK(L == b.spline.n_pts() && L == (int)b.profile.vel[0].size());
        for (int j = 0; j < L; ++j) {
            CHECK(re.pts(j, 0) == b.spline.pts(j, 0) && re.pts(j, 1) == b.spline.pts(j, 1));
            CHECK(prof.pos[0](j) == b.profile.pos[0](j) && prof.vel[0](j) == b.profile.vel[0](j));
            CHECK(prof.acc[0](j) == b.profile.acc[0](j) && prof.time(j) == b.profile.time(j));
        }
        CHECK(L >= plain[i].spline.n_pts());
        slower += L > plain[i].spline.n_pts();
        samples += (size_t)L;
    }
    CHECK(slower >= on.size() / 2);
    // (3)
    std::vector<smooth_request> bad(1, on[0]);
    bad[0].alat_max = -1.0;
    bool threw = false;
    try { smooth_paths_batch(bad, space); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    std::printf("%zu paths, %zu samples with limits, %zu of them slower\nspeed limits OK\n", on.size(), samples, slower);
    return 0;
}
