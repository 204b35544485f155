// smooth_paths_batch through sea-current_amd/sea_current.hpp: 64 Halton start/goal pairs planned with plan_batch and
// simplify_paths on the non-dyadic world of test_waypoints.cpp (bounding_rect {4.4, -3.3, 4.4, -3.3}, 300 cells,
// clearance 2 cells), every path smoothed in ONE batched call, and each result checked against the one-path chain
// from_path -> arclength -> gen_vel_prof<1> -> resample(nudge): status OK, finite control points, pts / vel / acc / time
// bit-equal, ang_vel within 1e-5 relative of angular_velocity(prof), and serialize_path_to_json identical but for
// ang_vel.  Exit code 0 and "smooth OK" = all passed.
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

// the one-path chain of examples/zmq_test.cpp:66-93 against the batched result
static int compare(const std::vector<Vector2f>& path, const planning_space& space, const smooth_request& rq, const smooth_result& b) {
    CHECK(b.status == SC_SMOOTH_OK);
    for (const auto& seg : b.spline.ctrl_pts)
        for (const auto& c : seg) CHECK(std::isfinite(c.x()) && std::isfinite(c.y()));
    bezier_spline pad = bezier_spline::from_path(path, space);
    CHECK(pad.n_segments() == b.spline.n_segments());
    for (int i = 0; i < pad.n_segments(); ++i)
        for (int k = 0; k < 4; ++k) CHECK(pad.ctrl_pts[i][k] == b.spline.ctrl_pts[i][k]);
    const arclength_data ad = pad.arclength();
    CHECK(ad.arclength == b.arclength.arclength);
    const double vmin = rq.vel_min, vmax = rq.vel_max;
    auto lim = [vmin, vmax](value_type) {
        toppra_compat::Vector lo(1), hi(1);
        lo(0) = vmin; hi(0) = vmax;
        return std::make_tuple(lo, hi);
    };
    velocity_profile prof = gen_vel_prof<1>(VectorNd<1>{ad.arclength}, VectorNd<1>{0}, VectorNd<1>{0}, VectorNd<1>{0}, lim,
                                            VectorNd<1>{rq.acc_min}, VectorNd<1>{rq.acc_max});
    bezier_spline re = pad.resample(prof.pos[0], ad, true);
    const int L = re.n_pts();
    CHECK(L == b.spline.n_pts() && L == (int)b.profile.vel[0].size() && L == (int)b.ang_vel.size());
    for (int j = 0; j < L; ++j) {
        CHECK(re.pts(j, 0) == b.spline.pts(j, 0) && re.pts(j, 1) == b.spline.pts(j, 1));
        CHECK(prof.pos[0](j) == b.profile.pos[0](j));
        CHECK(prof.vel[0](j) == b.profile.vel[0](j) && prof.acc[0](j) == b.profile.acc[0](j));
        CHECK(prof.time(j) == b.profile.time(j));
    }
    CHECK(re.positions.size() == b.spline.positions.size());
    for (size_t i = 0; i < re.positions.size(); ++i) {
        CHECK(re.positions[i].size() == b.spline.positions[i].size());
        for (size_t k = 0; k < (size_t)re.positions[i].size(); ++k) CHECK(re.positions[i](k) == b.spline.positions[i](k));
    }
    const std::vector<float> w = re.angular_velocity(prof);
    for (int j = 0; j < L; ++j) CHECK(std::fabs(w[j] - b.ang_vel[j]) <= 1e-5f * std::max(1.0f, std::fabs(w[j])));
    CHECK(serialize_path_to_json(re, prof, ad, b.ang_vel) == serialize_path_to_json(b.spline, b.profile, b.arclength, b.ang_vel));
    return 0;
}

int main() {
    const bounding_rect br{4.4f, -3.3f, 4.4f, -3.3f};
    planning_space space(br);
    space.obstacles = examples_obstacles(3.0f);
    obstacle wall({Vector2f(-2.5f, -2.0f), Vector2f(-0.5f, -2.8f)}, {{0, 1}});
    wall.closed = false;
    space.obstacles.push_back(wall);
    space.grid_cells = 300;
    space.clearance = 2.0f * (br.x_max - br.x_min) / 300.0f;
    space.simplify_paths = true;
    std::vector<Vector2f> starts, goals;
    halton_state hx, hy;
    while (starts.size() < 64 || goals.size() < 64) {
        const float u = halton(2, 1, hx)[0], v = halton(3, 1, hy)[0];
        const Vector2f p(br.x_min + (br.x_max - br.x_min) * u, br.y_min + (br.y_max - br.y_min) * v);
        if (std::get<0>(space.is_obstacle(p))) continue;
        (starts.size() <= goals.size() ? starts : goals).push_back(p);
    }
    const auto plans = space.plan_batch(starts, goals);
    std::vector<smooth_request> reqs;
    std::vector<int> which;
    const double lims[3][2] = {{1.0, 0.5}, {0.6, 0.3}, {1.5, 1.0}};   // (vel, acc) pairs, per request as the service reads them
    for (int q = 0; q < 64; ++q) {
        if (!plans[q]) continue;
        const double* l = lims[q % 3];
        reqs.push_back(smooth_request{*plans[q], -l[0], l[0], -l[1], l[1]});
        which.push_back(q);
    }
    CHECK(reqs.size() >= 32);
    const auto res = smooth_paths_batch(reqs, space);
    CHECK(res.size() == reqs.size());
    size_t samples = 0;
    for (size_t i = 0; i < reqs.size(); ++i) {
        if (compare(reqs[i].path, space, reqs[i], res[i])) { std::printf("  query %d\n", which[i]); return 1; }
        samples += (size_t)res[i].spline.n_pts();
    }
    std::printf("%zu paths, %zu samples in one call\nsmooth OK\n", reqs.size(), samples);
    return 0;
}
