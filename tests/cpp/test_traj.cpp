// Conflicts between timed paths through sea-current_amd/sea_current.hpp: fleet_conflicts on smooth_results filled by hand
// (status, spline.pts, profile.time: what a moving obstacle looks like), the hand cases of tests/test_traj_twin.py with
// their exact answers:
//   (1) head-on along y = 0 from x = 0 and x = 8 at speed 1, radius 0.5 each: first_t 3.5, min_sep 0, at dt_c 0.25, 1 and 3;
//   (2) a path that arrives at (8, 0) at t = 8 and holds, and one that starts at t0 = 10 from (8, 8) towards it: first_t 17;
//       with the hold flag cleared no conflict and min_sep 8;
//   (3) same group: never compared; a result whose status is not OK is skipped and invisible; sep_cap below the separation;
//   (4) arguments that do not fit throw.
// Exit code 0 and "traj OK" = all passed.
#include <cmath>
#include <cstdio>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

// 9 samples 1 s apart, uniformly from (x0, y0) to (x1, y1)
static smooth_result line(float x0, float y0, float x1, float y1) {
    smooth_result r;
    r.status = SC_SMOOTH_OK;
    r.spline.pts = points_matrix::Zero(9, 2);
    toppra_compat::Vector t(9);
    for (int i = 0; i < 9; ++i) {
        r.spline.pts(i, 0) = x0 + (x1 - x0) * (float)i / 8.0f;
        r.spline.pts(i, 1) = y0 + (y1 - y0) * (float)i / 8.0f;
        t(i) = (double)i;
    }
    r.profile.time = t;
    return r;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    // (1)
    const std::vector<smooth_result> head{line(0, 0, 8, 0), line(8, 0, 0, 0)};
    for (double dt_c : {0.25, 1.0, 3.0}) {
        const conflict_result c = fleet_conflicts(head, {0.5, 0.5}, {}, {}, {}, dt_c);
        CHECK(c.status == std::vector<int>({SC_TRAJ_OK, SC_TRAJ_OK}));
        CHECK(c.first_t == std::vector<double>({3.5, 3.5}) && c.min_sep == std::vector<double>({0.0, 0.0}));
        CHECK(c.first_with == std::vector<int>({1, 0}) && c.min_with == std::vector<int>({1, 0}) && c.n_conf == std::vector<int>({1, 1}));
    }
    // (2)
    const std::vector<smooth_result> park{line(0, 0, 8, 0), line(8, 8, 8, 0)};
    conflict_result c = fleet_conflicts(park, {0.5, 0.5}, {0.0, 10.0}, {3, 3}, {}, 0.5);
    CHECK(c.first_t == std::vector<double>({17.0, 17.0}) && c.n_conf == std::vector<int>({1, 1}));
    c = fleet_conflicts(park, {0.5, 0.5}, {0.0, 10.0}, {1, 3}, {}, 0.5);
    CHECK(c.first_t == std::vector<double>({inf, inf}) && c.min_sep == std::vector<double>({8.0, 8.0}) && c.first_with == std::vector<int>({-1, -1}));
    CHECK(c.min_with == std::vector<int>({1, 0}) && c.n_conf == std::vector<int>({0, 0}));
    // (3)
    c = fleet_conflicts(head, {0.5, 0.5}, {}, {}, {4, 4});
    CHECK(c.first_t == std::vector<double>({inf, inf}) && c.min_sep == std::vector<double>({inf, inf}) && c.min_with == std::vector<int>({-1, -1}));
    std::vector<smooth_result> three{line(0, 0, 8, 0), line(8, 0, 0, 0), line(8, 0, 0, 0)};
    three[1].status = SC_SMOOTH_TOPPRA_FAILED;
    c = fleet_conflicts(three, {0.5, 0.5, 0.5});
    CHECK(c.status == std::vector<int>({SC_TRAJ_OK, SC_TRAJ_SKIPPED, SC_TRAJ_OK}));
    CHECK(c.first_t == std::vector<double>({3.5, inf, 3.5}) && c.first_with == std::vector<int>({2, -1, 0}) && c.n_conf == std::vector<int>({1, 0, 1}));
    c = fleet_conflicts(park, {0.5, 0.5}, {0.0, 10.0}, {1, 3}, {}, 0.5, 4.0);
    CHECK(c.min_sep == std::vector<double>({inf, inf}) && c.min_with == std::vector<int>({-1, -1}));
    CHECK(fleet_conflicts({}, {}).first_t.empty());
    // (4)
    int threw = 0;
    try { fleet_conflicts(head, {0.5}); } catch (const std::invalid_argument&) { ++threw; }
    try { fleet_conflicts(head, {0.5, 0.5}, {1.0}); } catch (const std::invalid_argument&) { ++threw; }
    try { fleet_conflicts(head, {0.5, -0.5}); } catch (const std::runtime_error&) { ++threw; }
    try { fleet_conflicts(head, {0.5, 0.5}, {}, {}, {}, 0.0); } catch (const std::invalid_argument&) { ++threw; }
    try { fleet_conflicts(head, {0.5, 0.5}, {}, {}, {}, std::nan("")); } catch (const std::invalid_argument&) { ++threw; }
    try { fleet_conflicts(head, {0.5, 0.5}, {}, {}, {}, 0.5, 0.0); } catch (const std::runtime_error&) { ++threw; }
    CHECK(threw == 6);
    std::printf("traj OK\n");
    return 0;
}
