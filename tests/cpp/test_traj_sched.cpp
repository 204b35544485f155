// Delay schedules through sea-current_amd/sea_current.hpp: fleet_schedule on smooth_results filled by hand, the hand cases
// of tests/test_traj_sched_twin.py with their exact answers:
//   (1) the right-angle crossing, (0,0) -> (8,0) and (4,-4) -> (4,4) at speed 1, radius 0.5 each, both absent outside their
//       runs, dt_c 0.5: delta seconds apart in time they pass delta / sqrt(2) apart, so shifts of up to 2 ticks still meet
//       and the second path gets slot 3 (1.5 s); with the order reversed the first one waits; with stride 2 slot 2 (2 s);
//   (2) a path that arrives at (8, 0) and holds, and one that starts at t0 = 10 from (8, 8) towards it: unresolved at every
//       delay; pinned it gets slot 0; with the hold flag cleared there is nothing to wait for;
//   (3) same group: never compared; a result whose status is not OK is SC_SLOT_NOT_OK; a path left out of order;
//   (4) arguments that do not fit throw.
// Exit code 0 and "traj_sched OK" = all passed.
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
    typedef std::vector<int> ints;
    // (1)
    const std::vector<smooth_result> cross{line(0, 0, 8, 0), line(4, -4, 4, 4)};
    schedule_result s = fleet_schedule(cross, {0.5, 0.5}, {}, {0, 0}, {}, 0.5);
    CHECK(s.status == ints({SC_TRAJ_OK, SC_TRAJ_OK}) && s.slot == ints({0, 3}) && s.delay == std::vector<double>({0.0, 1.5}));
    CHECK(s.counts[0] == 1 && s.counts[1] == 1 && s.counts[2] == 0 && s.counts[3] == 0);
    s = fleet_schedule(cross, {0.5, 0.5}, {}, {0, 0}, {}, 0.5, 8, 1, {1, 0});
    CHECK(s.slot == ints({3, 0}));
    s = fleet_schedule(cross, {0.5, 0.5}, {}, {0, 0}, {}, 0.5, 4, 2);
    CHECK(s.slot == ints({0, 2}) && s.delay[1] == 2.0);
    s = fleet_schedule(cross, {0.5, 0.5}, {}, {0, 0}, {}, 0.5, 3, 1);
    CHECK(s.slot == ints({0, SC_SLOT_UNRESOLVED}) && std::isnan(s.delay[1]) && s.counts[2] == 1);
    // (2)
    const std::vector<smooth_result> park{line(0, 0, 8, 0), line(8, 8, 8, 0)};
    s = fleet_schedule(park, {0.5, 0.5}, {0.0, 10.0}, {3, 3}, {}, 0.5, 6);
    CHECK(s.slot == ints({0, SC_SLOT_UNRESOLVED}));
    s = fleet_schedule(park, {0.5, 0.5}, {0.0, 10.0}, {3, 3}, {}, 0.5, 6, 1, {}, {5, -1});
    CHECK(s.slot == ints({0, 0}) && s.counts[0] == 2);
    s = fleet_schedule(park, {0.5, 0.5}, {0.0, 10.0}, {1, 3}, {}, 0.5, 6);
    CHECK(s.slot == ints({0, 0}));
    // (3)
    s = fleet_schedule(cross, {0.5, 0.5}, {}, {0, 0}, {4, 4}, 0.5);
    CHECK(s.slot == ints({0, 0}));
    std::vector<smooth_result> three{line(0, 0, 8, 0), line(4, -4, 4, 4), line(4, -4, 4, 4)};
    three[1].status = SC_SMOOTH_TOPPRA_FAILED;
    s = fleet_schedule(three, {0.5, 0.5, 0.5}, {}, {0, 0, 0}, {}, 0.5);
    CHECK(s.status == ints({SC_TRAJ_OK, SC_TRAJ_SKIPPED, SC_TRAJ_OK}) && s.slot == ints({0, SC_SLOT_NOT_OK, 3}) && s.counts[3] == 1);
    s = fleet_schedule(three, {0.5, 0.5, 0.5}, {}, {0, 0, 0}, {}, 0.5, 8, 1, {2, 2, 1});
    CHECK(s.slot == ints({SC_SLOT_UNNAMED, SC_SLOT_NOT_OK, 0}) && s.counts[3] == 2);
    CHECK(fleet_schedule({}, {}).slot.empty());
    // (4)
    int threw = 0;
    try { fleet_schedule(cross, {0.5}); } catch (const std::invalid_argument&) { ++threw; }
    try { fleet_schedule(cross, {0.5, 0.5}, {1.0}); } catch (const std::invalid_argument&) { ++threw; }
    try { fleet_schedule(cross, {0.5, -0.5}); } catch (const std::runtime_error&) { ++threw; }
    try { fleet_schedule(cross, {0.5, 0.5}, {}, {}, {}, 0.0); } catch (const std::invalid_argument&) { ++threw; }
    try { fleet_schedule(cross, {0.5, 0.5}, {}, {}, {}, 0.5, 33); } catch (const std::invalid_argument&) { ++threw; }
    try { fleet_schedule(cross, {0.5, 0.5}, {}, {}, {}, 0.5, 8, 0); } catch (const std::invalid_argument&) { ++threw; }
    try { fleet_schedule(cross, {0.5, 0.5}, {}, {}, {}, 0.5, 8, 1, {0}); } catch (const std::invalid_argument&) { ++threw; }
    CHECK(threw == 7);
    std::printf("traj_sched OK\n");
    return 0;
}
