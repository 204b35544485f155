// planning_space::soft_clearance / soft_penalty and occupancy_grid::clearance_penalty / cost_fields / field_paths with a
// costmap, through sea-current_amd/sea_current.hpp, on a two-room world: a wall across the middle with one door.
//   knobs off: plan_from(start, goals) == plan_batch(std::vector(goals.size(), start), goals), as before;
//   knobs on:  every returned path stays on cells that keep the hard clearance and steps between neighbouring cells, at
//              least one differs from the unweighted path, none passes closer to an obstacle than the unweighted one
//              does at its closest, and plan_to returns plan_from's cells reversed;
//   the grid calls: a weighted field costs at least the unweighted one everywhere, with pen_cap 0 exactly as much.
// Exit code 0 and "weighted fields OK" = all passed.
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
    const bounding_rect br{5.0f, -5.0f, 5.0f, -5.0f};
    planning_space space(br);
    // the wall x in [-0.2, 0.2] with a door y in [-0.6, 0.6]
    space.obstacles = {obstacle({Vector2f(-0.2f, 0.6f), Vector2f(0.2f, 0.6f), Vector2f(0.2f, 5.0f), Vector2f(-0.2f, 5.0f)}),
                       obstacle({Vector2f(-0.2f, -5.0f), Vector2f(0.2f, -5.0f), Vector2f(0.2f, -0.6f), Vector2f(-0.2f, -0.6f)})};
    space.grid_cells = 200;
    const float cell = (br.x_max - br.x_min) / 200.0f;
    space.clearance = 2.0f * cell;
    const Vector2f start(-4.0f, 3.0f);
    std::vector<Vector2f> goals;
    for (int k = 0; k < 12; ++k) goals.push_back(Vector2f(1.0f + 0.3f * k, -4.0f + 0.7f * k));
    goals.push_back(Vector2f(0.0f, 3.0f));   // inside the wall: no path

    // knobs off: today's result
    const plans base = space.plan_from(start, goals);
    const plans ref = space.plan_batch(std::vector<Vector2f>(goals.size(), start), goals);
    CHECK(base.size() == goals.size());
    for (size_t q = 0; q < goals.size(); ++q) CHECK(same(base[q], ref[q]));
    CHECK(!base.back().has_value());
    space.soft_clearance = 8.0f * cell;
    CHECK(same(space.plan_from(start, goals)[0], base[0]));   // one knob alone is off
    space.soft_clearance = 0.0f;
    space.soft_penalty = 60;
    CHECK(same(space.plan_from(start, goals)[0], base[0]));

    // knobs on
    space.soft_clearance = 8.0f * cell;
    const plans soft = space.plan_from(start, goals);
    const plans soft_to = space.plan_to(goals, start);
    occupancy_grid g = space.make_grid();
    g.edt();
    const float cc = space.clearance / g.resolution;
    const int32_t r2 = (int32_t)std::ceil(cc * cc);
    CHECK(r2 >= 4);
    int differ = 0, found = 0;
    for (size_t q = 0; q < goals.size(); ++q) {
        CHECK(soft[q].has_value() == base[q].has_value() && soft_to[q].has_value() == base[q].has_value());
        if (!soft[q]) continue;
        ++found;
        const auto& p = *soft[q];
        CHECK(p.front() == start && p.back() == goals[q]);
        int32_t dmin = INT32_MAX, dmin_base = INT32_MAX;
        for (size_t i = 0; i < p.size(); ++i) {
            const int32_t c = g.cell_of(p[i]);
            CHECK(g.d2[c] >= r2);
            dmin = std::min(dmin, g.d2[c]);
            if (i) {
                const int32_t b = g.cell_of(p[i - 1]);
                CHECK(std::abs(c % g.W - b % g.W) <= 1 && std::abs(c / g.W - b / g.W) <= 1);
            }
        }
        for (const auto& v : *base[q]) dmin_base = std::min(dmin_base, g.d2[g.cell_of(v)]);
        CHECK(dmin >= dmin_base);
        if (p != *base[q]) ++differ;
        CHECK(soft_to[q]->size() == p.size());
        for (size_t i = 0; i < p.size(); ++i) CHECK(g.cell_of((*soft_to[q])[i]) == g.cell_of(p[p.size() - 1 - i]));
    }
    CHECK(found == 12 && differ >= 1);

    // the grid calls
    const float sc_cells = space.soft_clearance / g.resolution;
    const int32_t r2_soft = (int32_t)std::ceil(sc_cells * sc_cells);
    const std::vector<uint8_t> pen = g.clearance_penalty(r2, r2_soft, 60);
    CHECK(pen.size() == g.occ.size());
    int positive = 0;
    for (size_t c = 0; c < pen.size(); ++c) {
        CHECK(pen[c] <= 60 && (pen[c] == 0 || (g.d2[c] >= r2 && g.d2[c] < r2_soft)));
        positive += pen[c] > 0;
    }
    CHECK(positive > 0);
    const std::vector<int32_t> roots{g.cell_of(start)};
    auto f0 = g.cost_fields(roots, r2);
    auto fw = g.cost_fields(roots, pen, 60, r2);
    auto fz = g.cost_fields(roots, pen, 0, r2);
    CHECK(f0.status[0] == SC_Q_OK && fw.status[0] == SC_Q_OK && fz.status[0] == SC_Q_OK);
    CHECK(fz.g == f0.g && fw.pen == pen && fw.pen_cap == 60 && f0.pen.empty());
    bool above = false;
    for (size_t c = 0; c < f0.g.size(); ++c) {
        CHECK(fw.g[c] >= f0.g[c] && (fw.g[c] == SC_FIELD_INF) == (f0.g[c] == SC_FIELD_INF));
        above = above || fw.g[c] > f0.g[c];
    }
    CHECK(above);
    std::vector<int32_t> t(goals.size()), qf(goals.size(), 0);
    for (size_t q = 0; q < goals.size(); ++q) t[q] = g.cell_of(goals[q]);
    auto bw = g.field_paths(fw, qf, t);
    auto bz = g.field_paths(fz, qf, t);
    auto b0 = g.field_paths(f0, qf, t);
    CHECK(bz.status == b0.status && bz.len == b0.len && bz.cost == b0.cost && bz.Lmax == b0.Lmax);
    for (size_t q = 0; q < goals.size(); ++q) {
        if (b0.status[q] == SC_Q_OK)   // cells past len are unspecified
            for (int i = 0; i < b0.len[q]; ++i) CHECK(bz.path[q * bz.Lmax + i] == b0.path[q * b0.Lmax + i]);
        CHECK(bw.status[q] == b0.status[q]);
        if (bw.status[q] == SC_Q_OK) CHECK(bw.cost[q] == fw.g[t[q]] && bw.cost[q] >= b0.cost[q]);
    }
    std::printf("plan_from with a soft margin: %d paths, %d differ from the unweighted ones\nweighted fields OK\n", found, differ);
    return 0;
}
