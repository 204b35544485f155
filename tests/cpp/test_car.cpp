// car_model, occupancy_grid::arc_mask / car_fields / car_paths and planning_space::plan_to_pose(.., car_model, ..) through
// sea-current_amd/sea_current.hpp, on test_pose.cpp's two-room world: bounding_rect {5, -5, 5, -5}, 40 cells, a wall three
// cells thick around x = 0 with a door three cells wide at y = 0, a body 5 cells long and 3 wide.
//   the arc mask against the definition restated on the host (every arc walked);
//   plan_to_pose with a car_model against a Dijkstra over the car graph restated on the host: for every start the first pose is
//     the start pose, the last the goal pose, the entries read as a chain of legal edges (an arc with its 2n - 1 cells in
//     between) whose costs add up to the optimal cost, no two consecutive entries share a cell; where the host finds no route
//     there is no plan; a body too wide for the door gets no path from the other room.
// Exit code 0 and "car OK" = all passed.
#include <cstdio>
#include <functional>
#include <map>
#include <queue>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static const int HX[8] = {1, 1, 0, -1, -1, -1, 0, 1}, HY[8] = {0, 1, 1, 1, 0, -1, -1, -1};

struct entry { int x, y, k; };
struct host_edge {
    int x, y, k, cost;
    std::vector<entry> mid;   // the entries between the two poses, in driving order
};

struct host_graph {
    int W, H, n, ac, rev;
    std::vector<char> T;
    std::vector<uint8_t> hm;
    bool t(int x, int y) const { return x >= 0 && y >= 0 && x < W && y < H && T[(size_t)y * W + x]; }
    bool valid(int x, int y, int k) const { return t(x, y) && ((hm[(size_t)y * W + x] >> k) & 1); }
    bool move(int x, int y, int dx, int dy) const {
        if (!t(x, y) || !t(x + dx, y + dy)) return false;
        return !(dx && dy) || (t(x + dx, y) && t(x, y + dy));
    }
    // A((x, y), k, s): legal?  cells receives p_0 .. p_2n
    bool arc(int x, int y, int k, int s, std::vector<entry>& cells) const {
        const int kn = (k + s + 8) & 7;
        cells.assign(1, entry{x, y, k});
        bool ok = valid(x, y, k);
        for (int i = 0; i < n; ++i) { ok = ok && move(x, y, HX[k], HY[k]) && valid(x + HX[k], y + HY[k], k); x += HX[k]; y += HY[k]; cells.push_back({x, y, k}); }
        ok = ok && valid(x, y, kn);
        for (int j = 0; j < n; ++j) { ok = ok && move(x, y, HX[kn], HY[kn]) && valid(x + HX[kn], y + HY[kn], kn); x += HX[kn]; y += HY[kn]; cells.push_back({x, y, kn}); }
        return ok;
    }
    // the legal edges out of the pose (x, y, k)
    std::vector<host_edge> out_edges(int x, int y, int k) const {
        std::vector<host_edge> e;
        if (!valid(x, y, k)) return e;
        const int w = (k & 1) ? 14 : 10;
        if (move(x, y, HX[k], HY[k]) && valid(x + HX[k], y + HY[k], k)) e.push_back({x + HX[k], y + HY[k], k, w, {}});
        if (rev >= 0 && move(x, y, -HX[k], -HY[k]) && valid(x - HX[k], y - HY[k], k)) e.push_back({x - HX[k], y - HY[k], k, w + rev, {}});
        std::vector<entry> c;
        for (int s = 1; s >= -1; s -= 2) {
            if (arc(x, y, k, s, c))      // forwards: the corner is reached by the first leg
                e.push_back({c.back().x, c.back().y, c.back().k, 24 * n + ac, std::vector<entry>(c.begin() + 1, c.end() - 1)});
            const int j = (k - s + 8) & 7, sx = x - n * HX[k] - n * HX[j], sy = y - n * HY[k] - n * HY[j];
            if (rev >= 0 && arc(sx, sy, j, s, c) && c.back().x == x && c.back().y == y) {   // backwards along the arc that ends here
                std::vector<entry> mid;
                for (int i = 2 * n - 1; i >= 1; --i) mid.push_back({c[(size_t)i].x, c[(size_t)i].y, i >= n ? k : j});
                e.push_back({sx, sy, j, 24 * n + ac + 2 * n * rev, mid});
            }
        }
        return e;
    }
    // the optimal cost from pose s to every pose
    std::vector<int64_t> dijkstra(int sx, int sy, int sk) const {
        const int64_t INF = INT64_MAX;
        std::vector<int64_t> g((size_t)8 * W * H, INF);
        using item = std::pair<int64_t, int64_t>;
        std::priority_queue<item, std::vector<item>, std::greater<item>> pq;
        if (!valid(sx, sy, sk)) return g;
        const int64_t cells = (int64_t)W * H;
        g[(size_t)(sk * cells + sy * W + sx)] = 0;
        pq.push({0, sk * cells + sy * W + sx});
        while (!pq.empty()) {
            const auto [d, s] = pq.top();
            pq.pop();
            if (d > g[(size_t)s]) continue;
            const int k = (int)(s / cells), x = (int)(s % cells) % W, y = (int)(s % cells) / W;
            for (const auto& e : out_edges(x, y, k)) {
                const int64_t s2 = e.k * cells + (int64_t)e.y * W + e.x;
                if (d + e.cost < g[(size_t)s2]) { g[(size_t)s2] = d + e.cost; pq.push({d + e.cost, s2}); }
            }
        }
        return g;
    }
    // the cheapest reading of p[i ..] as a chain of legal edges, -1 where there is none
    int64_t chain(const std::vector<planning_space::pose>& p, size_t i, std::map<size_t, int64_t>& memo) const {
        if (i + 1 == p.size()) return 0;
        auto it = memo.find(i);
        if (it != memo.end()) return it->second;
        int64_t best = -1;
        for (const auto& e : out_edges(p[i].cell % W, p[i].cell / W, p[i].heading)) {
            std::vector<entry> want = e.mid;
            want.push_back({e.x, e.y, e.k});
            if (i + want.size() >= p.size()) continue;
            bool same = true;
            for (size_t j = 0; j < want.size() && same; ++j)
                same = p[i + 1 + j].cell == want[j].y * W + want[j].x && p[i + 1 + j].heading == want[j].k;
            if (!same) continue;
            const int64_t rest = chain(p, i + want.size(), memo);
            if (rest >= 0 && (best < 0 || e.cost + rest < best)) best = e.cost + rest;
        }
        memo[i] = best;
        return best;
    }
};

int main() {
    const bounding_rect br{5.0f, -5.0f, 5.0f, -5.0f};
    planning_space space(br);
    space.obstacles = {obstacle({Vector2f(-0.3f, -4.99f), Vector2f(0.3f, -4.99f), Vector2f(0.3f, -0.3f), Vector2f(-0.3f, -0.3f)}),
                       obstacle({Vector2f(-0.3f, 0.55f), Vector2f(0.3f, 0.55f), Vector2f(0.3f, 4.99f), Vector2f(-0.3f, 4.99f)})};
    for (auto& ob : space.obstacles) ob.closed = true;
    space.grid_cells = 40;
    gpu_context& ctx = default_context();
    occupancy_grid g = space.make_grid(ctx);
    g.edt(ctx);
    CHECK(g.W == 40 && g.H == 40);
    const footprint body{2, 2, 1, 1}, wide{3, 3, 3, 3};
    const car_model car{1, 2, 4};
    const std::vector<uint8_t> hm = g.footprint_mask(body, 0, ctx);

    host_graph hg{g.W, g.H, car.arc_n, car.arc_cost, car.rev_cost, std::vector<char>(g.occ.size()), hm};
    for (size_t c = 0; c < g.occ.size(); ++c) hg.T[c] = g.d2[c] >= 1;

    // the arc mask against the definition, for every arc_n
    for (int an = 1; an <= SC_ARC_MAX; ++an) {
        host_graph h2 = hg;
        h2.n = an;
        const std::vector<uint16_t> am = g.arc_mask(an, 0, hm, ctx);
        std::vector<entry> c;
        for (int y = 0; y < g.H; ++y)
            for (int x = 0; x < g.W; ++x)
                for (int k = 0; k < 8; ++k) {
                    CHECK((bool)((am[(size_t)y * g.W + x] >> (2 * k)) & 1) == h2.arc(x, y, k, 1, c));
                    CHECK((bool)((am[(size_t)y * g.W + x] >> (2 * k + 1)) & 1) == h2.arc(x, y, k, -1, c));
                }
    }
    bool threw = false;
    try { g.arc_mask(5, 0, hm, ctx); } catch (const std::exception&) { threw = true; }
    CHECK(threw);

    // plan_to_pose: starts in both rooms, the goal in the right room heading up
    const Vector2f goal(3.1f, 2.6f);
    const int goal_heading = 2;
    const std::vector<Vector2f> starts = {Vector2f(-3.1f, -2.6f), Vector2f(-2.0f, 3.0f), Vector2f(2.0f, -3.0f), Vector2f(3.1f, 2.6f), Vector2f(-4.0f, 0.1f)};
    const std::vector<int32_t> sh = {6, 0, 3, 2, 4};
    auto plans = space.plan_to_pose(starts, sh, goal, goal_heading, car, body, ctx);
    CHECK(plans.size() == starts.size());
    const int32_t gc = g.cell_of(goal);
    const int64_t n = (int64_t)g.W * g.H;
    int found = 0;
    bool through_door = false, turned = false;
    for (size_t q = 0; q < starts.size(); ++q) {
        const int32_t sc0 = g.cell_of(starts[q]);
        const auto dist = hg.dijkstra(sc0 % g.W, sc0 / g.W, sh[q]);
        const int64_t want = dist[(size_t)(goal_heading * n + gc)];
        CHECK(plans[q].has_value() == (want != INT64_MAX));
        if (!plans[q].has_value()) continue;
        ++found;
        const auto& p = *plans[q];
        CHECK(!p.empty() && p.front().cell == sc0 && p.front().heading == sh[q] && p.back().cell == gc && p.back().heading == goal_heading);
        std::map<size_t, int64_t> memo;
        CHECK(hg.chain(p, 0, memo) == want);                                   // legal edges that add up to the optimum
        for (size_t i = 1; i < p.size(); ++i) {
            CHECK(p[i].cell != p[i - 1].cell);                                 // a car never turns on the spot
            CHECK(std::abs(p[i].cell % g.W - p[i - 1].cell % g.W) <= 1 && std::abs(p[i].cell / g.W - p[i - 1].cell / g.W) <= 1);
            turned = turned || p[i].heading != p[i - 1].heading;
        }
        for (const auto& s : p) {
            const Vector2f ctr = g.centre_of(s.cell);
            CHECK(s.position.x() == ctr.x() && s.position.y() == ctr.y());
            if (g.occ[(size_t)5 * g.W + s.cell % g.W]) through_door = true;    // a column of the wall: this is the door
        }
        if (q == 3) CHECK(p.size() == 1);
    }
    CHECK(found >= 3 && through_door && turned);
    // the wide body fits no heading in the door: nothing from the left room
    auto none = space.plan_to_pose(starts, sh, goal, goal_heading, car, wide, ctx);
    CHECK(!none[0].has_value() && !none[1].has_value() && !none[4].has_value() && none[3].has_value());
    // without reversing nothing gets cheaper
    auto fwd = space.plan_to_pose(starts, sh, goal, goal_heading, car_model{1, 2, -1}, body, ctx);
    host_graph hf = hg;
    hf.rev = -1;
    for (size_t q = 0; q < starts.size(); ++q) {
        if (!fwd[q].has_value()) continue;
        CHECK(plans[q].has_value());
        std::map<size_t, int64_t> m1, m2;
        CHECK(hf.chain(*fwd[q], 0, m1) >= hg.chain(*plans[q], 0, m2));
    }
    // the size and range checks of the header
    threw = false;
    try { space.plan_to_pose(starts, {0}, goal, 0, car); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { space.plan_to_pose(starts, sh, goal, 0, car_model{0, 0, 0}); } catch (const std::exception&) { threw = true; }
    CHECK(threw);

    // car_fields / car_paths directly: the cost of a read-out is gp at its target pose
    auto fr = g.car_fields({gc}, {goal_heading}, car, true, 0, hm, -1, ctx);
    CHECK(fr.status[0] == SC_Q_OK && fr.gp.size() == (size_t)8 * n && fr.amask == g.arc_mask(car.arc_n, 0, hm, ctx));
    std::vector<int32_t> tg, th, qf;
    for (size_t q = 0; q < starts.size(); ++q) { tg.push_back(g.cell_of(starts[q])); th.push_back(-1); qf.push_back(0); }
    auto pr = g.car_paths(fr, qf, tg, th, 0, true, ctx);
    for (size_t q = 0; q < starts.size(); ++q) {
        int32_t best = SC_FIELD_INF;
        for (int k = 0; k < 8; ++k) best = std::min(best, fr.gp[(size_t)(k * n + tg[q])]);
        if (best == SC_FIELD_INF) { CHECK(pr.status[q] == SC_Q_NO_PATH); continue; }
        CHECK(pr.status[q] == SC_Q_OK && pr.len[q] >= 1 && pr.cost[q] == best);
    }
    std::printf("car OK\n");
    return 0;
}
