// footprint, occupancy_grid::footprint_mask / pose_fields / pose_paths and planning_space::plan_to_pose through
// sea-current_amd/sea_current.hpp, on a two-room world: bounding_rect {5, -5, 5, -5}, 40 cells, a wall three cells thick
// around x = 0 with a door three cells wide (rows 19 .. 21) at y = 0, a body 7 cells long and 3 wide.
//   the mask against the definition restated on the host (every covered offset, looped);
//   plan_to_pose against a Dijkstra over the pose graph restated on the host: for every start the first pose is the start
//     pose, the last the goal pose, every step is a legal edge, and the edge costs add up to the optimal cost; the door is
//     passed at headings 0 and 4 only; a body too wide for the door gets no path from the other room;
//   pose_fields / pose_paths: the cost of every read-out is gp at its target pose, a start heading of -1 takes the cheapest.
// Exit code 0 and "pose OK" = all passed.
#include <cstdio>
#include <queue>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static const int HX[8] = {1, 1, 0, -1, -1, -1, 0, 1}, HY[8] = {0, 1, 1, 1, 0, -1, -1, -1};

struct host_graph {
    int W, H, turn, rev;
    std::vector<char> T;
    std::vector<uint8_t> hm;
    bool t(int x, int y) const { return x >= 0 && y >= 0 && x < W && y < H && T[(size_t)y * W + x]; }
    bool valid(int x, int y, int k) const { return t(x, y) && ((hm[(size_t)y * W + x] >> k) & 1); }
    bool move(int x, int y, int dx, int dy) const {
        if (!t(x, y) || !t(x + dx, y + dy)) return false;
        return !(dx && dy) || (t(x + dx, y) && t(x, y + dy));
    }
    // the cost of the legal edge a -> b, -1 where there is none
    int edge(int ax, int ay, int ak, int bx, int by, int bk) const {
        if (!valid(ax, ay, ak) || !valid(bx, by, bk)) return -1;
        const int w = (ak & 1) ? 14 : 10;
        if (ak == bk) {
            if (bx == ax + HX[ak] && by == ay + HY[ak]) return move(ax, ay, HX[ak], HY[ak]) ? w : -1;
            if (bx == ax - HX[ak] && by == ay - HY[ak]) return rev >= 0 && move(ax, ay, -HX[ak], -HY[ak]) ? w + rev : -1;
            return -1;
        }
        if (ax == bx && ay == by && (bk == ((ak + 1) & 7) || bk == ((ak + 7) & 7))) return turn;
        return -1;
    }
    // the optimal cost from pose s to every pose
    std::vector<int64_t> dijkstra(int sx, int sy, int sk) const {
        const int64_t INF = INT64_MAX;
        std::vector<int64_t> g((size_t)8 * W * H, INF);
        using item = std::pair<int64_t, int64_t>;
        std::priority_queue<item, std::vector<item>, std::greater<item>> pq;
        if (!valid(sx, sy, sk)) return g;
        const int64_t n = (int64_t)W * H;
        g[(size_t)(sk * n + sy * W + sx)] = 0;
        pq.push({0, sk * n + sy * W + sx});
        while (!pq.empty()) {
            const auto [d, s] = pq.top();
            pq.pop();
            if (d > g[(size_t)s]) continue;
            const int k = (int)(s / n), x = (int)(s % n) % W, y = (int)(s % n) / W;
            const int nx[4] = {x + HX[k], x - HX[k], x, x}, ny[4] = {y + HY[k], y - HY[k], y, y}, nk[4] = {k, k, (k + 1) & 7, (k + 7) & 7};
            for (int j = 0; j < 4; ++j) {
                const int c = edge(x, y, k, nx[j], ny[j], nk[j]);
                if (c < 0) continue;
                const int64_t s2 = nk[j] * n + (int64_t)ny[j] * W + nx[j];
                if (d + c < g[(size_t)s2]) { g[(size_t)s2] = d + c; pq.push({d + c, s2}); }
            }
        }
        return g;
    }
};

static bool covered(int k, int dx, int dy, const footprint& f) {
    const int n = HX[k] * HX[k] + HY[k] * HY[k], u = dx * HX[k] + dy * HY[k], v = -dx * HY[k] + dy * HX[k];
    return (u >= 0 ? u * u <= n * f.front * f.front : u * u <= n * f.back * f.back) && (v >= 0 ? v * v <= n * f.left * f.left : v * v <= n * f.right * f.right);
}

static std::vector<uint8_t> mask_naive(const occupancy_grid& g, const footprint& f, int32_t r2) {
    const int32_t thr = std::max(r2, 1);
    const int R = 2 * std::max(std::max(f.front, f.back), std::max(f.left, f.right));
    std::vector<uint8_t> m((size_t)g.W * g.H, 0);
    for (int y = 0; y < g.H; ++y)
        for (int x = 0; x < g.W; ++x)
            for (int k = 0; k < 8; ++k) {
                bool ok = true;
                for (int dy = -R; dy <= R && ok; ++dy)
                    for (int dx = -R; dx <= R && ok; ++dx) {
                        const int nx = x + dx, ny = y + dy;
                        if (nx < 0 || ny < 0 || nx >= g.W || ny >= g.H || !covered(k, dx, dy, f)) continue;
                        if (g.d2[(size_t)ny * g.W + nx] < thr) ok = false;
                    }
                if (ok) m[(size_t)y * g.W + x] |= (uint8_t)(1u << k);
            }
    return m;
}

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
    const footprint body{3, 3, 1, 1}, wide{3, 3, 3, 3};
    const int turn = 3, rev = 4;

    // the mask against the definition
    const std::vector<uint8_t> hm = g.footprint_mask(body, 0, ctx), hw = g.footprint_mask(wide, 0, ctx);
    CHECK(hm == mask_naive(g, body, 0) && hw == mask_naive(g, wide, 0));
    const std::vector<uint8_t> h0 = g.footprint_mask(footprint{}, 0, ctx);
    for (size_t c = 0; c < h0.size(); ++c) CHECK(h0[c] == (g.d2[c] >= 1 ? 0xFF : 0));
    // the wall is there, the door is open, and the long body fits the door lengthwise only
    const int door_y = g.cell_y(0.0f), wall_x = g.cell_x(0.0f);
    CHECK(g.occ[(size_t)5 * g.W + wall_x] && !g.occ[(size_t)door_y * g.W + wall_x]);
    CHECK((hm[(size_t)door_y * g.W + wall_x] & 0x11) == 0x11 && (hm[(size_t)door_y * g.W + wall_x] & 0xEE) == 0);
    CHECK(hw[(size_t)door_y * g.W + wall_x] == 0);

    host_graph hg{g.W, g.H, turn, rev, std::vector<char>(g.occ.size()), hm};
    for (size_t c = 0; c < g.occ.size(); ++c) hg.T[c] = g.d2[c] >= 1;

    // plan_to_pose: starts in both rooms, the goal in the right room heading up
    const Vector2f goal(3.1f, 2.6f);
    const int goal_heading = 2;
    const std::vector<Vector2f> starts = {Vector2f(-3.1f, -2.6f), Vector2f(-2.0f, 3.0f), Vector2f(2.0f, -3.0f), Vector2f(3.1f, 2.6f), Vector2f(-4.0f, 0.1f)};
    const std::vector<int32_t> sh = {6, 0, 3, 2, 4};
    auto plans = space.plan_to_pose(starts, sh, goal, goal_heading, turn, rev, body, ctx);
    CHECK(plans.size() == starts.size());
    const int32_t gc = g.cell_of(goal);
    const int64_t n = (int64_t)g.W * g.H;
    bool through_door = false;
    for (size_t q = 0; q < starts.size(); ++q) {
        const int32_t sc0 = g.cell_of(starts[q]);
        const auto dist = hg.dijkstra(sc0 % g.W, sc0 / g.W, sh[q]);
        const int64_t want = dist[(size_t)(goal_heading * n + gc)];
        CHECK(want != INT64_MAX);
        CHECK(plans[q].has_value());
        const auto& p = *plans[q];
        CHECK(!p.empty() && p.front().cell == sc0 && p.front().heading == sh[q] && p.back().cell == gc && p.back().heading == goal_heading);
        int64_t sum = 0;
        for (size_t i = 1; i < p.size(); ++i) {
            const int c = hg.edge(p[i - 1].cell % g.W, p[i - 1].cell / g.W, p[i - 1].heading, p[i].cell % g.W, p[i].cell / g.W, p[i].heading);
            CHECK(c >= 0);                                                     // every step is a legal edge
            sum += c;
        }
        CHECK(sum == want);                                                    // and the chain is optimal
        for (const auto& s : p) {
            const Vector2f ctr = g.centre_of(s.cell);
            CHECK(s.position.x() == ctr.x() && s.position.y() == ctr.y());
            if (g.occ[(size_t)5 * g.W + s.cell % g.W]) {                       // a column of the wall: this is the door
                CHECK(s.heading == 0 || s.heading == 4);
                through_door = true;
            }
        }
        if (q == 3) CHECK(p.size() == 1);
    }
    CHECK(through_door);
    // the wide body fits no heading in the door: nothing from the left room, a path inside the right room
    auto none = space.plan_to_pose(starts, sh, goal, goal_heading, turn, rev, wide, ctx);
    CHECK(!none[0].has_value() && !none[1].has_value() && !none[4].has_value() && none[2].has_value() && none[3].has_value());
    // a goal heading of -1 and start headings of -1: never dearer than a fixed pair
    auto freeh = space.plan_to_pose(starts, std::vector<int32_t>(starts.size(), -1), goal, -1, turn, rev, body, ctx);
    auto chain_cost = [&](const std::vector<planning_space::pose>& p) {
        int64_t sum = 0;
        for (size_t i = 1; i < p.size(); ++i) {
            const int c = hg.edge(p[i - 1].cell % g.W, p[i - 1].cell / g.W, p[i - 1].heading, p[i].cell % g.W, p[i].cell / g.W, p[i].heading);
            if (c < 0) return (int64_t)-1;
            sum += c;
        }
        return sum;
    };
    for (size_t q = 0; q < starts.size(); ++q) {
        CHECK(freeh[q].has_value() && freeh[q]->front().cell == g.cell_of(starts[q]) && freeh[q]->back().cell == gc);
        const int64_t a = chain_cost(*freeh[q]), b = chain_cost(*plans[q]);
        CHECK(a >= 0 && a <= b);
    }
    // the size checks of the header
    bool threw = false;
    try { space.plan_to_pose(starts, {0}, goal, 0, turn); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { space.plan_to_pose(starts, sh, goal, 0, 0); } catch (const std::exception&) { threw = true; }      // turn_cost 0: no unique walk
    CHECK(threw);

    // pose_fields / pose_paths directly: the cost of a read-out is gp at its target pose
    auto fr = g.pose_fields({gc}, {goal_heading}, turn, rev, true, 0, hm, -1, ctx);
    CHECK(fr.status[0] == SC_Q_OK && fr.gp.size() == (size_t)8 * n);
    std::vector<int32_t> tg, th, qf;
    for (size_t q = 0; q < starts.size(); ++q) { tg.push_back(g.cell_of(starts[q])); th.push_back(q % 2 ? -1 : sh[q]); qf.push_back(0); }
    auto pr = g.pose_paths(fr, qf, tg, th, 0, true, true, ctx);
    for (size_t q = 0; q < starts.size(); ++q) {
        CHECK(pr.status[q] == SC_Q_OK && pr.len[q] >= 1);
        int32_t best = SC_FIELD_INF;
        for (int k = 0; k < 8; ++k) best = std::min(best, fr.gp[(size_t)(k * n + tg[q])]);
        CHECK(pr.cost[q] == (th[q] < 0 ? best : fr.gp[(size_t)(th[q] * n + tg[q])]));
        for (int i = 1; i < pr.len[q]; ++i) {                                  // cells_only: an 8-connected cell path
            const int32_t a = pr.path[q * (size_t)pr.Lmax + i - 1], b = pr.path[q * (size_t)pr.Lmax + i];
            CHECK(a != b && std::abs(a % g.W - b % g.W) <= 1 && std::abs(a / g.W - b / g.W) <= 1);
        }
    }
    std::printf("pose OK\n");
    return 0;
}
