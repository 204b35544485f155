// The header's host rasteriser on worlds given as text (tests/occ_twin.py writes them): no gpu_context is created.
//   rasterize_dump WORLDS            for every world, writes int32 W, int32 H and the W*H occupancy bytes to its file
//   rasterize_dump WORLDS --time R   prints one JSON line per world: the median of R host rasterisations, in ms
// A world: its output path; grid_cells W H x_max x_min y_max y_min (grid_cells > 0: planning_space::make_grid(), else
// occupancy_grid(bound_rect, W, H).rasterize); the obstacle count; per obstacle "closed nv ne", nv vertices, ne edges
// (ne < 0: the polygon constructor).  Floats may be hexadecimal.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sea-current_amd/sea_current.hpp"

using namespace turtle::sc;

static float rdf(FILE* f) {
    char tok[128];
    if (std::fscanf(f, "%127s", tok) != 1) throw std::runtime_error("world file: expected a float");
    return std::strtof(tok, nullptr);
}
static int rdi(FILE* f) {
    int v;
    if (std::fscanf(f, "%d", &v) != 1) throw std::runtime_error("world file: expected an int");
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: rasterize_dump WORLDS [--time REPS]\n"); return 2; }
    const int reps = (argc >= 4 && std::strcmp(argv[2], "--time") == 0) ? std::atoi(argv[3]) : 0;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    const int nw = rdi(f);
    for (int w = 0; w < nw; ++w) {
        char out[4096];
        if (std::fscanf(f, "%4095s", out) != 1) return 2;
        const int cells = rdi(f), W = rdi(f), H = rdi(f);
        const float x_max = rdf(f), x_min = rdf(f), y_max = rdf(f), y_min = rdf(f);
        const bounding_rect br(x_max, x_min, y_max, y_min);
        planning_space space(br);
        const int n_obs = rdi(f);
        for (int o = 0; o < n_obs; ++o) {
            const int closed = rdi(f), nv = rdi(f), ne = rdi(f);
            std::vector<Vector2f> v;
            for (int i = 0; i < nv; ++i) { const float x = rdf(f), y = rdf(f); v.push_back(Vector2f(x, y)); }
            obstacle ob;
            if (ne < 0) {
                ob = obstacle(v);
            } else {
                std::vector<std::tuple<int, int>> e;
                for (int i = 0; i < ne; ++i) { const int a = rdi(f), b = rdi(f); e.push_back({a, b}); }
                ob = obstacle(v, e);
            }
            ob.closed = closed != 0;
            space.obstacles.push_back(ob);
        }
        space.grid_cells = cells > 0 ? cells : 1;
        auto make = [&]() {
            if (cells > 0) return space.make_grid();
            occupancy_grid g(br, W, H);
            g.rasterize(space.obstacles);
            return g;
        };
        if (reps > 0) {
            std::vector<double> ms;
            for (int r = 0; r < reps; ++r) {
                const auto t0 = std::chrono::steady_clock::now();
                const occupancy_grid g = make();
                const auto t1 = std::chrono::steady_clock::now();
                if (g.occ.empty()) return 3;
                ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            std::printf("{\"world\": \"%s\", \"host_make_grid_ms_median\": %.4f, \"reps\": %d}\n", out, ms[ms.size() / 2], reps);
            continue;
        }
        const occupancy_grid g = make();
        FILE* o = std::fopen(out, "wb");
        if (!o) { std::perror(out); return 2; }
        const int32_t wh[2] = {g.W, g.H};
        std::fwrite(wh, 4, 2, o);
        std::fwrite(g.occ.data(), 1, g.occ.size(), o);
        std::fclose(o);
    }
    std::fclose(f);
    return 0;
}
