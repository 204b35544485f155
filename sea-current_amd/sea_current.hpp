// sea_current.hpp -- MI355X-native successor of turtle-robotics/sea-current's single header.
//
// Keeps the `turtle::sc` names, argument order and result types of the reference's planning path
// and velocity-profile path (citations: file:line in the reference's sea_current.hpp), and routes
// the work to libsea_current_hip.so through the C ABI in include/sea_current_hip.h:
//
//   reference                                             here
//   ---------------------------------------------------   ------------------------------------------
//   bounding_rect                      :61-83             same members / constructor order
//   obstacle (polygon, ray casting)    :193-284           same members; rasterised into occupancy_grid
//   planning_space::is_obstacle        :1274-1280         same signature (polygon test, host)
//   planning_space::is_free            :1289-1292         same signature
//   planning_space::cost               :1315-1326         same signature and FLT_MAX convention
//   planning_space::fast_marching_trees:1339-1407         same signature; grid EDT + batched A* on the GPU
//   (new) planning_space::fast_marching_trees_sampled      the reference's FMT* itself (Halton samples, radius), batched on the GPU
//   bezier_spline::from_path / arclength :599-683,:767-896  same signatures, GPU tangents + GL-32 tables
//   bezier_spline::resample            :898-1005          same signature; nudge, split, Chebyshev fit and evaluation on the GPU
//   bezier_spline::curvature / angular_velocity :1017-1067  same signatures
//   velocity_profile                   :379-386           same members
//   vel_lim_func                       :1175              same shape
//   gen_vel_prof<N>                    :1191-1265         same argument order (END before START), GPU TOPP-RA
//   (new) occupancy_grid, planning_space::plan_batch, gen_vel_prof_batch: the batched entry points
//   (new) occupancy_grid::waypoints_batch, planning_space::simplify_paths: A* cell paths -> line-of-sight waypoints
//   (new) smooth_paths_batch: from_path -> arclength -> gen_vel_prof<1> -> resample(nudge) -> ang_vel for many paths, one call
//   (new) occupancy_grid::rasterize(obstacles, ctx), planning_space::make_grid(ctx): the polygon rasteriser on the GPU
//   (new) occupancy_grid::cost_fields / field_paths, planning_space::plan_from / plan_to: one search per shared endpoint
//   (new) occupancy_grid::clearance_penalty, cost_fields / field_paths with a costmap, planning_space::soft_clearance /
//         soft_penalty: clearance-weighted cost fields (an inflation layer) behind plan_from / plan_to
//   (new) occupancy_grid::cost_fields_multi / field_paths_multi, planning_space::plan_to_nearest: one field from many
//         goals, every start to the cheapest of them
//   (new) occupancy_grid::cost_fields_update: fields repaired after a map change instead of built again, bit-equal
//   (new) fleet_conflicts: who meets whom among the results of smooth_paths_batch, when first, and how close
//   (new) fleet_schedule: start slots by priority that let the lower-priority path wait until it meets nobody
//   (new) fleet_replan: the paths no slot was free for, planned again in (cell, tick) around the scheduled ones
//   (new) planning_space::plan_assigned: one goal per robot, the cheapest such assignment, from fields rooted at the goals
//   planner (ps, goal_point_cache, past_id) :433-441      same members
//   planner::pick_next_goal_point      :465-519           same signature; unfinished there ("TODO: fix condition"), so no
//                                                         parity: frontier clusters of the known space on the GPU
//   (new) occupancy_grid::frontiers / explore_goals, planning_space::known_grid: exploration frontiers, a goal per robot
//   (new) occupancy_grid::known_from_views / view_gain, planner::line_of_sight: sensing that walls block
//   (new) heading_dirs, occupancy_grid::known_from_sectors / sector_gain / view_gain_headings, planner::fov_span: sensors
//         with a field of view, and the heading that reveals most
//   (new) occupancy_grid::scan_cast, logodds_grid, beams_from_ranges, square_fan, planner::range_scan: range beams in, a
//         log-odds occupancy map out
//   (new) occupancy_grid::scan_match, logodds_grid::match, points_from_hits, rotate_points: a scan's pose against the map
//   (new) occupancy_grid::scan_match_wide, logodds_grid::relocalise: the same over windows of thousands of cells, pruned
//   (new) footprint, occupancy_grid::footprint_mask / pose_fields / pose_paths, planning_space::plan_to_pose: planning in
//         poses (cell, heading) with a price for turning and reversing and a rectangular body
//   (new) car_model, occupancy_grid::arc_mask / car_fields / car_paths, planning_space::plan_to_pose(.., car_model, ..):
//         car-like bodies, whose heading changes only along arcs
//   (new) occupancy_grid::frontier_centres / explore_goals_by_gain, planner::gain_weight: goals picked by what each view
//         reveals, every pick discounting the others
//
// Differences that are deliberate: obstacle::closed is initialised (the reference leaves it
// uninitialised, :197); library code never prints or calls std::exit (SC_ASSERT throws in DEBUG);
// all functions are `inline` (the reference defines non-inline functions in a header).
// Also mirrored from the "next" rows: bezier_spline::from_path, ::arclength, ::resample,
// ::curvature, ::angular_velocity -- with these the reference's whole example pipeline (examples/zmq_test.cpp:66-93)
// runs through this header.  bezier_spline::pts is an n x 2 matrix (Eigen's when present) as in the reference (:390).
// The planner's sampling helpers keep their signatures as host functions (halton, sample_free, near, point_set,
// x_state / y_state); fast_marching_trees itself plans on the grid.  Q_cache (the reference's cached Fourier coefficients) is
// kept and filled on the host; not mirrored: the ZMQ transport.  The service's request text and JSON reply are parse_path_request / serialize_path_to_json.
//
// Eigen and toppra are NOT required: if <Eigen/Dense> is on the include path it is used for
// Vector2f / VectorXf, otherwise small stand-ins with the same accessors are provided.
// There is no CPU fallback: without a gfx950 GPU every planning call throws std::runtime_error.
#pragma once

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <optional>
#include <stack>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <unordered_set>
#include <vector>

#include "../include/sea_current_hip.h"
#include "../include/sea_current_hip_update.h"
#include "../include/sea_current_hip_car.h"

#if __has_include(<Eigen/Dense>)
#include <Eigen/Dense>
#define SC_HAVE_EIGEN 1
#endif

#ifdef DEBUG
#define SC_ASSERT(cnd, msg)                                                                       \
    do {                                                                                          \
        if (!bool(cnd)) throw std::logic_error(std::string("SC_ASSERT failed: ") + #cnd + ": " + (msg)); \
    } while (0)
#else
#define SC_ASSERT(cnd, msg)
#endif

namespace turtle::sc {

#ifdef SC_HAVE_EIGEN
using Eigen::Vector2f;
using Eigen::VectorXf;
using VectorXd = Eigen::VectorXd;
template <int N> using VectorNd = Eigen::Matrix<double, N, 1>;
using points_matrix = Eigen::Matrix<float, Eigen::Dynamic, 2>;   // bezier_spline::pts (sea_current.hpp:390)
using fourier_matrix = Eigen::Matrix<std::complex<float>, Eigen::Dynamic, 2>;   // an entry of bezier_spline::Q_cache (:393)
#else
// minimal stand-ins with the accessors the API and the reference's call sites use
struct Vector2f {
    float v[2] = {0, 0};
    Vector2f() = default;
    Vector2f(float x, float y) : v{x, y} {}
    float x() const { return v[0]; }
    float y() const { return v[1]; }
    float& x() { return v[0]; }
    float& y() { return v[1]; }
    float operator()(int i) const { return v[i]; }
    float& operator()(int i) { return v[i]; }
    Vector2f operator+(const Vector2f& o) const { return {v[0] + o.v[0], v[1] + o.v[1]}; }
    Vector2f operator-(const Vector2f& o) const { return {v[0] - o.v[0], v[1] - o.v[1]}; }
    Vector2f operator-() const { return {-v[0], -v[1]}; }
    Vector2f operator*(float s) const { return {v[0] * s, v[1] * s}; }
    Vector2f operator/(float s) const { return {v[0] / s, v[1] / s}; }
    bool operator==(const Vector2f& o) const { return v[0] == o.v[0] && v[1] == o.v[1]; }
    float dot(const Vector2f& o) const { return v[0] * o.v[0] + v[1] * o.v[1]; }
    float norm() const { return std::sqrt(v[0] * v[0] + v[1] * v[1]); }
    Vector2f normalized() const { const float n = norm(); return n > 0 ? Vector2f(v[0] / n, v[1] / n) : *this; }
};
template <class S, class = std::enable_if_t<std::is_arithmetic_v<S>>>
inline Vector2f operator*(S s, const Vector2f& a) { return a * (float)s; }
// dynamic column vector: `Vec v{n}` / `Vec v(n)` give n elements (as Eigen's size constructor does), v(i), v(i, 0), v[i]
template <class T> struct VectorX_ {
    std::vector<T> d;
    VectorX_() = default;
    explicit VectorX_(size_t n) : d(n) {}
    static VectorX_ Zero(size_t n) { return VectorX_(n); }
    static VectorX_ Ones(size_t n) { VectorX_ v(n); std::fill(v.d.begin(), v.d.end(), T(1)); return v; }
    size_t rows() const { return d.size(); }
    size_t cols() const { return 1; }
    size_t size() const { return d.size(); }
    T& operator()(size_t i) { return d[i]; }
    const T& operator()(size_t i) const { return d[i]; }
    T& operator()(size_t i, size_t) { return d[i]; }
    const T& operator()(size_t i, size_t) const { return d[i]; }
    T& operator[](size_t i) { return d[i]; }
    const T& operator[](size_t i) const { return d[i]; }
    T* data() { return d.data(); }
    const T* data() const { return d.data(); }
    auto begin() { return d.begin(); }
    auto end() { return d.end(); }
    auto begin() const { return d.begin(); }
    auto end() const { return d.end(); }
    T minCoeff() const { return *std::min_element(d.begin(), d.end()); }
    T maxCoeff() const { return *std::max_element(d.begin(), d.end()); }
};
using VectorXf = VectorX_<float>;
using VectorXd = VectorX_<double>;
// fixed-size column vector: `Vec<1> v{x}` lists the coefficients
template <class T, int N> struct VectorN_ {
    T d[N] = {};
    VectorN_() = default;
    VectorN_(std::initializer_list<T> l) { int i = 0; for (T x : l) if (i < N) d[i++] = x; }
    int rows() const { return N; }
    T& operator()(int i) { return d[i]; }
    const T& operator()(int i) const { return d[i]; }
    T& operator()(int i, int) { return d[i]; }
    const T& operator()(int i, int) const { return d[i]; }
    T& operator[](int i) { return d[i]; }
    const T& operator[](int i) const { return d[i]; }
};
template <int N> using VectorNd = VectorN_<double, N>;
// n x 2 matrix of points, row-major: m(i, c), m.rows(), m.col(c) (a copy), m.row(i)
struct points_matrix {
    std::vector<float> d;
    points_matrix() = default;
    explicit points_matrix(size_t n, size_t = 2) : d(2 * n) {}
    static points_matrix Zero(size_t n, size_t = 2) { return points_matrix(n); }
    void resize(size_t n, size_t = 2) { d.resize(2 * n); }
    size_t rows() const { return d.size() / 2; }
    size_t cols() const { return 2; }
    float& operator()(size_t i, size_t c) { return d[2 * i + c]; }
    const float& operator()(size_t i, size_t c) const { return d[2 * i + c]; }
    Vector2f row(size_t i) const { return Vector2f(d[2 * i], d[2 * i + 1]); }
    VectorXf col(size_t c) const { VectorXf v(rows()); for (size_t i = 0; i < rows(); ++i) v(i) = d[2 * i + c]; return v; }
    const float* data() const { return d.data(); }
    float* data() { return d.data(); }
};
// (degree + 1) x 2 complex coefficients: an entry of bezier_spline::Q_cache (sea_current.hpp:393)
struct fourier_matrix {
    std::vector<std::complex<float>> d;
    fourier_matrix() = default;
    explicit fourier_matrix(size_t n, size_t = 2) : d(2 * n) {}
    static fourier_matrix Zero(size_t n, size_t = 2) { return fourier_matrix(n); }
    size_t rows() const { return d.size() / 2; }
    size_t cols() const { return 2; }
    std::complex<float>& operator()(size_t i, size_t c) { return d[2 * i + c]; }
    const std::complex<float>& operator()(size_t i, size_t c) const { return d[2 * i + c]; }
};
#endif

}  // namespace turtle::sc

// The names the reference's callers spell (examples/zmq_test.cpp:69-86, examples/test.cpp:184-204, examples/json_test.cpp:
// 29-47): toppra::Vector / toppra::value_type, and Eigen::Vector<value_type, N> for the arguments of gen_vel_prof.  With
// toppra / Eigen on the include path they are the real types; otherwise these aliases of the stand-ins above keep
// those call sites compiling unchanged (define SC_NO_NAMESPACE_STANDINS to keep namespaces `toppra` / `Eigen` untouched).
#if __has_include(<toppra/toppra.hpp>)
#include <toppra/toppra.hpp>
#elif !defined(SC_NO_NAMESPACE_STANDINS)
namespace toppra {
using value_type = double;
using Vector = turtle::sc::VectorXd;
}  // namespace toppra
#endif
#if !defined(SC_HAVE_EIGEN) && !defined(SC_NO_NAMESPACE_STANDINS)
namespace Eigen {
template <class T, int N> using Vector = turtle::sc::VectorN_<T, N>;
}  // namespace Eigen
#endif

namespace turtle::sc {

// the toppra types that appear in the reference's signatures (`using toppra::value_type`, sea_current.hpp:1172)
using value_type = double;
namespace toppra_compat { using Vector = VectorXd; }

// ---- GPU context -------------------------------------------------------------------------------
class gpu_context {
public:
    explicit gpu_context(int device = 0) {
        int st = sc_ctx_create(device, &h_);
        if (st != SC_OK)
            throw std::runtime_error(std::string("sea_current: no usable MI355X context (") + sc_status_string(st) +
                                     "); there is no CPU fallback");
    }
    ~gpu_context() { if (h_) sc_ctx_destroy(h_); }
    gpu_context(const gpu_context&) = delete;
    gpu_context& operator=(const gpu_context&) = delete;
    sc_ctx* get() const { return h_; }
    void check(int st, const char* what) const {
        if (st != SC_OK) throw std::runtime_error(std::string(what) + ": " + sc_status_string(st) + ": " + sc_last_error(h_));
    }
private:
    sc_ctx* h_ = nullptr;
};
// one context per host thread (contexts are not shared between threads: sea_current_hip.h)
inline gpu_context& default_context() {
    thread_local gpu_context ctx(0);
    return ctx;
}

// ---- geometry (sea_current.hpp:61-83) -------------------------------------------------------------
struct bounding_rect {
    float x_max;
    float x_min;
    float y_max;
    float y_min;
    bounding_rect(const float x_max, const float x_min, const float y_max, const float y_min)
        : x_max(x_max), x_min(x_min), y_max(y_max), y_min(y_min) {}
    inline bool contains(const Vector2f& p) const { return p.x() <= x_max && p.x() >= x_min && p.y() <= y_max && p.y() >= y_min; }
    inline void enclose_point(const Vector2f& p) {
        x_max = std::max(x_max, p.x()); x_min = std::min(x_min, p.x());
        y_max = std::max(y_max, p.y()); y_min = std::min(y_min, p.y());
    }
};

// L2 distance, in the reference's arithmetic (:86-88): float differences, squared and rooted in double -- the GPU planner
// (csrc/fmt.hip) and this host function then agree to the bit on the radius tests of near()
inline float pt_dist(const Vector2f& u, const Vector2f& v = {0, 0}) {
    const double dx = v.x() - u.x(), dy = v.y() - u.y();
    return (float)std::sqrt(dx * dx + dy * dy);
}
// distance from point a to the (infinite) line through p1 and p2 (:181-190)
inline float dist_pt_line(const Vector2f& p1, const Vector2f& p2, const Vector2f a) {
    const float twice_area = std::abs((p2.x() - p1.x()) * (p1.y() - a.y()) - (p1.x() - a.x()) * (p2.y() - p1.y()));
    return twice_area / (p2 - p1).norm();
}
inline float cross2d(const Vector2f& a, const Vector2f& b) { return a.x() * b.y() - a.y() * b.x(); }

// proper intersection of segments p1p2 and q1q2 (colinear overlap counts as no hit, as in :142-178)
inline std::tuple<bool, Vector2f> intersects(const Vector2f& p1, const Vector2f& p2, const Vector2f& q1, const Vector2f& q2) {
    const Vector2f r = p2 - p1, s = q2 - q1, qp = q1 - p1;
    const float den = cross2d(r, s);
    if (den == 0.0f) return {false, Vector2f(0, 0)};
    const float t = cross2d(qp, s) / den, u = cross2d(qp, r) / den;
    if (t < 0 || t > 1 || u < 0 || u > 1) return {false, Vector2f(0, 0)};
    return {true, p1 + r * t};
}

// ---- obstacle (sea_current.hpp:193-284) -----------------------------------------------------------
struct obstacle {
    std::vector<std::tuple<Vector2f, Vector2f>> lines;
    std::vector<Vector2f> vertices;
    bounding_rect bound_rect = {0, 0, 0, 0};
    bool closed = true;  // the reference never initialises this member
    int64_t id = 0;

    obstacle() {}
    // closed polygon through `vertices` (the last edge returns to the first vertex)
    obstacle(std::vector<Vector2f> verts) : vertices(std::move(verts)) {
        if (vertices.empty()) return;
        bound_rect = {vertices[0].x(), vertices[0].x(), vertices[0].y(), vertices[0].y()};
        for (size_t i = 0; i < vertices.size(); ++i) {
            lines.push_back({vertices[i], vertices[(i + 1) % vertices.size()]});
            bound_rect.enclose_point(vertices[i]);
        }
    }
    // explicit edge list (open or closed shapes)
    obstacle(std::vector<Vector2f> verts, std::vector<std::tuple<int, int>> edges) : vertices(std::move(verts)) {
        if (vertices.empty()) return;
        bound_rect = {vertices[0].x(), vertices[0].x(), vertices[0].y(), vertices[0].y()};
        for (const auto& e : edges) {
            SC_ASSERT(std::get<0>(e) < (int)vertices.size() && std::get<1>(e) < (int)vertices.size(), "edge index out of range");
            lines.push_back({vertices[std::get<0>(e)], vertices[std::get<1>(e)]});
            bound_rect.enclose_point(vertices[std::get<0>(e)]);
            bound_rect.enclose_point(vertices[std::get<1>(e)]);
        }
    }
    // even-odd rule on the edge list (closed) / distance-to-edge test (open), after the AABB reject
    bool contains(const Vector2f& p) const {
        if (!bound_rect.contains(p)) return false;
        if (!closed) {
            for (const auto& [a, b] : lines) {
                const Vector2f ab = b - a, ap = p - a;
                const float len = ab.norm();
                if (len > 0 && std::fabs(cross2d(ab, ap)) / len < 0.01f) return true;
            }
            return false;
        }
        bool inside = false;
        for (const auto& [a, b] : lines) {
            if ((a.y() > p.y()) != (b.y() > p.y())) {
                const float xi = a.x() + (p.y() - a.y()) * (b.x() - a.x()) / (b.y() - a.y());
                if (p.x() < xi) inside = !inside;
            }
        }
        return inside;
    }
};

// ---- scan matching (new; the reference has no counterpart) ------------------------------------------
// A scan's end points as cell offsets (px, py) from the sensor cell; SC_MATCH_ABSENT in both for a beam without an end point.
using scan_points = std::vector<std::array<int32_t, 2>>;
// The window (+-wx, +-wy cells around the prior), the cap of the squared distance a point can cost, what a point on an unknown
// cell or outside the grid costs, and the number of candidate rotations the points come in (sc_scan_match_batch).
struct match_params {
    int wx = 8, wy = 8;
    int32_t d2_cap = 64, unk = 1;
    int rotations = 1;
};
// The same for a wide window (sc_scan_match_wide_batch): +-wx, +-wy up to SC_MATCH_WIDE_MAX_HALF cells, searched from nodes
// of 4^top x 4^top poses down, with room for max_nodes nodes per scan and level.
struct wide_match_params {
    int wx = 256, wy = 256;
    int32_t d2_cap = 64, unk = 1;
    int rotations = 1;
    int top = 3, max_nodes = 1 << 16;
};

// A heading table of B evenly spaced directions, counter-clockwise: round(32767 (cos, sin)(2 pi (b + phase) / B)),
// 3 <= B <= SC_VIEW_MAX_BINS (sc_view_gain_headings_batch's dirs).  Consecutive entries bound the bins; heading h of a sensor that
// covers `span` bins is the sector from entry h to entry (h + span) % B.  Computed in double; valid, no bit claim beyond that.
using heading_table = std::vector<std::array<int32_t, 2>>;
inline heading_table heading_dirs(int B, double phase = 0.0) {
    if (B < 3 || B > SC_VIEW_MAX_BINS) throw std::invalid_argument("heading_dirs: B outside 3 .. SC_VIEW_MAX_BINS");
    heading_table d((size_t)B);
    const double turn = 2.0 * std::acos(-1.0);
    for (int b = 0; b < B; ++b) {
        const double t = turn * (b + phase) / B;
        d[(size_t)b] = {(int32_t)std::nearbyint(32767.0 * std::cos(t)), (int32_t)std::nearbyint(32767.0 * std::sin(t))};
    }
    return d;
}
// A view with a heading as a sector row (cx, cy, r2, a, b) of sc_known_from_sectors; span == B: a = b = 0, the full circle.
inline std::array<int32_t, 7> sector_view(const std::array<int32_t, 3>& view, const heading_table& dirs, int h, int span) {
    const int B = (int)dirs.size();
    if (B < 1 || span < 1 || span > B) throw std::invalid_argument("sector_view: span outside 1 .. B");
    std::array<int32_t, 7> r{view[0], view[1], view[2], 0, 0, 0, 0};
    if (span < B) {
        const auto &a = dirs[(size_t)(((h % B) + B) % B)], &b = dirs[(size_t)(((h % B) + B + span) % B)];
        r[3] = a[0]; r[4] = a[1]; r[5] = b[0]; r[6] = b[1];
    }
    return r;
}

// A rectangular body in the robot's frame, in whole cells from the reference cell: `left` is counter-clockwise of the heading.
// Each extent 0 .. SC_FOOTPRINT_MAX.  All zero: the disc that the clearance already stands for.
struct footprint {
    int front = 0, back = 0, left = 0, right = 0;
};

// The motion model of a car-like body (include/sea_current_hip_car.h): the heading changes only along arcs of arc_n cells
// straight, 45 degrees, arc_n cells straight (1 .. SC_ARC_MAX; a turning radius of about 3 arc_n cells), never on the spot.  An
// arc costs 24 arc_n + arc_cost, reversing rev_cost more per cell (-1: no reversing), in the units of the move costs.
struct car_model {
    int arc_n = 1, arc_cost = 0, rev_cost = -1;
};

// ---- occupancy grid (new): the world model the GPU path works on ----------------------------------
// Row-major uint8 occupancy over a bounding_rect; cell (ix, iy) covers
// [x_min + ix*res, x_min + (ix+1)*res) x [y_min + iy*res, ...).  d2 is the exact squared distance (in
// cells) to the nearest occupied cell, computed on the GPU (sc_edt_u8_i32).
class occupancy_grid {
public:
    int W = 0, H = 0;
    float resolution = 1.0f;
    bounding_rect bound_rect = {0, 0, 0, 0};
    std::vector<uint8_t> occ;
    std::vector<int32_t> d2;  // filled by edt()

    occupancy_grid() = default;
    occupancy_grid(const bounding_rect& br, int cells_x, int cells_y)
        : W(cells_x), H(cells_y), resolution((br.x_max - br.x_min) / (float)cells_x), bound_rect(br),
          occ((size_t)cells_x * cells_y, 0) {}

    int cell_x(float x) const { return std::clamp((int)std::floor((x - bound_rect.x_min) / resolution), 0, W - 1); }
    int cell_y(float y) const { return std::clamp((int)std::floor((y - bound_rect.y_min) / ((bound_rect.y_max - bound_rect.y_min) / (float)H)), 0, H - 1); }
    int32_t cell_of(const Vector2f& p) const { return cell_y(p.y()) * W + cell_x(p.x()); }
    Vector2f centre_of(int32_t c) const {
        const float ry = (bound_rect.y_max - bound_rect.y_min) / (float)H;
        return Vector2f(bound_rect.x_min + ((c % W) + 0.5f) * resolution, bound_rect.y_min + ((c / W) + 0.5f) * ry);
    }
    // mark every cell whose centre lies inside a closed obstacle or that an obstacle edge passes through
    void rasterize(const std::vector<obstacle>& obstacles) {
        const float ry = (bound_rect.y_max - bound_rect.y_min) / (float)H;
        for (const auto& ob : obstacles) {
            if (ob.lines.empty()) continue;
            if (ob.closed) {
                const int x0 = cell_x(ob.bound_rect.x_min), x1 = cell_x(ob.bound_rect.x_max);
                const int y0 = cell_y(ob.bound_rect.y_min), y1 = cell_y(ob.bound_rect.y_max);
                for (int iy = y0; iy <= y1; ++iy)
                    for (int ix = x0; ix <= x1; ++ix)
                        if (ob.contains(centre_of(iy * W + ix))) occ[(size_t)iy * W + ix] = 1;
            }
            for (const auto& [a, b] : ob.lines) {  // edges: sample at sub-cell steps
                const float len = (b - a).norm();
                const int n = std::max(1, (int)std::ceil(len / (0.5f * std::min(resolution, ry))));
                for (int k = 0; k <= n; ++k) occ[(size_t)cell_of(a + (b - a) * ((float)k / n))] = 1;
            }
        }
    }
    // the same bytes as rasterize(obstacles), painted over the current occ on the GPU (sc_occ_from_polygons_host: throws
    // when an obstacle breaks the contract of sea_current_hip.h -- finite coordinates within 2^30 cells, edges of at
    // most 2^24 samples)
    void rasterize(const std::vector<obstacle>& obstacles, gpu_context& ctx) {
        const float ry = (bound_rect.y_max - bound_rect.y_min) / (float)H;
        std::vector<float> lines, box;
        std::vector<int32_t> off{0};
        std::vector<uint8_t> closed;
        for (const auto& ob : obstacles) {
            for (const auto& [a, b] : ob.lines) { lines.push_back(a.x()); lines.push_back(a.y()); lines.push_back(b.x()); lines.push_back(b.y()); }
            off.push_back((int32_t)(lines.size() / 4));
            box.push_back(ob.bound_rect.x_max); box.push_back(ob.bound_rect.x_min); box.push_back(ob.bound_rect.y_max); box.push_back(ob.bound_rect.y_min);
            closed.push_back(ob.closed ? 1 : 0);
        }
        const int n_obs = (int)obstacles.size();
        ctx.check(sc_occ_from_polygons_host(ctx.get(), occ.data(), 1, W, H, bound_rect.x_min, bound_rect.y_min, resolution, ry,
                                            lines.empty() ? nullptr : lines.data(), (int)(lines.size() / 4), off.data(), n_obs,
                                            n_obs ? box.data() : nullptr, n_obs ? closed.data() : nullptr, nullptr, occ.data()),
                  "sc_occ_from_polygons_host");
    }
    // exact squared EDT on the GPU
    void edt(gpu_context& ctx = default_context()) {
        d2.resize(occ.size());
        ctx.check(sc_edt_u8_i32_host(ctx.get(), occ.data(), W, H, 1, d2.data()), "sc_edt_u8_i32_host");
    }
    struct batch_result {
        std::vector<int32_t> path, len, cost, status;  // path is [Q][Lmax]
        int Lmax = 0;
    };
    // Q independent start->goal queries (linear cell indices); r2_clear = squared clearance in cells
    batch_result astar_batch(const std::vector<int32_t>& start, const std::vector<int32_t>& goal, int32_t r2_clear = 0,
                             int Lmax = 0, gpu_context& ctx = default_context()) {
        if (d2.size() != occ.size()) edt(ctx);
        batch_result r;
        const int Q = (int)start.size();
        r.Lmax = Lmax > 0 ? Lmax : 4 * (W + H);
        r.path.assign((size_t)Q * r.Lmax, -1); r.len.assign(Q, 0); r.cost.assign(Q, -1); r.status.assign(Q, SC_Q_NO_PATH);
        if (Q == 0) return r;
        ctx.check(sc_astar_batch_host(ctx.get(), d2.data(), W, H, r2_clear, start.data(), goal.data(), Q, r.Lmax,
                                      r.path.data(), r.len.data(), r.cost.data(), r.status.data()), "sc_astar_batch_host");
        return r;
    }
    // Connected components of the traversable cells (sc_components_batch): label[c] = the smallest cell index of c's
    // component, -1 where d2[c] < max(r2_clear, 1); size[c] = the cell count at every representative (label[c] == c), 0
    // elsewhere; ncomp components; largest = the representative of the largest one (ties to the smaller index), -1 when no
    // cell is traversable.  Two traversable cells have an A* path iff their labels are equal.
    struct component_result {
        std::vector<int32_t> label, size;  // [H][W]
        int32_t ncomp = 0, largest = -1;
        int32_t r2 = 0;
    };
    component_result components(int32_t r2_clear = 0, gpu_context& ctx = default_context()) {
        if (d2.size() != occ.size()) edt(ctx);
        component_result r;
        r.r2 = r2_clear;
        r.label.assign(occ.size(), -1); r.size.assign(occ.size(), 0);
        if (occ.empty()) return r;
        ctx.check(sc_components_batch_host(ctx.get(), d2.data(), 1, W, H, r2_clear, r.label.data(), r.size.data(), &r.ncomp, &r.largest),
                  "sc_components_batch_host");
        return r;
    }
    // The status astar_batch gives every query, from the labels alone (sc_reachable_batch): SC_Q_BAD_ENDPOINT, SC_Q_NO_PATH, or
    // SC_Q_OK where A* returns SC_Q_OK or SC_Q_TRUNCATED.
    std::vector<int32_t> reachable(const component_result& cr, const std::vector<int32_t>& start, const std::vector<int32_t>& goal,
                                   gpu_context& ctx = default_context()) const {
        if (start.size() != goal.size()) throw std::invalid_argument("occupancy_grid::reachable: start and goal differ in size");
        std::vector<int32_t> st(start.size(), SC_Q_BAD_ENDPOINT);
        if (start.empty() || cr.label.size() != occ.size() || occ.empty()) return st;
        ctx.check(sc_reachable_batch_host(ctx.get(), cr.label.data(), 1, nullptr, W, H, start.data(), goal.data(), (int)start.size(), st.data()),
                  "sc_reachable_batch_host");
        return st;
    }
    // astar_batch that never searches a query whose endpoints lie in different components of `cr` (components() with the
    // same r2_clear): the results are those of astar_batch.  The labels are on the host here, so the three steps of
    // sc_astar_batch_screened are taken on the host: such a query's start becomes -1, the search leaves it at once as a bad
    // endpoint (len 0, cost -1), and its status is set to SC_Q_NO_PATH.
    batch_result astar_batch_screened(const component_result& cr, const std::vector<int32_t>& start, const std::vector<int32_t>& goal,
                                      int Lmax = 0, gpu_context& ctx = default_context()) {
        if (cr.label.size() != occ.size()) throw std::invalid_argument("occupancy_grid::astar_batch_screened: labels are not [H][W]");
        const int32_t n = (int32_t)occ.size();
        std::vector<int32_t> masked(start);
        std::vector<char> cut(start.size(), 0);
        for (size_t q = 0; q < start.size() && q < goal.size(); ++q) {
            const int32_t s = start[q], t = goal[q];
            if (s < 0 || t < 0 || s >= n || t >= n) continue;
            const int32_t ls = cr.label[(size_t)s], lt = cr.label[(size_t)t];
            if (ls >= 0 && lt >= 0 && ls != lt) { masked[q] = -1; cut[q] = 1; }
        }
        batch_result r = astar_batch(masked, goal, cr.r2, Lmax, ctx);
        for (size_t q = 0; q < cut.size(); ++q)
            if (cut[q]) r.status[q] = SC_Q_NO_PATH;
        return r;
    }
    // Cost-to-come fields (sc_cost_field_batch): g[f] = the optimal A* cost from roots[f] to every cell, SC_FIELD_INF where
    // there is none; status[f] SC_Q_OK or SC_Q_BAD_ENDPOINT.  rounds < 0: the library default.
    struct field_result {
        std::vector<int32_t> g, status, roots;  // g is [F][H][W]
        int32_t r2 = 0;
        std::vector<uint8_t> pen;               // the costmap of a weighted field ([H][W]), empty for an unweighted one:
        int pen_cap = 0;                        // field_paths reads a field with what cost_fields computed it with
        int rounds = -1;                        // what cost_fields was called with: cost_fields_update repeats it
        int32_t r2_soft = 0;                    // > 0: pen is clearance_penalty(r2, r2_soft, pen_max) of the grid (the soft knobs of
        int pen_max = 0;                        // planning_space), and cost_fields_update recomputes it; 0: pen is the caller's own
    };
    // Repair fields after a map change (sc_cost_field_update_batch): `fields` is what cost_fields
    // returned on `before`, a grid of this grid's size; on return it is, bit for bit, what cost_fields returns on this
    // grid for the roots, r2, rounds and costmap it remembers.  A costmap from the soft knobs (r2_soft > 0) is computed
    // again for this grid; a caller's own costmap stays as it is.  stats (may be NULL): per field the changed cells and the
    // cells that lost their support.
    field_result& cost_fields_update(const occupancy_grid& before, field_result& fields, gpu_context& ctx = default_context(),
                                     std::vector<std::array<int32_t, 2>>* stats = nullptr) {
        if (before.W != W || before.H != H) throw std::invalid_argument("occupancy_grid::cost_fields_update: the grids differ in size");
        if (before.d2.size() != before.occ.size()) throw std::invalid_argument("occupancy_grid::cost_fields_update: `before` has no distance map (edt)");
        const int F = (int)fields.roots.size();
        if (fields.g.size() != (size_t)F * W * H) throw std::invalid_argument("occupancy_grid::cost_fields_update: fields.g is not [F][H][W]");
        if (d2.size() != occ.size()) edt(ctx);
        fields.status.assign(F, SC_Q_BAD_ENDPOINT);
        if (stats) stats->assign(F, std::array<int32_t, 2>{0, 0});
        if (F == 0) return fields;
        int32_t* st = stats ? (*stats)[0].data() : nullptr;
        if (fields.pen.empty()) {
            ctx.check(sc_cost_field_update_batch_host(ctx.get(), before.d2.data(), d2.data(), 1, nullptr, W, H, fields.r2, fields.roots.data(), F,
                                                      fields.rounds, fields.g.data(), fields.status.data(), st),
                      "sc_cost_field_update_batch_host");
            return fields;
        }
        std::vector<uint8_t> pen_new = fields.r2_soft > 0 ? clearance_penalty(fields.r2, fields.r2_soft, fields.pen_max, ctx) : fields.pen;
        ctx.check(sc_cost_field_weighted_update_batch_host(ctx.get(), before.d2.data(), fields.pen.data(), d2.data(), pen_new.data(),
                                                           fields.pen_cap, 1, nullptr, W, H, fields.r2, fields.roots.data(), F, fields.rounds,
                                                           fields.g.data(), fields.status.data(), st),
                  "sc_cost_field_weighted_update_batch_host");
        fields.pen = std::move(pen_new);
        return fields;
    }
    field_result cost_fields(const std::vector<int32_t>& roots, int32_t r2_clear = 0, int rounds = -1,
                             gpu_context& ctx = default_context()) {
        return cost_fields_with(roots, nullptr, 0, r2_clear, rounds, ctx);
    }
    // The costmap of the weighted fields from d2 (sc_clearance_penalty_u8): pen_max next to the hard clearance r2_clear,
    // falling linearly with the distance to 0 at sqrt(r2_soft) cells.
    std::vector<uint8_t> clearance_penalty(int32_t r2_clear, int32_t r2_soft, int pen_max, gpu_context& ctx = default_context()) {
        if (d2.size() != occ.size()) edt(ctx);
        std::vector<uint8_t> pen(occ.size(), 0);
        ctx.check(sc_clearance_penalty_u8_host(ctx.get(), d2.data(), W, H, 1, r2_clear, r2_soft, pen_max, pen.data()),
                  "sc_clearance_penalty_u8_host");
        return pen;
    }
    // Weighted cost fields (sc_cost_field_weighted_batch): entering cell c costs min(pen[c], pen_cap) on top of the 10 / 14
    // of the move; pen is [H][W].  The result remembers pen and pen_cap for field_paths.
    field_result cost_fields(const std::vector<int32_t>& roots, const std::vector<uint8_t>& pen, int pen_cap, int32_t r2_clear = 0,
                             int rounds = -1, gpu_context& ctx = default_context()) {
        return cost_fields_with(roots, &pen, pen_cap, r2_clear, rounds, ctx);
    }
    // Paths read from fields (sc_field_paths_batch): query q follows field qfield[q] to targets[q].  Equal to astar_batch
    // with start roots[qfield[q]] and goal targets[q] (to_root = false), or to its paths reversed (to_root = true).  A
    // weighted field is read with its own costmap (sc_field_paths_weighted_batch).
    batch_result field_paths(const field_result& fr, const std::vector<int32_t>& qfield, const std::vector<int32_t>& targets,
                             int Lmax = 0, bool to_root = false, gpu_context& ctx = default_context()) {
        if (d2.size() != occ.size()) edt(ctx);
        batch_result r;
        const int Q = (int)targets.size(), F = (int)fr.roots.size();
        if (qfield.size() != targets.size()) throw std::invalid_argument("occupancy_grid::field_paths: qfield and targets differ in size");
        r.Lmax = Lmax > 0 ? Lmax : 4 * (W + H);
        r.path.assign((size_t)Q * r.Lmax, -1); r.len.assign(Q, 0); r.cost.assign(Q, -1); r.status.assign(Q, SC_Q_NO_PATH);
        if (Q == 0) return r;
        if (F == 0) { r.status.assign(Q, SC_Q_BAD_ENDPOINT); return r; }
        // the weighted entry takes the costmap after d2, the rest is one argument list
        auto call = [&](auto entry, auto... costmap) {
            return entry(ctx.get(), d2.data(), costmap..., 1, nullptr, W, H, fr.r2, fr.g.data(), fr.roots.data(), F, qfield.data(),
                         targets.data(), Q, r.Lmax, to_root ? 1 : 0, r.path.data(), r.len.data(), r.cost.data(), r.status.data());
        };
        if (fr.pen.empty()) ctx.check(call(sc_field_paths_batch_host), "sc_field_paths_batch_host");
        else ctx.check(call(sc_field_paths_weighted_batch_host, fr.pen.data(), fr.pen_cap), "sc_field_paths_weighted_batch_host");
        return r;
    }
    // The per-heading collision mask of a body (sc_footprint_mask_u8): bit k of mask[c] is set iff the body, at heading k
    // (SC_POSE_HEADINGS = 8, counter-clockwise from +x) and inflated by the disc r2_clear stands for, covers no blocked cell.
    std::vector<uint8_t> footprint_mask(const footprint& fp, int32_t r2_clear = 0, gpu_context& ctx = default_context()) {
        if (d2.size() != occ.size()) edt(ctx);
        std::vector<uint8_t> m(occ.size(), 0);
        if (occ.empty()) return m;
        ctx.check(sc_footprint_mask_u8_host(ctx.get(), d2.data(), W, H, 1, r2_clear, fp.front, fp.back, fp.left, fp.right, m.data()),
                  "sc_footprint_mask_u8_host");
        return m;
    }
    // Cost fields over poses (sc_pose_field_batch): gp[f][k][c] = the optimal cost from the pose (roots[f], rhead[f]) to (c, k)
    // -- toward: from (c, k) to it -- with forward moves at 10 / 14, reverse moves rev_cost dearer (-1: none) and turns of 45
    // degrees on the spot at turn_cost; SC_FIELD_INF where there is none.  rhead[f] = -1 roots the field at every heading that
    // fits.  hmask: what footprint_mask returned, or empty for the disc.  The result remembers what pose_paths needs.
    struct pose_field_result {
        std::vector<int32_t> gp, status, roots, rhead;  // gp is [F][8][H][W]
        std::vector<uint8_t> hmask;
        int32_t r2 = 0;
        int turn_cost = 0, rev_cost = -1;
        bool toward = false;
    };
    pose_field_result pose_fields(const std::vector<int32_t>& roots, const std::vector<int32_t>& rhead, int turn_cost, int rev_cost = -1,
                                  bool toward = false, int32_t r2_clear = 0, const std::vector<uint8_t>& hmask = {}, int rounds = -1,
                                  gpu_context& ctx = default_context()) {
        if (roots.size() != rhead.size()) throw std::invalid_argument("occupancy_grid::pose_fields: roots and rhead differ in size");
        if (!hmask.empty() && hmask.size() != occ.size()) throw std::invalid_argument("occupancy_grid::pose_fields: hmask is not [H][W]");
        if (d2.size() != occ.size()) edt(ctx);
        pose_field_result r;
        r.roots = roots; r.rhead = rhead; r.hmask = hmask; r.r2 = r2_clear; r.turn_cost = turn_cost; r.rev_cost = rev_cost; r.toward = toward;
        const int F = (int)roots.size();
        r.gp.assign((size_t)F * SC_POSE_HEADINGS * occ.size(), SC_FIELD_INF); r.status.assign(F, SC_Q_BAD_ENDPOINT);
        if (F == 0) return r;
        ctx.check(sc_pose_field_batch_host(ctx.get(), d2.data(), hmask.empty() ? nullptr : hmask.data(), 1, nullptr, W, H, r2_clear, turn_cost,
                                           rev_cost, toward ? 1 : 0, roots.data(), rhead.data(), F, rounds, r.gp.data(), r.status.data()),
                  "sc_pose_field_batch_host");
        return r;
    }
    // Pose paths read from pose fields (sc_pose_paths_batch): query q follows field qfield[q] to the pose (targets[q],
    // thead[q]) (thead -1: the cheapest heading there).  One entry per pose in path and head; to_root writes target..root, the
    // driving order of a toward field; cells_only keeps the first pose of every cell.
    struct pose_paths_result {
        std::vector<int32_t> path, len, cost, status;  // path is [Q][Lmax]
        std::vector<uint8_t> head;                     // [Q][Lmax]
        int Lmax = 0;
    };
    pose_paths_result pose_paths(const pose_field_result& fr, const std::vector<int32_t>& qfield, const std::vector<int32_t>& targets,
                                 const std::vector<int32_t>& thead, int Lmax = 0, bool to_root = false, bool cells_only = false,
                                 gpu_context& ctx = default_context()) {
        if (qfield.size() != targets.size() || thead.size() != targets.size())
            throw std::invalid_argument("occupancy_grid::pose_paths: qfield, targets and thead differ in size");
        if (d2.size() != occ.size()) edt(ctx);
        pose_paths_result r;
        const int Q = (int)targets.size(), F = (int)fr.roots.size();
        r.Lmax = Lmax > 0 ? Lmax : 16 * (W + H);
        r.path.assign((size_t)Q * r.Lmax, -1); r.head.assign((size_t)Q * r.Lmax, 0);
        r.len.assign(Q, 0); r.cost.assign(Q, -1); r.status.assign(Q, SC_Q_NO_PATH);
        if (Q == 0) return r;
        if (F == 0) { r.status.assign(Q, SC_Q_BAD_ENDPOINT); return r; }
        ctx.check(sc_pose_paths_batch_host(ctx.get(), d2.data(), fr.hmask.empty() ? nullptr : fr.hmask.data(), 1, nullptr, W, H, fr.r2,
                                           fr.turn_cost, fr.rev_cost, fr.toward ? 1 : 0, fr.gp.data(), fr.roots.data(), fr.rhead.data(), F,
                                           qfield.data(), targets.data(), thead.data(), Q, r.Lmax, to_root ? 1 : 0, cells_only ? 1 : 0,
                                           r.path.data(), r.head.data(), r.len.data(), r.cost.data(), r.status.data()),
                  "sc_pose_paths_batch_host");
        return r;
    }
    // The legal arcs of every pose (sc_arc_mask_u16): bit 2k of mask[c] is set iff the arc from (c, k) to heading k + 1 is legal
    // for the body of hmask (what footprint_mask returned, or empty for the disc), bit 2k + 1 iff the one to k - 1 is.
    std::vector<uint16_t> arc_mask(int arc_n, int32_t r2_clear = 0, const std::vector<uint8_t>& hmask = {}, gpu_context& ctx = default_context()) {
        if (!hmask.empty() && hmask.size() != occ.size()) throw std::invalid_argument("occupancy_grid::arc_mask: hmask is not [H][W]");
        if (d2.size() != occ.size()) edt(ctx);
        std::vector<uint16_t> m(occ.size(), 0);
        if (occ.empty()) return m;
        ctx.check(sc_arc_mask_u16_host(ctx.get(), d2.data(), hmask.empty() ? nullptr : hmask.data(), W, H, 1, r2_clear, arc_n, m.data()),
                  "sc_arc_mask_u16_host");
        return m;
    }
    // Cost fields over poses for a car-like body (sc_car_field_batch): pose_fields with car.arc_n-cell arcs in the place of
    // turns on the spot.  The arc mask is computed here; the result remembers what car_paths needs.
    struct car_field_result {
        std::vector<int32_t> gp, status, roots, rhead;  // gp is [F][8][H][W]
        std::vector<uint8_t> hmask;
        std::vector<uint16_t> amask;
        int32_t r2 = 0;
        car_model car;
        bool toward = false;
    };
    car_field_result car_fields(const std::vector<int32_t>& roots, const std::vector<int32_t>& rhead, const car_model& car, bool toward = false,
                                int32_t r2_clear = 0, const std::vector<uint8_t>& hmask = {}, int rounds = -1,
                                gpu_context& ctx = default_context()) {
        if (roots.size() != rhead.size()) throw std::invalid_argument("occupancy_grid::car_fields: roots and rhead differ in size");
        if (!hmask.empty() && hmask.size() != occ.size()) throw std::invalid_argument("occupancy_grid::car_fields: hmask is not [H][W]");
        if (d2.size() != occ.size()) edt(ctx);
        car_field_result r;
        r.roots = roots; r.rhead = rhead; r.hmask = hmask; r.r2 = r2_clear; r.car = car; r.toward = toward;
        const int F = (int)roots.size();
        r.gp.assign((size_t)F * SC_POSE_HEADINGS * occ.size(), SC_FIELD_INF); r.status.assign(F, SC_Q_BAD_ENDPOINT);
        r.amask = arc_mask(car.arc_n, r2_clear, hmask, ctx);
        if (F == 0) return r;
        ctx.check(sc_car_field_batch_host(ctx.get(), d2.data(), hmask.empty() ? nullptr : hmask.data(), r.amask.data(), 1, nullptr, W, H,
                                          r2_clear, car.arc_n, car.arc_cost, car.rev_cost, toward ? 1 : 0, roots.data(), rhead.data(), F, rounds,
                                          r.gp.data(), r.status.data()),
                  "sc_car_field_batch_host");
        return r;
    }
    // Car paths read from car fields (sc_car_paths_batch): one entry per cell, the cells of an arc included, so path is
    // 8-connected; to_root writes target..root, the driving order of a toward field.
    pose_paths_result car_paths(const car_field_result& fr, const std::vector<int32_t>& qfield, const std::vector<int32_t>& targets,
                                const std::vector<int32_t>& thead, int Lmax = 0, bool to_root = false, gpu_context& ctx = default_context()) {
        if (qfield.size() != targets.size() || thead.size() != targets.size())
            throw std::invalid_argument("occupancy_grid::car_paths: qfield, targets and thead differ in size");
        if (d2.size() != occ.size()) edt(ctx);
        pose_paths_result r;
        const int Q = (int)targets.size(), F = (int)fr.roots.size();
        r.Lmax = Lmax > 0 ? Lmax : 16 * (W + H);
        r.path.assign((size_t)Q * r.Lmax, -1); r.head.assign((size_t)Q * r.Lmax, 0);
        r.len.assign(Q, 0); r.cost.assign(Q, -1); r.status.assign(Q, SC_Q_NO_PATH);
        if (Q == 0) return r;
        if (F == 0) { r.status.assign(Q, SC_Q_BAD_ENDPOINT); return r; }
        ctx.check(sc_car_paths_batch_host(ctx.get(), d2.data(), fr.hmask.empty() ? nullptr : fr.hmask.data(), fr.amask.data(), 1, nullptr, W, H,
                                          fr.r2, fr.car.arc_n, fr.car.arc_cost, fr.car.rev_cost, fr.toward ? 1 : 0, fr.gp.data(),
                                          fr.roots.data(), fr.rhead.data(), F, qfield.data(), targets.data(), thead.data(), Q, r.Lmax,
                                          to_root ? 1 : 0, r.path.data(), r.head.data(), r.len.data(), r.cost.data(), r.status.data()),
                  "sc_car_paths_batch_host");
        return r;
    }
    // Multi-source cost fields (sc_cost_field_multi_batch): field f starts from seeds[seed_off[f] .. seed_off[f+1]-1], each
    // with the start cost seed_cost[s] (empty: all 0); g[f] = the cost to the cheapest of them, owner[f] = for every cell the
    // index into seeds of the seed its path ends at (-1 where g is SC_FIELD_INF).  pen ([H][W], empty: unweighted) and
    // pen_cap: the costmap of the weighted fields.  The result remembers what field_paths_multi needs.
    struct multi_field_result {
        std::vector<int32_t> g, owner, status, seeds, seed_off, seed_cost;  // g and owner are [F][H][W]
        int32_t r2 = 0;
        std::vector<uint8_t> pen;
        int pen_cap = 0;
    };
    multi_field_result cost_fields_multi(const std::vector<int32_t>& seeds, const std::vector<int32_t>& seed_off,
                                         const std::vector<int32_t>& seed_cost = {}, int32_t r2_clear = 0, int rounds = -1,
                                         const std::vector<uint8_t>& pen = {}, int pen_cap = 255, gpu_context& ctx = default_context()) {
        if (d2.size() != occ.size()) edt(ctx);
        if (seed_off.empty()) throw std::invalid_argument("occupancy_grid::cost_fields_multi: seed_off needs one entry per field and one more");
        if (!seed_cost.empty() && seed_cost.size() != seeds.size())
            throw std::invalid_argument("occupancy_grid::cost_fields_multi: seeds and seed_cost differ in size");
        if (!pen.empty() && pen.size() != occ.size()) throw std::invalid_argument("occupancy_grid::cost_fields_multi: pen is not [H][W]");
        multi_field_result r;
        const int F = (int)seed_off.size() - 1;
        r.seeds = seeds; r.seed_off = seed_off; r.seed_cost = seed_cost;
        r.r2 = r2_clear;
        r.pen = pen;
        r.pen_cap = pen.empty() ? 0 : pen_cap;
        r.g.assign((size_t)F * W * H, SC_FIELD_INF); r.owner.assign((size_t)F * W * H, -1); r.status.assign(F, SC_Q_BAD_ENDPOINT);
        if (F == 0) return r;
        ctx.check(sc_cost_field_multi_batch_host(ctx.get(), d2.data(), pen.empty() ? nullptr : pen.data(), r.pen_cap, 1, nullptr, W, H, r2_clear,
                                                 seeds.data(), seed_cost.empty() ? nullptr : seed_cost.data(), seed_off.data(),
                                                 (int)seeds.size(), F, rounds, r.g.data(), r.owner.data(), r.status.data()),
                  "sc_cost_field_multi_batch_host");
        return r;
    }
    // Paths read from multi-source fields (sc_field_paths_multi_batch): query q walks field qfield[q] from targets[q] to the
    // seed that owns it; which[q] = that seed's index into seeds, -1 without a path.  to_seed = false writes seed..target,
    // true target..seed.  Unweighted, path, len and cost - seed_cost[which] equal astar_batch(seeds[which], target).
    struct multi_batch_result : batch_result {
        std::vector<int32_t> which;
    };
    multi_batch_result field_paths_multi(const multi_field_result& fr, const std::vector<int32_t>& qfield, const std::vector<int32_t>& targets,
                                         int Lmax = 0, bool to_seed = false, gpu_context& ctx = default_context()) {
        if (d2.size() != occ.size()) edt(ctx);
        multi_batch_result r;
        const int Q = (int)targets.size(), F = (int)fr.status.size();
        if (qfield.size() != targets.size()) throw std::invalid_argument("occupancy_grid::field_paths_multi: qfield and targets differ in size");
        r.Lmax = Lmax > 0 ? Lmax : 4 * (W + H);
        r.path.assign((size_t)Q * r.Lmax, -1); r.len.assign(Q, 0); r.cost.assign(Q, -1); r.status.assign(Q, SC_Q_NO_PATH); r.which.assign(Q, -1);
        if (Q == 0) return r;
        if (F == 0) { r.status.assign(Q, SC_Q_BAD_ENDPOINT); return r; }
        ctx.check(sc_field_paths_multi_batch_host(ctx.get(), d2.data(), fr.pen.empty() ? nullptr : fr.pen.data(), fr.pen_cap, 1, nullptr, W, H,
                                                  fr.r2, fr.g.data(), fr.owner.data(), fr.seeds.data(), (int)fr.seeds.size(), F, qfield.data(),
                                                  targets.data(), Q, r.Lmax, to_seed ? 1 : 0, r.path.data(), r.len.data(), r.cost.data(),
                                                  r.status.data(), r.which.data()),
                  "sc_field_paths_multi_batch_host");
        return r;
    }
    struct waypoint_result {
        std::vector<int32_t> wp, n, status;  // wp is [Q][Wmax] cell indices, start..goal; n / status [Q]
        int Wmax = 0;
    };
    // Line-of-sight waypoints of astar_batch's paths (sc_path_waypoints_batch, same r2_clear): every cell path shortened to
    // the cells where it has to turn, each leg a straight segment whose cells (supercover) are all traversable, no interior
    // waypoint collinear with its neighbours.  Wmax = the batch's Lmax, so no path is truncated.
    waypoint_result waypoints_batch(const batch_result& br, int32_t r2_clear = 0, gpu_context& ctx = default_context()) {
        if (d2.size() != occ.size()) edt(ctx);
        waypoint_result r;
        const int Q = (int)br.len.size();
        r.Wmax = br.Lmax;
        r.wp.assign((size_t)Q * r.Wmax, -1); r.n.assign(Q, 0); r.status.assign(Q, SC_Q_NO_PATH);
        if (Q == 0) return r;
        ctx.check(sc_path_waypoints_batch_host(ctx.get(), d2.data(), W, H, r2_clear, br.path.data(), br.len.data(), br.status.data(), Q,
                                               br.Lmax, r.Wmax, r.wp.data(), r.n.data(), r.status.data()),
                  "sc_path_waypoints_batch_host");
        return r;
    }
    // Exploration frontiers (sc_frontier_batch): `known` is [H][W], != 0 where the map has been seen.  A frontier cell is
    // known, has d2 >= max(r2_clear, 1) and touches an unknown cell orthogonally; clusters are 8-connected.  label[c] = the
    // smallest cell of c's cluster (-1 off the frontier), slot[c] = its column among the listed clusters (at least min_size
    // cells, ascending by representative, at most Cmax) or -1; rep / csize / cbox {x0, y0, x1, y1} / csum {sum x, sum y} per
    // column; listed and total count the clusters, listed in full even beyond Cmax.
    struct frontier_result {
        std::vector<int32_t> label, slot, rep, csize, cbox;
        std::vector<int64_t> csum;
        int32_t listed = 0, total = 0;
        int Cmax = 0;
    };
    frontier_result frontiers(const std::vector<uint8_t>& known, int32_t r2_clear = 0, int min_size = 1, int Cmax = 128,
                              gpu_context& ctx = default_context()) {
        if (known.size() != occ.size()) throw std::invalid_argument("occupancy_grid::frontiers: known is not [H][W]");
        if (d2.size() != occ.size()) edt(ctx);
        frontier_result r;
        r.Cmax = Cmax;
        r.label.assign(occ.size(), -1); r.slot.assign(occ.size(), -1);
        r.rep.assign((size_t)std::max(Cmax, 0), -1); r.csize.assign(r.rep.size(), 0); r.cbox.assign(4 * r.rep.size(), 0); r.csum.assign(2 * r.rep.size(), 0);
        if (occ.empty()) return r;
        int32_t ncl[2] = {0, 0};
        ctx.check(sc_frontier_batch_host(ctx.get(), d2.data(), known.data(), 1, W, H, r2_clear, min_size, Cmax, r.label.data(), r.slot.data(), ncl,
                                         r.rep.data(), r.csize.data(), r.cbox.data(), r.csum.data()), "sc_frontier_batch_host");
        r.listed = ncl[0]; r.total = ncl[1];
        return r;
    }
    // A frontier goal per robot (sc_d2_known_i32, sc_cost_field_batch, sc_fleet_explore_batch): the robots stand on the cells
    // `robots`; their cost fields run through known free space only; cost / cell [R][Cmax] is the robots x clusters matrix
    // (cost = the cheapest cell of the cluster + gain * (size_cap - min(size, size_cap)), SC_FIELD_INF when out of reach), an
    // optimal matching gives every robot a cluster of its own: goal[r] = the cell to drive to, -1 without one, gcost[r] its
    // cost-to-come, col_of[r] the cluster's column.  1 <= robots, Cmax <= SC_ASSIGN_MAX_DIM.
    struct explore_result {
        std::vector<int32_t> goal, gcost, col_of, cost, cell;
        frontier_result fr;
    };
    explore_result explore_goals(const std::vector<uint8_t>& known, const std::vector<int32_t>& robots, int32_t r2_clear = 0, int min_size = 1,
                                 int Cmax = 128, int32_t gain = 0, int32_t size_cap = 0, gpu_context& ctx = default_context()) {
        if (known.size() != occ.size()) throw std::invalid_argument("occupancy_grid::explore_goals: known is not [H][W]");
        if (d2.size() != occ.size()) edt(ctx);
        const int R = (int)robots.size();
        explore_result r;
        frontier_result& f = r.fr;
        f.Cmax = Cmax;
        const size_t C = (size_t)std::max(Cmax, 0);
        f.label.assign(occ.size(), -1); f.slot.assign(occ.size(), -1);
        f.rep.assign(C, -1); f.csize.assign(C, 0); f.cbox.assign(4 * C, 0); f.csum.assign(2 * C, 0);
        r.goal.assign(R, -1); r.gcost.assign(R, -1); r.col_of.assign(R, -1);
        r.cost.assign((size_t)R * C, SC_FIELD_INF); r.cell.assign((size_t)R * C, -1);
        if (R == 0 || occ.empty()) return r;
        std::vector<int32_t> d2k(occ.size()), g((size_t)R * occ.size()), fstatus(R);
        ctx.check(sc_d2_known_i32_host(ctx.get(), d2.data(), known.data(), 1, W, H, d2k.data()), "sc_d2_known_i32_host");
        ctx.check(sc_cost_field_batch_host(ctx.get(), d2k.data(), 1, nullptr, W, H, r2_clear, robots.data(), R, -1, g.data(), fstatus.data()),
                  "sc_cost_field_batch_host");
        int32_t ncl[2] = {0, 0};
        int64_t info[4] = {0, 0, 0, 0};
        ctx.check(sc_fleet_explore_batch_host(ctx.get(), d2k.data(), known.data(), W, H, r2_clear, min_size, Cmax, g.data(), R, gain, size_cap,
                                              f.label.data(), f.slot.data(), ncl, f.rep.data(), f.csize.data(), f.cbox.data(), f.csum.data(),
                                              r.cost.data(), r.cell.data(), r.col_of.data(), nullptr, info, r.goal.data(), r.gcost.data()),
                  "sc_fleet_explore_batch_host");
        f.listed = ncl[0]; f.total = ncl[1];
        return r;
    }
    // A central cell per listed cluster (sc_frontier_centres): the cluster's cell nearest its centroid in the 1-norm (ties to
    // the smallest cell), -1 for the rows beyond the listed clusters; [Cmax].  Unlike explore_goals' cell it does not depend on
    // a robot, so it can stand for the cluster as a candidate pose.
    std::vector<int32_t> frontier_centres(const frontier_result& fr, gpu_context& ctx = default_context()) const {
        if (fr.slot.size() != occ.size() || fr.csize.size() != (size_t)std::max(fr.Cmax, 0) || fr.csum.size() != 2 * fr.csize.size())
            throw std::invalid_argument("occupancy_grid::frontier_centres: fr is not this grid's frontier_result");
        std::vector<int32_t> centre(fr.csize.size(), -1);
        if (occ.empty() || centre.empty()) return centre;
        ctx.check(sc_frontier_centres_host(ctx.get(), fr.slot.data(), fr.csize.data(), fr.csum.data(), 1, W, H, fr.Cmax, centre.data()),
                  "sc_frontier_centres_host");
        return centre;
    }
    // Goals by what each view reveals (sc_d2_known_i32, sc_cost_field_batch, sc_fleet_explore_gain_batch): this grid's occ is
    // the observed map (unknown cells 0).  The candidates are the clusters' centres; the pair (robot, centre) of largest
    // wg * gain - wc * travel cost is picked, its view (r2_sense: the sensing radius squared in cells; with dirs and span < B the
    // sector of the heading of largest gain) is applied to a copy of known, every other centre's gain falls by what it
    // revealed, and so on, one pick per robot at most.  goal[r] the cell to drive to (-1: none), head[r] the bin of dirs the
    // sensor should start at there (-1 for the full circle), ggain[r] the free cells the pick was predicted to reveal,
    // known_out the predicted known map, g [R][H][W] the robots' fields the travel costs came from.
    // 1 <= robots <= SC_ASSIGN_MAX_DIM, 1 <= Cmax <= SC_FRONTIER_MAX_CLUSTERS.
    struct gain_result {
        std::vector<int32_t> goal, gcost, ggain, head, cand_of, pick, centre, gain0, gain_end, g;
        int32_t npick = 0;
        std::vector<uint8_t> known_out;
        frontier_result fr;
    };
    gain_result explore_goals_by_gain(const std::vector<uint8_t>& known, const std::vector<int32_t>& robots, int32_t r2_sense,
                                      const heading_table& dirs = {}, int span = 0, int32_t wg = 1, int32_t wc = 1, int32_t min_gain = 1,
                                      int32_t r2_clear = 0, int min_size = 1, int Cmax = 128, gpu_context& ctx = default_context()) {
        if (known.size() != occ.size()) throw std::invalid_argument("occupancy_grid::explore_goals_by_gain: known is not [H][W]");
        if (d2.size() != occ.size()) edt(ctx);
        const int R = (int)robots.size();
        gain_result r;
        frontier_result& f = r.fr;
        f.Cmax = Cmax;
        const size_t C = (size_t)std::max(Cmax, 0);
        f.label.assign(occ.size(), -1); f.slot.assign(occ.size(), -1);
        f.rep.assign(C, -1); f.csize.assign(C, 0); f.cbox.assign(4 * C, 0); f.csum.assign(2 * C, 0);
        r.centre.assign(C, -1); r.gain0.assign(C, 0); r.gain_end.assign(C, 0);
        r.goal.assign(R, -1); r.gcost.assign(R, -1); r.ggain.assign(R, 0); r.head.assign(R, -1); r.cand_of.assign(R, -1); r.pick.assign(R, -1);
        r.known_out = known;
        if (R == 0 || occ.empty()) return r;
        std::vector<int32_t> d2k(occ.size()), fstatus(R);
        r.g.assign((size_t)R * occ.size(), SC_FIELD_INF);
        ctx.check(sc_d2_known_i32_host(ctx.get(), d2.data(), known.data(), 1, W, H, d2k.data()), "sc_d2_known_i32_host");
        ctx.check(sc_cost_field_batch_host(ctx.get(), d2k.data(), 1, nullptr, W, H, r2_clear, robots.data(), R, -1, r.g.data(), fstatus.data()),
                  "sc_cost_field_batch_host");
        int32_t ncl[2] = {0, 0};
        ctx.check(sc_fleet_explore_gain_batch_host(ctx.get(), d2k.data(), known.data(), W, H, r2_clear, min_size, Cmax, occ.data(), r.g.data(), R,
                                                   r2_sense, dirs.empty() ? nullptr : dirs[0].data(), (int)dirs.size(), span, wg, wc, min_gain,
                                                   std::min(R, SC_ASSIGN_MAX_DIM), f.label.data(), f.slot.data(), ncl, f.rep.data(),
                                                   f.csize.data(), f.cbox.data(), f.csum.data(), r.centre.data(), r.goal.data(), r.gcost.data(),
                                                   r.ggain.data(), r.head.data(), r.cand_of.data(), r.pick.data(), &r.npick, r.gain0.data(),
                                                   r.gain_end.data(), r.known_out.data()),
                  "sc_fleet_explore_gain_batch_host");
        f.listed = ncl[0]; f.total = ncl[1];
        return r;
    }
    // Line-of-sight sensing (sc_known_from_views): `views` are (cx, cy, r2) in cells, one std::array<int32_t, 3> each -- the
    // rows of the C call; this grid's occ is the map the sensor meets.  A free cell is seen when it lies in a view's disc and
    // every cell the segment from the view's centre touches is free; an occupied cell is known when it borders a seen free
    // cell.  known = base (empty: nothing known before) | seen | surface; occ_seen = occ where known, 0 elsewhere: the map the
    // robot has observed.  A view with r2 < 0, off the grid or on an occupied cell sees nothing.
    struct view_result {
        std::vector<uint8_t> known, occ_seen;
    };
    view_result known_from_views(const std::vector<std::array<int32_t, 3>>& views, const std::vector<uint8_t>& base = {},
                                 gpu_context& ctx = default_context()) const {
        if (!base.empty() && base.size() != occ.size()) throw std::invalid_argument("occupancy_grid::known_from_views: base is not [H][W]");
        view_result r;
        r.known.assign(occ.size(), 0); r.occ_seen.assign(occ.size(), 0);
        if (occ.empty()) return r;
        ctx.check(sc_known_from_views_host(ctx.get(), base.empty() ? nullptr : base.data(), occ.data(), views.empty() ? nullptr : views[0].data(),
                                           (int)views.size(), W, H, r.known.data(), r.occ_seen.data()), "sc_known_from_views_host");
        return r;
    }
    // The unknown cells every candidate pose would see (sc_view_gain_batch): gain[i] = the cells with known == 0 that view i
    // alone sees on this grid's occ.  With occ the observed map (occ_seen) it predicts what driving to pose i would reveal.
    std::vector<int32_t> view_gain(const std::vector<uint8_t>& known, const std::vector<std::array<int32_t, 3>>& views,
                                   gpu_context& ctx = default_context()) const {
        if (known.size() != occ.size()) throw std::invalid_argument("occupancy_grid::view_gain: known is not [H][W]");
        std::vector<int32_t> gain(views.size(), 0);
        if (views.empty() || occ.empty()) return gain;
        ctx.check(sc_view_gain_batch_host(ctx.get(), occ.data(), known.data(), views[0].data(), (int)views.size(), W, H, gain.data()),
                  "sc_view_gain_batch_host");
        return gain;
    }
    // Sensors with a field of view (sc_known_from_sectors): known_from_views for rows (cx, cy, r2, ax, ay, bx, by); a row sees
    // what its view sees inside the sector counter-clockwise from direction a (inclusive) to b (exclusive); a = b = 0 is the
    // full circle (sector_view builds rows from a heading table).
    view_result known_from_sectors(const std::vector<std::array<int32_t, 7>>& sviews, const std::vector<uint8_t>& base = {},
                                   gpu_context& ctx = default_context()) const {
        if (!base.empty() && base.size() != occ.size()) throw std::invalid_argument("occupancy_grid::known_from_sectors: base is not [H][W]");
        view_result r;
        r.known.assign(occ.size(), 0); r.occ_seen.assign(occ.size(), 0);
        if (occ.empty()) return r;
        ctx.check(sc_known_from_sectors_host(ctx.get(), base.empty() ? nullptr : base.data(), occ.data(),
                                             sviews.empty() ? nullptr : sviews[0].data(), (int)sviews.size(), W, H, r.known.data(),
                                             r.occ_seen.data()), "sc_known_from_sectors_host");
        return r;
    }
    // The unknown cells every sector pose would see (sc_sector_gain_batch).
    std::vector<int32_t> sector_gain(const std::vector<uint8_t>& known, const std::vector<std::array<int32_t, 7>>& sviews,
                                     gpu_context& ctx = default_context()) const {
        if (known.size() != occ.size()) throw std::invalid_argument("occupancy_grid::sector_gain: known is not [H][W]");
        std::vector<int32_t> gain(sviews.size(), 0);
        if (sviews.empty() || occ.empty()) return gain;
        ctx.check(sc_sector_gain_batch_host(ctx.get(), occ.data(), known.data(), sviews[0].data(), (int)sviews.size(), W, H, gain.data()),
                  "sc_sector_gain_batch_host");
        return gain;
    }
    // The gain of every heading of every candidate pose, from one pass of rays (sc_view_gain_headings_batch): hist [N][B] the
    // unknown cells pose i sees in bin b of the table, gainh [N][B] what a sensor of `span` bins sees at heading h, best [N]
    // = (the largest of them, the smallest heading that attains it).
    struct heading_result {
        int B = 0;
        std::vector<std::array<int32_t, 2>> best;
        std::vector<int32_t> hist, gainh;
    };
    heading_result view_gain_headings(const std::vector<uint8_t>& known, const std::vector<std::array<int32_t, 3>>& views,
                                      const heading_table& dirs, int span, gpu_context& ctx = default_context()) const {
        if (known.size() != occ.size()) throw std::invalid_argument("occupancy_grid::view_gain_headings: known is not [H][W]");
        heading_result r;
        r.B = (int)dirs.size();
        r.best.assign(views.size(), {0, 0});
        r.hist.assign(views.size() * dirs.size(), 0);
        r.gainh.assign(views.size() * dirs.size(), 0);
        if (views.empty() || occ.empty()) return r;
        ctx.check(sc_view_gain_headings_batch_host(ctx.get(), occ.data(), known.data(), views[0].data(), (int)views.size(), W, H,
                                                   dirs.empty() ? nullptr : dirs[0].data(), r.B, span, r.hist.data(), r.gainh.data(),
                                                   r.best[0].data()), "sc_view_gain_headings_batch_host");
        return r;
    }
    // The simulated range sensor (sc_scan_cast_batch): `rays` are (ax, ay, bx, by) in cells, one std::array<int32_t, 4> each;
    // this grid's occ is the true map.  hit[k] = the first occupied cell the beam from a towards b meets, SC_SCAN_NO_RETURN
    // when there is none before b or the edge of the grid (b may lie outside it), SC_SCAN_IGNORED for a beam whose origin lies
    // off the grid or on an occupied cell or whose reach exceeds SC_SCAN_MAX_REACH.  logodds_grid::update takes rays and hit.
    std::vector<int32_t> scan_cast(const std::vector<std::array<int32_t, 4>>& rays, gpu_context& ctx = default_context()) const {
        std::vector<int32_t> hit(rays.size(), SC_SCAN_IGNORED);
        if (rays.empty() || occ.empty()) return hit;
        ctx.check(sc_scan_cast_batch_host(ctx.get(), occ.data(), rays[0].data(), (int)rays.size(), W, H, hit.data()), "sc_scan_cast_batch_host");
        return hit;
    }
    // Where was the sensor (sc_scan_match_batch)?  `pts` holds [S][p.rotations][N] points, S = centres.size() scans with
    // their candidate rotations (points_from_hits, rotate_points), `centres` the prior sensor cell of each scan; this grid's
    // d2 (of occ, normally an estimate: computed if it is not there) is the likelihood field, `known` (empty: every cell)
    // says which cells may be scored.  Returns per scan (r, dx, dy, score, n_points, n_ties): the best rotation and shift of
    // the prior, and how many poses of the window score as well (1: unique).  Throws for a centre further than
    // SC_SCAN_MAX_REACH outside the largest grid.  `score` (optional) receives the volume [S][R][2 wy + 1][2 wx + 1].
    std::vector<std::array<int32_t, 6>> scan_match(const scan_points& pts, const std::vector<std::array<int32_t, 2>>& centres,
                                                   const match_params& p = {}, gpu_context& ctx = default_context(),
                                                   const std::vector<uint8_t>& known = {}, std::vector<int32_t>* score = nullptr) {
        const size_t S = centres.size(), per_scan = S ? pts.size() / S : 0;
        if (p.rotations < 1 || (S && (pts.size() % S || per_scan % (size_t)p.rotations || per_scan == 0)))
            throw std::invalid_argument("occupancy_grid::scan_match: pts is not [S][rotations][N]");
        if (!known.empty() && known.size() != occ.size()) throw std::invalid_argument("occupancy_grid::scan_match: known is not [H][W]");
        std::vector<std::array<int32_t, 6>> best(S, std::array<int32_t, 6>{SC_MATCH_IGNORED, 0, 0, 0, 0, 0});
        if (score) score->assign(S * (size_t)p.rotations * (2 * p.wy + 1) * (2 * p.wx + 1), 0);
        if (S == 0 || occ.empty()) return best;
        if (d2.size() != occ.size()) edt(ctx);
        ctx.check(sc_scan_match_batch_host(ctx.get(), d2.data(), known.empty() ? nullptr : known.data(), pts[0].data(), centres[0].data(), (int)S,
                                           p.rotations, (int)(per_scan / (size_t)p.rotations), W, H, p.wx, p.wy, p.d2_cap, p.unk, best[0].data(),
                                           score ? score->data() : nullptr), "sc_scan_match_batch_host");
        return best;
    }
    // The same question over a wide window (sc_scan_match_wide_batch): the arguments and the result of scan_match, found by
    // an exact pruned search, so a row equals what the dense volume would give, ties included; a scan that needed more than
    // p.max_nodes nodes at a level reads (SC_MATCH_OVERFLOW, 0, 0, 0, 0, 0).  `stats` (optional) receives per scan
    // (n_0 .. n_5, n_dive, U): the nodes bounded per level, the children bounded in dives and the last upper bound.
    std::vector<std::array<int32_t, 6>> scan_match_wide(const scan_points& pts, const std::vector<std::array<int32_t, 2>>& centres,
                                                        const wide_match_params& p = {}, gpu_context& ctx = default_context(),
                                                        const std::vector<uint8_t>& known = {},
                                                        std::vector<std::array<int32_t, 8>>* stats = nullptr) {
        const size_t S = centres.size(), per_scan = S ? pts.size() / S : 0;
        if (p.rotations < 1 || (S && (pts.size() % S || per_scan % (size_t)p.rotations || per_scan == 0)))
            throw std::invalid_argument("occupancy_grid::scan_match_wide: pts is not [S][rotations][N]");
        if (!known.empty() && known.size() != occ.size()) throw std::invalid_argument("occupancy_grid::scan_match_wide: known is not [H][W]");
        std::vector<std::array<int32_t, 6>> best(S, std::array<int32_t, 6>{SC_MATCH_IGNORED, 0, 0, 0, 0, 0});
        if (stats) stats->assign(S, std::array<int32_t, 8>{0, 0, 0, 0, 0, 0, 0, 0});
        if (S == 0 || occ.empty()) return best;
        if (d2.size() != occ.size()) edt(ctx);
        ctx.check(sc_scan_match_wide_batch_host(ctx.get(), d2.data(), known.empty() ? nullptr : known.data(), pts[0].data(), centres[0].data(),
                                                (int)S, p.rotations, (int)(per_scan / (size_t)p.rotations), W, H, p.wx, p.wy, p.d2_cap, p.unk,
                                                p.top, p.max_nodes, best[0].data(), stats ? (*stats)[0].data() : nullptr),
                  "sc_scan_match_wide_batch_host");
        return best;
    }
private:
    // both cost_fields overloads; pen NULL: the unweighted fields
    field_result cost_fields_with(const std::vector<int32_t>& roots, const std::vector<uint8_t>* pen, int pen_cap, int32_t r2_clear, int rounds,
                                  gpu_context& ctx) {
        if (d2.size() != occ.size()) edt(ctx);
        if (pen && pen->size() != occ.size()) throw std::invalid_argument("occupancy_grid::cost_fields: pen is not [H][W]");
        field_result r;
        const int F = (int)roots.size();
        r.roots = roots;
        r.r2 = r2_clear;
        r.rounds = rounds;
        if (pen) { r.pen = *pen; r.pen_cap = pen_cap; }
        r.g.assign((size_t)F * W * H, SC_FIELD_INF); r.status.assign(F, SC_Q_BAD_ENDPOINT);
        if (F == 0) return r;
        auto call = [&](auto entry, auto... costmap) {
            return entry(ctx.get(), d2.data(), costmap..., 1, nullptr, W, H, r2_clear, roots.data(), F, rounds, r.g.data(), r.status.data());
        };
        if (!pen) ctx.check(call(sc_cost_field_batch_host), "sc_cost_field_batch_host");
        else ctx.check(call(sc_cost_field_weighted_batch_host, pen->data(), pen_cap), "sc_cost_field_weighted_batch_host");
        return r;
    }
};

// ---- occupancy from range scans (new; the reference has no counterpart) -----------------------------
// The increments, the clamp and the two thresholds of logodds_grid (sc_logodds_update).  The defaults let one look decide a
// cell (l_hit >= t_occ, l_miss >= t_free: the estimate never contradicts a static true map) and make the clamp four hits or
// eight misses deep, so a cell that changed is taken back after a few scans.
struct logodds_params {
    int32_t l_hit = 2, l_miss = 1, l_clamp = 8, t_occ = 2, t_free = 1;
};

// A log-odds occupancy map that accumulates beams: every cell some beam of a call hits gains l_hit, every other cell some beam
// passes loses l_miss (once per call however many beams cross it), clamped to +-l_clamp.  occ_est = L >= t_occ and known =
// occ_est or L <= -t_free are the (occ_seen, known) pair occupancy_grid::explore_goals and the planners take.
class logodds_grid {
public:
    int W = 0, H = 0;
    std::vector<int32_t> L;

    struct masks_result {
        std::vector<uint8_t> occ_est, known;
    };

    logodds_grid() = default;
    logodds_grid(int cells_x, int cells_y) : W(cells_x), H(cells_y), L((size_t)cells_x * cells_y, 0) {}

    // one scan: `rays` as occupancy_grid::scan_cast takes them, hit[k] what it returned -- or, for recorded data, the cell of
    // the beam's end (with b that cell) and SC_SCAN_NO_RETURN for a beam that returned nothing (with b at maximum range)
    masks_result update(const std::vector<std::array<int32_t, 4>>& rays, const std::vector<int32_t>& hit, const logodds_params& p = {},
                        gpu_context& ctx = default_context()) {
        if (hit.size() != rays.size()) throw std::invalid_argument("logodds_grid::update: one hit per ray");
        masks_result r;
        r.occ_est.assign(L.size(), 0); r.known.assign(L.size(), 0);
        if (L.empty()) return r;
        ctx.check(sc_logodds_update_host(ctx.get(), L.data(), rays.empty() ? nullptr : rays[0].data(), rays.empty() ? nullptr : hit.data(),
                                         (int)rays.size(), W, H, p.l_hit, p.l_miss, p.l_clamp, p.t_occ, p.t_free, L.data(), r.occ_est.data(),
                                         r.known.data()), "sc_logodds_update_host");
        return r;
    }
    // the masks of the stored map (the call with no beams; it also clamps L to p.l_clamp)
    masks_result masks(const logodds_params& p = {}, gpu_context& ctx = default_context()) { return update({}, {}, p, ctx); }
    // The pose of one scan against the map so far: masks -> the EDT of occ_est -> occupancy_grid::scan_match with known, three
    // calls on the context's stream.  `pts` holds [m.rotations][N] points, `centre` the prior sensor cell.  Returns the best row
    // (r, dx, dy, score, n_points, n_ties); like masks() it clamps L to p.l_clamp.
    std::array<int32_t, 6> match(const scan_points& pts, const std::array<int32_t, 2>& centre, const match_params& m = {},
                                 const logodds_params& p = {}, gpu_context& ctx = default_context()) {
        masks_result k = masks(p, ctx);
        occupancy_grid est;
        est.W = W; est.H = H;
        est.occ = std::move(k.occ_est);
        return est.scan_match(pts, {centre}, m, ctx, k.known)[0];
    }
    // The same chain with the wide-window search at its end: where is a robot that has lost its pose, or that comes back to
    // a mapped place after a long loop?  masks -> the EDT of occ_est -> occupancy_grid::scan_match_wide with known.
    std::array<int32_t, 6> relocalise(const scan_points& pts, const std::array<int32_t, 2>& centre, const wide_match_params& m = {},
                                      const logodds_params& p = {}, gpu_context& ctx = default_context()) {
        masks_result k = masks(p, ctx);
        occupancy_grid est;
        est.W = W; est.H = H;
        est.occ = std::move(k.occ_est);
        return est.scan_match_wide(pts, {centre}, m, ctx, k.known)[0];
    }
};

// The 8 r rays from cell (cx, cy) to every cell on the perimeter of the square of half-side r around it, going round once: a
// full scan without trigonometry.  On a free grid they pass exactly the cells of that square.
inline std::vector<std::array<int32_t, 4>> square_fan(int32_t cx, int32_t cy, int r) {
    std::vector<std::array<int32_t, 4>> rays;
    for (int t = -r; t < r; ++t) rays.push_back({cx, cy, cx + t, cy - r});
    for (int t = -r; t < r; ++t) rays.push_back({cx, cy, cx + r, cy + t});
    for (int t = -r; t < r; ++t) rays.push_back({cx, cy, cx - t, cy + r});
    for (int t = -r; t < r; ++t) rays.push_back({cx, cy, cx - r, cy - t});
    return rays;
}

// A range scan in world coordinates -> what logodds_grid::update takes.  Beam k leaves `origin` at angle bearings[k] (radians,
// from +x towards +y) and returned ranges[k]; a range that is not finite, negative, or >= max_range is no return.  A cell
// is floor((p - min) / resolution) per axis, NOT clamped: an end may lie outside the grid, and the beam then counts up to the
// edge.  A return outside the grid marks no cell.  Float arithmetic on the host: no bit-exactness is claimed for oblique beams.
struct scan_beams {
    std::vector<std::array<int32_t, 4>> rays;
    std::vector<int32_t> hit;
};
inline scan_beams beams_from_ranges(const occupancy_grid& g, const Vector2f& origin, const std::vector<float>& bearings,
                                    const std::vector<float>& ranges, float max_range) {
    if (bearings.size() != ranges.size()) throw std::invalid_argument("beams_from_ranges: one range per bearing");
    const float ry = (g.bound_rect.y_max - g.bound_rect.y_min) / (float)g.H;
    // a cell coordinate, floored; a point so far out that the beam would be ignored anyway is held at that distance, so the
    // conversion to int32 is always defined (NaN becomes the far end too)
    constexpr float far = (float)(SC_MAX_DIM + SC_SCAN_MAX_REACH + 1);
    auto cell = [&](float v) { const float c = std::floor(v); return (int32_t)(c >= -far && c <= far ? c : (c < 0.0f ? -far : far)); };
    auto cx = [&](float x) { return cell((x - g.bound_rect.x_min) / g.resolution); };
    auto cy = [&](float y) { return cell((y - g.bound_rect.y_min) / ry); };
    scan_beams b;
    for (size_t k = 0; k < bearings.size(); ++k) {
        const bool ret = std::isfinite(ranges[k]) && ranges[k] >= 0.0f && ranges[k] < max_range;
        const float d = ret ? ranges[k] : max_range;
        const int32_t ex = cx(origin.x() + d * std::cos(bearings[k])), ey = cy(origin.y() + d * std::sin(bearings[k]));
        b.rays.push_back({cx(origin.x()), cy(origin.y()), ex, ey});
        b.hit.push_back(ret && ex >= 0 && ey >= 0 && ex < g.W && ey < g.H ? ey * g.W + ex : SC_SCAN_NO_RETURN);
    }
    return b;
}

// scan_cast's output -> scan_match's points: the hit cell of every beam as a cell offset from its ray's origin (W the grid's
// width).  Integer and exact.  A beam without a return, or an ignored one (hit < 0), becomes SC_MATCH_ABSENT.
inline scan_points points_from_hits(const std::vector<std::array<int32_t, 4>>& rays, const std::vector<int32_t>& hit, int W) {
    if (hit.size() != rays.size()) throw std::invalid_argument("points_from_hits: one hit per ray");
    scan_points pts(hit.size(), {SC_MATCH_ABSENT, SC_MATCH_ABSENT});
    for (size_t k = 0; k < hit.size(); ++k)
        if (hit[k] >= 0) pts[k] = {hit[k] % W - rays[k][0], hit[k] / W - rays[k][1]};
    return pts;
}

// Candidate rotations of a scan: [N] points and R angles (radians, from +x towards +y) -> [R][N] points, every point turned
// about the sensor in double precision and rounded to the nearest cell; absent points stay absent.  No bit-exactness is
// claimed but at multiples of a quarter turn, where the result is the integer rotation (x, y) -> (-y, x) applied that often.
inline scan_points rotate_points(const scan_points& pts, const std::vector<double>& angles) {
    scan_points out;
    out.reserve(pts.size() * angles.size());
    auto absent = [](int32_t v) { return v < -SC_SCAN_MAX_REACH || v > SC_SCAN_MAX_REACH; };
    for (double a : angles) {
        const double c = std::cos(a), s = std::sin(a);
        for (const auto& q : pts) {
            if (absent(q[0]) || absent(q[1])) out.push_back({SC_MATCH_ABSENT, SC_MATCH_ABSENT});
            else out.push_back({(int32_t)std::lrint(q[0] * c - q[1] * s), (int32_t)std::lrint(q[0] * s + q[1] * c)});
        }
    }
    return out;
}

// ---- planning_space (sea_current.hpp:298-319, 1272-1407) --------------------------------------------
// ---- sampling helpers of the reference's planner (sea_current.hpp:90-132, 287-296) ----------------
// State of the incremental Halton generator: the last fraction was f / i.
struct halton_state {
    int f = 0;
    int i = 0;
    halton_state(int f, int i) : f(f), i(i) {}
    halton_state() : f(0), i(0) {}
};

// next n numbers of the base-b Halton sequence (1/b, 2/b, ..., 1/b^2, ...), continuing from `state` (same signature and
// float results as :100-132: integer numerator / denominator, one float division per number)
inline std::vector<float> halton(const int b, const int n, halton_state& state) {
    std::vector<float> nums(n);
    int num = 0, den = 1;
    if (state.i != 0 && state.f != 0) { den = state.i; num = state.f; }
    for (int j = 0; j < n; ++j) {
        const int gap = den - num;
        if (gap == 1) {              // the current power of b is used up: start the next one
            num = 1;
            den *= b;
        } else {
            int y = den / b;
            while (gap <= y) y /= b;
            num = (b + 1) * y - gap;
        }
        nums[j] = static_cast<float>(num) / den;
    }
    state.f = num;
    state.i = den;
    return nums;
}

// hash of a point by the bit patterns of its coordinates (:287-295)
struct hash_vector2f {
    size_t operator()(const Vector2f v) const {
        const float fa = v.x(), fb = v.y();
        int32_t a, b;
        std::memcpy(&a, &fa, 4);
        std::memcpy(&b, &fb, 4);
        return std::hash<int32_t>()(a) ^ std::hash<int32_t>()(b);
    }
};
struct equal_vector2f {
    bool operator()(const Vector2f& a, const Vector2f& b) const { return a.x() == b.x() && a.y() == b.y(); }
};
using point_set = std::unordered_set<Vector2f, hash_vector2f, equal_vector2f>;

class planning_space {
public:
    std::vector<obstacle> obstacles;
    std::vector<std::function<bool(Vector2f)>> free_space_allocations;
    bounding_rect bound_rect;
    halton_state x_state;       // Halton state of sample_free (bases 2 and 3), advanced by every call (:317-318)
    halton_state y_state;
    int grid_cells = 256;       // cells along the longer side of bound_rect (new knob)
    float clearance = 0.0f;     // required obstacle clearance in world units (new knob)
    // (new knobs, off by default) a soft margin for plan_from / plan_to: when both are positive, cells closer to an obstacle
    // than soft_clearance (world units, converted like clearance) cost up to soft_penalty more to enter (tenths of a cell
    // of detour; occupancy_grid::clearance_penalty), so paths keep their distance where there is room and still pass where
    // there is none.  plan_batch and fast_marching_trees (A*) are unchanged: they minimise length only.  simplify_paths
    // shortcuts by visibility under the hard clearance only, so it can straighten a path back towards a wall.
    float soft_clearance = 0.0f;
    int soft_penalty = 0;
    // (new knob) plan_batch / fast_marching_trees return the exact start, the centres of the path's line-of-sight waypoints
    // (occupancy_grid::waypoints_batch) and the exact goal instead of every cell centre: the short, non-collinear list the
    // reference's planner hands to bezier_spline::from_path (examples/test.cpp:284 -> :300).  Limits:
    //   - clearance 0: the guarantee is visibility on the grid only.  Polygon edges are rasterised by sampling, so a long
    //     leg can graze an edge that missed a corner cell.
    //   - clearance >= 1.5 cells (r2 >= 3): a free cell that an edge only grazed borders a marked cell, so its d2 <= 2 and it
    //     is not traversable; legs should then also clear the polygons (cost() < FLT_MAX).  An argument, not a proof; the
    //     tests check it with cost() on their worlds.
    bool simplify_paths = false;

    planning_space(const bounding_rect& br) : bound_rect(br) {}

    std::tuple<bool, obstacle> is_obstacle(const Vector2f& p) {
        for (auto& ob : obstacles)
            if (ob.contains(p)) return {true, ob};
        return {false, obstacle()};
    }
    bool is_free_space_allocated(const Vector2f& p) {
        for (auto& f : free_space_allocations)
            if (f(p)) return true;
        return false;
    }
    bool is_free(const Vector2f& p) { return !std::get<0>(is_obstacle(p)) && is_free_space_allocated(p); }
    // n free points of the bounding rectangle from the Halton sequence, (0,0) included (:1294-1313; no stdout print).
    // The reference never returns when nothing can be free (no free-space allocation); this throws instead.
    point_set sample_free(const int n) {
        if (free_space_allocations.empty() && n > 1)
            throw std::logic_error("planning_space::sample_free: no free-space allocation, no point can be free");
        point_set pts = {Vector2f(0, 0)};
        pts.reserve(n);
        size_t tested = 0;
        while ((size_t)n > pts.size()) {
            const int want = n - (int)pts.size();
            const std::vector<float> xs = halton(2, want, x_state), ys = halton(3, want, y_state);
            for (int i = 0; i < want; ++i) {
                const Vector2f test((bound_rect.x_max - bound_rect.x_min) * xs[i] + bound_rect.x_min,
                                    (bound_rect.y_max - bound_rect.y_min) * ys[i] + bound_rect.y_min);
                if (is_free(test)) pts.insert(test);
            }
            tested += (size_t)want;
            if (tested > 1000 * (size_t)n + 100000 && pts.size() <= 1)
                throw std::runtime_error("planning_space::sample_free: no free point found");
        }
        return pts;
    }
    // points of `nodes` within `dist` of b, b itself excluded.  The reference compares the (unsquared) distance with
    // dist squared (:1331); kept, so that radii mean the same thing in both libraries.
    point_set near(const Vector2f b, const point_set& nodes, const float dist) const {
        point_set out;
        out.reserve(nodes.size());
        for (const auto& a : nodes)
            if (pt_dist(a, b) <= std::pow(dist, 2) && !(a.x() == b.x() && a.y() == b.y())) out.insert(a);
        return out;
    }
    // both points within epsilon of (the supporting lines of) one obstacle's edges (:444-463; the reference tests `a`
    // twice, so does this)
    bool is_same_obstacle_fuzzy(const Vector2f& a, const Vector2f& b, const float epsilon) {
        (void)b;
        for (const auto& ob : obstacles) {
            bool tag = false;
            for (const auto& [p1, p2] : ob.lines) {
                const Vector2f e = p2 - p1;
                const float len = e.norm();
                if (len > 0 && std::fabs((p2.x() - p1.x()) * (p1.y() - a.y()) - (p1.x() - a.x()) * (p2.y() - p1.y())) / len < epsilon) tag = true;
            }
            if (tag) return true;
        }
        return false;
    }
    // length of segment ab, FLT_MAX if it crosses any obstacle edge (:1315-1326)
    float cost(const Vector2f a, const Vector2f b) const {
        for (const auto& ob : obstacles)
            for (const auto& [p, q] : ob.lines)
                if (std::get<0>(intersects(a, b, p, q))) return FLT_MAX;
        return pt_dist(a, b);
    }
    occupancy_grid make_grid() const {
        occupancy_grid g = empty_grid();
        g.rasterize(obstacles);
        return g;
    }
    // the same grid, rasterised on the GPU (occupancy_grid::rasterize(obstacles, ctx))
    occupancy_grid make_grid(gpu_context& ctx) const {
        occupancy_grid g = empty_grid();
        g.rasterize(obstacles, ctx);
        return g;
    }
    occupancy_grid empty_grid() const {
        const float wx = bound_rect.x_max - bound_rect.x_min, wy = bound_rect.y_max - bound_rect.y_min;
        const float res = std::max(wx, wy) / (float)grid_cells;
        return occupancy_grid(bound_rect, std::max(1, (int)std::ceil(wx / res)), std::max(1, (int)std::ceil(wy / res)));
    }
    // The known-space mask of a W x H grid over bound_rect: 1 where a free-space allocation holds the cell's centre.  The
    // allocations are std::functions, so this is evaluated on the host; occupancy_grid::frontiers / explore_goals take it.
    std::vector<uint8_t> known_grid(int W, int H) {
        const occupancy_grid g(bound_rect, W, H);
        std::vector<uint8_t> known((size_t)W * H);
        for (int32_t c = 0; c < W * H; ++c) known[(size_t)c] = is_free_space_allocated(g.centre_of(c)) ? 1 : 0;
        return known;
    }
    // Same role and result type as the reference's FMT* planner: start -> goal waypoint list, nullopt if
    // no path.  `n` and `rn` (sample count, connection radius) are accepted for source compatibility;
    // the grid resolution is `grid_cells`.
    std::optional<std::vector<Vector2f>> fast_marching_trees(const Vector2f& x_init, const Vector2f& x_goal, const int n = 0, const float rn = 0) {
        (void)n; (void)rn;
        auto r = plan_batch({x_init}, {x_goal});
        return r[0];
    }
    // The reference's own algorithm (FMT* over n Halton samples with connection radius rn, :1339-1407) for a batch of
    // queries, on the GPU (sc_fmt_star_batch): one sample set (drawn like the reference does inside the call, advancing
    // x_state / y_state once) shared by all queries.  Needs a free-space allocation, like sample_free.
    std::vector<std::optional<std::vector<Vector2f>>> fast_marching_trees_sampled(const std::vector<Vector2f>& starts,
                                                                                  const std::vector<Vector2f>& goals, const int n,
                                                                                  const float rn, gpu_context& ctx = default_context()) {
        const point_set ps = sample_free(n);
        std::vector<float> smp, lines, st, gl;
        smp.push_back(0.f); smp.push_back(0.f);                     // (0,0) first, as the reference inserts it (:1297)
        for (const auto& p : ps)
            if (!(p.x() == 0.f && p.y() == 0.f)) { smp.push_back(p.x()); smp.push_back(p.y()); }
        for (const auto& ob : obstacles)
            for (const auto& [a, b] : ob.lines) { lines.push_back(a.x()); lines.push_back(a.y()); lines.push_back(b.x()); lines.push_back(b.y()); }
        const int Q = (int)starts.size(), Lmax = (int)smp.size() / 2 + 2;
        for (int q = 0; q < Q; ++q) { st.push_back(starts[q].x()); st.push_back(starts[q].y()); gl.push_back(goals[q].x()); gl.push_back(goals[q].y()); }
        std::vector<float> path((size_t)Q * Lmax * 2), cost(Q);
        std::vector<int32_t> len(Q), status(Q);
        ctx.check(sc_fmt_star_batch_host(ctx.get(), smp.data(), (int)smp.size() / 2, st.data(), gl.data(), Q, rn, lines.empty() ? nullptr : lines.data(),
                                         (int)lines.size() / 4, Lmax, path.data(), len.data(), cost.data(), status.data()),
                  "sc_fmt_star_batch_host");
        std::vector<std::optional<std::vector<Vector2f>>> out(Q);
        for (int q = 0; q < Q; ++q) {
            if (status[q] != SC_Q_OK) continue;
            std::vector<Vector2f> wp;
            for (int i = 0; i < len[q]; ++i) wp.push_back(Vector2f(path[((size_t)q * Lmax + i) * 2], path[((size_t)q * Lmax + i) * 2 + 1]));
            out[q] = std::move(wp);
        }
        return out;
    }
    // batched form: one grid, one EDT, Q queries in one GPU launch.  screen = true labels the grid's components once
    // (occupancy_grid::components) and leaves the queries whose endpoints lie in different components unsearched
    // (astar_batch_screened): the same results, without the cost of expanding a whole component for every hopeless query.
    std::vector<std::optional<std::vector<Vector2f>>> plan_batch(const std::vector<Vector2f>& starts, const std::vector<Vector2f>& goals,
                                                                 gpu_context& ctx = default_context(), bool screen = false) {
        occupancy_grid g = make_grid(ctx);
        g.edt(ctx);
        std::vector<int32_t> s(starts.size()), t(goals.size());
        for (size_t i = 0; i < starts.size(); ++i) { s[i] = g.cell_of(starts[i]); t[i] = g.cell_of(goals[i]); }
        const int32_t r2 = clearance_r2(g);
        auto br = screen ? g.astar_batch_screened(g.components(r2, ctx), s, t, 0, ctx) : g.astar_batch(s, t, r2, 0, ctx);
        return to_points(g, br, r2, starts, goals, "plan_batch", ctx);
    }
    // Is there a path between two world points?  Answered from the component labels, without a search: true iff
    // plan_batch({a}, {b}) finds a path.  r2_clear < 0: the squared clearance in cells that `clearance` gives, as in plan_batch.
    bool reachable(const Vector2f& a, const Vector2f& b, int32_t r2_clear = -1, gpu_context& ctx = default_context()) {
        occupancy_grid g = make_grid(ctx);
        g.edt(ctx);
        const int32_t r2 = r2_clear < 0 ? clearance_r2(g) : r2_clear;
        return g.reachable(g.components(r2, ctx), {g.cell_of(a)}, {g.cell_of(b)}, ctx)[0] == SC_Q_OK;
    }
    // One start, many goals (ranking candidate goals): one cost field rooted at the start's cell instead of one A* search
    // per goal.  Returns exactly plan_batch(std::vector<Vector2f>(goals.size(), start), goals, ctx).
    std::vector<std::optional<std::vector<Vector2f>>> plan_from(const Vector2f& start, const std::vector<Vector2f>& goals,
                                                                gpu_context& ctx = default_context()) {
        occupancy_grid g = make_grid(ctx);
        g.edt(ctx);
        std::vector<int32_t> t(goals.size()), qf(goals.size(), 0);
        for (size_t i = 0; i < goals.size(); ++i) t[i] = g.cell_of(goals[i]);
        const int32_t r2 = clearance_r2(g);
        auto fr = fields_of(g, g.cell_of(start), r2, ctx);
        auto br = g.field_paths(fr, qf, t, 0, false, ctx);
        return to_points(g, br, r2, std::vector<Vector2f>(goals.size(), start), goals, "plan_from", ctx);
    }
    // Many starts, one goal (a fleet heading to one goal): one cost field rooted at the goal's cell.  Entry q runs
    // starts[q]..goal; with simplify_paths off it is plan_batch({goal}, {starts[q]})[0] reversed, with it on the waypoints
    // of that start..goal cell path.
    std::vector<std::optional<std::vector<Vector2f>>> plan_to(const std::vector<Vector2f>& starts, const Vector2f& goal,
                                                              gpu_context& ctx = default_context()) {
        occupancy_grid g = make_grid(ctx);
        g.edt(ctx);
        std::vector<int32_t> s(starts.size()), qf(starts.size(), 0);
        for (size_t i = 0; i < starts.size(); ++i) s[i] = g.cell_of(starts[i]);
        const int32_t r2 = clearance_r2(g);
        auto fr = fields_of(g, g.cell_of(goal), r2, ctx);
        auto br = g.field_paths(fr, qf, s, 0, true, ctx);
        return to_points(g, br, r2, starts, std::vector<Vector2f>(starts.size(), goal), "plan_to", ctx);
    }
    // Many starts with headings, one goal pose, for a body that turns at a price: one toward pose field rooted at the goal pose
    // (occupancy_grid::pose_fields over the mask of `body`).  Per start the poses in driving order, first (start cell,
    // start_heading[q]), last (goal cell, goal_heading); nullopt where there is none (the body does not fit an endpoint, or
    // no route).  Headings are 0 .. 7 counter-clockwise from +x (SC_POSE_HEADINGS); goal_heading -1: any heading that fits,
    // start_heading[q] -1: the cheapest.  turn_cost >= 1 per 45 degrees, rev_cost per reverse move (-1: no reversing), both in
    // the units of the move costs (10 per cell step).  Not smoothed: a cells_only read-out feeds the waypoint chain instead.
    struct pose {
        Vector2f position;   // the cell's centre
        int32_t cell;
        int heading;
    };
    std::vector<std::optional<std::vector<pose>>> plan_to_pose(const std::vector<Vector2f>& starts, const std::vector<int32_t>& start_heading,
                                                               const Vector2f& goal, int goal_heading, int turn_cost, int rev_cost = -1,
                                                               const footprint& body = {}, gpu_context& ctx = default_context()) {
        if (starts.size() != start_heading.size())
            throw std::invalid_argument("planning_space::plan_to_pose: starts and start_heading differ in size");
        occupancy_grid g = make_grid(ctx);
        g.edt(ctx);
        const int32_t r2 = clearance_r2(g);
        const bool disc = body.front == 0 && body.back == 0 && body.left == 0 && body.right == 0;
        auto fr = g.pose_fields({g.cell_of(goal)}, {(int32_t)goal_heading}, turn_cost, rev_cost, true, r2,
                                disc ? std::vector<uint8_t>{} : g.footprint_mask(body, r2, ctx), -1, ctx);
        std::vector<int32_t> s(starts.size()), qf(starts.size(), 0);
        for (size_t i = 0; i < starts.size(); ++i) s[i] = g.cell_of(starts[i]);
        auto pr = g.pose_paths(fr, qf, s, start_heading, 0, true, false, ctx);
        int need = 0;                                       // a truncated read-out reports the count it needs: read again with room
        for (size_t q = 0; q < starts.size(); ++q)
            if (pr.status[q] == SC_Q_TRUNCATED) need = std::max(need, (int)pr.len[q]);
        if (need > 0) pr = g.pose_paths(fr, qf, s, start_heading, need, true, false, ctx);
        std::vector<std::optional<std::vector<pose>>> out(starts.size());
        for (size_t q = 0; q < starts.size(); ++q) {
            if (pr.status[q] != SC_Q_OK) continue;
            std::vector<pose> poses((size_t)pr.len[q]);
            for (int i = 0; i < pr.len[q]; ++i) {
                const int32_t c = pr.path[q * (size_t)pr.Lmax + i];
                poses[(size_t)i] = pose{g.centre_of(c), c, (int)pr.head[q * (size_t)pr.Lmax + i]};
            }
            out[q] = std::move(poses);
        }
        return out;
    }
    // The same for a car-like body: one toward car field rooted at the goal pose (occupancy_grid::car_fields).  The heading
    // changes only along arcs, so a route never pivots; one entry per cell, the cells of an arc included.
    std::vector<std::optional<std::vector<pose>>> plan_to_pose(const std::vector<Vector2f>& starts, const std::vector<int32_t>& start_heading,
                                                               const Vector2f& goal, int goal_heading, const car_model& car,
                                                               const footprint& body = {}, gpu_context& ctx = default_context()) {
        if (starts.size() != start_heading.size())
            throw std::invalid_argument("planning_space::plan_to_pose: starts and start_heading differ in size");
        occupancy_grid g = make_grid(ctx);
        g.edt(ctx);
        const int32_t r2 = clearance_r2(g);
        const bool disc = body.front == 0 && body.back == 0 && body.left == 0 && body.right == 0;
        auto fr = g.car_fields({g.cell_of(goal)}, {(int32_t)goal_heading}, car, true, r2,
                               disc ? std::vector<uint8_t>{} : g.footprint_mask(body, r2, ctx), -1, ctx);
        std::vector<int32_t> s(starts.size()), qf(starts.size(), 0);
        for (size_t i = 0; i < starts.size(); ++i) s[i] = g.cell_of(starts[i]);
        auto pr = g.car_paths(fr, qf, s, start_heading, 0, true, ctx);
        int need = 0;                                       // a truncated read-out reports the count it needs: read again with room
        for (size_t q = 0; q < starts.size(); ++q)
            if (pr.status[q] == SC_Q_TRUNCATED) need = std::max(need, (int)pr.len[q]);
        if (need > 0) pr = g.car_paths(fr, qf, s, start_heading, need, true, ctx);
        std::vector<std::optional<std::vector<pose>>> out(starts.size());
        for (size_t q = 0; q < starts.size(); ++q) {
            if (pr.status[q] != SC_Q_OK) continue;
            std::vector<pose> poses((size_t)pr.len[q]);
            for (int i = 0; i < pr.len[q]; ++i) {
                const int32_t c = pr.path[q * (size_t)pr.Lmax + i];
                poses[(size_t)i] = pose{g.centre_of(c), c, (int)pr.head[q * (size_t)pr.Lmax + i]};
            }
            out[q] = std::move(poses);
        }
        return out;
    }
    // Many starts, many goals (a fleet where every robot goes to the cheapest of K docks): one multi-source field seeded at
    // all goal cells, goal k with the start cost goal_costs[k] (empty: all 0; in the units of the move costs, 10 per cell
    // step) -- weighted when the soft knobs are on, as for plan_to.  Per start: the path start..goal, the index of the chosen
    // goal (-1 without a path) and the cost, goal cost included (-1 without a path).  paths[q] equals
    // plan_to(starts, goals[goal[q]])[q].
    struct nearest_result {
        std::vector<std::optional<std::vector<Vector2f>>> paths;
        std::vector<int32_t> goal, cost;
    };
    nearest_result plan_to_nearest(const std::vector<Vector2f>& starts, const std::vector<Vector2f>& goals,
                                   const std::vector<int32_t>& goal_costs = {}, gpu_context& ctx = default_context()) {
        if (!goal_costs.empty() && goal_costs.size() != goals.size())
            throw std::invalid_argument("planning_space::plan_to_nearest: goals and goal_costs differ in size");
        occupancy_grid g = make_grid(ctx);
        g.edt(ctx);
        std::vector<int32_t> s(starts.size()), qf(starts.size(), 0), seeds(goals.size());
        for (size_t i = 0; i < starts.size(); ++i) s[i] = g.cell_of(starts[i]);
        for (size_t k = 0; k < goals.size(); ++k) seeds[k] = g.cell_of(goals[k]);
        const int32_t r2 = clearance_r2(g);
        occupancy_grid::multi_field_result fr;
        if (soft_clearance > 0.0f && soft_penalty > 0) {
            int32_t r2_soft;
            int pen_max;
            soft_knobs(g, r2_soft, pen_max);
            fr = g.cost_fields_multi(seeds, {0, (int32_t)seeds.size()}, goal_costs, r2, -1, g.clearance_penalty(r2, r2_soft, pen_max, ctx),
                                     pen_max, ctx);
        } else {
            fr = g.cost_fields_multi(seeds, {0, (int32_t)seeds.size()}, goal_costs, r2, -1, {}, 255, ctx);
        }
        auto br = g.field_paths_multi(fr, qf, s, 0, true, ctx);
        std::vector<Vector2f> ends(starts.size(), Vector2f(0, 0));
        for (size_t q = 0; q < starts.size(); ++q)
            if (br.which[q] >= 0) ends[q] = goals[(size_t)br.which[q]];
        nearest_result out;
        out.paths = to_points(g, br, r2, starts, ends, "plan_to_nearest", ctx);
        out.goal = br.which;
        out.cost = br.cost;
        for (size_t q = 0; q < starts.size(); ++q)
            if (!out.paths[q]) { out.goal[q] = -1; out.cost[q] = -1; }
        return out;
    }

    // Many starts, many goals, one goal per start (a fleet and its docks): one cost field per goal -- weighted when the soft
    // knobs are on, exactly as for plan_to -- then the matching that pairs as many starts as possible and, among those, at the
    // smallest sum of costs (sc_fleet_assign_batch_host; goal k priced at goal_costs[k], empty: all 0, in the units of the move
    // costs), then the paths read from the fields.  At most SC_ASSIGN_MAX_DIM starts and goals.  Per start: the path
    // start..goal, the index of its goal and the cost, goal cost included; nullopt, -1 and -1 for a start left without a goal.
    // paths[q] equals plan_to(starts, goals[goal[q]])[q]; matched starts have a goal, and their costs add up to total.
    struct assigned_result {
        std::vector<std::optional<std::vector<Vector2f>>> paths;
        std::vector<int32_t> goal, cost;
        int64_t matched = 0, total = 0;
    };
    assigned_result plan_assigned(const std::vector<Vector2f>& starts, const std::vector<Vector2f>& goals,
                                  const std::vector<int32_t>& goal_costs = {}, gpu_context& ctx = default_context()) {
        if (!goal_costs.empty() && goal_costs.size() != goals.size())
            throw std::invalid_argument("planning_space::plan_assigned: goals and goal_costs differ in size");
        if (starts.size() > SC_ASSIGN_MAX_DIM || goals.size() > SC_ASSIGN_MAX_DIM)
            throw std::invalid_argument("planning_space::plan_assigned: at most SC_ASSIGN_MAX_DIM starts and goals");
        assigned_result out;
        const int R = (int)starts.size(), F = (int)goals.size();
        out.paths.resize(R);
        out.goal.assign(R, -1);
        out.cost.assign(R, -1);
        if (R == 0 || F == 0) return out;
        occupancy_grid g = make_grid(ctx);
        g.edt(ctx);
        std::vector<int32_t> s(R), roots(F);
        for (int i = 0; i < R; ++i) s[i] = g.cell_of(starts[i]);
        for (int k = 0; k < F; ++k) roots[k] = g.cell_of(goals[k]);
        const int32_t r2 = clearance_r2(g);
        auto fr = fields_of(g, roots, r2, ctx);
        std::vector<int32_t> col_of(R, -1);
        int64_t info[4] = {0, 0, 0, 0};
        ctx.check(sc_fleet_assign_batch_host(ctx.get(), fr.g.data(), F, g.W, g.H, s.data(), R, goal_costs.empty() ? nullptr : goal_costs.data(),
                                             nullptr, col_of.data(), nullptr, nullptr, nullptr, info),
                  "sc_fleet_assign_batch_host");
        auto br = g.field_paths(fr, col_of, s, 0, true, ctx);
        std::vector<Vector2f> ends(R, Vector2f(0, 0));
        for (int q = 0; q < R; ++q)
            if (col_of[q] >= 0) ends[q] = goals[(size_t)col_of[q]];
        out.paths = to_points(g, br, r2, starts, ends, "plan_assigned", ctx);
        out.matched = info[0];
        out.total = info[1];
        for (int q = 0; q < R; ++q)
            if (out.paths[q]) {
                out.goal[q] = col_of[q];
                out.cost[q] = br.cost[q] + (goal_costs.empty() ? 0 : goal_costs[(size_t)col_of[q]]);
            }
        return out;
    }

private:
    friend class planner;
    int32_t clearance_r2(const occupancy_grid& g) const {
        const float cc = clearance / g.resolution;
        return (int32_t)std::ceil(cc * cc);
    }
    // the field of plan_from / plan_to: weighted when both soft knobs are positive, else today's
    occupancy_grid::field_result fields_of(occupancy_grid& g, int32_t root, int32_t r2, gpu_context& ctx) const {
        return fields_of(g, std::vector<int32_t>{root}, r2, ctx);
    }
    // the same for several roots (plan_assigned: one field per goal)
    occupancy_grid::field_result fields_of(occupancy_grid& g, const std::vector<int32_t>& roots, int32_t r2, gpu_context& ctx) const {
        if (!(soft_clearance > 0.0f && soft_penalty > 0)) return g.cost_fields(roots, r2, -1, ctx);
        int32_t r2_soft;
        int pen_max;
        soft_knobs(g, r2_soft, pen_max);
        occupancy_grid::field_result fr = g.cost_fields(roots, g.clearance_penalty(r2, r2_soft, pen_max, ctx), pen_max, r2, -1, ctx);
        fr.r2_soft = r2_soft;   // cost_fields_update computes the costmap of a changed grid with the same knobs
        fr.pen_max = pen_max;
        return fr;
    }
    // the costmap parameters the soft knobs stand for
    void soft_knobs(const occupancy_grid& g, int32_t& r2_soft, int& pen_max) const {
        const float sc = soft_clearance / g.resolution;
        r2_soft = std::max((int32_t)std::ceil(sc * sc), (int32_t)1);
        pen_max = std::min(soft_penalty, 255);
    }
    // cell paths (astar_batch's layout) -> the exact endpoints around the centres of the interior cells or waypoints
    std::vector<std::optional<std::vector<Vector2f>>> to_points(occupancy_grid& g, const occupancy_grid::batch_result& br, int32_t r2,
                                                                const std::vector<Vector2f>& starts, const std::vector<Vector2f>& goals,
                                                                const char* who, gpu_context& ctx) const {
        occupancy_grid::waypoint_result wr;
        if (simplify_paths) wr = g.waypoints_batch(br, r2, ctx);
        std::vector<std::optional<std::vector<Vector2f>>> out(starts.size());
        for (size_t q = 0; q < starts.size(); ++q) {
            if (br.status[q] != SC_Q_OK) continue;
            if (simplify_paths && wr.status[q] != SC_Q_OK)
                throw std::runtime_error(std::string("planning_space::") + who + ": waypoints of an A* path: status " +
                                         std::to_string(wr.status[q]));
            const int32_t* cells = simplify_paths ? &wr.wp[(size_t)q * wr.Wmax] : &br.path[(size_t)q * br.Lmax];
            const int n = simplify_paths ? wr.n[q] : br.len[q];
            std::vector<Vector2f> wp;
            wp.reserve(n + 2);
            wp.push_back(starts[q]);
            for (int i = 1; i + 1 < n; ++i) wp.push_back(g.centre_of(cells[i]));
            wp.push_back(goals[q]);
            out[q] = std::move(wp);
        }
        return out;
    }
};

// ---- planner (sea_current.hpp:433-441, 465-519): where to drive next to see more ---------------------
// The reference's members and signature.  Its pick_next_goal_point is unfinished (it traces a circle around the origin with
// a condition marked "TODO: fix", never fills the cache and reads an empty stack when it finds nothing), so there is nothing
// to be equal to; this one does what its comments aim at, on the grid:
//   the disc of search_radius around start is allocated as known space (ps.free_space_allocations, as the reference's
//   comment says: "our local area of known space will be circular"); the obstacles inside the known space are what the robot
//   has observed; the frontier clusters of the grid (occupancy_grid::explore_goals, at most n of them listed, gain 0) are
//   ranked by the cost of the robot's path to their cheapest cell; the cheapest is returned, the other clusters' best cells
//   are pushed onto goal_point_cache, cheapest on top.  Without a reachable frontier the top of the cache is returned and
//   popped; with the cache empty as well it throws std::runtime_error.
// line_of_sight (false: the above, unchanged).  With it set the disc is not allocated; instead the robot senses the true grid
//   (ps.make_grid) along clear rays: seen = occupancy_grid::known_from_views(one view at start's cell, base = seen), with
//   r2 = (int32_t)((search_radius / g.resolution)^2), the squared radius in cells truncated to an integer.  `seen` is the
//   known mask kept between calls ([H][W], sized and zeroed on first use); the grid the frontiers are taken on is occ_seen.
// range_scan (false: the above, unchanged; setting both flags throws std::logic_error).  With it set the disc is not
//   allocated; the robot casts square_fan(start's cell, max(1, (int)(search_radius / g.resolution))) on the true grid
//   (occupancy_grid::scan_cast) and updates `map` with scan_params (logodds_grid::update; sized and zeroed on first use).
//   `seen` is the map's known mask, the grid the frontiers are taken on its occ_est: the robot explores on what its beams
//   have accumulated, not on a mask handed to it.
// fov_span (0: off; every path above runs unchanged and nothing new is allocated).  With fov_span > 0 the sensor covers
//   fov_span bins of heading_dirs(headings); line_of_sight must be set, else std::logic_error.  The robot senses at its cell
//   with the sector of `heading` (-1: the heading of largest predicted gain there on the map observed so far, ties to the
//   smallest; `heading` receives the one used, so set it again before the next call: to goal_heading once the robot stands at
//   the goal, or to -1); if that look adds no known cell it senses the full circle once, a turn on the
//   spot, so a look from a frontier cell always adds one.  After the goal is picked, goal_heading is view_gain_headings' best
//   heading at the goal on the observed map (-1 when the goal came from the cache).
// gain_weight (0: off; every path above runs unchanged and nothing new is allocated).  With gain_weight > 0 the goal is
//   occupancy_grid::explore_goals_by_gain's on the observed map with wg = gain_weight, wc = 1, min_gain = 1 and the sensing
//   radius of line_of_sight, which must be set, else std::logic_error: the cluster centre of largest gain_weight * (the
//   unknown cells a look from there is predicted to reveal) - path cost, not the nearest cluster cell.  With fov_span > 0
//   (< headings here) the gain is that of the best heading and goal_heading is that heading.  The other clusters are not
//   pushed onto goal_point_cache; without an eligible centre the cache's top is returned as above.
class planner {
public:
    planning_space ps;
    std::stack<Vector2f> goal_point_cache;
    int64_t past_id = 0;
    bool line_of_sight = false;
    std::vector<uint8_t> seen;
    bool range_scan = false;
    logodds_grid map;
    logodds_params scan_params;
    int fov_span = 0;
    int gain_weight = 0;
    int headings = 16;
    int heading = -1;
    int goal_heading = -1;

    explicit planner(const planning_space& space) : ps(space) {}

    Vector2f pick_next_goal_point(const Vector2f& start, const int n, const float search_radius, gpu_context& ctx = default_context()) {
        if (line_of_sight && range_scan) throw std::logic_error("planner::pick_next_goal_point: line_of_sight and range_scan are both set");
        if (fov_span > 0 && !line_of_sight) throw std::logic_error("planner::pick_next_goal_point: fov_span needs line_of_sight");
        if (gain_weight > 0 && !line_of_sight) throw std::logic_error("planner::pick_next_goal_point: gain_weight needs line_of_sight");
        if (!line_of_sight && !range_scan)
            ps.free_space_allocations.push_back([start, search_radius](Vector2f p) { return pt_dist(p, start) <= search_radius; });
        occupancy_grid g = ps.make_grid(ctx);
        if (range_scan) {
            if (map.W != g.W || map.H != g.H) map = logodds_grid(g.W, g.H);
            const int32_t sc = g.cell_of(start);
            const auto rays = square_fan(sc % g.W, sc / g.W, std::max(1, (int)(search_radius / g.resolution)));
            auto m = map.update(rays, g.scan_cast(rays, ctx), scan_params, ctx);
            seen = std::move(m.known);
            g.occ = std::move(m.occ_est);
        }
        if (line_of_sight) {
            if (seen.size() != g.occ.size()) seen.assign(g.occ.size(), 0);
            const int32_t sc = g.cell_of(start);
            const float rc = search_radius / g.resolution;
            const std::array<int32_t, 3> here{sc % g.W, sc / g.W, (int32_t)(rc * rc)};
            auto view = fov_span > 0 ? look_with_sector(g, here, ctx) : g.known_from_views({here}, seen, ctx);
            seen = std::move(view.known);
            g.occ = std::move(view.occ_seen);
        }
        const std::vector<uint8_t> known = (line_of_sight || range_scan) ? seen : ps.known_grid(g.W, g.H);
        for (size_t c = 0; c < known.size(); ++c)
            if (!known[c]) g.occ[c] = 0;                       // an obstacle the robot has not seen is not on its map
        g.edt(ctx);
        const int Cmax = std::clamp(n, 1, SC_ASSIGN_MAX_DIM);
        if (gain_weight > 0) {
            const float rc = search_radius / g.resolution;
            const auto by_gain = g.explore_goals_by_gain(known, {g.cell_of(start)}, (int32_t)(rc * rc),
                                                         fov_span > 0 ? heading_dirs(headings) : heading_table{}, fov_span, gain_weight, 1, 1,
                                                         ps.clearance_r2(g), 1, Cmax, ctx);
            goal_heading = by_gain.head[0];                    // -1 for the full circle and when nothing was picked
            if (by_gain.goal[0] >= 0) return g.centre_of(by_gain.goal[0]);
            if (goal_point_cache.empty()) throw std::runtime_error("planner::pick_next_goal_point: no reachable frontier and no cached goal");
            const Vector2f cached = goal_point_cache.top();
            goal_point_cache.pop();
            return cached;
        }
        const auto ex = g.explore_goals(known, {g.cell_of(start)}, ps.clearance_r2(g), 1, Cmax, 0, 0, ctx);
        if (ex.goal[0] >= 0) {
            std::vector<std::pair<int32_t, int32_t>> rest;     // (cost, cell) of the clusters not chosen
            for (int k = 0; k < Cmax; ++k)
                if (k != ex.col_of[0] && ex.cost[(size_t)k] != SC_FIELD_INF) rest.push_back({ex.cost[(size_t)k], ex.cell[(size_t)k]});
            std::sort(rest.begin(), rest.end());
            for (auto it = rest.rbegin(); it != rest.rend(); ++it) goal_point_cache.push(g.centre_of(it->second));
            if (fov_span > 0) {
                const float rc = search_radius / g.resolution;
                goal_heading = g.view_gain_headings(known, {{ex.goal[0] % g.W, ex.goal[0] / g.W, (int32_t)(rc * rc)}}, heading_dirs(headings),
                                                    fov_span, ctx).best[0][1];
            }
            return g.centre_of(ex.goal[0]);
        }
        goal_heading = -1;
        if (goal_point_cache.empty()) throw std::runtime_error("planner::pick_next_goal_point: no reachable frontier and no cached goal");
        const Vector2f next = goal_point_cache.top();
        goal_point_cache.pop();
        return next;
    }

private:
    // One look of a sensor of fov_span bins from `here` on the true grid g, on top of `seen`: the sector of `heading`, or of the
    // heading of largest predicted gain on the observed map; the full circle when the sector adds nothing.
    occupancy_grid::view_result look_with_sector(const occupancy_grid& g, const std::array<int32_t, 3>& here, gpu_context& ctx) {
        const heading_table dirs = heading_dirs(headings);
        if (fov_span > headings) throw std::invalid_argument("planner::pick_next_goal_point: fov_span exceeds headings");
        if (heading < 0 || heading >= headings) {
            occupancy_grid observed = g;
            for (size_t c = 0; c < seen.size(); ++c)
                if (!seen[c]) observed.occ[c] = 0;
            heading = observed.view_gain_headings(seen, {here}, dirs, fov_span, ctx).best[0][1];
        }
        size_t before = 0, after = 0;
        for (uint8_t k : seen) before += k != 0;
        auto view = g.known_from_sectors({sector_view(here, dirs, heading, fov_span)}, seen, ctx);
        for (uint8_t k : view.known) after += k != 0;
        if (after == before) view = g.known_from_views({here}, seen, ctx);
        return view;
    }
};

// ---- path smoothing (sea_current.hpp:321-431, 522-1170) ---------------------------------------------
struct arclength_data {
    float arclength = 0;
    std::vector<VectorXf> segments;   // cumulative arclength of each segment at t = k * precision
    std::vector<VectorXf> positions;  // the parameters t of those table entries
};

// Chebyshev polynomial: coefficients of T_0 .. T_{degree-1} on [xmin, xmax] (:328-335)
struct chebpoly {
    VectorXf coeffs;
    float xmin;
    float xmax;
    chebpoly(VectorXf coeffs, const float xmin, const float xmax) : coeffs(std::move(coeffs)), xmin(xmin), xmax(xmax) {}
};

// Least-squares fit of y(x) by `degree` Chebyshev columns (:1109-1138; Householder least squares on the GPU,
// sc_chebfit_batch) and its evaluation (:1140-1170, sc_chebeval_batch).
inline chebpoly chebfit(const VectorXf& x, const VectorXf& y, const int degree, gpu_context& ctx = default_context()) {
    SC_ASSERT(degree >= 1, "degree must be a positive integer");
    SC_ASSERT(x.rows() == y.rows(), "x and y must have the same number of rows");
    const int m = (int)x.rows();
    SC_ASSERT(m > 0 && std::abs(x.maxCoeff() - x.minCoeff()) > 0.00001, "Error: vector x should not have all equal values");
    std::vector<float> xs(m), ys(m), coef(degree);
    for (int i = 0; i < m; ++i) { xs[i] = x(i); ys[i] = y(i); }
    const int32_t off[2] = {0, m};
    float xr[2] = {0, 0};
    ctx.check(sc_chebfit_batch_host(ctx.get(), xs.data(), ys.data(), off, 1, degree, coef.data(), xr), "sc_chebfit_batch_host");
    VectorXf c = VectorXf::Zero(degree);
    for (int k = 0; k < degree; ++k) c(k) = coef[k];
    return chebpoly(std::move(c), xr[0], xr[1]);
}
inline VectorXf chebeval(const VectorXf& x, const chebpoly& b, const int degree, gpu_context& ctx = default_context()) {
    SC_ASSERT(degree >= 1 && (int)b.coeffs.rows() >= degree, "degree must be a positive integer within the polynomial");
    const int m = (int)x.rows();
    VectorXf y = VectorXf::Zero(m);
    if (m == 0) return y;
    std::vector<float> xs(m), ys(m), coef(degree);
    for (int i = 0; i < m; ++i) xs[i] = x(i);
    for (int k = 0; k < degree; ++k) coef[k] = b.coeffs(k);
    const int32_t off[2] = {0, m};
    const float xr[2] = {b.xmin, b.xmax};
    ctx.check(sc_chebeval_batch_host(ctx.get(), xs.data(), off, 1, degree, coef.data(), xr, ys.data()), "sc_chebeval_batch_host");
    for (int i = 0; i < m; ++i) y(i) = ys[i];
    return y;
}

// Tangent heuristics of Lau, Sprunk, Burgard (IROS 2009) as the reference states them (:339-377): scalar host
// helpers for callers that build control points by hand (examples/test.cpp:88-104); from_path computes the same on the GPU.
inline float tangent_magnitude(const Vector2f& W_0, const Vector2f& W_1, const Vector2f& W_2) {
    return 0.5f * std::min(pt_dist(W_0, W_1), pt_dist(W_1, W_2));
}
// tangent at W_1: perpendicular to the bisector of the angle W_0 W_1 W_2, pointing on towards W_2
inline Vector2f calc_tangent(const Vector2f& W_0, const Vector2f& W_1, const Vector2f& W_2) {
    const Vector2f u = W_0 - W_1, v = W_2 - W_1;
    const float half = std::acos(u.dot(v) / (pt_dist(u) * pt_dist(v))) / 2;
    const float a_u = std::atan2(u.y(), u.x()), a_v = std::atan2(v.y(), v.x());
    const float ang = a_u + (a_v - a_u < 0 ? -half : half);
    Vector2f l90 = Vector2f(std::sin(ang), -std::cos(ang)).normalized();
    const float sign = pt_dist(W_1 + l90, W_2) < pt_dist(W_1 + (-l90), W_2) ? 1.0f : -1.0f;
    return tangent_magnitude(W_0, W_1, W_2) * (sign * l90);
}
inline Vector2f calc_start_tangent(const Vector2f& W_0, const Vector2f& W_1, const float theta) {
    return tangent_magnitude(W_0, W_1, W_0) * Vector2f(std::cos(theta), std::sin(theta));
}
inline Vector2f calc_end_tangent(const Vector2f& W_1, const Vector2f W_2) {
    return tangent_magnitude(W_1, W_2, W_1) * (W_2 - W_1).normalized();
}

struct velocity_profile;

class bezier_spline {
public:
    std::vector<std::vector<Vector2f>> ctrl_pts;  // control points per segment (degree + 1 each)
    points_matrix pts;                            // sampled points, one row each, in sample order
    std::vector<VectorXf> positions;              // per segment: the curve parameters of its samples (as :392)
    // per segment: the inverse discrete Fourier transform of its control points, the coefficients of the reference's
    // Bernstein-Fourier evaluation (:393, filled as :700-716 and :746 / :554-567 do).  Curves are evaluated from the control
    // points here (on the GPU); the member is kept, and kept filled, for callers that read it.
    std::vector<fourier_matrix> Q_cache;
    static fourier_matrix fourier_coefficients(const std::vector<Vector2f>& cp) {
        const size_t n = cp.size();
        fourier_matrix Q = fourier_matrix::Zero(n, 2);
        for (size_t k = 0; k < n; ++k) {
            std::complex<double> ax(0, 0), ay(0, 0);
            for (size_t j = 0; j < n; ++j) {
                const double ang = 2.0 * 3.14159265358979323846 * (double)((j * k) % n) / (double)n;      // inverse transform: e^{+2 pi i jk / n} / n
                const std::complex<double> w(std::cos(ang), std::sin(ang));
                ax += (double)cp[j].x() * w; ay += (double)cp[j].y() * w;
            }
            Q(k, 0) = std::complex<float>((float)(ax.real() / n), (float)(ax.imag() / n));
            Q(k, 1) = std::complex<float>((float)(ay.real() / n), (float)(ay.imag() / n));
        }
        return Q;
    }

    bezier_spline() = default;
    bezier_spline(const std::vector<std::vector<Vector2f>>& ctrl_pts, const points_matrix& pts, const std::vector<VectorXf>& positions)
        : ctrl_pts(ctrl_pts), pts(pts), positions(positions) {}
    int n_segments() const { return (int)ctrl_pts.size(); }
    int n_pts() const { return (int)pts.rows(); }
    int degree() const { return ctrl_pts.empty() ? 0 : (int)ctrl_pts[0].size() - 1; }

    // points of segments[i] (all of one degree) at parameters t[i], on the GPU: cubics through sc_bezier_eval_batch (the
    // arithmetic pinned to the recorded run), any other degree through sc_bezier_curve_batch
    static points_matrix evaluate(const std::vector<std::vector<Vector2f>>& cps, const std::vector<int32_t>& seg, const std::vector<float>& t,
                                  gpu_context& ctx = default_context()) {
        const int S = (int)cps.size(), M = (int)t.size(), deg = S ? (int)cps[0].size() - 1 : 0;
        points_matrix out(M, 2);
        if (M == 0) return out;
        SC_ASSERT(deg >= 1 && deg <= SC_BEZIER_MAX_DEGREE, "ctrl_pts must have at least 2 points");
        std::vector<float> c((size_t)S * (deg + 1) * 2), xy(2 * (size_t)M);
        for (int i = 0; i < S; ++i)
            for (int k = 0; k <= deg; ++k) { c[((size_t)i * (deg + 1) + k) * 2] = cps[i][k].x(); c[((size_t)i * (deg + 1) + k) * 2 + 1] = cps[i][k].y(); }
        if (deg == 3) ctx.check(sc_bezier_eval_batch_host(ctx.get(), c.data(), S, seg.data(), t.data(), M, 0, xy.data()), "sc_bezier_eval_batch_host");
        else ctx.check(sc_bezier_curve_batch_host(ctx.get(), c.data(), S, deg, seg.data(), t.data(), M, xy.data()), "sc_bezier_curve_batch_host");
        for (int i = 0; i < M; ++i) { out(i, 0) = xy[2 * i]; out(i, 1) = xy[2 * i + 1]; }
        return out;
    }

    // one curve from its control polygon, sampled at `positions` in [0, 1] (:684-752)
    static bezier_spline bezier_curve(const std::vector<Vector2f>& ctrl_pts, const VectorXf& positions, gpu_context& ctx = default_context()) {
        SC_ASSERT(ctrl_pts.size() >= 2, "ctrl_pts must have at least 2 points");
        const int M = (int)positions.rows();
        std::vector<float> t(M);
        for (int i = 0; i < M; ++i) t[i] = positions(i);
        bezier_spline bs({ctrl_pts}, evaluate({ctrl_pts}, std::vector<int32_t>(M, 0), t, ctx), {positions});
        bs.Q_cache = {fourier_coefficients(ctrl_pts)};
        return bs;
    }
    static bezier_spline bezier_curve(const std::vector<Vector2f>& ctrl_pts, const std::vector<float>& positions, gpu_context& ctx = default_context()) {
        VectorXf p = VectorXf::Zero(positions.size());
        for (size_t i = 0; i < positions.size(); ++i) p(i) = positions[i];
        return bezier_curve(ctrl_pts, p, ctx);
    }
    // ... sampled at k * precision, k = 0 .. 1/precision (:754-763)
    static bezier_spline bezier_curve(const std::vector<Vector2f>& ctrl_pts, const float precision, gpu_context& ctx = default_context()) {
        SC_ASSERT(precision < 1 && precision > 0, "spline percision must be in (0, 1)");
        const int n = (int)std::lround(1.0f / precision);
        VectorXf p = VectorXf::Zero(n + 1);
        for (int i = 0; i <= n; ++i) p(i) = std::max(0.0f, std::min(i * precision, 1.0f));
        return bezier_curve(ctrl_pts, p, ctx);
    }

    // the segments, sample positions and points of several splines, one after the other (:543-570)
    static bezier_spline join_splines(const std::vector<bezier_spline>& splines) {
        bezier_spline bs;
        size_t n = 0;
        for (const auto& sp : splines) n += (size_t)sp.n_pts();
        bs.pts = points_matrix::Zero(n, 2);
        size_t o = 0;
        for (const auto& sp : splines) {
            for (int i = 0; i < sp.n_segments(); ++i) {
                bs.ctrl_pts.push_back(sp.ctrl_pts[i]);
                if (i < (int)sp.positions.size()) bs.positions.push_back(sp.positions[i]);
                bs.Q_cache.push_back(i < (int)sp.Q_cache.size() ? sp.Q_cache[i] : fourier_coefficients(sp.ctrl_pts[i]));
            }
            for (int r = 0; r < sp.n_pts(); ++r, ++o) { bs.pts(o, 0) = sp.pts(r, 0); bs.pts(o, 1) = sp.pts(r, 1); }
        }
        return bs;
    }

    // k * T, cut where the stretch W +- k T crosses an obstacle edge of `ps` (same signature as :401 / :575-596; the edge
    // tests run on the GPU, sc_bezier_shrink_tangent_batch: what from_path applies to every waypoint's tangent)
    static Vector2f shrink_tangent(const Vector2f& T, const Vector2f& W, const float k, const planning_space& ps,
                                   gpu_context& ctx = default_context()) {
        std::vector<float> lines;
        for (const auto& ob : ps.obstacles)
            for (const auto& [a, b] : ob.lines) { lines.push_back(a.x()); lines.push_back(a.y()); lines.push_back(b.x()); lines.push_back(b.y()); }
        const float t[2] = {T.x(), T.y()}, w[2] = {W.x(), W.y()};
        float out[2] = {k * T.x(), k * T.y()};
        if (!lines.empty())
            ctx.check(sc_bezier_shrink_tangent_batch_host(ctx.get(), t, w, 1, k, lines.data(), (int)(lines.size() / 4), out), "sc_bezier_shrink_tangent_batch_host");
        return Vector2f(out[0], out[1]);
    }

    // the (degree + 1)-th roots of unity the reference's Bernstein-Fourier evaluation runs over (:422, :1096-1106): kept for
    // callers that use it; curves are evaluated from their control points here
    static inline std::vector<std::complex<float>> omega_table(const int degree) {
        std::vector<std::complex<float>> omegas((size_t)degree + 1);
        const double step = -2.0 * 3.14159265358979323846 / (double)(degree + 1);
        for (int i = 0; i <= degree; ++i) omegas[(size_t)i] = std::complex<float>((float)std::cos(step * i), (float)std::sin(step * i));
        return omegas;
    }

    // cubic Bezier spline through a piecewise-linear path; tangents by the Lau09 heuristics, shrunk against the
    // obstacle edges of `ps` (same signature as :599; tangents and control points on the GPU,
    // sc_bezier_from_path_batch), every leg sampled at 1e-4 like the reference's (:679)
    static bezier_spline from_path(const std::vector<Vector2f>& path, const planning_space& ps, float start_angle = NAN,
                                   gpu_context& ctx = default_context()) {
        SC_ASSERT(path.size() >= 2, "Not enough points for a path");
        const int n = (int)path.size();
        std::vector<float> xy(2 * (size_t)n), lines;
        for (int i = 0; i < n; ++i) { xy[2 * i] = path[i].x(); xy[2 * i + 1] = path[i].y(); }
        for (const auto& ob : ps.obstacles)
            for (const auto& [a, b] : ob.lines) { lines.push_back(a.x()); lines.push_back(a.y()); lines.push_back(b.x()); lines.push_back(b.y()); }
        const int32_t npts = n;
        std::vector<float> c(8 * (size_t)(n - 1));
        ctx.check(sc_bezier_from_path_batch_host(ctx.get(), xy.data(), &npts, 1, n, start_angle, lines.empty() ? nullptr : lines.data(),
                                                 (int)(lines.size() / 4), c.data()), "sc_bezier_from_path_batch_host");
        bezier_spline bs;
        bs.ctrl_pts.resize(n - 1);
        for (int i = 0; i < n - 1; ++i)
            for (int k = 0; k < 4; ++k) bs.ctrl_pts[i].push_back(Vector2f(c[8 * i + 2 * k], c[8 * i + 2 * k + 1]));
        constexpr int NS = 10000;   // 1 / 1e-4
        VectorXf p = VectorXf::Zero(NS + 1);
        for (int k = 0; k <= NS; ++k) p(k) = std::min(k * 1e-4f, 1.0f);
        std::vector<int32_t> seg((size_t)(n - 1) * (NS + 1));
        std::vector<float> t(seg.size());
        for (int i = 0; i < n - 1; ++i)
            for (int k = 0; k <= NS; ++k) { seg[(size_t)i * (NS + 1) + k] = i; t[(size_t)i * (NS + 1) + k] = p(k); }
        bs.pts = evaluate(bs.ctrl_pts, seg, t, ctx);
        bs.positions.assign(n - 1, p);
        for (const auto& cp : bs.ctrl_pts) bs.Q_cache.push_back(fourier_coefficients(cp));
        return bs;
    }

    // 32-point Gauss-Legendre arclength tables, 1/precision sub-intervals per segment (same as :765-896)
    arclength_data arclength(const float precision = 0.01f, gpu_context& ctx = default_context()) const {
        arclength_data ad;
        const int S = n_segments(), nsub = (int)std::lround(1.0f / precision);
        if (S == 0) return ad;
        SC_ASSERT(degree() == 3, "arclength tables are built for cubic segments");
        std::vector<float> c(8 * (size_t)S), cum((size_t)S * (nsub + 1)), len(S);
        for (int i = 0; i < S; ++i)
            for (int k = 0; k < 4; ++k) { c[8 * i + 2 * k] = ctrl_pts[i][k].x(); c[8 * i + 2 * k + 1] = ctrl_pts[i][k].y(); }
        ctx.check(sc_bezier_arclength_batch_host(ctx.get(), c.data(), S, nsub, cum.data(), len.data()), "sc_bezier_arclength_batch_host");
        ad.segments.assign(S, VectorXf::Zero(nsub + 1));
        ad.positions.assign(S, VectorXf::Zero(nsub + 1));
        for (int i = 0; i < S; ++i) {
            for (int k = 0; k <= nsub; ++k) { ad.segments[i](k) = cum[(size_t)i * (nsub + 1) + k]; ad.positions[i](k) = std::min(k * precision, 1.0f); }
            ad.arclength += len[i];
        }
        return ad;
    }

    // Map the arclength positions of a velocity profile back onto the curve (same signature as :898; profile_pos is
    // repaired in place when nudge_positions is set, as the reference's by-reference argument is).  Returns the spline
    // with one point per profile sample; throws if a segment receives no sample (the reference indexes out of range).
    bezier_spline resample(VectorXf& profile_pos, arclength_data ad, bool nudge_positions = false,
                           gpu_context& ctx = default_context()) const {
        SC_ASSERT(profile_pos.rows() > 0, "The vector of positions to be sampled must not be empty");
        const int S = n_segments(), n = (int)profile_pos.rows();
        SC_ASSERT((int)ad.segments.size() == S && S > 0, "arclength_data does not belong to this spline");
        const int nsub = (int)ad.segments[0].rows() - 1;
        std::vector<float> c(8 * (size_t)S), cum((size_t)S * (nsub + 1)), pp(n), out_pts(2 * (size_t)n), tp(n), cv(n);
        std::vector<int32_t> sg(n);
        for (int i = 0; i < S; ++i) {
            for (int k = 0; k < 4; ++k) { c[8 * i + 2 * k] = ctrl_pts[i][k].x(); c[8 * i + 2 * k + 1] = ctrl_pts[i][k].y(); }
            for (int k = 0; k <= nsub; ++k) cum[(size_t)i * (nsub + 1) + k] = ad.segments[i](k);
        }
        for (int i = 0; i < n; ++i) pp[i] = profile_pos(i);
        const int32_t seg_off[2] = {0, S}, prof_off[2] = {0, n};
        int32_t status = 0;
        ctx.check(sc_bezier_resample_batch_host(ctx.get(), c.data(), cum.data(), &ad.arclength, seg_off, 1, S, nsub, pp.data(), prof_off,
                                                nudge_positions ? 1 : 0, out_pts.data(), tp.data(), sg.data(), cv.data(), &status),
                  "sc_bezier_resample_batch_host");
        if (status != 0) throw std::runtime_error("bezier_spline::resample: a segment of the spline received no profile sample");
        for (int i = 0; i < n; ++i) profile_pos(i) = pp[i];
        bezier_spline re;
        re.ctrl_pts = ctrl_pts;
        re.pts = points_matrix::Zero(n, 2);
        std::vector<int> cnt(S, 0);
        for (int i = 0; i < n; ++i) { re.pts(i, 0) = out_pts[2 * i]; re.pts(i, 1) = out_pts[2 * i + 1]; ++cnt[sg[i]]; }
        re.positions.clear();
        for (int s = 0, o = 0; s < S; ++s) {
            VectorXf v = VectorXf::Zero(cnt[s]);
            for (int k = 0; k < cnt[s]; ++k) v(k) = tp[o + k];
            o += cnt[s];
            re.positions.push_back(std::move(v));
        }
        return re;
    }

    // first derivative as a spline of its own: control points degree * (P[j+1] - P[j]) per segment, sampled at the same
    // positions (:1041-1053)
    bezier_spline hodograph(gpu_context& ctx = default_context()) const {
        bezier_spline h;
        const int S = n_segments(), deg = degree();
        SC_ASSERT(deg >= 2, "the hodograph of a line has no control polygon");
        std::vector<int32_t> seg;
        std::vector<float> t;
        for (int i = 0; i < S; ++i) {
            std::vector<Vector2f> dc(deg);
            for (int j = 0; j < deg; ++j) dc[j] = (ctrl_pts[i][j + 1] - ctrl_pts[i][j]) * (float)deg;
            h.ctrl_pts.push_back(std::move(dc));
            if (i < (int)positions.size())
                for (size_t k = 0; k < (size_t)positions[i].rows(); ++k) { seg.push_back(i); t.push_back(positions[i](k)); }
        }
        h.positions = positions;
        h.pts = evaluate(h.ctrl_pts, seg, t, ctx);
        return h;
    }

    // signed curvature at every sample of `positions` (:1017-1039: hodograph and its hodograph)
    std::vector<float> curvature(gpu_context& ctx = default_context()) const {
        const bezier_spline d = hodograph(ctx), dd = d.hodograph(ctx);
        std::vector<float> res((size_t)d.n_pts());
        for (size_t i = 0; i < res.size(); ++i) {
            const float dx = d.pts(i, 0), dy = d.pts(i, 1), ddx = dd.pts(i, 0), ddy = dd.pts(i, 1);
            res[i] = (dx * ddy - dy * ddx) / std::pow(dx * dx + dy * dy, 1.5f);
        }
        return res;
    }

    inline std::vector<float> angular_velocity(const velocity_profile& vel_prof) const;    // :1055-1067
    inline std::vector<float> angular_velocity2(const velocity_profile& vel_prof) const;   // :1069-1094 (no stdout prints)
};

// ---- velocity profile (sea_current.hpp:379-386, 1172-1265) ------------------------------------------
struct velocity_profile {
    std::vector<VectorXf> pos;
    std::vector<VectorXf> vel;
    std::vector<VectorXf> acc;
    toppra_compat::Vector time;
    velocity_profile(std::vector<VectorXf> pos, std::vector<VectorXf> vel, std::vector<VectorXf> acc, toppra_compat::Vector time)
        : pos(std::move(pos)), vel(std::move(vel)), acc(std::move(acc)), time(std::move(time)) {}
};

inline std::vector<float> bezier_spline::angular_velocity(const velocity_profile& vel_prof) const {
    const std::vector<float> curv = curvature();
    SC_ASSERT(curv.size() == (size_t)vel_prof.vel[0].size(), "curvature and velocity vectors must be the same size");
    std::vector<float> w(curv.size());
    for (size_t i = 0; i < w.size(); ++i) w[i] = vel_prof.vel[0](i) * curv[i];
    return w;
}
// heading change of the tangent between consecutive samples over their time difference; zero at both ends
inline std::vector<float> bezier_spline::angular_velocity2(const velocity_profile& vel_prof) const {
    const bezier_spline d = hodograph();
    const size_t n = (size_t)d.n_pts();
    SC_ASSERT(n == (size_t)vel_prof.vel[0].size(), "hodograph and velocity vectors must be the same size");
    std::vector<float> rads(n), res(n, 0.0f);
    for (size_t i = 0; i < n; ++i) rads[i] = std::atan2(d.pts(i, 1), d.pts(i, 0));
    for (size_t i = 1; i + 1 < n; ++i) res[i] = (rads[i + 1] - rads[i]) / (float)(vel_prof.time(i + 1) - vel_prof.time(i));
    return res;
}

// limits as a function of the GRIDPOINT value s in [0,1] (the reference names the argument "time", :1175, :1185)
using vel_lim_func = std::function<std::tuple<toppra_compat::Vector, toppra_compat::Vector>(value_type time)>;   // = toppra::Vector

constexpr int SC_TOPPRA_GRID = 100;  // toppra's default number of grid intervals (confirmed by examples/output.json)

// P plans of `dof` joints in one GPU launch.  Arrays are [P][dof] row-major; limits per plan.
struct plan_request {
    std::vector<double> pos_end, pos_start, vel_end, vel_start, acc_min, acc_max;  // [dof] each
    vel_lim_func vel_lim;
};
inline std::vector<velocity_profile> gen_vel_prof_batch(const std::vector<plan_request>& plans, const float dt = 0.02f,
                                                        gpu_context& ctx = default_context()) {
    const int P = (int)plans.size();
    if (P == 0) return {};
    const int dof = (int)plans[0].pos_end.size(), N = SC_TOPPRA_GRID;
    std::vector<double> p0((size_t)P * dof), p1(p0), v0(p0), v1(p0), alo(p0), ahi(p0);
    std::vector<double> vlo((size_t)P * (N + 1) * dof), vhi(vlo);
    for (int p = 0; p < P; ++p) {
        const auto& r = plans[p];
        SC_ASSERT((int)r.pos_end.size() == dof, "all plans of a batch must have the same dof");
        for (int k = 0; k < dof; ++k) {
            const size_t o = (size_t)p * dof + k;
            p0[o] = r.pos_start[k]; p1[o] = r.pos_end[k]; v0[o] = r.vel_start[k]; v1[o] = r.vel_end[k];
            alo[o] = r.acc_min[k]; ahi[o] = r.acc_max[k];
        }
        for (int i = 0; i <= N; ++i) {
            auto [lo, hi] = r.vel_lim((double)i / N);
            for (int k = 0; k < dof; ++k) {
                // the reference's LinearJointVelocityVarying is built with size-1 limit vectors (:1179);
                // a 1-vector is broadcast over the joints
                vlo[((size_t)p * (N + 1) + i) * dof + k] = lo((size_t)lo.rows() == 1 ? 0 : k);
                vhi[((size_t)p * (N + 1) + i) * dof + k] = hi((size_t)hi.rows() == 1 ? 0 : k);
            }
        }
    }
    std::vector<double> K((size_t)P * (N + 1) * 2), x((size_t)P * (N + 1)), u((size_t)P * N), t((size_t)P * (N + 1));
    std::vector<int32_t> status(P);
    ctx.check(sc_toppra_hermite_batch_host(ctx.get(), P, dof, N, p0.data(), p1.data(), v0.data(), v1.data(), vlo.data(), vhi.data(), 1,
                                           alo.data(), ahi.data(), 0.0, 0.0, K.data(), x.data(), u.data(), t.data(), status.data()),
              "sc_toppra_hermite_batch_host");
    int max_len = 1;
    for (int p = 0; p < P; ++p) {
        SC_ASSERT(status[p] == 0, "TOPP-RA failed");  // the reference only SC_ASSERTs the return code (:1227)
        max_len = std::max(max_len, (int)std::ceil(t[(size_t)p * (N + 1) + N] / (double)dt) + 1);
    }
    std::vector<float> pos((size_t)P * dof * max_len), vel(pos.size()), acc(pos.size());
    std::vector<double> times((size_t)P * max_len);
    std::vector<int32_t> length(P);
    ctx.check(sc_toppra_sample_batch_host(ctx.get(), P, dof, N, p0.data(), p1.data(), v0.data(), v1.data(), x.data(), t.data(), (double)dt,
                                          max_len, pos.data(), vel.data(), acc.data(), times.data(), length.data()),
              "sc_toppra_sample_batch_host");
    std::vector<velocity_profile> out;
    out.reserve(P);
    for (int p = 0; p < P; ++p) {
        const int L = std::min(length[p], max_len);
        std::vector<VectorXf> ps(dof, VectorXf::Zero(L)), vs(dof, VectorXf::Zero(L)), as(dof, VectorXf::Zero(L));
        toppra_compat::Vector tm(L);
        for (int k = 0; k < dof; ++k)
            for (int j = 0; j < L; ++j) {
                const size_t o = ((size_t)p * dof + k) * max_len + j;
                ps[k](j) = pos[o]; vs[k](j) = vel[o]; as[k](j) = acc[o];
            }
        for (int j = 0; j < L; ++j) tm(j) = times[(size_t)p * max_len + j];
        out.emplace_back(std::move(ps), std::move(vs), std::move(as), std::move(tm));
    }
    return out;
}

// Same argument order as the reference: END before START (sea_current.hpp:1191-1199).
template <int N>
velocity_profile gen_vel_prof(const VectorNd<N>& pos_end, const VectorNd<N>& pos_start, const VectorNd<N>& vel_end,
                              const VectorNd<N>& vel_start, const vel_lim_func& vel_lim, const VectorNd<N>& acc_min,
                              const VectorNd<N>& acc_max, const float dt = 0.02f) {
    static_assert(N >= 1, "gen_vel_prof needs at least one degree of freedom");
    plan_request r;
    for (int k = 0; k < N; ++k) {
        r.pos_end.push_back(pos_end(k)); r.pos_start.push_back(pos_start(k));
        r.vel_end.push_back(vel_end(k)); r.vel_start.push_back(vel_start(k));
        r.acc_min.push_back(acc_min(k)); r.acc_max.push_back(acc_max(k));
    }
    r.vel_lim = vel_lim;
    return std::move(gen_vel_prof_batch({r}, dt)[0]);
}

// ---- the service's per-request sequence for a batch (examples/zmq_test.cpp:66-93) ------------------------------------
// from_path(path, space) -> arclength -> gen_vel_prof<1>(arclength, 0, 0, 0, limits) -> resample(nudge) -> angular velocity
// for every request, in ONE sc_smooth_paths_batch_host call.  Each result holds what serialize_path_to_json takes: the
// resampled spline (ctrl_pts, pts, positions), the profile, the arclength (the tables are not returned) and ang_vel =
// vel * curvature (the curvature of the resample kernel; bezier_spline::curvature goes through the hodograph on the host,
// so the two agree to rounding).  status is an sc_smooth_status; the other members are empty unless it is SC_SMOOTH_OK.
//
// Per-stage speed limits (sc_smooth_paths_limited_batch; the definition is in sea_current_hip.h): a request may bound the
// angular velocity (v <= omega_max / |kappa|), the lateral acceleration (v <= sqrt(alat_max / |kappa|)) and, in the overload
// that takes an occupancy_grid with its d2, the speed near obstacles (v <= clear_floor + clear_gain * clearance).  +inf
// switches a term off; with every term off and no grid the call is sc_smooth_paths_batch_host as before.  vmax_stage then
// holds the limit TOPP-RA ran with at each of its SC_TOPPRA_GRID + 1 stages, min_clear the smallest sampled clearance.
//
// Curves clear of the grid (sc_smooth_paths_clear_batch; the definition, its guarantee and what it does not guarantee are in
// sea_current_hip.h): when any request of a batch sets clear_r2 >= 0, the overload that takes an occupancy_grid checks which
// cells every Bezier leg visits and halves the tangents at the ends of legs that visit a cell with d2 < max(clear_r2, 1), up
// to clear_levels times.  The call takes one clearance and one depth for the batch: the largest clear_r2 and the largest
// clear_levels among the requests that ask.  tangent_level then holds the level of every waypoint, leg_min_d2 the smallest
// d2 under every leg of the final curve, rounds the repair rounds; a path shrinking cannot fix reads SC_SMOOTH_COLLIDES.
struct smooth_request {
    std::vector<Vector2f> path;
    double vel_min, vel_max, acc_min, acc_max;
    double omega_max = std::numeric_limits<double>::infinity();
    double alat_max = std::numeric_limits<double>::infinity();
    double clear_floor = std::numeric_limits<double>::infinity();
    double clear_gain = 0.0;
    int clear_r2 = -1;      // >= 0: keep the curve out of cells with d2 < max(clear_r2, 1) (needs the grid overload); -1: off
    int clear_levels = 6;   // halvings of a tangent at the most, 1 .. SC_CURVE_MAX_LEVEL
};
struct smooth_result {
    int status = SC_SMOOTH_BAD_INPUT;
    bezier_spline spline;
    velocity_profile profile{{}, {}, {}, toppra_compat::Vector()};
    arclength_data arclength;
    std::vector<float> ang_vel;
    std::vector<double> vmax_stage;   // [SC_TOPPRA_GRID + 1] when limits were asked for, else empty
    float min_clear = std::numeric_limits<float>::infinity();
    std::vector<uint8_t> tangent_level;   // [waypoints] when the batch asked for clear curves, else empty
    std::vector<int32_t> leg_min_d2;      // [legs], likewise
    int rounds = 0;
};
constexpr int SC_SPEED_SAMPLES = 4;   // J: samples to each side of a stage
inline std::vector<smooth_result> smooth_paths_batch_impl(const std::vector<smooth_request>& requests, const planning_space& space,
                                                          const occupancy_grid* grid, float dt, float precision, gpu_context& ctx) {
    const int P = (int)requests.size();
    std::vector<smooth_result> out(P);
    if (P == 0) return out;
    int n_max = 2;
    for (const auto& r : requests) n_max = std::max(n_max, (int)r.path.size());
    std::vector<float> xy((size_t)P * n_max * 2, 0.f), lines;
    std::vector<int32_t> npts(P);
    std::vector<double> lim((size_t)P * 4), dyn((size_t)P * 4), vstage;
    std::vector<float> min_clear;
    bool limited = grid != nullptr;
    int clear_r2 = -1, clear_levels = 0;
    int64_t cap = 0;
    for (int p = 0; p < P; ++p) {
        const auto& r = requests[p];
        const double inf = std::numeric_limits<double>::infinity();
        dyn[4 * (size_t)p] = r.omega_max; dyn[4 * (size_t)p + 1] = r.alat_max; dyn[4 * (size_t)p + 2] = r.clear_floor; dyn[4 * (size_t)p + 3] = r.clear_gain;
        limited = limited || r.omega_max != inf || r.alat_max != inf || r.clear_floor != inf;
        if (grid && r.clear_r2 >= 0) { clear_r2 = std::max(clear_r2, r.clear_r2); clear_levels = std::max(clear_levels, r.clear_levels); }
        npts[p] = (int32_t)r.path.size();
        float poly = 0;
        for (size_t i = 0; i < r.path.size(); ++i) {
            xy[((size_t)p * n_max + i) * 2] = r.path[i].x(); xy[((size_t)p * n_max + i) * 2 + 1] = r.path[i].y();
            if (i) poly += pt_dist(r.path[i], r.path[i - 1]);
        }
        lim[4 * (size_t)p] = r.vel_min; lim[4 * (size_t)p + 1] = r.vel_max; lim[4 * (size_t)p + 2] = r.acc_min; lim[4 * (size_t)p + 3] = r.acc_max;
        // a first guess of the samples (the call is repeated with the exact count if it was short)
        const double v = r.vel_max > 0 ? r.vel_max : 1.0, a = r.acc_max > 0 ? r.acc_max : 1.0;
        const double T = 1.5 * poly / v + 2.0 * v / a;
        cap += std::isfinite(T) ? (int64_t)std::min(T / dt * 1.25, 1e6) + 64 : 64;
    }
    for (const auto& ob : space.obstacles)
        for (const auto& [a, b] : ob.lines) { lines.push_back(a.x()); lines.push_back(a.y()); lines.push_back(b.x()); lines.push_back(b.y()); }
    const int nsub = (int)std::lround(1.0f / precision), S = P * (n_max - 1);
    std::vector<float> ctrl((size_t)S * 8), al(P), pos, vel, acc, pts, ang, tpar;
    std::vector<int32_t> seg_off(P + 1), length(P), offsets(P + 1), status(P), seg;
    std::vector<double> times;
    int64_t needed = 0;
    if (limited) { vstage.resize((size_t)P * (SC_TOPPRA_GRID + 1)); min_clear.resize(P); }
    std::vector<uint8_t> level;
    std::vector<int32_t> leg_min, rounds;
    if (clear_r2 >= 0) { level.resize((size_t)S + P); leg_min.resize(S); rounds.resize(P); }
    if (grid) { SC_ASSERT(grid->d2.size() == grid->occ.size() && !grid->d2.empty(), "the grid's d2 is missing: call edt() first"); }
    for (int attempt = 0; attempt < 2; ++attempt) {
        cap = std::min<int64_t>(std::max<int64_t>(cap, 1), INT32_MAX);
        pos.resize(cap); vel.resize(cap); acc.resize(cap); pts.resize(2 * (size_t)cap); ang.resize(cap); tpar.resize(cap); seg.resize(cap);
        times.resize(cap);
        if (!limited)
            ctx.check(sc_smooth_paths_batch_host(ctx.get(), xy.data(), npts.data(), P, n_max, lim.data(), NAN, lines.empty() ? nullptr : lines.data(),
                                                 (int)(lines.size() / 4), dt, SC_TOPPRA_GRID, nsub, cap, ctrl.data(), seg_off.data(), al.data(),
                                                 length.data(), offsets.data(), status.data(), &needed, times.data(), pos.data(), vel.data(),
                                                 acc.data(), pts.data(), nullptr, ang.data(), tpar.data(), seg.data()),
                      "sc_smooth_paths_batch_host");
        else if (clear_r2 >= 0)
            ctx.check(sc_smooth_paths_clear_batch_host(
                          ctx.get(), xy.data(), npts.data(), P, n_max, lim.data(), NAN, lines.empty() ? nullptr : lines.data(),
                          (int)(lines.size() / 4), dt, SC_TOPPRA_GRID, nsub, cap, ctrl.data(), seg_off.data(), al.data(), length.data(),
                          offsets.data(), status.data(), &needed, times.data(), pos.data(), vel.data(), acc.data(), pts.data(), nullptr,
                          ang.data(), tpar.data(), seg.data(), dyn.data(), SC_SPEED_SAMPLES, grid->d2.data(), grid->W, grid->H,
                          grid->bound_rect.x_min, grid->bound_rect.y_min, grid->resolution,
                          (grid->bound_rect.y_max - grid->bound_rect.y_min) / (float)grid->H, vstage.data(), min_clear.data(), clear_r2,
                          clear_levels, level.data(), leg_min.data(), rounds.data()),
                      "sc_smooth_paths_clear_batch_host");
        else
            ctx.check(sc_smooth_paths_limited_batch_host(
                          ctx.get(), xy.data(), npts.data(), P, n_max, lim.data(), NAN, lines.empty() ? nullptr : lines.data(),
                          (int)(lines.size() / 4), dt, SC_TOPPRA_GRID, nsub, cap, ctrl.data(), seg_off.data(), al.data(), length.data(),
                          offsets.data(), status.data(), &needed, times.data(), pos.data(), vel.data(), acc.data(), pts.data(), nullptr,
                          ang.data(), tpar.data(), seg.data(), dyn.data(), SC_SPEED_SAMPLES, grid ? grid->d2.data() : nullptr,
                          grid ? grid->W : 0, grid ? grid->H : 0, grid ? grid->bound_rect.x_min : 0.f, grid ? grid->bound_rect.y_min : 0.f,
                          grid ? grid->resolution : 0.f, grid ? (grid->bound_rect.y_max - grid->bound_rect.y_min) / (float)grid->H : 0.f,
                          vstage.data(), min_clear.data()),
                      "sc_smooth_paths_limited_batch_host");
        if (needed <= cap) break;
        cap = needed;
    }
    for (int p = 0; p < P; ++p) {
        smooth_result& res = out[p];
        res.status = status[p];
        res.arclength.arclength = al[p];
        if (limited) {
            res.vmax_stage.assign(vstage.begin() + (size_t)p * (SC_TOPPRA_GRID + 1), vstage.begin() + (size_t)(p + 1) * (SC_TOPPRA_GRID + 1));
            res.min_clear = min_clear[p];
        }
        if (clear_r2 >= 0 && seg_off[p + 1] > seg_off[p]) {
            res.tangent_level.assign(level.begin() + seg_off[p] + p, level.begin() + seg_off[p + 1] + p + 1);
            res.leg_min_d2.assign(leg_min.begin() + seg_off[p], leg_min.begin() + seg_off[p + 1]);
            res.rounds = rounds[p];
        }
        if (status[p] != SC_SMOOTH_OK) continue;
        const int s0 = seg_off[p], ns = seg_off[p + 1] - s0, o = offsets[p], L = length[p];
        bezier_spline& bs = res.spline;
        bs.ctrl_pts.resize(ns);
        for (int i = 0; i < ns; ++i)
            for (int k = 0; k < 4; ++k) bs.ctrl_pts[i].push_back(Vector2f(ctrl[((size_t)(s0 + i)) * 8 + 2 * k], ctrl[((size_t)(s0 + i)) * 8 + 2 * k + 1]));
        bs.pts = points_matrix::Zero(L, 2);
        std::vector<int> cnt(ns, 0);
        for (int j = 0; j < L; ++j) { bs.pts(j, 0) = pts[2 * (size_t)(o + j)]; bs.pts(j, 1) = pts[2 * (size_t)(o + j) + 1]; ++cnt[seg[o + j]]; }
        for (int i = 0, k0 = o; i < ns; ++i) {
            VectorXf v = VectorXf::Zero(cnt[i]);
            for (int k = 0; k < cnt[i]; ++k) v(k) = tpar[k0 + k];
            k0 += cnt[i];
            bs.positions.push_back(std::move(v));
        }
        std::vector<VectorXf> ps(1, VectorXf::Zero(L)), vs(1, VectorXf::Zero(L)), as(1, VectorXf::Zero(L));
        toppra_compat::Vector tm(L);
        for (int j = 0; j < L; ++j) { ps[0](j) = pos[o + j]; vs[0](j) = vel[o + j]; as[0](j) = acc[o + j]; tm(j) = times[o + j]; }
        res.profile = velocity_profile(std::move(ps), std::move(vs), std::move(as), std::move(tm));
        res.ang_vel.assign(ang.begin() + o, ang.begin() + o + L);
    }
    return out;
}
inline std::vector<smooth_result> smooth_paths_batch(const std::vector<smooth_request>& requests, const planning_space& space,
                                                     float dt = 0.02f, float precision = 0.01f, gpu_context& ctx = default_context()) {
    return smooth_paths_batch_impl(requests, space, nullptr, dt, precision, ctx);
}
// the same with a grid (its d2 filled by edt()): the clearance term of every request that has a finite clear_floor reads it
inline std::vector<smooth_result> smooth_paths_batch(const std::vector<smooth_request>& requests, const planning_space& space,
                                                     const occupancy_grid& grid, float dt = 0.02f, float precision = 0.01f,
                                                     gpu_context& ctx = default_context()) {
    return smooth_paths_batch_impl(requests, space, &grid, dt, precision, ctx);
}

// ---- (new) conflicts between timed paths (sc_fleet_conflicts_batch_host; the definition is in sea_current_hip.h) -------
// Who comes within radius[p] + radius[q] of whom among the results of smooth_paths_batch, when first, and how close
// everybody gets, on the common clock k * dt_c from 0 to past the end of the longest path plus its delay.  Detection only.
// delays (start delay of every path, default 0), flags (bit 0 / 1: stands at its first / last point before / after its run,
// default 3) and groups (paths with the same group >= 0 are never compared, default all different) are empty or one entry
// per path.  A moving obstacle is one more smooth_result: status SC_SMOOTH_OK, spline.pts and profile.time filled.
// status holds an sc_traj_status per path; a path that is not SC_TRAJ_OK (its smooth status was not OK, or it has no
// sample) reads first_t = min_sep = +inf, first_with = min_with = -1, n_conf = 0 and is invisible to the others.
struct conflict_result {
    std::vector<double> first_t, min_sep;
    std::vector<int> first_with, min_with, n_conf, status;
};
// smooth_results in the packed layout the sc_traj_* / sc_fleet_* host forms read, and the end of the last path plus its delay
struct packed_timed_paths {
    std::vector<int32_t> offsets, length, status, flags, groups;
    std::vector<double> time;
    std::vector<float> pts;
    double end = 0.0;
};
inline packed_timed_paths pack_timed_paths(const char* who, const std::vector<smooth_result>& paths, const std::vector<double>& radius,
                                           const std::vector<double>& delays, const std::vector<int>& flags, const std::vector<int>& groups,
                                           double dt_c) {
    const int P = (int)paths.size();
    if ((int)radius.size() != P) throw std::invalid_argument(std::string(who) + ": one radius per path expected");
    if (!(std::isfinite(dt_c) && dt_c > 0.0)) throw std::invalid_argument(std::string(who) + ": dt_c must be finite and > 0");
    if ((!delays.empty() && (int)delays.size() != P) || (!flags.empty() && (int)flags.size() != P) || (!groups.empty() && (int)groups.size() != P))
        throw std::invalid_argument(std::string(who) + ": delays, flags and groups are empty or hold one entry per path");
    packed_timed_paths k;
    k.offsets.assign(P + 1, 0); k.length.resize(P); k.status.resize(P);
    k.flags.assign(flags.begin(), flags.end()); k.groups.assign(groups.begin(), groups.end());
    for (int p = 0; p < P; ++p) {
        const int L = paths[p].status == SC_SMOOTH_OK ? std::min((int)paths[p].spline.pts.rows(), (int)paths[p].profile.time.size()) : 0;
        k.status[p] = paths[p].status;
        k.length[p] = L;
        k.offsets[p + 1] = k.offsets[p] + L;
    }
    const size_t M = (size_t)k.offsets[P];
    k.time.resize(std::max<size_t>(M, 1));
    k.pts.resize(2 * std::max<size_t>(M, 1));
    for (int p = 0; p < P; ++p) {
        for (int j = 0; j < k.length[p]; ++j) {
            k.time[(size_t)k.offsets[p] + j] = paths[p].profile.time(j);
            k.pts[2 * ((size_t)k.offsets[p] + j)] = paths[p].spline.pts(j, 0);
            k.pts[2 * ((size_t)k.offsets[p] + j) + 1] = paths[p].spline.pts(j, 1);
        }
        if (k.length[p] > 0) {
            const double e = paths[p].profile.time(k.length[p] - 1) + (delays.empty() ? 0.0 : delays[p]);
            if (std::isfinite(e)) k.end = std::max(k.end, e);
        }
    }
    return k;
}
inline conflict_result fleet_conflicts(const std::vector<smooth_result>& paths, const std::vector<double>& radius,
                                       const std::vector<double>& delays = {}, const std::vector<int>& flags = {},
                                       const std::vector<int>& groups = {}, double dt_c = 0.1,
                                       double sep_cap = std::numeric_limits<double>::infinity(), gpu_context& ctx = default_context()) {
    const int P = (int)paths.size();
    conflict_result out;
    if (P == 0) return out;
    const packed_timed_paths k = pack_timed_paths("fleet_conflicts", paths, radius, delays, flags, groups, dt_c);
    const int K = (int)std::min(std::max(std::ceil(k.end / dt_c), 1.0), 65535.0);
    out.first_t.resize(P); out.min_sep.resize(P);
    std::vector<int32_t> fw(P), mw(P), nc(P), ts(P);
    ctx.check(sc_fleet_conflicts_batch_host(ctx.get(), k.time.data(), k.pts.data(), k.offsets.data(), k.length.data(), k.status.data(), P,
                                            delays.empty() ? nullptr : delays.data(), k.flags.empty() ? nullptr : k.flags.data(), 0.0, dt_c, K,
                                            nullptr, ts.data(), radius.data(), k.groups.empty() ? nullptr : k.groups.data(), sep_cap,
                                            out.first_t.data(), fw.data(), out.min_sep.data(), mw.data(), nc.data(), nullptr),
              "sc_fleet_conflicts_batch_host");
    out.first_with.assign(fw.begin(), fw.end()); out.min_with.assign(mw.begin(), mw.end());
    out.n_conf.assign(nc.begin(), nc.end()); out.status.assign(ts.begin(), ts.end());
    return out;
}

// ---- (new) delay schedules for timed paths (sc_fleet_schedule_batch_host; the definition is in sea_current_hip.h) -------
// The cheapest resolution of what fleet_conflicts reports: the lower-priority path waits.  paths, radius, delays, flags and
// groups as in fleet_conflicts.  Every path gets one of D start slots (1 .. 32) of `stride` ticks of dt_c: walking `order`
// (empty = 0, 1, 2, ..; earlier = higher priority), a path takes the first slot <= jmax[p] (empty = D-1 everywhere; negative
// = pinned to slot 0, a moving obstacle) in which it meets none of the paths placed before it.  slot[p] >= 0, or
// SC_SLOT_UNRESOLVED (no slot is free: re-plan it; it blocks nobody), SC_SLOT_NOT_OK, SC_SLOT_UNNAMED (not in order).
// delay[p] = slot * stride * dt_c seconds to add to the path's start delay, NaN for slot < 0.  The clock runs (D-1) * stride
// ticks past the end of the longest path, so every path rests where the shifts end and the paths with slot >= 0 are
// conflict-free among themselves.  counts: slot 0, slot > 0, unresolved, not scheduled.
struct schedule_result {
    std::vector<int> slot, status;
    std::vector<double> delay;
    int counts[4] = {0, 0, 0, 0};
};
inline schedule_result fleet_schedule(const std::vector<smooth_result>& paths, const std::vector<double>& radius,
                                      const std::vector<double>& delays = {}, const std::vector<int>& flags = {},
                                      const std::vector<int>& groups = {}, double dt_c = 0.1, int D = 8, int stride = 1,
                                      const std::vector<int>& order = {}, const std::vector<int>& jmax = {},
                                      gpu_context& ctx = default_context()) {
    const int P = (int)paths.size();
    schedule_result out;
    if (P == 0) return out;
    const packed_timed_paths k = pack_timed_paths("fleet_schedule", paths, radius, delays, flags, groups, dt_c);
    if (D < 1 || D > 32 || stride < 1) throw std::invalid_argument("fleet_schedule: D in 1 .. 32 and stride >= 1 expected");
    if ((!order.empty() && (int)order.size() != P) || (!jmax.empty() && (int)jmax.size() != P))
        throw std::invalid_argument("fleet_schedule: order and jmax are empty or hold one entry per path");
    const int K = (int)std::min(std::max(std::ceil(k.end / dt_c), 1.0) + (double)(D - 1) * stride, 65535.0);
    const std::vector<int32_t> ord(order.begin(), order.end()), jm(jmax.begin(), jmax.end());
    std::vector<int32_t> sl(P), ts(P), cnt(4);
    ctx.check(sc_fleet_schedule_batch_host(ctx.get(), k.time.data(), k.pts.data(), k.offsets.data(), k.length.data(), k.status.data(), P,
                                           delays.empty() ? nullptr : delays.data(), k.flags.empty() ? nullptr : k.flags.data(), 0.0, dt_c, K,
                                           nullptr, ts.data(), radius.data(), k.groups.empty() ? nullptr : k.groups.data(), D, stride, nullptr,
                                           ord.empty() ? nullptr : ord.data(), jm.empty() ? nullptr : jm.data(), sl.data(), cnt.data(),
                                           nullptr),
              "sc_fleet_schedule_batch_host");
    out.slot.assign(sl.begin(), sl.end()); out.status.assign(ts.begin(), ts.end());
    out.delay.resize(P);
    for (int p = 0; p < P; ++p) out.delay[p] = sl[p] >= 0 ? (double)(sl[p] * stride) * dt_c : std::numeric_limits<double>::quiet_NaN();
    for (int v = 0; v < 4; ++v) out.counts[v] = cnt[v];
    return out;
}

// ---- (new) re-planning in space-time around the scheduled fleet (sc_fleet_replan_batch_host; the definition is in
// sea_current_hip.h) -------
// What fleet_schedule leaves SC_SLOT_UNRESOLVED is planned again on the grid, in (cell, tick), around the paths that did get a
// slot: paths, radius, delays and flags as given to fleet_schedule, `sched` its result, stride its stride.  The fleet is the
// paths with slot >= 0, each delayed by its slot; the robots are the unresolved ones, robot p from cell start[p] to cell
// goal[p] (one entry per path; those of scheduled paths are not read), appearing at the first tick at or after its delay and
// staying at its goal.  One grid move takes one tick of dt_c.  r_new is the robots' radius; the reservations are padded by
// r_new plus half the grid's diagonal move, which keeps a robot clear of every scheduled path (see the header).  With
// sequential (the default) the robots are planned in index order and each one's path is reserved before the next: they also
// stay clear of each other.  The clock runs `extra_ticks` (default 2 * (W + H)) past the end of the last scheduled path.
// Per path: status = an sc_tplan_status, or -1 for a path that is not a robot; arrive = the arrival tick (-1 without one);
// t_start = the tick it appears at; path = the timed cell path, path[p][i] the cell at tick t_start[p] + i (waits repeat a
// cell).  This is one earliest-arrival path, not the shortest in metres, and it is not smoothed.
struct replan_result {
    std::vector<int> status, arrive, t_start;
    std::vector<std::vector<int>> path;
    int K = 0;   // the last tick of the clock
};
inline replan_result fleet_replan(const std::vector<smooth_result>& paths, const std::vector<double>& radius, const schedule_result& sched,
                                  const occupancy_grid& grid, const std::vector<int>& start, const std::vector<int>& goal, double r_new,
                                  const std::vector<double>& delays = {}, const std::vector<int>& flags = {}, double dt_c = 0.1,
                                  int stride = 1, bool sequential = true, int r2_clear = 0, int extra_ticks = -1,
                                  gpu_context& ctx = default_context()) {
    const int P = (int)paths.size();
    replan_result out;
    if (P == 0) return out;
    const packed_timed_paths k = pack_timed_paths("fleet_replan", paths, radius, delays, flags, {}, dt_c);
    if ((int)sched.slot.size() != P || (int)start.size() != P || (int)goal.size() != P)
        throw std::invalid_argument("fleet_replan: the schedule, start and goal hold one entry per path");
    if (stride < 1 || !(std::isfinite(r_new) && r_new >= 0.0)) throw std::invalid_argument("fleet_replan: stride >= 1 and r_new >= 0 expected");
    if (grid.d2.size() != grid.occ.size() || grid.d2.empty()) throw std::invalid_argument("fleet_replan: the grid's d2 is missing: call edt() first");
    int max_slot = 0;
    std::vector<int32_t> sl(sched.slot.begin(), sched.slot.end()), select(P), robots;
    for (int p = 0; p < P; ++p) {
        max_slot = std::max(max_slot, (int)sl[p]);
        select[p] = sl[p] >= 0;
        if (sl[p] == SC_SLOT_UNRESOLVED) robots.push_back(p);
    }
    out.status.assign(P, -1); out.arrive.assign(P, -1); out.t_start.assign(P, 0); out.path.resize(P);
    const int B = (int)robots.size();
    const int extra = extra_ticks >= 0 ? extra_ticks : 2 * (grid.W + grid.H);
    const int K = (int)std::min(std::max(std::ceil(k.end / dt_c), 1.0) + (double)max_slot * stride + (double)extra, 65535.0);
    out.K = K;
    if (B == 0) return out;
    const int L = K + 1, Wq = (grid.W + 31) / 32;
    std::vector<double> knots((size_t)P * L * 2), shifted((size_t)P * L * 2);
    std::vector<int32_t> ts(P);
    ctx.check(sc_traj_knots_batch_host(ctx.get(), k.time.data(), k.pts.data(), k.offsets.data(), k.length.data(), k.status.data(), P,
                                       delays.empty() ? nullptr : delays.data(), k.flags.empty() ? nullptr : k.flags.data(), 0.0, dt_c, K,
                                       knots.data(), ts.data()),
              "sc_traj_knots_batch_host");
    ctx.check(sc_traj_shift_knots_batch_host(ctx.get(), knots.data(), P, K, sl.data(), stride, shifted.data()), "sc_traj_shift_knots_batch_host");
    const float ry = (grid.bound_rect.y_max - grid.bound_rect.y_min) / (float)grid.H;
    const double hyp = std::sqrt((double)grid.resolution * (double)grid.resolution + (double)ry * (double)ry);
    const double pad = r_new + 0.5 * hyp * (1.0 + std::ldexp(1.0, -20));
    std::vector<int32_t> s(B), g(B), t0(B), path((size_t)B * L), len(B), arr(B), st(B);
    for (int i = 0; i < B; ++i) {
        const int p = robots[i];
        s[i] = start[p]; g[i] = goal[p];
        t0[i] = (int)std::min(std::max(std::ceil((delays.empty() ? 0.0 : delays[p]) / dt_c), 0.0), (double)K);
    }
    std::vector<double> rn(B, r_new), knots_out((size_t)B * L * 2);
    std::vector<uint32_t> res((size_t)L * grid.H * Wq, 0u);
    ctx.check(sc_fleet_replan_batch_host(ctx.get(), shifted.data(), ts.data(), P, K, radius.data(), select.data(), pad, grid.W, grid.H,
                                         grid.bound_rect.x_min, grid.bound_rect.y_min, grid.resolution, ry, res.data(), grid.d2.data(), r2_clear, L,
                                         s.data(), g.data(), t0.data(), B, 1, path.data(), len.data(), arr.data(), st.data(), knots_out.data(),
                                         nullptr, rn.data(), sequential ? 1 : 0),
              "sc_fleet_replan_batch_host");
    for (int i = 0; i < B; ++i) {
        const int p = robots[i];
        out.status[p] = st[i]; out.arrive[p] = arr[i]; out.t_start[p] = t0[i];
        out.path[p].assign(path.begin() + (size_t)i * L, path.begin() + (size_t)i * L + len[i]);
    }
    return out;
}

// The same limits through the reference's own hook: a vel_lim_func for gen_vel_prof<1>(ad.arclength, 0, 0, 0, f, ..) along
// `spline` (its legs) with the tables `ad` of spline.arclength().  sc_speed_limits_batch_host runs once, here; the function
// answers s with the limit of stage round(s * SC_TOPPRA_GRID).  `rq` gives vel_min, vel_max and the four terms (its path
// is not read).  Throws when rq breaks the contract of the terms.
inline vel_lim_func speed_limit_func(const bezier_spline& spline, const arclength_data& ad, const smooth_request& rq,
                                     const occupancy_grid* grid = nullptr, int J = SC_SPEED_SAMPLES, gpu_context& ctx = default_context()) {
    const int ns = spline.n_segments(), N = SC_TOPPRA_GRID;
    SC_ASSERT(ns >= 1 && (int)ad.segments.size() == ns, "the tables must be those of the spline");
    const int nsub = (int)ad.segments[0].size() - 1;
    std::vector<float> ctrl((size_t)ns * 8), cum((size_t)ns * (nsub + 1));
    for (int i = 0; i < ns; ++i) {
        SC_ASSERT((int)ad.segments[i].size() == nsub + 1 && spline.ctrl_pts[i].size() == 4, "cubic legs with equal tables");
        for (int k = 0; k < 4; ++k) { ctrl[(size_t)i * 8 + 2 * k] = spline.ctrl_pts[i][k].x(); ctrl[(size_t)i * 8 + 2 * k + 1] = spline.ctrl_pts[i][k].y(); }
        for (int k = 0; k <= nsub; ++k) cum[(size_t)i * (nsub + 1) + k] = ad.segments[i](k);
    }
    if (grid) { SC_ASSERT(grid->d2.size() == grid->occ.size() && !grid->d2.empty(), "the grid's d2 is missing: call edt() first"); }
    const int32_t seg_off[2] = {0, ns};
    const double lim[4] = {rq.vel_min, rq.vel_max, rq.acc_min, rq.acc_max}, dyn[4] = {rq.omega_max, rq.alat_max, rq.clear_floor, rq.clear_gain};
    std::vector<double> vhi(N + 1);
    ctx.check(sc_speed_limits_batch_host(ctx.get(), ctrl.data(), cum.data(), seg_off, &ad.arclength, nullptr, 1, nsub, N, J, lim, dyn,
                                         grid ? grid->d2.data() : nullptr, grid ? grid->W : 0, grid ? grid->H : 0,
                                         grid ? grid->bound_rect.x_min : 0.f, grid ? grid->bound_rect.y_min : 0.f, grid ? grid->resolution : 0.f,
                                         grid ? (grid->bound_rect.y_max - grid->bound_rect.y_min) / (float)grid->H : 0.f, vhi.data(), nullptr,
                                         nullptr),
              "sc_speed_limits_batch_host");
    const double vel_min = rq.vel_min;
    return [vhi = std::move(vhi), vel_min, N](value_type s) {
        const int i = std::clamp((int)std::lround((double)s * N), 0, N);
        toppra_compat::Vector lo(1), hi(1);
        lo(0) = vel_min; hi(0) = vhi[i];
        return std::make_tuple(lo, hi);
    };
}

// ---- wire formats of the example service ---------------------------------------------------
// Request text of examples/zmq_test.cpp:30-59: "acc_min acc_max vel_min vel_max" then one "x y" pair per waypoint.
struct path_request {
    float acc_min = 0, acc_max = 0, vel_min = 0, vel_max = 0;
    std::vector<Vector2f> path;
    float max_x = 0, max_y = 0;   // largest |x|, |y|: the service builds its bounding_rect from them (:61)
};
inline path_request parse_path_request(const std::string& req) {
    path_request r;
    const char* p = req.c_str();
    char* end = nullptr;
    auto next = [&](float& v) {
        v = std::strtof(p, &end);
        const bool ok = end != p;
        p = end;
        return ok;
    };
    if (!(next(r.acc_min) && next(r.acc_max) && next(r.vel_min) && next(r.vel_max))) throw std::invalid_argument("path request: four limits expected");
    float x, y;
    while (next(x) && next(y)) {
        r.max_x = std::max(r.max_x, std::fabs(x));
        r.max_y = std::max(r.max_y, std::fabs(y));
        r.path.push_back(Vector2f(x, y));
    }
    return r;
}

// Reply of the service: a JSON array with one state per sample, the keys of serialize_path_to_json (:1423-1457).  (The
// reference flattens vel / acc through format_vec_vecx, which repeats element [i] of DOF i for every sample (:1414);
// this writes the per-sample values.)  Floats are printed with 9 significant digits, which round-trips float32.
inline std::string serialize_path_to_json(const bezier_spline& spline, const velocity_profile& vel_prof, const arclength_data& arclens,
                                          const std::vector<float>& ang_vel) {
    (void)arclens;
    std::string out = "[";
    char buf[512];
    const size_t n = (size_t)spline.pts.rows();
    for (size_t i = 0; i < n; ++i) {
        std::snprintf(buf, sizeof(buf),
                      "%s{\"acceleration\":%.9g,\"angularVelocity\":%.9g,\"holonomicAngularVelocity\":0.0,\"holonomicRotation\":0.0,"
                      "\"pose\":{\"translation\":{\"x\":%.9g,\"y\":%.9g}},\"time\":%.9g,\"velocity\":%.9g}",
                      i ? "," : "", (double)vel_prof.acc[0](i), (double)ang_vel[i], (double)spline.pts(i, 0), (double)spline.pts(i, 1),
                      (double)(float)vel_prof.time(i), (double)vel_prof.vel[0](i));
        out += buf;
    }
    out += "]";
    return out;
}

}  // namespace turtle::sc
