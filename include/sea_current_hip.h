/*
 * sea_current_hip.h -- C ABI of libsea_current_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for sea-current's planning hot path.  The
 * reference (turtle-robotics/sea-current @ 2024-10-16) is a header-only C++20
 * library with NO FFI of its own; the boundary it exposes is the `turtle::sc`
 * API of sea_current.hpp.  Each entry point below names the reference
 * interface whose work it takes over (file:line relative to the reference
 * root).  The C++ successor header sea-current_amd/sea_current.hpp keeps the
 * reference signatures and calls these functions; INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types.
 *   - functions without a suffix take DEVICE pointers and enqueue work on the
 *     context's stream without synchronising (inputs already resident in HBM);
 *     `_host` variants take host pointers, copy, run, copy back and synchronise.
 *   - every function returns an sc_status (0 = ok) and never exits the process
 *     (the reference's SC_ASSERT calls std::exit(1), sea_current.hpp:34-52).
 *   - a context is bound to one GPU and one stream; calls on one context are
 *     serialised on its stream, contexts are independent (one per host
 *     thread / rank).  No allocation happens in steady state: scratch is owned
 *     by the context and only grows.
 */
#ifndef SEA_CURRENT_HIP_H
#define SEA_CURRENT_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SC_ABI_VERSION 1

typedef struct sc_ctx sc_ctx;

typedef enum {
    SC_OK = 0,
    SC_ERR_INVALID = 1,  /* bad argument (null pointer, non-positive size, W or H too large) */
    SC_ERR_HIP = 2,      /* a HIP runtime call failed; see sc_last_error */
    SC_ERR_NOMEM = 3,    /* device allocation failed */
    SC_ERR_NO_DEVICE = 4 /* no usable gfx950 device */
} sc_status;

/* per-query status written by sc_astar_batch (mirrors the reference planner's
 * std::optional result: nullopt == SC_Q_NO_PATH, sea_current.hpp:1383-1385) */
typedef enum {
    SC_Q_OK = 0,
    SC_Q_NO_PATH = 1,
    SC_Q_BAD_ENDPOINT = 2, /* start/goal out of range or not traversable */
    SC_Q_TRUNCATED = 3,    /* path longer than Lmax: len holds the needed length, path is unspecified */
    SC_Q_RING_OVERFLOW = 4, /* the search's frontier outgrew the device queues twice (16x the usual space on the second
                             * attempt); no result for this query.  sc_ctx_synchronize enlarges the queues of later calls */
    SC_Q_BAD_PATH = 5       /* sc_path_waypoints_batch: the input path is not a legal A* move sequence */
} sc_query_status;

/* kernels timed by sc_ctx_set_timing (indices for sc_ctx_get_timing) */
typedef enum {
    SC_K_EDT_COLBITS = 0, /* occupancy bytes -> transposed per-band column bit words */
    SC_K_EDT_BAND = 1,    /* per 32-row band: vertical distances + exact row envelope -> d2 */
    SC_K_MOVES = 2,       /* d2 + clearance -> legal-move byte per cell; also sc_clearance_penalty_u8, sc_components_batch,
                           * sc_reachable_batch */
    SC_K_ASTAR = 3,       /* batched A*: two wavefronts per query (prep + search + retry launches); also the cost fields and
                           * their read-out (sc_cost_field_batch, sc_field_paths_batch, the weighted and the multi-source forms),
                           * the assignment on them (sc_field_cost_matrix, sc_assign_batch, sc_fleet_assign_batch), and the
                           * space-time plans (sc_traj_reserve_batch, sc_tplan_batch, sc_fleet_replan_batch) */
    SC_K_TOPPRA = 4,      /* batched TOPP-RA: computeParams + backward + forward sweep */
    SC_K_TOPPRA_SAMPLE = 5,
    SC_K_BEZIER = 6,      /* tangents + control points, curve evaluation */
    SC_K_ARCLENGTH = 7,   /* GL-32 arclength tables */
    SC_K_RESAMPLE = 8,    /* resample: nudge + split, Chebyshev fit + evaluation */
    SC_K_OCC = 9,         /* occupancy grids from rectangles or polygons (sc_occ_from_rects, sc_occ_from_polygons) */
    SC_K_NEAREST = 10,    /* nearest obstacle cell from d2 */
    SC_K_FMT = 11,        /* FMT* over Halton samples (the reference's own planner), one wavefront per query */
    SC_K_GATHER = 12,     /* gather of result paths: pack, ncclAllGather, unpack */
    SC_K_WAYPOINTS = 13,  /* A* cell paths -> line-of-sight waypoints, one wavefront per path */
    SC_K_SMOOTH = 14,     /* sc_smooth_paths_batch's own kernels (checks, scans, compaction, TOPP-RA inputs, ang_vel),
                           * sc_cells_to_points_batch, the speed limits, the curve check and repair (sc_curve_*) and the path conflicts (sc_traj_*, sc_fleet_conflicts_batch);
                           * the library kernels it runs keep their own ids */
    SC_K_COUNT = 15
} sc_kernel_id;

#define SC_EDT_INF INT32_MAX /* d2 of every cell of a grid without obstacles */
#define SC_MAX_DIM 8192      /* W, H <= SC_MAX_DIM (LDS row buffers) */

int sc_abi_version(void);
const char* sc_status_string(int status);
/* message of the last failing HIP call on this context ("" if none) */
const char* sc_last_error(const sc_ctx* ctx);

/* ---- context ----------------------------------------------------------- */
int sc_ctx_create(int device, sc_ctx** out);
int sc_ctx_destroy(sc_ctx* ctx);
/* Use the caller's hipStream_t (e.g. torch's current stream) instead of the
 * context's own; NULL means HIP's null (legacy default) stream.
 * Switching streams: the context's scratch and what one call leaves enqueued for
 * the next (zeroed flag maps, stamps and lists of the field calls, the A* slots,
 * the status block) are ordered on the OLD stream only.  Before the first call
 * after a switch the caller synchronises (sc_ctx_synchronize, or on the old
 * stream), or makes the new stream wait on an event recorded on the old one; the
 * same holds for sc_ctx_use_own_stream.  The switch itself waits for nothing. */
int sc_ctx_set_stream(sc_ctx* ctx, void* hip_stream);
/* Go back to the context's own non-blocking stream (the default after create). */
int sc_ctx_use_own_stream(sc_ctx* ctx);
/* Wait for everything enqueued on the context's stream.  Also where a context adapts to what its OWN launches met (the
 * state is per context: contexts that share a device do not see each other's): A* rings that overflowed (later calls
 * start with larger ones), maps of open space at widths of 513 .. 1024 (later EDTs run the band kernel's build with the
 * site search, until a launch meets none), and where a wide-row EDT whose bounded waits ran out is reported (SC_ERR_HIP).
 * Results never depend on the adapted state. */
int sc_ctx_synchronize(sc_ctx* ctx);
/* Kernel timing: when enabled every kernel launch is bracketed by HIP events on
 * the context's stream; sc_ctx_get_timing synchronises and returns the summed
 * device time and the number of launches since the last reset. */
int sc_ctx_set_timing(sc_ctx* ctx, int enable);
int sc_ctx_reset_timing(sc_ctx* ctx);
int sc_ctx_get_timing(sc_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);
/* Bytes of device scratch currently owned by the context. */
int sc_ctx_scratch_bytes(sc_ctx* ctx, int64_t* bytes);

/* ---- EDT ---------------------------------------------------------------
 * Exact squared Euclidean distance transform of `batch` occupancy grids.
 *   occ : uint8 [batch][H][W] row-major, != 0 means occupied
 *   d2  : int32 [batch][H][W]; SC_EDT_INF everywhere if a grid has no obstacle
 * Takes over the collision/clearance queries the reference answers by ray
 * casting and segment tests: obstacle::contains (sea_current.hpp:201-251),
 * planning_space::is_obstacle (:1274-1280), ::is_free (:1289-1292), ::cost
 * (:1315-1326).  The reference has no grid; the result is defined
 * mathematically (oracle/sc_oracle.h). */
int sc_edt_u8_i32(sc_ctx* ctx, const uint8_t* occ, int W, int H, int batch, int32_t* d2);
int sc_edt_u8_i32_host(sc_ctx* ctx, const uint8_t* occ, int W, int H, int batch, int32_t* d2);

/* Optional second output of the EDT: nearest[b][y][x] = linear index (y' * W + x') of the occupied cell
 * nearest to (x, y) in grid b, the smallest index among equidistant ones, -1 when the grid has no obstacle.  Needs
 * the d2 of sc_edt_u8_i32 for the same occ.  9 B/cell with d2 instead of 5.  Device pointers. */
int sc_edt_nearest_i32(sc_ctx* ctx, const uint8_t* occ, const int32_t* d2, int W, int H, int batch, int32_t* nearest);

/* Occupancy grid of a frame of the dynamic-obstacle replan loop (BASELINE.json configs[4]): occ = base (or all free
 * when base is NULL; base == occ paints in place) with R cell rectangles (x0, y0, x1, y1; x1/y1 exclusive; clipped)
 * painted as occupied; free_border != 0 keeps the outermost ring of cells free.  Stands where the
 * reference edits planning_space::obstacles (sea_current.hpp:314) between plans; the EDT is then recomputed in full
 * by sc_edt_u8_i32 (exact, ~10 us at 1024^2).  Device pointers; rects int32 [R][4]. */
int sc_occ_from_rects(sc_ctx* ctx, const uint8_t* base, const int32_t* rects, int R, int W, int H, int free_border, uint8_t* occ);

/* Occupancy grids from polygon obstacles: the successor header's host occupancy_grid::rasterize (sea_current.hpp), which
 * stays the definition, byte for byte, for G grids at once.  The reference describes its world as polygons (obstacle,
 * sea_current.hpp:193-284); this puts them on the grid the EDT, A*, waypoints and smoothing work on, on the device.
 *   Frame, shared by the G grids: W, H, x_min, y_min, res_x, res_y (what sc_cells_to_points_batch takes; the header passes
 *   bound_rect.x_min, bound_rect.y_min, resolution and (y_max - y_min) / (float)H).
 *     cx(x) = clamp((int)floor((x - x_min) / res_x), 0, W-1), cy(y) likewise with y_min, res_y, H;
 *     centre of cell (ix, iy) = (x_min + ((float)ix + 0.5f) * res_x, y_min + ((float)iy + 0.5f) * res_y).
 *   Obstacle o: lines obs_off[o] .. obs_off[o+1]-1 of lines (float [n_lines][4] x0,y0,x1,y1, the layout of
 *     sc_fmt_star_batch), each an edge (a, b); box B = obs_box[o] (x_max, x_min, y_max, y_min: bound_rect's member order;
 *     obs_box NULL = min / max of o's own lines); closed = obs_closed[o] (NULL = all closed, the header's default).
 *     Grid g owns obstacles grid_off[g] .. grid_off[g+1]-1 (grid_off int32 [G+1]; NULL only with G == 1: all of them).
 *     An obstacle without edges is skipped.  The edge-list constructor starts its box at vertices[0] even when no edge
 *     uses it (sea_current.hpp), so such obstacles need an explicit obs_box.
 *   Closed fill: for iy in cy(B.y_min) .. cy(B.y_max), ix in cx(B.x_min) .. cx(B.x_max), with p the cell's centre: set if
 *     p is inside B (inclusive) and odd is the count of edges with (a.y > p.y) != (b.y > p.y) and
 *     p.x < a.x + (p.y - a.y) * (b.x - a.x) / (b.y - a.y)   (evaluated in exactly that order).
 *   Edges of every obstacle, open or closed: dx = b.x - a.x, dy = b.y - a.y, len = sqrt(dx*dx + dy*dy) (float sum, correctly
 *     rounded float sqrt), n = max(1, (int)ceil(len / (0.5f * min(res_x, res_y)))); for k = 0 .. n: t = (float)k / (float)n,
 *     set cell (cx(a.x + dx*t), cy(a.y + dy*t)).  Clamping: an edge outside the frame paints border cells, as the host does.
 *   occ uint8 [G][H][W] = base [G][H][W] (all free when base is NULL; base == occ paints in place) OR the cells set by grid
 *     g's obstacles.
 *   Arithmetic: IEEE float32 throughout, no contraction, correctly rounded division and sqrt.  The header's host code gives
 *     these bytes when built as the tests build it (g++ -std=c++17, x86-64, no FMA contraction).
 * Contract: every coordinate (lines, obs_box, the frame) is finite, res_x, res_y > 0; every (x - x_min) / res_x and
 *   (y - y_min) / res_y of a vertex or box lies within +-2^30 (the host's float-to-int casts are undefined past it); every
 *   edge has n <= 2^24 (an edge about 8 M cells long); 0 <= obs_off[0] <= .. <= obs_off[n_obs] <= n_lines and
 *   0 <= grid_off[0] <= .. <= grid_off[G] <= n_obs.  Limits: W, H <= SC_MAX_DIM, 1 <= G <= 65535, n_obs >= 0.
 * sc_occ_from_polygons: device pointers; enqueues only (no host synchronisation, no device-to-host copy), so it chains as
 *   sc_occ_from_polygons -> sc_edt_u8_i32 (batch = G) -> sc_astar_batch_multi on one stream.  Scratch: 24 B per obstacle
 *   (grows only).  Outside the contract the result is unspecified; every index is clamped, so writes stay inside occ.
 * sc_occ_from_polygons_host: host pointers; checks the contract on the data and returns SC_ERR_INVALID before any launch,
 *   then copies, runs, copies occ back and synchronises.  Timed as SC_K_OCC. */
int sc_occ_from_polygons(sc_ctx* ctx, const uint8_t* base, int G, int W, int H, float x_min, float y_min, float res_x, float res_y,
                         const float* lines, int n_lines, const int32_t* obs_off, int n_obs, const float* obs_box,
                         const uint8_t* obs_closed, const int32_t* grid_off, uint8_t* occ);
int sc_occ_from_polygons_host(sc_ctx* ctx, const uint8_t* base, int G, int W, int H, float x_min, float y_min, float res_x,
                              float res_y, const float* lines, int n_lines, const int32_t* obs_off, int n_obs, const float* obs_box,
                              const uint8_t* obs_closed, const int32_t* grid_off, uint8_t* occ);

/* Legal-move mask per cell: bit d set iff move d (dx={1,-1,0,0,1,-1,1,-1},
 * dy={0,0,1,-1,1,1,-1,-1}) out of the cell is allowed: both cells have
 * d2 >= max(r2_clear,1) and, for diagonals, both side cells too. */
int sc_moves_i32_u8(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear, uint8_t* moves);

/* ---- batched A* --------------------------------------------------------
 * Q independent start->goal queries on one grid; 8-connected, costs 10/14,
 * octile heuristic, no corner cutting, canonical parent rule (sc_oracle.h).
 *   d2          : int32 [H][W] from sc_edt_u8_i32
 *   start, goal : int32 [Q] linear cell indices (y*W + x)
 *   path        : int32 [Q][Lmax], cells start..goal in path[q][0..len[q])
 *   len, cost, status : int32 [Q]  (cost = -1, len = 0 when there is no path)
 * Takes over planning_space::fast_marching_trees (sea_current.hpp:1339-1407)
 * with its helpers near (:1328-1337) and sample_free (:1294-1313): same role
 * (start, goal) -> optional waypoint list, on a grid instead of Halton samples.
 * Scratch: every search in flight owns W*H bytes of g, W*H/8 of closed bits and its open-list rings (9 MiB at 1024^2,
 * 50 MiB at 4096^2); a context takes at most 96 GiB for them (environment SC_ASTAR_SLOT_GB when the context is created)
 * and serves longer query lists from the same slots.  Only enqueues: a full ring is handled on the device (a second,
 * normally empty, launch with 16x the ring space); what that cannot hold either reports SC_Q_RING_OVERFLOW. */
int sc_astar_batch(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear,
                   const int32_t* start, const int32_t* goal, int Q, int Lmax,
                   int32_t* path, int32_t* len, int32_t* cost, int32_t* status);
int sc_astar_batch_host(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear,
                        const int32_t* start, const int32_t* goal, int Q, int Lmax,
                        int32_t* path, int32_t* len, int32_t* cost, int32_t* status);
/* Several grids in one launch: d2 int32 [G][H][W] (e.g. from sc_edt_u8_i32 with batch = G), qgrid int32 [Q] the grid of
 * every query.  Independent problems (several maps, several robots' local maps, consecutive frames) then share ONE
 * launch and its single tail: the persistent wavefronts pull queries of all grids from one queue, longest first. */
int sc_astar_batch_multi(sc_ctx* ctx, const int32_t* d2, int G, const int32_t* qgrid, int W, int H, int32_t r2_clear,
                         const int32_t* start, const int32_t* goal, int Q, int Lmax,
                         int32_t* path, int32_t* len, int32_t* cost, int32_t* status);
/* Node expansions of the last sc_astar_batch call on this context (synchronises). */
int sc_astar_last_expansions(sc_ctx* ctx, int64_t* expansions);
/* Debug: per-query expansions, popped queue entries, kilo-cycles and steps (int32 [4][Q]) of the last sc_astar_batch
 * (synchronises).  sc_astar_debug_peek: the launch counters (words 0 .. 3: queue positions and overflow counts of the main
 * and the retry pass; words 4 .. 15 are reserved and read 0), read without waiting for the stream. */
int sc_astar_debug_stats(sc_ctx* ctx, int32_t* stats4, int Q);
int sc_astar_debug_peek(sc_ctx* ctx, int32_t* out16);
/* Debug/parity: g field of ONE query (uint32 [H][W]): the optimal cost-to-come g* of every node the search
 * expanded -- E = {n : g*(n) + h(n) <= C*}, all that paths and parents are read from -- and 0xFFFFFFFF elsewhere. */
int sc_astar_gfield(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear,
                    int32_t start, int32_t goal, uint32_t* gfield, int32_t* cost, int32_t* status);

/* ---- cost-to-come fields ------------------------------------------------------------------------------
 * One exact shortest-path search from a root over the whole grid, then paths to any number of targets read from it.
 * Queries that share an endpoint (a fleet heading to one goal, one robot ranking candidate goals, the replan loop) need
 * one field instead of one A* search each.  Graph: the one A* uses -- 8 moves dx = {1,-1,0,0,1,-1,1,-1}, dy =
 * {0,0,1,-1,1,1,-1,-1}, cost 10 for d < 4 and 14 for d >= 4, cell c traversable iff d2[c] >= max(r2_clear, 1), a diagonal
 * needs both orthogonal side cells traversable, no move leaves the grid.
 *   Field of root r: g[c] = the optimal cost from r to c (exact integer), SC_FIELD_INF when c is unreachable or not
 *     traversable.  r out of range or not traversable: every cell SC_FIELD_INF and status SC_Q_BAD_ENDPOINT.  Costs fit
 *     in int32 at every allowed size (14 * 8192^2 < 2^31).
 *   Path to target t: the oracle's parent rule from t back to r -- parent(c) = the smallest d such that n = c - (dx_d,
 *     dy_d), the move n->c is legal and g[n] + w_d == g[c].  to_root = 0 writes r..t, to_root = 1 the same cells t..r
 *     (what a robot standing at t follows to reach r).
 *   Equality with A*: for every (r, t), status, len, cost and (when SC_Q_OK) path equal what sc_astar_batch returns for
 *     start r and goal t with the same r2_clear and Lmax: SC_Q_BAD_ENDPOINT if r or t is out of range or not traversable,
 *     r == t gives len 1 and cost 0, SC_Q_NO_PATH gives len 0 and cost -1, SC_Q_TRUNCATED gives len = the needed count
 *     and cost (path unspecified).  DESIGN.md section 12 has the argument.
 * sc_cost_field_batch: F fields; field f is rooted at root[f] on grid fgrid[f] of d2 int32 [G][H][W] (fgrid may be NULL
 *   only when G == 1).  g: int32 [F][H][W] (4 MiB per 1024^2 field, the caller's); fstatus: int32 [F] (SC_Q_OK /
 *   SC_Q_BAD_ENDPOINT), may be NULL.  An out-of-range fgrid[f] gives that field SC_Q_BAD_ENDPOINT.  The call fills g
 *   itself.  rounds: the chip-wide relaxation launches before the per-field finisher completes what is left; the result
 *   is identical for every value.  rounds < 0 = the library default 2 * (ceil(W/64) + ceil(H/64)) + 16 (80 at 1024^2).
 * sc_field_paths_batch: Q read-outs; query q reads field qfield[q] (its root root[qfield[q]], its grid fgrid[qfield[q]],
 *   its values g[qfield[q]]) towards target[q].  path [Q][Lmax], len / cost / status [Q]: sc_astar_batch's layout and
 *   conventions.  An out-of-range qfield[q] gives that query SC_Q_BAD_ENDPOINT.  g must be what sc_cost_field_batch wrote
 *   for the same d2, fgrid, root and r2_clear.
 * Both device forms only enqueue (no host synchronisation, no device-to-host copy), so this chain runs on one stream:
 *   sc_occ_from_polygons / sc_occ_from_rects -> sc_edt_u8_i32 -> sc_cost_field_batch -> sc_field_paths_batch ->
 *   sc_path_waypoints_batch -> sc_cells_to_points_batch -> sc_smooth_paths_batch.
 * Errors: SC_ERR_INVALID for NULL pointers, W or H outside 1..SC_MAX_DIM, F <= 0, G <= 0, Q < 0, Lmax <= 0.  Q == 0 is a
 *   no-op.  Scratch: G * W * ceil(H/64) * 8 B of traversability masks and about 16 B per (field, 64 x 64 tile), grows
 *   only.  The _host forms take host pointers, check the data (sc_field_paths_batch_host: every g value >= 0) before any
 *   launch, copy, run, copy back and synchronise.  Timed as SC_K_ASTAR. */
#define SC_FIELD_INF INT32_MAX
int sc_cost_field_batch(sc_ctx* ctx, const int32_t* d2, int G, const int32_t* fgrid, int W, int H, int32_t r2_clear,
                        const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus);
int sc_cost_field_batch_host(sc_ctx* ctx, const int32_t* d2, int G, const int32_t* fgrid, int W, int H, int32_t r2_clear,
                             const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus);
int sc_field_paths_batch(sc_ctx* ctx, const int32_t* d2, int G, const int32_t* fgrid, int W, int H, int32_t r2_clear,
                         const int32_t* g, const int32_t* root, int F, const int32_t* qfield, const int32_t* target, int Q,
                         int Lmax, int to_root, int32_t* path, int32_t* len, int32_t* cost, int32_t* status);
int sc_field_paths_batch_host(sc_ctx* ctx, const int32_t* d2, int G, const int32_t* fgrid, int W, int H, int32_t r2_clear,
                              const int32_t* g, const int32_t* root, int F, const int32_t* qfield, const int32_t* target, int Q,
                              int Lmax, int to_root, int32_t* path, int32_t* len, int32_t* cost, int32_t* status);

/* ---- clearance-weighted cost fields ------------------------------------------------------------------
 * The cost fields above with a per-cell entry cost: an inflation layer.  Paths keep their distance from obstacles where
 * there is room and still pass where there is none, instead of scraping every corner (small r2_clear) or losing the
 * narrow passages (large r2_clear).  DESIGN.md section 14.
 *   Costmap: pen uint8 [G][H][W], indexed like d2: any entry cost of the caller's (clearance, terrain, traffic).  pen_cap
 *     in 0..255; the effective penalty of cell c is min(pen[c], pen_cap).
 *   Graph: that of the cost fields -- the same 8 moves in the same order, the same T(c) <=> d2[c] >= max(r2_clear, 1), the
 *     same no-corner-cutting rule.  The move n -> c in direction d costs w_d + min(pen[c], pen_cap), w_d = 10 for d < 4
 *     and 14 otherwise: the penalty is paid on entering a cell, and the root's own penalty is never paid.
 *   Field: g[c] = the exact optimal cost from the root, SC_FIELD_INF when c is unreachable or not traversable; a bad
 *     root as in sc_cost_field_batch.
 *   Overflow contract: the device forms return SC_ERR_INVALID before any launch or allocation unless 0 <= pen_cap <= 255
 *     and (14 + pen_cap) * (W*H - 1) <= INT32_MAX - 1 (64-bit arithmetic).  A simple path enters each cell at most once,
 *     so every finite cost stays below SC_FIELD_INF: every cap passes up to 2048^2, caps up to 114 at 4096^2, up to 18 at
 *     8192^2.  Inside a tile the kernels add at most the entry costs of 63 cells of a row to a value in uint32, and
 *     INF + 63 * (10 + 255) < 2^32, so nothing wraps.
 *   Parent rule: parent(c) = the smallest d such that n = c - (dx_d, dy_d), the move n -> c is legal and
 *     g[n] + w_d + min(pen[c], pen_cap) == g[c].  Outputs, statuses, to_root, Lmax and truncation, qfield and fgrid out of
 *     range: those of sc_field_paths_batch; cost[q] = g[target].
 *   Asymmetry: the cost r -> t and the cost t -> r differ by pen[t] - pen[r] (each enters the other's end cell), and by
 *     nothing else: the optimal cell sequences are the same reversed, so to_root keeps its meaning.
 *   Anchor: with pen_cap == 0 (whatever pen holds) or pen all zero, g, fstatus and every read-out output are bit-identical
 *     to sc_cost_field_batch / sc_field_paths_batch on the same inputs, hence equal to sc_astar_batch.
 * sc_clearance_penalty_u8: the costmap from d2 [batch][H][W], integer arithmetic only.  thr = max(r2_clear, 1), isqrt =
 *   the exact floor square root, s10 = isqrt(100 * r2_soft); pen[c] = 0 if d2[c] < thr or d2[c] >= r2_soft, else
 *   (pen_max * (s10 - isqrt(100 * d2[c]))) / s10 (floor): it falls linearly with the distance, in tenths of a cell (the
 *   unit of the 10 / 14 move costs), and reaches 0 at the soft radius.  SC_ERR_INVALID for pen_max outside 0..255,
 *   r2_soft < 1, batch <= 0, W or H outside 1..SC_MAX_DIM, NULL pointers.  One kernel, timed as SC_K_MOVES.
 * The device forms only enqueue (no host synchronisation, no device-to-host copy): sc_edt_u8_i32 ->
 *   sc_clearance_penalty_u8 -> sc_cost_field_weighted_batch -> sc_field_paths_weighted_batch -> sc_path_waypoints_batch ->
 *   sc_cells_to_points_batch -> sc_smooth_paths_batch runs on one stream.  Arguments, errors and scratch otherwise as
 *   sc_cost_field_batch / sc_field_paths_batch (pen NULL: SC_ERR_INVALID); the _host forms copy pen as well.  The two
 *   field entries are timed as SC_K_ASTAR. */
int sc_clearance_penalty_u8(sc_ctx* ctx, const int32_t* d2, int W, int H, int batch, int32_t r2_clear, int32_t r2_soft, int pen_max,
                            uint8_t* pen);
int sc_clearance_penalty_u8_host(sc_ctx* ctx, const int32_t* d2, int W, int H, int batch, int32_t r2_clear, int32_t r2_soft,
                                 int pen_max, uint8_t* pen);
int sc_cost_field_weighted_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid, int W,
                                 int H, int32_t r2_clear, const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus);
int sc_cost_field_weighted_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid,
                                      int W, int H, int32_t r2_clear, const int32_t* root, int F, int rounds, int32_t* g,
                                      int32_t* fstatus);
int sc_field_paths_weighted_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid, int W,
                                  int H, int32_t r2_clear, const int32_t* g, const int32_t* root, int F, const int32_t* qfield,
                                  const int32_t* target, int Q, int Lmax, int to_root, int32_t* path, int32_t* len, int32_t* cost,
                                  int32_t* status);
int sc_field_paths_weighted_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid,
                                       int W, int H, int32_t r2_clear, const int32_t* g, const int32_t* root, int F,
                                       const int32_t* qfield, const int32_t* target, int Q, int Lmax, int to_root, int32_t* path,
                                       int32_t* len, int32_t* cost, int32_t* status);

/* ---- multi-source cost fields -------------------------------------------------------------------------
 * One field from many seeds: every cell's cost to the cheapest of K goals (docks, exits, chargers, frontier cells), each
 * with an optional start cost of its own (queue time at a dock), and for every cell which seed that is.  One relaxation
 * instead of K fields and a minimum over them.  DESIGN.md section 16.
 *   Graph: that of the cost fields above -- the moves, their order, costs 10 / 14, T(c) <=> d2[c] >= max(r2_clear, 1), the
 *     no-corner-cutting rule; with a costmap the move n -> c costs w_d + min(pen[c], pen_cap) as in the weighted fields.
 *     pen == NULL: unweighted (pen_cap is ignored).
 *   Seeds: field f owns seeds seed_off[f] .. seed_off[f+1] - 1 of seed int32 [n_seed] (cell indices on grid fgrid[f]) and
 *     seed_cost int32 [n_seed] (NULL: all zero).  A seed is valid iff its cell is in range and traversable and
 *     0 <= seed_cost <= SC_FIELD_SEED_COST_MAX (1 << 24, in the units of the move costs).  Invalid seeds are skipped.  A
 *     field with no valid seed (an empty list, an out-of-range fgrid[f]) is all SC_FIELD_INF with fstatus
 *     SC_Q_BAD_ENDPOINT.
 *   Field: g[c] = min over f's valid seeds s of seed_cost[s] + dist(seed[s], c); SC_FIELD_INF where no seed reaches c or c
 *     is not traversable.  A seed's own penalty is never paid, as for a root.  A seed may be dominated:
 *     g[seed[s]] < seed_cost[s].
 *   Overflow contract: the device forms return SC_ERR_INVALID before any launch unless
 *     (14 + cap) * (W*H - 1) + SC_FIELD_SEED_COST_MAX <= INT32_MAX - 1 (64-bit arithmetic; cap = pen_cap in 0..255, or 0
 *     when pen is NULL).  Unweighted it holds at every size up to 8192^2; every cap passes up to 2048^2, caps up to 113 at
 *     4096^2, up to 17 at 8192^2.
 *   Terminal and owner: cell c is terminal iff some valid seed s of the field has seed[s] == c and seed_cost[s] == g[c];
 *     its owner is the smallest such s (an index into the call's seed array: seed[owner] is the cell).  A terminal cell is
 *     terminal even when a parent would also satisfy the equality.  A finite non-terminal cell has owner[c] =
 *     owner[parent(c)], parent being the rule of the fields above; owner[c] = -1 where g is SC_FIELD_INF.  g falls by at
 *     least 10 per step and every finite non-terminal cell has a parent, so the owner is unique.
 *   Read-out: query q walks the parent rule from target[q] on field qfield[q] to the first terminal cell.  which[q] = its
 *     owner (-1 unless the status is SC_Q_OK or SC_Q_TRUNCATED); cost[q] = g[target], seed cost included.  to_seed = 0
 *     writes seed..target, to_seed = 1 target..seed.  SC_Q_BAD_ENDPOINT: target out of range or not traversable, or a bad
 *     qfield; SC_Q_NO_PATH: g is SC_FIELD_INF (every target of a field without a valid seed); SC_Q_TRUNCATED as in
 *     sc_field_paths_batch; a target on a terminal cell gives len 1.
 *   Anchors: with one valid seed of cost 0 per field, g and fstatus are bit-identical to sc_cost_field_batch (with pen: to
 *     sc_cost_field_weighted_batch), the read-out to sc_field_paths_batch / sc_field_paths_weighted_batch, and owner is that
 *     seed wherever g is finite.  In general g is the elementwise minimum of the single-root fields plus their seed costs,
 *     and, unweighted, path, len and cost - seed_cost[which] equal sc_astar_batch(seed[which], target).
 * sc_cost_field_multi_batch: g int32 [F][H][W]; owner int32 [F][H][W] or NULL (no owner pass); fstatus [F] or NULL;
 *   seed_off int32 [F + 1]; seed may be NULL only when n_seed == 0 (every field SC_Q_BAD_ENDPOINT).  On the device
 *   seed_off is clamped into 0..n_seed.  The owner pass takes ceil(log2(W*H)) + 3 launches, fixed on the host; a launch
 *   that finds nothing left returns at once.
 * sc_field_paths_multi_batch: g, owner and seed as sc_cost_field_multi_batch took and wrote them; which int32 [Q] or
 *   NULL.  An owner outside 0..n_seed-1 gives SC_Q_NO_PATH, so nothing is read out of bounds whatever the arrays hold.
 * The device forms only enqueue (no host synchronisation, no device-to-host copy).  Errors otherwise as
 *   sc_cost_field_batch / sc_field_paths_batch, and n_seed < 0 or seed_off NULL.  The _host forms check the data before
 *   any launch (seed_off non-decreasing within 0..n_seed, seed costs inside the contract, every g value >= 0:
 *   SC_ERR_INVALID).  Scratch: that of sc_cost_field_batch, which now takes about 16 B per (field, 64 x 64 tile) (4 B more:
 *   the flag of the tiles that hold a seed), plus 4 * (ceil(log2(W*H)) + 1) B of owner-pass counts; grows only.  Timed as
 *   SC_K_ASTAR. */
#define SC_FIELD_SEED_COST_MAX (1 << 24)
int sc_cost_field_multi_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid, int W, int H,
                              int32_t r2_clear, const int32_t* seed, const int32_t* seed_cost, const int32_t* seed_off, int n_seed, int F,
                              int rounds, int32_t* g, int32_t* owner, int32_t* fstatus);
int sc_cost_field_multi_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid, int W,
                                   int H, int32_t r2_clear, const int32_t* seed, const int32_t* seed_cost, const int32_t* seed_off,
                                   int n_seed, int F, int rounds, int32_t* g, int32_t* owner, int32_t* fstatus);
int sc_field_paths_multi_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid, int W, int H,
                               int32_t r2_clear, const int32_t* g, const int32_t* owner, const int32_t* seed, int n_seed, int F,
                               const int32_t* qfield, const int32_t* target, int Q, int Lmax, int to_seed, int32_t* path, int32_t* len,
                               int32_t* cost, int32_t* status, int32_t* which);
int sc_field_paths_multi_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* pen, int pen_cap, int G, const int32_t* fgrid, int W,
                                    int H, int32_t r2_clear, const int32_t* g, const int32_t* owner, const int32_t* seed, int n_seed,
                                    int F, const int32_t* qfield, const int32_t* target, int Q, int Lmax, int to_seed, int32_t* path,
                                    int32_t* len, int32_t* cost, int32_t* status, int32_t* which);

/* ---- free-space components ---------------------------------------------------------------------------
 * Labels the connected components of the traversable cells once, so that "is there a path from a to b" is answered
 * without searching, connected start and goal cells can be handed out, and a hopeless query is refused in O(1) instead
 * of expanding the start's whole component.  DESIGN.md section 15.
 *   Definition: T(c) <=> d2[c] >= max(r2_clear, 1).  Two traversable cells are in one component iff a chain of orthogonal
 *     moves through traversable cells joins them.  label[c] = the smallest linear index y*W + x of c's component, -1
 *     where c is not traversable: unique and independent of any execution order.
 *   This is exactly A*'s reachability: a diagonal move needs both orthogonal side cells traversable, so it can always be
 *     replaced by two orthogonal moves, and 8-connected reachability under the no-corner-cutting rule equals 4-connected
 *     reachability.  Two traversable cells have a path (SC_Q_OK or SC_Q_TRUNCATED from sc_astar_batch) iff their labels
 *     are equal.
 * sc_components_batch: d2 and label int32 [G][H][W].  size, ncomp and largest may each be NULL.  size int32 [G][H][W]:
 *   the cell count of the component at its representative cell (label[c] == c), 0 everywhere else.  ncomp int32 [G]: the
 *   number of components.  largest int32 [G]: the representative of the largest component, ties going to the smaller
 *   index, -1 on a grid with no traversable cell.  Integer atomics only; every output is independent of execution order.
 *   A constant number of kernels (at most five) and no host synchronisation.  Timed as SC_K_MOVES.  Scratch: G * 8 B, plus
 *   G * W * H * 4 B when largest is asked for without size; grows only.
 * sc_reachable_batch: status[q] = SC_Q_BAD_ENDPOINT if start[q] or goal[q] is out of range, qgrid[q] is out of range or a
 *   label is negative; SC_Q_NO_PATH if the labels differ; SC_Q_OK otherwise -- the status sc_astar_batch returns for the
 *   same query, SC_Q_OK standing for both SC_Q_OK and SC_Q_TRUNCATED.  qgrid int32 [Q] may be NULL only when G == 1.  One
 *   kernel, timed as SC_K_MOVES.
 * sc_astar_batch_screened: sc_astar_batch_multi (sc_astar_batch when G == 1 and qgrid is NULL) that never searches a query
 *   whose endpoints lie in different components.  status, len, cost, and path wherever status is SC_Q_OK, are bit-identical
 *   to the unscreened call on the same inputs.  label must be what sc_components_batch wrote for the same d2 and r2_clear
 *   (the contract of g in sc_field_paths_batch).  A kernel writes the starts into context scratch with -1 where the labels
 *   differ, the unscreened entry runs on those (such a query leaves at once as a bad endpoint: len 0, cost -1), a second
 *   kernel sets their status to SC_Q_NO_PATH.  Only enqueues, like the call it wraps; timed as SC_K_ASTAR.
 *   sc_astar_last_expansions then counts only the searches that ran.  Scratch: Q * 4 B on top of the search's.
 * All three device forms only enqueue: sc_edt_u8_i32 -> sc_components_batch -> sc_astar_batch_screened ->
 *   sc_path_waypoints_batch runs on one stream.
 * Errors: SC_ERR_INVALID for NULL pointers (other than the optional ones), W or H outside 1..SC_MAX_DIM, G <= 0, Q < 0,
 *   Lmax <= 0.  Q == 0 is a no-op.  The _host forms take host pointers, copy, run, copy back and synchronise. */
int sc_components_batch(sc_ctx* ctx, const int32_t* d2, int G, int W, int H, int32_t r2_clear, int32_t* label, int32_t* size,
                        int32_t* ncomp, int32_t* largest);
int sc_components_batch_host(sc_ctx* ctx, const int32_t* d2, int G, int W, int H, int32_t r2_clear, int32_t* label, int32_t* size,
                             int32_t* ncomp, int32_t* largest);
int sc_reachable_batch(sc_ctx* ctx, const int32_t* label, int G, const int32_t* qgrid, int W, int H, const int32_t* start,
                       const int32_t* goal, int Q, int32_t* status);
int sc_reachable_batch_host(sc_ctx* ctx, const int32_t* label, int G, const int32_t* qgrid, int W, int H, const int32_t* start,
                            const int32_t* goal, int Q, int32_t* status);
int sc_astar_batch_screened(sc_ctx* ctx, const int32_t* d2, const int32_t* label, int G, const int32_t* qgrid, int W, int H,
                            int32_t r2_clear, const int32_t* start, const int32_t* goal, int Q, int Lmax, int32_t* path, int32_t* len,
                            int32_t* cost, int32_t* status);

/* ---- line-of-sight waypoints of A* paths ---------------------------------------------------------------
 * Shortcuts every cell path of sc_astar_batch to the cells where it has to turn, the short waypoint list the
 * reference's planner hands to from_path (examples/test.cpp:284 -> :300).  Cells are integer points (x, y), index
 * y*W + x; T(c) <=> d2[c] >= max(r2_clear, 1) (the rule of sc_moves_i32_u8 and A*).
 *   Visible(a, b): every cell whose CLOSED unit square meets the closed segment between the centres of a and b is
 *     traversable (the segment's supercover; through a cell corner it needs both side cells: A*'s no-corner-cutting
 *     rule).  Exact integer arithmetic.
 *   Greedy prefix shortcut: out = [p0], anchor a = 0; j = the largest index with Visible(p[a], p[k]) for every k in
 *     a+1..j; emit p[j]; stop at j = L-1, else a = j and repeat.
 *   Collinear merge, as points are emitted: before w is appended, the last output point b is dropped while
 *     out[-2], b, w are collinear in the same direction (cross = 0, dot > 0).
 *   Reverse rule: if out[-2], p[a], p[j] are collinear in the reverse direction (cross = 0, dot < 0), j is lowered
 *     (not below a+1) until they are not.  A defined treatment: it fires on no A* path of the tests.
 *   So no interior waypoint is collinear with its neighbours, every output leg is Visible, and the output is a
 *   subsequence of the path from its first to its last cell.  All integers: bit-exact.
 * Inputs: d2 int32 [H][W]; path int32 [Q][Lmax], len [Q] and astar_status [Q] (may be NULL) as sc_astar_batch writes
 * them, so the device form chains on the stream.  Outputs: wp int32 [Q][Wmax] (cell indices, start..goal), n_wp and
 * status int32 [Q]:
 *   SC_Q_OK; the input status passed through with n_wp = 0 when astar_status[q] != SC_Q_OK; SC_Q_TRUNCATED with n_wp
 *   = the count needed when Wmax is too small (wp then holds the first Wmax points); SC_Q_BAD_PATH with n_wp = 0 when
 *   len is outside 1..Lmax, a cell is outside the grid, consecutive cells are not 8-adjacent or not Visible, or the
 *   only cell of a len-1 path is not traversable.
 * Scratch: Q * (Lmax - Wmax) int32 when Wmax < Lmax. */
int sc_path_waypoints_batch(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear, const int32_t* path, const int32_t* len,
                            const int32_t* astar_status, int Q, int Lmax, int Wmax, int32_t* wp, int32_t* n_wp, int32_t* status);
int sc_path_waypoints_batch_host(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear, const int32_t* path, const int32_t* len,
                                 const int32_t* astar_status, int Q, int Lmax, int Wmax, int32_t* wp, int32_t* n_wp, int32_t* status);

/* ---- batched TOPP-RA ---------------------------------------------------
 * P independent plans; path of plan p is the 2-knot cubic Hermite spline the
 * reference builds in gen_vel_prof<N> (sea_current.hpp:1213-1220) from
 * p0,p1 (positions) and v0,v1 (path tangents), all [P][dof] fp64.
 *   vlim_lo/hi : [P][dof] if vlim_per_stage == 0, else [P][N+1][dof] (limits
 *                evaluated at each gridpoint, LinearJointVelocityVarying,
 *                sea_current.hpp:1177-1188)
 *   alim_lo/hi : [P][dof]
 *   K [P][N+1][2], x [P][N+1] (= sdot^2), u [P][N], t [P][N+1], status [P]
 *   status: 0 ok, 1 backward pass infeasible, 2 forward pass infeasible
 * One kernel fuses LinearConstraint::computeParams of both constraints with
 * the backward (controllable sets) and forward sweeps of
 * TOPPRA::computePathParametrization(0,0) (:1224-1225) and the knot times of
 * parametrizer::Spline (:1233).  dof <= 16. */
int sc_toppra_hermite_batch(sc_ctx* ctx, int P, int dof, int N,
                            const double* p0, const double* p1, const double* v0, const double* v1,
                            const double* vlim_lo, const double* vlim_hi, int vlim_per_stage,
                            const double* alim_lo, const double* alim_hi,
                            double sd_start, double sd_end,
                            double* K, double* x, double* u, double* t, int32_t* status);
int sc_toppra_hermite_batch_host(sc_ctx* ctx, int P, int dof, int N,
                                 const double* p0, const double* p1, const double* v0, const double* v1,
                                 const double* vlim_lo, const double* vlim_hi, int vlim_per_stage,
                                 const double* alim_lo, const double* alim_hi,
                                 double sd_start, double sd_end,
                                 double* K, double* x, double* u, double* t, int32_t* status);
/* Spline parametrizer + uniform sampling (sea_current.hpp:1233-1262):
 *   length[p] = ceil(T_p/dt); samples at linspace(0, T_p, length[p]);
 *   pos/vel/acc float32 [P][dof][max_len] (the reference casts to VectorXf),
 *   times fp64 [P][max_len].  Only min(length, max_len) samples are written. */
int sc_toppra_sample_batch(sc_ctx* ctx, int P, int dof, int N,
                           const double* p0, const double* p1, const double* v0, const double* v1,
                           const double* x, const double* t, double dt, int max_len,
                           float* pos, float* vel, float* acc, double* times, int32_t* length);
int sc_toppra_sample_batch_host(sc_ctx* ctx, int P, int dof, int N,
                                const double* p0, const double* p1, const double* v0, const double* v1,
                                const double* x, const double* t, double dt, int max_len,
                                float* pos, float* vel, float* acc, double* times, int32_t* length);

/* ---- path smoothing and arclength ----------------
 * P paths of up to n_max waypoints (float [P][n_max][2], npts [P] valid counts).
 * ctrl: float [P][n_max-1][4][2], the cubic Bezier of every leg (zeros past a
 * path's last leg).  lines: float [nlines][4] obstacle edges (x0,y0,x1,y1) used
 * to shrink tangents; start_angle NaN = along the first leg.  Takes over
 * bezier_spline::from_path (sea_current.hpp:599-683) with calc_start_tangent /
 * calc_tangent / calc_end_tangent (:343-377) and shrink_tangent (:575-596). */
int sc_bezier_from_path_batch(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, float start_angle,
                              const float* lines, int nlines, float* ctrl);
int sc_bezier_from_path_batch_host(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, float start_angle,
                                   const float* lines, int nlines, float* ctrl);
/* bezier_spline::shrink_tangent (sea_current.hpp:575-596) on its own: tangent i becomes k * T[i], cut where the stretch
 * Wp[i] +- k T[i] crosses an obstacle edge (edges in order, the shortened tangent carried from edge to edge as the
 * reference does).  T, Wp, out float [M][2]; lines float [nlines][4]. */
int sc_bezier_shrink_tangent_batch(sc_ctx* ctx, const float* T, const float* Wp, int M, float k, const float* lines, int nlines, float* out);
int sc_bezier_shrink_tangent_batch_host(sc_ctx* ctx, const float* T, const float* Wp, int M, float k, const float* lines, int nlines, float* out);
/* Point (order 0), hodograph (1) or second derivative (2) of segment seg[i] (index
 * into ctrl viewed as [S][4][2]) at parameter t[i]; out float [M][2].  Takes over
 * bezier_spline::bezier_curve (:700-763) and ::hodograph (:1041-1053). */
int sc_bezier_eval_batch(sc_ctx* ctx, const float* ctrl, const int32_t* seg, const float* t, int M, int order, float* out);
/* host-pointer form; S = number of segments in ctrl */
int sc_bezier_eval_batch_host(sc_ctx* ctx, const float* ctrl, int S, const int32_t* seg, const float* t, int M, int order, float* out);
/* General degree (1 .. SC_BEZIER_MAX_DEGREE): point of segment seg[i] of ctrl viewed as [S][degree+1][2] at parameter
 * t[i].  Takes over bezier_spline::bezier_curve for any control polygon (:700-763) and, fed with the derivative control
 * points degree * (P[j+1] - P[j]), ::hodograph (:1041-1053) and the hodograph of a hodograph (::curvature :1017-1039). */
#define SC_BEZIER_MAX_DEGREE 15
int sc_bezier_curve_batch(sc_ctx* ctx, const float* ctrl, int degree, const int32_t* seg, const float* t, int M, float* out);
int sc_bezier_curve_batch_host(sc_ctx* ctx, const float* ctrl, int S, int degree, const int32_t* seg, const float* t, int M, float* out);
/* The free functions chebfit / chebeval (:1109-1170): B independent least-squares fits y(x) over the Chebyshev columns
 * T_0 .. T_{degree-1} of x normalised to [-1, 1] by its own range (the reference builds `degree` columns).  Problem b owns
 * rows off[b] .. off[b+1]-1 of x / y (total = off[B] rows); coef float [B][degree], xrange float [B][2] = (xmin, xmax) --
 * the three members of the reference's chebpoly.  chebeval evaluates problem b's polynomial at its rows of x. */
#define SC_CHEB_MAX_DEGREE 32
int sc_chebfit_batch(sc_ctx* ctx, const float* x, const float* y, const int32_t* off, int B, int total, int degree, float* coef, float* xrange);
int sc_chebfit_batch_host(sc_ctx* ctx, const float* x, const float* y, const int32_t* off, int B, int degree, float* coef, float* xrange);
int sc_chebeval_batch(sc_ctx* ctx, const float* x, const int32_t* off, int B, int degree, const float* coef, const float* xrange, float* y);
int sc_chebeval_batch_host(sc_ctx* ctx, const float* x, const int32_t* off, int B, int degree, const float* coef, const float* xrange, float* y);
/* bezier_spline::arclength (:767-896): 32-point Gauss-Legendre on nsub (= 1/precision)
 * sub-intervals of every segment.  cum float [S][nsub+1] cumulative length at
 * t = k/nsub, seg_len float [S] (the reference's arclength_data: segments, and
 * arclength = sum of seg_len over a path). */
int sc_bezier_arclength_batch(sc_ctx* ctx, const float* ctrl, int S, int nsub, float* cum, float* seg_len);
int sc_bezier_arclength_batch_host(sc_ctx* ctx, const float* ctrl, int S, int nsub, float* cum, float* seg_len);
/* bezier_spline::resample (:898-1005) with chebfit / chebeval (:1109-1170) and ::curvature (:1017-1039): map the
 * arclength positions of a velocity profile back onto the curve.  B splines; spline b owns segments
 * seg_off[b] .. seg_off[b+1]-1 (S = seg_off[B] in total) of ctrl [S][4][2] and of the tables cum [S][nsub+1]
 * (sc_bezier_arclength_batch), has total length arclength[b], and samples prof_off[b] .. prof_off[b+1]-1 of
 * profile_pos (M = prof_off[B] in total).  nudge != 0 first repairs profile_pos IN PLACE the way the reference does
 * (:902-913: ends pinned to 0 / arclength, non-monotone samples averaged, clamped).  Per sample: pts float [M][2],
 * tpar float [M] (curve parameter), seg int32 [M] (segment within the spline), curvature float [M] -- each may be
 * NULL.  status int32 [B]: 0, or 1 when a segment received no sample (the reference indexes out of range there; the
 * spline's outputs are then unspecified).  nsub <= SC_RESAMPLE_MAX_NSUB. */
#define SC_RESAMPLE_MAX_NSUB 512
int sc_bezier_resample_batch(sc_ctx* ctx, const float* ctrl, const float* cum, const float* arclength, const int32_t* seg_off,
                             int B, int S, int nsub, float* profile_pos, const int32_t* prof_off, int nudge, float* pts,
                             float* tpar, int32_t* seg, float* curvature, int32_t* status);
int sc_bezier_resample_batch_host(sc_ctx* ctx, const float* ctrl, const float* cum, const float* arclength, const int32_t* seg_off,
                                  int B, int S, int nsub, float* profile_pos, const int32_t* prof_off, int nudge, float* pts,
                                  float* tpar, int32_t* seg, float* curvature, int32_t* status);

/* ---- the post-planner sequence in one call ---------------------------------------------------------------
 * What the reference runs on every planned path (examples/zmq_test.cpp:66-93), for P paths at once:
 *   from_path(path, space) -> arclength -> gen_vel_prof<1>(arclength, 0, 0, 0, limits) -> resample(nudge) -> angular velocity
 * with the library kernels of those steps (sc_bezier_from_path_batch, sc_bezier_arclength_batch, sc_toppra_hermite_batch
 * with vlim_per_stage = 0, the sampler of sc_toppra_sample_batch, sc_bezier_resample_batch), so every value is the one
 * those calls give on the same inputs.  Device pointers; enqueues only: no host synchronisation, no device-to-host copy.
 * Inputs
 *   path float [P][n_max][2], npts int32 [P] (ragged, as sc_bezier_from_path_batch); limits fp64 [P][4] = (vel_min, vel_max,
 *   acc_min, acc_max) of every path; start_angle (NaN = along the first leg); lines float [nlines][4] obstacle edges (may be
 *   NULL); dt (the reference's float), N TOPP-RA stages, nsub = 1/precision sub-intervals (<= SC_RESAMPLE_MAX_NSUB);
 *   sample_capacity: the samples the per-sample outputs have room for (<= INT32_MAX).  P <= SC_SMOOTH_MAX_PATHS.
 * Per path
 *   ctrl float [P*(n_max-1)][4][2] (room for every leg): path p's legs at seg_off[p] .. seg_off[p+1]-1, int32 [P+1];
 *   arclength float [P]: the float32 sum of the legs' lengths in leg order (bezier_spline::arclength);
 *   length int32 [P]: samples of the profile, ceil(T / dt) with T the time of the last knot the sampler keeps;
 *   offsets int32 [P+1]: exclusive scan of length (saturated at INT32_MAX); status int32 [P] (sc_smooth_status);
 *   needed int64 [1]: offsets[P] without saturation, the sample_capacity that holds every path.
 * Per sample, path p's samples at offsets[p] .. offsets[p] + length[p] - 1 (what serialize_path_to_json prints):
 *   time fp64, pos float (nudged as resample leaves it), vel, acc float, pts float [2], curvature float, ang_vel float =
 *   vel * curvature, tpar float (curve parameter), seg int32 (leg within the path).  pos and pts are required, the
 *   others may be NULL.
 * Status, first that applies: SC_SMOOTH_BAD_INPUT (npts < 2, npts > n_max or a waypoint not finite; no legs),
 *   SC_SMOOTH_NONFINITE (a control point or the arclength not finite, as the reference's tangent rule gives on float-collinear
 *   triples), SC_SMOOTH_TOPPRA_FAILED (TOPP-RA status != 0, or a final time that is not finite), SC_SMOOTH_TRUNCATED
 *   (offsets[p] + length[p] > sample_capacity: length holds the count, no sample of the path is written; every path after
 *   it that has samples is truncated too), SC_SMOOTH_EMPTY_SEGMENT (resample status 1: a leg received no sample, where the
 *   reference indexes out of range; the samples were written, pts are unspecified).  For every status but OK and
 *   TRUNCATED length is 0; an EMPTY_SEGMENT path keeps its slot offsets[p] .. offsets[p+1]-1.  Samples past the written
 *   ones are not touched.
 * Launches are sized by P, P*(n_max-1) and sample_capacity; kernels read the real counts on the device.  Scratch: about
 * P*(n_max-1)*(4 nsub + 40) + P*(40 N + 120) bytes. */
#define SC_SMOOTH_MAX_PATHS 65536
typedef enum {
    SC_SMOOTH_OK = 0,
    SC_SMOOTH_BAD_INPUT = 1,
    SC_SMOOTH_NONFINITE = 2,
    SC_SMOOTH_TOPPRA_FAILED = 3,
    SC_SMOOTH_TRUNCATED = 4,
    SC_SMOOTH_EMPTY_SEGMENT = 5,
    SC_SMOOTH_COLLIDES = 6 /* sc_curve_clear_batch, sc_smooth_paths_clear_batch: a leg still hits the grid with the tangents at
                            * its ends shrunk to 2^-max_level; shrinking cannot fix it (the straight leg is not clear either) */
} sc_smooth_status;
int sc_smooth_paths_batch(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits, float start_angle,
                          const float* lines, int nlines, float dt, int N, int nsub, int64_t sample_capacity, float* ctrl,
                          int32_t* seg_off, float* arclength, int32_t* length, int32_t* offsets, int32_t* status, int64_t* needed,
                          double* time, float* pos, float* vel, float* acc, float* pts, float* curvature, float* ang_vel, float* tpar,
                          int32_t* seg);
/* Host pointers: the same call on device copies, then the results copied back (synchronises).  sample_capacity is the
 * room of the caller's per-sample arrays; *needed says how much a call that truncated would have needed. */
int sc_smooth_paths_batch_host(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits,
                               float start_angle, const float* lines, int nlines, float dt, int N, int nsub, int64_t sample_capacity,
                               float* ctrl, int32_t* seg_off, float* arclength, int32_t* length, int32_t* offsets, int32_t* status,
                               int64_t* needed, double* time, float* pos, float* vel, float* acc, float* pts, float* curvature,
                               float* ang_vel, float* tpar, int32_t* seg);
/* sc_path_waypoints_batch's cells -> the path input above, on the device: path[q][i] = the centre of cell wp[q][i] of a
 * W-wide grid, (x_min + (c % W + 0.5) * res_x, y_min + (c / W + 0.5) * res_y) in float32 without contraction
 * (occupancy_grid::centre_of); npts[q] = n_wp[q] when status[q] == SC_Q_OK and 1 <= n_wp[q] <= Wmax, else 0.  With starts
 * / goals (float [Q][2], both or neither) the first and last points are the exact start and goal, as
 * planning_space::plan_batch does: a one-cell path then becomes (start, goal), npts 2 (needs Wmax >= 2).  status may be
 * NULL (all OK).  Points past npts[q] are not written. */
int sc_cells_to_points_batch(sc_ctx* ctx, const int32_t* wp, const int32_t* n_wp, const int32_t* status, int Q, int Wmax, int W,
                             float x_min, float y_min, float res_x, float res_y, const float* starts, const float* goals, float* path,
                             int32_t* npts);

/* ---- per-stage speed limits from curvature and clearance ------------------------------------------------------
 * The reference's gen_vel_prof takes a vel_lim_func, a limit that varies along the path (examples/test.cpp:194-209);
 * sc_toppra_hermite_batch takes it as vlim_per_stage = 1.  These calls compute such a limit for curves that have legs
 * and arclength tables, and sc_smooth_paths_limited_batch puts it between the arclength and TOPP-RA of
 * sc_smooth_paths_batch.  Curves are not moved or shrunk: only the speed is limited (sc_curve_clear_batch below shrinks tangents).
 *
 * Per path: ctrl float [ns][4][2] (its legs), cum float [ns][nsub+1] (sc_bezier_arclength_batch), seg_len[j] = cum[j][nsub],
 * AL = arclength (float), limits fp64 (vel_min, vel_max, acc_min, acc_max), dyn fp64 [4] = (omega_max, alat_max, clear_floor,
 * clear_gain), optionally a grid d2 int32 [H][W] in the frame (W, H, x_min, y_min, res_x, res_y) of
 * sc_cells_to_points_batch and sc_occ_from_polygons.  All arithmetic is fp64 on the float32 inputs.
 *   Stage i of N: s_i = i / N, a_i = (double)AL * (3 s_i^2 - 2 s_i^3), the TOPP-RA path of gen_vel_prof<1>(AL, 0, 0, 0, ..)
 *     at gridpoint i, where the limit of stage i applies.
 *   Window: TOPP-RA enforces limits at gridpoints only (up to 1.5 AL / N apart), so a stage answers for the curve half
 *     way to its neighbours: lo_i = a_0 for i = 0, else (a_{i-1} + a_i) / 2; hi_i = a_N for i = N, else (a_i + a_{i+1}) / 2;
 *     samples j = -J .. J at x = a_i + (j/J) (a_i - lo_i) for j < 0, a_i + (j/J) (hi_i - a_i) for j >= 0.  1 <= J <= SC_SPEED_MAX_J.
 *   Position -> (leg, t): B_0 = 0, B_{j+1} = B_j + (double)seg_len[j] in leg order; x clamped to [0, AL]; leg j = the last with
 *     B_j <= x, at most ns-1; r = clamp(x - B_j, 0, seg_len[j]); k = the last index with cum[j][k] <= r, at most nsub-1;
 *     t = clamp((k + f) / nsub, 0, 1), f = (r - c_k) / (c_{k+1} - c_k), or 0 when that denominator is <= 0.
 *   Curvature: kappa = |x'y'' - y'x''| / (x'^2 + y'^2)^1.5 from the hodograph and the second derivative at t (the formula of
 *     the resample's curvature output); a kappa that is not finite counts as 0.
 *   Clearance (only with a grid and a finite clear_floor): fx = clamp((x - x_min) / res_x - 0.5, 0, W-1), ix = min((int)fx,
 *     max(W-2, 0)), ux = fx - ix (W == 1: the second column is the first), the same in y; c = the bilinear interpolation of
 *     min(res_x, res_y) * sqrt((double)d2[cell]) over the four cell centres.  Bilinear on purpose: the limit is continuous in
 *     the position.  It can overestimate the true clearance by a fraction of a cell (d2 is the distance between cell
 *     centres, and the interpolant of a distance field lies above it between samples of a convex stretch).
 *   Limit of a sample: v = vel_max; kappa > 0: v = min(v, omega_max / kappa, sqrt(alat_max / kappa)); clearance on:
 *     v = min(v, clear_floor + clear_gain * c).  vhi[i] = the minimum over the 2J+1 samples, vlo[i] = vel_min.
 *     min_clear = the minimum of c over every sample of the path (float), +inf when the clearance is off.
 * Contract of dyn: omega_max > 0, alat_max > 0 (+inf switches the term off), clear_floor >= 0 or +inf (off), clear_gain >= 0
 * and finite, no NaN.  A path whose dyn breaks it gets SC_SMOOTH_BAD_INPUT, decided on the device; the _host forms return
 * SC_ERR_INVALID for such data (and for a NaN in limits) before any launch.  With clear_floor = 0 a curve through a
 * spot of zero clearance has limit 0 there, and no profile passes a stage of limit 0 in finite time.  The parametriser
 * would not say so (like the reference's, it gives an interval of zero speed 5 s), so the limits kernel decides it: a
 * path with a term-made limit of 0 at an interior stage (0 < i < N) reports SC_SMOOTH_TOPPRA_FAILED, vhi and min_clear
 * hold what was computed, and the other paths are not affected.  A positive clear_floor is the crawl speed that avoids it.
 *
 * sc_speed_limits_batch: P curves; curve p owns legs seg_off[p] .. seg_off[p+1]-1 of ctrl and cum, arclength float [P],
 * limits and dyn fp64 [P][4]; status int32 [P] may be NULL (all SC_SMOOTH_OK); d2 NULL = no grid (the frame is then
 * ignored).  vhi fp64 [P][N+1]; min_clear float [P] and status_out int32 [P] may be NULL.  status_out[p] = status[p] when
 * that is not OK, else SC_SMOOTH_BAD_INPUT (dyn, or no leg), SC_SMOOTH_NONFINITE (arclength), SC_SMOOTH_TOPPRA_FAILED (a
 * limit of 0 inside, see above) or SC_SMOOTH_OK; a path with one of the first three gets vhi = 1 and min_clear = 0.  Device pointers; enqueues one kernel (timed under SC_K_SMOOTH), no host
 * synchronisation, no device-to-host copy; the launch is sized by P and reads the leg counts from seg_off on the device.
 * Errors: SC_ERR_INVALID for NULL pointers, P outside 1..SC_SMOOTH_MAX_PATHS, nsub outside 1..SC_RESAMPLE_MAX_NSUB, N <= 0,
 * J outside 1..SC_SPEED_MAX_J, and with a grid W or H outside 1..SC_MAX_DIM or a frame that is not finite with res > 0. */
#define SC_SPEED_MAX_J 32
int sc_speed_limits_batch(sc_ctx* ctx, const float* ctrl, const float* cum, const int32_t* seg_off, const float* arclength,
                          const int32_t* status, int P, int nsub, int N, int J, const double* limits, const double* dyn,
                          const int32_t* d2, int W, int H, float x_min, float y_min, float res_x, float res_y, double* vhi,
                          float* min_clear, int32_t* status_out);
/* host pointers; S = seg_off[P] legs (seg_off must not decrease) */
int sc_speed_limits_batch_host(sc_ctx* ctx, const float* ctrl, const float* cum, const int32_t* seg_off, const float* arclength,
                               const int32_t* status, int P, int nsub, int N, int J, const double* limits, const double* dyn,
                               const int32_t* d2, int W, int H, float x_min, float y_min, float res_x, float res_y, double* vhi,
                               float* min_clear, int32_t* status_out);
/* sc_smooth_paths_batch with these limits between the arclength and TOPP-RA: the same arguments in the same order, then
 * dyn fp64 [P][4], J, the grid (d2 NULL = none) and two more outputs, vmax_stage fp64 [P][N+1] (the vhi TOPP-RA ran with)
 * and min_clear float [P], each may be NULL.  TOPP-RA runs with vlim_per_stage = 1 on (vel_min replicated, vhi); every
 * other step is the one of sc_smooth_paths_batch, so with every term off (omega_max = alat_max = clear_floor = +inf) all
 * outputs are bit-identical to that call.  A path whose dyn breaks the contract reports SC_SMOOTH_BAD_INPUT (it keeps its
 * legs, length 0).  Chains behind sc_cells_to_points_batch on one stream like that call; scratch grows by
 * 2 * P * (N+1) doubles. */
int sc_smooth_paths_limited_batch(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits,
                                  float start_angle, const float* lines, int nlines, float dt, int N, int nsub, int64_t sample_capacity,
                                  float* ctrl, int32_t* seg_off, float* arclength, int32_t* length, int32_t* offsets, int32_t* status,
                                  int64_t* needed, double* time, float* pos, float* vel, float* acc, float* pts, float* curvature,
                                  float* ang_vel, float* tpar, int32_t* seg, const double* dyn, int J, const int32_t* d2, int W, int H,
                                  float x_min, float y_min, float res_x, float res_y, double* vmax_stage, float* min_clear);
int sc_smooth_paths_limited_batch_host(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits,
                                       float start_angle, const float* lines, int nlines, float dt, int N, int nsub,
                                       int64_t sample_capacity, float* ctrl, int32_t* seg_off, float* arclength, int32_t* length,
                                       int32_t* offsets, int32_t* status, int64_t* needed, double* time, float* pos, float* vel,
                                       float* acc, float* pts, float* curvature, float* ang_vel, float* tpar, int32_t* seg,
                                       const double* dyn, int J, const int32_t* d2, int W, int H, float x_min, float y_min, float res_x,
                                       float res_y, double* vmax_stage, float* min_clear);

/* ---- smoothed curves against the grid: check the cells a curve visits, shrink tangents where it hits --------------
 * A* cell paths and their line-of-sight waypoints never touch a cell with d2 < max(r2_clear, 1).  The Bezier legs that
 * sc_bezier_from_path_batch lays through those waypoints swing wide on the outside of turns and may enter such cells.
 * The reference's shrink_tangent tests the stretch Wp +- T against polygon edges, never the curve; on a grid these calls
 * test the curve itself against the distance map and shrink the tangents of legs that hit.
 *
 * Definition.  A leg is its float32 control polygon P0..P3 [4][2]; the grid is d2 int32 [H][W] in the frame (W, H, x_min,
 * y_min, res_x, res_y) of sc_cells_to_points_batch; r2c = max(r2_clear, 1), the traversability rule of A*.  All arithmetic
 * is fp64 on the float32 inputs, without contraction.
 *   Samples of a leg: h = min(res_x, res_y); Lp = |P1-P0| + |P2-P1| + |P3-P2|, each term sqrt(dx*dx + dy*dy) (correctly
 *     rounded), summed in that order; n = clamp(ceil(6 * Lp / h), 1, 2^20), n = 1 when Lp is not finite; t_k = (double)k / n,
 *     k = 0..n; the point is B(t) = r r r P0 + 3 r r t P1 + 3 r t t P2 + t t t P3, r = 1 - t, products and sums from the left.
 *     |B'| <= 3 max|P_{j+1} - P_j| <= 3 Lp, so consecutive samples are at most h / 2 apart along the curve and every point of
 *     the curve lies within h / 4 of a sample.
 *   Cell of a point: fx = (x - x_min) / res_x, ix = floor(fx), the same in y; the sample's value is d2[iy][ix], and 0 when fx
 *     or fy is not finite or the cell is outside 0..W-1 x 0..H-1: leaving the map is a hit.
 *   leg_min = the minimum of the values of the leg's samples.  A leg HITS iff leg_min < r2c, or n had to be clamped at 2^20,
 *     or Lp is not finite.
 *   First hit of a path: hit_leg = the lowest hitting leg, hit_t = (float)t_k of the lowest hitting sample k on it (0 when
 *     the leg hits without a hitting sample); both -1 when no leg hits.
 * Guarantee: no sample of a leg that does not hit lies in a blocked cell or outside the map, and no point of the curve is
 * further than a quarter of a cell from a sample.  It is a sampled test of cell membership, NOT a swept-disc proof: between
 * two samples the curve may clip the corner of a blocked cell by less than that quarter cell, and a robot's extent enters
 * only through r2_clear.
 *   Repair: waypoint j of a path with ns legs (j = 0..ns) has a level lv[j] in 0..max_level (1 <= max_level <=
 *     SC_CURVE_MAX_LEVEL) and the scale s_j = 2^-lv[j].  The control points are a function of the level-0 float32 control
 *     points only: leg j keeps P0 and P3; with lv[j] = 0 it keeps P1's bits, else P1 = (float)(P0 + s_j * (P1_0 - P0)); with
 *     lv[j+1] = 0 it keeps P2's bits, else P2 = (float)(P3 - s_{j+1} * (P3 - P2_0)), in fp64 on the widened floats.  Both legs
 *     at a waypoint share its level, so the tangent direction stays continuous.  Rounds r = 0, 1, ...: evaluate the legs at
 *     the current levels; if none hits the path is done with rounds = r; otherwise every waypoint at an end of a hitting leg
 *     gets lv += 1, saturating at max_level; if that changes no level the path is unresolved (rounds = r, the control points
 *     of this last round are kept).  The rule is Jacobi: all hits of a round are decided before any level changes, so no
 *     result depends on the order of execution.  At most max_level * (ns + 1) + 1 rounds occur.
 * Waypoints of sc_path_waypoints_batch under the same d2, r2_clear and frame are EXPECTED to resolve, not guaranteed to:
 * their straight legs lie in traversable cells of the supercover, and the curve tends to the straight leg as the levels
 * rise; float32 cell centres and exact start and goal points can break this where a leg grazes a corner, and
 * SC_SMOOTH_COLLIDES reports those.  A corridor of d2 < r2c (the straight legs are not clear either) cannot be fixed by
 * shrinking.
 *
 * Layout of all three calls: the packed legs of sc_smooth_paths_batch, ctrl float [S][4][2], seg_off int32 [P+1] read on the
 * device; status int32 [P] may be NULL (all SC_SMOOTH_OK).  Device pointers; each call enqueues one kernel on the context's
 * stream (one 256-thread workgroup per path, timed under SC_K_SMOOTH): no host synchronisation, no device-to-host copy.
 * Errors: SC_ERR_INVALID for NULL pointers, P outside 1..SC_SMOOTH_MAX_PATHS, d2 NULL, r2_clear < 0, W or H outside
 * 1..SC_MAX_DIM, a frame that is not finite with res > 0, max_level outside 1..SC_CURVE_MAX_LEVEL.
 *
 * sc_curve_clearance_batch: the check alone.  leg_min_d2 int32 [S], path_min_d2 int32 [P] (the minimum over the path's legs,
 * INT32_MAX for a path without legs), hit_legs int32 [P] (how many legs hit), hit_leg int32 [P], hit_t float [P]; each may
 * be NULL, but not all.  A path whose status is not SC_SMOOTH_OK is skipped: path_min_d2 = 0, hit_legs = 0, hit_leg = -1,
 * hit_t = -1, its legs' entries of leg_min_d2 untouched. */
#define SC_CURVE_MAX_LEVEL 30
#define SC_CURVE_MAX_LEGS 1024 /* legs of one path sc_curve_clear_batch takes: 39 B of LDS per leg, under 40 KiB, four workgroups per CU */
int sc_curve_clearance_batch(sc_ctx* ctx, const float* ctrl, const int32_t* seg_off, const int32_t* status, int P, const int32_t* d2,
                             int W, int H, float x_min, float y_min, float res_x, float res_y, int32_t r2_clear, int32_t* leg_min_d2,
                             int32_t* path_min_d2, int32_t* hit_legs, int32_t* hit_leg, float* hit_t);
/* host pointers; S = seg_off[P] legs (seg_off must start at or above 0 and not decrease) */
int sc_curve_clearance_batch_host(sc_ctx* ctx, const float* ctrl, const int32_t* seg_off, const int32_t* status, int P,
                                  const int32_t* d2, int W, int H, float x_min, float y_min, float res_x, float res_y, int32_t r2_clear,
                                  int32_t* leg_min_d2, int32_t* path_min_d2, int32_t* hit_legs, int32_t* hit_leg, float* hit_t);
/* sc_curve_clear_batch: the repair, every round inside the one kernel.  ctrl_out float [S][4][2] may be ctrl_in; level uint8
 * [S + P], waypoint j of path p at seg_off[p] + p + j; rounds int32 [P]; leg_min_d2 int32 [S] of the last round; status_out
 * int32 [P] (may be status) = status[p] when that is not SC_SMOOTH_OK, else SC_SMOOTH_COLLIDES for an unresolved path, else
 * SC_SMOOTH_OK.  level, rounds, leg_min_d2 and status_out may each be NULL.  With no hitting leg ctrl_out is ctrl_in bit for
 * bit and every level is 0.  A skipped path keeps its control points, gets levels 0 and rounds 0, and leaves its legs'
 * entries of leg_min_d2 untouched.  A path may have SC_CURVE_MAX_LEGS legs at the most (the kernel's LDS): the device form,
 * which cannot see the counts, treats a longer one as skipped with SC_SMOOTH_BAD_INPUT; the host form returns
 * SC_ERR_INVALID. */
int sc_curve_clear_batch(sc_ctx* ctx, const float* ctrl_in, const int32_t* seg_off, const int32_t* status, int P, const int32_t* d2,
                         int W, int H, float x_min, float y_min, float res_x, float res_y, int32_t r2_clear, int max_level,
                         float* ctrl_out, uint8_t* level, int32_t* rounds, int32_t* leg_min_d2, int32_t* status_out);
int sc_curve_clear_batch_host(sc_ctx* ctx, const float* ctrl_in, const int32_t* seg_off, const int32_t* status, int P, const int32_t* d2,
                              int W, int H, float x_min, float y_min, float res_x, float res_y, int32_t r2_clear, int max_level,
                              float* ctrl_out, uint8_t* level, int32_t* rounds, int32_t* leg_min_d2, int32_t* status_out);
/* sc_smooth_paths_limited_batch with the repair between the compaction of the legs and the arclength: the same arguments in
 * the same order, then r2_clear, max_level and three more outputs, level uint8 [P*(n_max-1) + P], leg_min_d2 int32
 * [P*(n_max-1)] (both in the layout above) and rounds int32 [P], each may be NULL.  The arclength, the speed limits, TOPP-RA
 * and the resample all see the repaired curve, and ctrl holds it.  It builds on the limited call on purpose: a tangent
 * shrunk by 2^-k is a tight corner, and omega_max / alat_max are what slow the robot down there.  It needs a grid: d2 NULL is
 * SC_ERR_INVALID, as is n_max - 1 > SC_CURVE_MAX_LEGS.  Status, first that applies: SC_SMOOTH_BAD_INPUT, SC_SMOOTH_NONFINITE,
 * SC_SMOOTH_COLLIDES (the path keeps its legs, those of its last round, and has length 0), then the rest as before.  When no
 * leg of the batch hits, every output is bit-identical to sc_smooth_paths_limited_batch on the same inputs.  Scratch grows
 * by P int32. */
int sc_smooth_paths_clear_batch(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits,
                                float start_angle, const float* lines, int nlines, float dt, int N, int nsub, int64_t sample_capacity,
                                float* ctrl, int32_t* seg_off, float* arclength, int32_t* length, int32_t* offsets, int32_t* status,
                                int64_t* needed, double* time, float* pos, float* vel, float* acc, float* pts, float* curvature,
                                float* ang_vel, float* tpar, int32_t* seg, const double* dyn, int J, const int32_t* d2, int W, int H,
                                float x_min, float y_min, float res_x, float res_y, double* vmax_stage, float* min_clear, int32_t r2_clear,
                                int max_level, uint8_t* level, int32_t* leg_min_d2, int32_t* rounds);
int sc_smooth_paths_clear_batch_host(sc_ctx* ctx, const float* path, const int32_t* npts, int P, int n_max, const double* limits,
                                     float start_angle, const float* lines, int nlines, float dt, int N, int nsub, int64_t sample_capacity,
                                     float* ctrl, int32_t* seg_off, float* arclength, int32_t* length, int32_t* offsets, int32_t* status,
                                     int64_t* needed, double* time, float* pos, float* vel, float* acc, float* pts, float* curvature,
                                     float* ang_vel, float* tpar, int32_t* seg, const double* dyn, int J, const int32_t* d2, int W, int H,
                                     float x_min, float y_min, float res_x, float res_y, double* vmax_stage, float* min_clear,
                                     int32_t r2_clear, int max_level, uint8_t* level, int32_t* leg_min_d2, int32_t* rounds);

/* ---- conflicts between timed paths: who meets whom, when, how close --------------------------------------------
 * sc_smooth_paths_batch leaves P timed paths on the device; these calls compare them with each other.  Detection only:
 * nothing is re-planned, delayed or moved (the caller can change a start delay and call again).  A moving obstacle is
 * one more timed path (two samples and a radius).  The reference has nothing of this kind.
 *
 * Definition.  All arithmetic is fp64 on the float32 inputs, in exactly this order of operations, without fused
 * multiply-adds (tests/traj_twin.py states it in NumPy, tests/cpp/traj_ref.c in C).
 *   Input: P timed paths in the packed layout sc_smooth_paths_batch writes: offsets int32 [P+1], length int32 [P], status
 *     int32 [P] (may be NULL = all SC_SMOOTH_OK), time fp64 [M], pts float [M][2]; path p's samples are offsets[p] ..
 *     offsets[p] + length[p] - 1.  Per path: t0 fp64 [P] start delay (NULL = 0); flags int32 [P], bit 0 = stands at its
 *     first point before it starts, bit 1 = stands at its last point after it ends (NULL = 3); radius fp64 [P]; group int32
 *     [P] (NULL = all different): two paths with the same group >= 0 are never compared, a negative group equals nobody.
 *   Path status (tstatus int32 [P], sc_traj_status): SC_TRAJ_SKIPPED when status[p] != SC_SMOOTH_OK or length[p] < 1;
 *     SC_TRAJ_BAD when a sample, t0 or radius is not finite, radius < 0, or time decreases; else SC_TRAJ_OK.  Paths that
 *     are not OK take part in nothing: their knots are NaN and their outputs read "none".  Decided on the device.
 *   Common clock: tau_k = T0 + k * dt_c for k = 0 .. K.
 *   Knot of path p at tau_k: u = tau_k - t0[p].  u < time[first]: the first point if flag bit 0 is set, else absent
 *     (NaN, NaN).  u > time[last]: the last point if flag bit 1 is set, else absent.  A path of one sample is its point.
 *     Otherwise j = the last index with time[j] <= u, at most len - 2; f = (u - time[j]) / (time[j+1] - time[j]), or 0 when
 *     that denominator is <= 0; knot = a + f * (b - a) per coordinate with a, b = (double)pts[j], (double)pts[j+1].  The
 *     motion compared is the piecewise-linear interpolant of the knots.
 *   Pair (lo < hi) on interval k, compared only when all four knots are present: d0 = knot[hi][k] - knot[lo][k],
 *     d1 = knot[hi][k+1] - knot[lo][k+1], e = d1 - d0; a = ex*ex + ey*ey, b = d0x*ex + d0y*ey, c = d0x*d0x + d0y*d0y;
 *     lam = a > 0 ? clamp(-b / a, 0, 1) : 0; m2 = (d0x + lam*ex)^2 + (d0y + lam*ey)^2; R = radius[lo] + radius[hi].  The
 *     interval conflicts iff m2 < R*R; then lc = 0 if c < R*R, else lc = clamp((-b - sqrt(max(b*b - a*(c - R*R), 0))) / a,
 *     0, lam), and the time of the conflict is tau_k + lc * dt_c.  clamp(x, l, h) = x < l ? l : (x > h ? h : x), max(x, 0) =
 *     x > 0 ? x : 0.  Everything is in terms of lo and hi, so (p, q) and (q, p) agree bit for bit.
 *   Pair result: first(p,q) = the minimum over k of those times (+inf if none); sep2(p,q) = the minimum over k of m2 (+inf
 *     if the two are never both present on an interval).
 *   Outputs per path, each may be NULL: first_t fp64 = the minimum over partners of first; first_with int32 = the smallest
 *     partner attaining it (-1 if none); min_sep fp64 = sqrt(min over partners of sep2) if that is < sep_cap, else +inf;
 *     min_with int32 = the smallest partner attaining it, else -1; n_conf int32 = the number of partners with a conflict.
 *   Optional bit matrix: conflict uint32 [P][ceil(P/32)], symmetric, bit q of row p set iff the pair conflicts.
 *   sep_cap: fp64 > 0, +inf = report every separation.  It exists so that far-apart pairs may be skipped by a
 *     conservative bound without changing any output; this version evaluates every pair.
 *   Every output is independent of the order of execution: minima, counts and bit-ORs only.
 *
 * sc_traj_knots_batch: the knots fp64 [P][K+1][2] and tstatus (samples, t0, time) of P paths.
 * sc_traj_conflicts_batch: the outputs above from knots; tstatus is read and written: a path that is OK on entry and whose
 *   radius is outside the contract becomes SC_TRAJ_BAD.  Knots of any origin may be passed (tstatus all 0 then).
 * sc_fleet_conflicts_batch: the two in sequence with the arguments of both; knots and tstatus may be NULL (context scratch).
 * Device pointers; the calls only enqueue on the context's stream (kernels timed under SC_K_SMOOTH): no host
 * synchronisation, no device-to-host copy, so they chain behind sc_smooth_paths_batch reading its offsets / length / status
 * / time / pts directly.  Scratch of the context: 24 bytes * P * slots with slots <= ceil(4096 / ceil(P/64)) (at most
 * 6 MiB, reached at P = 1024; 4096 is the number of workgroups a launch aims for), P * ceil(P/32) * 4 bytes when n_conf is asked without the matrix, and in sc_fleet_conflicts_batch
 * 16 * P * (K+1) bytes when knots is NULL.
 * The _host forms take host pointers and return SC_ERR_INVALID before any launch for offsets that decrease or are
 * negative, a readable path (status OK, length >= 1) that ends past offsets[P] (= M), flags outside 0..3 and for t0 or
 * radius outside the contract (what the kernel would mark SC_TRAJ_BAD from the per-path arguments; samples are judged on
 * the device).
 * Errors: SC_ERR_INVALID for NULL required pointers, P outside 1..16384, K outside 1..65535, P * (K+1) > 2^26, dt_c not
 * finite or <= 0, T0 not finite, sep_cap NaN or <= 0. */
typedef enum {
    SC_TRAJ_OK = 0,
    SC_TRAJ_SKIPPED = 1,
    SC_TRAJ_BAD = 2
} sc_traj_status;
int sc_traj_knots_batch(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets, const int32_t* length,
                        const int32_t* status, int P, const double* t0, const int32_t* flags, double T0, double dt_c, int K,
                        double* knots, int32_t* tstatus);
int sc_traj_knots_batch_host(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets, const int32_t* length,
                             const int32_t* status, int P, const double* t0, const int32_t* flags, double T0, double dt_c, int K,
                             double* knots, int32_t* tstatus);
int sc_traj_conflicts_batch(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, double T0, double dt_c,
                            const double* radius, const int32_t* group, double sep_cap, double* first_t, int32_t* first_with,
                            double* min_sep, int32_t* min_with, int32_t* n_conf, uint32_t* conflict);
int sc_traj_conflicts_batch_host(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, double T0, double dt_c,
                                 const double* radius, const int32_t* group, double sep_cap, double* first_t, int32_t* first_with,
                                 double* min_sep, int32_t* min_with, int32_t* n_conf, uint32_t* conflict);
int sc_fleet_conflicts_batch(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets, const int32_t* length,
                             const int32_t* status, int P, const double* t0, const int32_t* flags, double T0, double dt_c, int K,
                             double* knots, int32_t* tstatus, const double* radius, const int32_t* group, double sep_cap,
                             double* first_t, int32_t* first_with, double* min_sep, int32_t* min_with, int32_t* n_conf,
                             uint32_t* conflict);
int sc_fleet_conflicts_batch_host(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets, const int32_t* length,
                                  const int32_t* status, int P, const double* t0, const int32_t* flags, double T0, double dt_c, int K,
                                  double* knots, int32_t* tstatus, const double* radius, const int32_t* group, double sep_cap,
                                  double* first_t, int32_t* first_with, double* min_sep, int32_t* min_with, int32_t* n_conf,
                                  uint32_t* conflict);

/* ---- delay schedules for timed paths: shift table and priority greedy ------------------------------------------
 * The cheapest resolution of a conflict is to let the lower-priority path wait.  These calls answer "does p, started s ticks
 * later than q, still meet q?" for every pair and every relative delay, and read a start slot per path off the answers.
 * They only delay: nothing is re-planned.  The reference has nothing of this kind.
 *
 * Definition.  Everything is defined on the knots fp64 [P][K+1][2] that sc_traj_knots_batch writes, with tstatus, radius and
 * group as sc_traj_conflicts_batch reads them.  No new floating-point formula: the only predicate is "interval conflicts iff
 * m2 < R*R" of the block above, the same operations in the same order, fp64, no fused multiply-adds; every output is
 * integers and bits and equals the CPU statements (tests/traj_sched_twin.py in NumPy, tests/cpp/traj_sched_ref.c in C) exactly.
 *   Delays are whole ticks.  D = the number of candidate slots, 1 .. 32; stride = ticks per slot, >= 1, (D-1) * stride <= K.
 *     Path p in slot j is its knot row shifted by s = j * stride ticks, holding the tick-0 knot while it waits:
 *       knot_s[p][k] = knots[p][max(k - s, 0)],  k = 0 .. K.
 *     A path whose tick-0 knot is absent (flag bit 0 clear, not yet started) stays absent while it waits.  The horizon stays
 *     tau_K: what a shift pushes beyond it is not compared.
 *   Pair at relative shift r = j_p - j_q, r in -(D-1) .. D-1: p is shifted by max(r, 0) * stride ticks, q by max(-r, 0) *
 *     stride, and the intervals k = 0 .. K-1 are compared exactly as above (differences hi - lo with lo = min(p, q); NaN knots
 *     fail the comparison).  conf(p, q, r) is true iff some interval conflicts; conf(p, q, r) == conf(q, p, -r).
 *     A pair is not compared, and all its bits are 0, when either path is not SC_TRAJ_OK, either radius is outside the
 *     contract (such a path becomes SC_TRAJ_BAD, as in the conflicts call), both have the same group >= 0, or p == q.
 *   Table: uint64 table[P][P]; bit r + D - 1 of table[p][q] = conf(p, q, r); bits from 2D-1 up are 0; every entry is written.
 *     8 MiB at P = 1024; calls that take a table accept P in 1 .. 8192 (512 MiB).
 *   Schedule.  order int32 [P] or NULL = 0, 1, 2, ..: earlier entries have higher priority; an entry outside 0 .. P-1 or
 *     one that repeats an earlier entry is skipped.  jmax int32 [P] or NULL = D-1 everywhere; a value >= 0 is clamped to
 *     D-1, a value < 0 means pinned.  Walk order; for each path p:
 *       1. p is not OK: slot[p] = SC_SLOT_NOT_OK.
 *       2. p is pinned: slot[p] = 0 unconditionally; it still blocks the paths after it (moving obstacles, paths under way).
 *       3. otherwise busy = OR over every earlier path q with slot[q] >= 0 of (table[p][q] >> (D-1-slot[q])) & (2^D - 1),
 *          and slot[p] = the smallest j <= jmax[p] whose bit in busy is 0;
 *       4. no such j: slot[p] = SC_SLOT_UNRESOLVED; the path takes no further part and blocks nobody (the caller re-plans it).
 *     A path never named in order gets SC_SLOT_UNNAMED and blocks nobody.  counts int32 [4]: the paths with slot 0, with
 *     slot > 0, unresolved, and not scheduled (SC_SLOT_NOT_OK or SC_SLOT_UNNAMED).
 *   Shifted knots: knots_out[p][k] = knots[p][max(k - max(slot[p], 0) * stride, 0)]; a path with slot < 0 becomes all NaN
 *     (absent), so that sc_traj_conflicts_batch on knots_out gives the residual report in the existing format.
 *   Note (the tests rely on it): equivalence with absolute delays.  Suppose every path is at rest or absent from tick
 *     K - (D-1) * stride onward.  Then two paths at slots j_p, j_q conflict in the absolute picture (both rows shifted, the
 *     predicate on intervals 0 .. K-1) iff conf(p, q, j_p - j_q): the intervals the relative picture sees beyond the absolute
 *     horizon repeat the last, stationary interval, and the intervals on which both paths wait are implied by interval 0 of
 *     any relative shift (lam = 0 gives the tick-0 distance).  Under that condition on K a schedule leaves no conflict among
 *     the paths with slot >= 0.  The Python Context.fleet_schedule(K=None) chooses K to cover the longest path, its delay and
 *     (D-1) * stride more ticks.
 *   Shifting knots is not bit-equal to recomputing them with t0 + j * stride * dt_c (tau - t0 rounds differently): the
 *     definition is the shift.
 *   A pair whose boxes of present knots are at least R apart is written 0 without its ticks being read.  The gap is taken
 *     conservatively (2^-48 of the boxes' span below the exact one), so the skip changes no bit; SC_TRAJ_SCHED_NOSKIP=1 in
 *     the environment when the context is created turns it off.
 *
 * sc_traj_shift_table_batch: table from knots; tstatus is read and written like in sc_traj_conflicts_batch.
 * sc_traj_schedule_batch: slot int32 [P] and counts from a table and the tstatus the table call left.
 * sc_traj_shift_knots_batch: knots_out fp64 [P][K+1][2] (not the knots array itself) from knots and slot.
 * sc_fleet_schedule_batch: sc_traj_knots_batch, then the three; knots, tstatus and table may be NULL (context scratch: 16 * P *
 *   (K+1), 4 * P and 8 * P * P bytes), knots_out may be NULL (not wanted).
 * Device pointers; the calls only enqueue on the context's stream (kernels timed under SC_K_SMOOTH): no host synchronisation,
 * no device-to-host copy.  Scratch of the context: 32 * P bytes of boxes.  The _host forms take host pointers and return
 * SC_ERR_INVALID before any launch for a radius outside the contract (and sc_fleet_schedule_batch_host for what
 * sc_traj_knots_batch_host refuses).
 * Errors: SC_ERR_INVALID for NULL required pointers (everything but group, order, jmax and the pointers named above), P outside
 * 1 .. 8192, K outside 1 .. 65535, D outside 1 .. 32, stride < 1, (D-1) * stride > K, P * (K+1) > 2^26, and in
 * sc_fleet_schedule_batch the clock errors of sc_traj_knots_batch. */
#define SC_SLOT_UNRESOLVED (-1)
#define SC_SLOT_NOT_OK (-2)
#define SC_SLOT_UNNAMED (-3)
int sc_traj_shift_table_batch(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius,
                              const int32_t* group, int D, int stride, uint64_t* table);
int sc_traj_shift_table_batch_host(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius,
                                   const int32_t* group, int D, int stride, uint64_t* table);
int sc_traj_schedule_batch(sc_ctx* ctx, const uint64_t* table, const int32_t* tstatus, int P, int D, const int32_t* order,
                           const int32_t* jmax, int32_t* slot, int32_t* counts);
int sc_traj_schedule_batch_host(sc_ctx* ctx, const uint64_t* table, const int32_t* tstatus, int P, int D, const int32_t* order,
                                const int32_t* jmax, int32_t* slot, int32_t* counts);
int sc_traj_shift_knots_batch(sc_ctx* ctx, const double* knots, int P, int K, const int32_t* slot, int stride, double* knots_out);
int sc_traj_shift_knots_batch_host(sc_ctx* ctx, const double* knots, int P, int K, const int32_t* slot, int stride, double* knots_out);
int sc_fleet_schedule_batch(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets, const int32_t* length,
                            const int32_t* status, int P, const double* t0, const int32_t* flags, double T0, double dt_c, int K,
                            double* knots, int32_t* tstatus, const double* radius, const int32_t* group, int D, int stride,
                            uint64_t* table, const int32_t* order, const int32_t* jmax, int32_t* slot, int32_t* counts,
                            double* knots_out);
int sc_fleet_schedule_batch_host(sc_ctx* ctx, const double* time, const float* pts, const int32_t* offsets, const int32_t* length,
                                 const int32_t* status, int P, const double* t0, const int32_t* flags, double T0, double dt_c, int K,
                                 double* knots, int32_t* tstatus, const double* radius, const int32_t* group, int D, int stride,
                                 uint64_t* table, const int32_t* order, const int32_t* jmax, int32_t* slot, int32_t* counts,
                                 double* knots_out);

/* ---- robots to goals: the cost matrix of the fields and an optimal one-to-one matching -------------------------
 * sc_cost_field_batch rooted at the goals gives every robot's exact cost to every goal.  These calls take the R x F matrix out
 * of the fields and match robots to goals one to one, on the device, in the form sc_field_paths_batch accepts:
 * qfield[q] = col_of[q], to_root = 1, and an unassigned robot's -1 becomes SC_Q_BAD_ENDPOINT by the rule for an out-of-range
 * qfield.  The reference has nothing of this kind.
 *
 * Problem.  cost int32 [B][R][C], rows contiguous, 1 <= R, C <= SC_ASSIGN_MAX_DIM (1024).  An entry is valid when
 *   0 <= c < INT32_MAX; c == SC_FIELD_INF means forbidden (the goal is unreachable for that robot).  A negative entry makes
 *   that one problem SC_ASSIGN_BAD: its outputs are col_of / row_of -1 and u, v, matched, total, steps 0; the other problems
 *   of the batch are unaffected.
 * Matching.  A set of (row, column) pairs over valid, not forbidden entries, every row and every column used at most once.
 *   The result has the most pairs possible and, among those, the smallest sum of costs.
 * Padded form.  a[r][c] = cost, or SC_ASSIGN_BIG = 2^42 where forbidden.  2^42 exceeds 1024 * 2^31, so one forbidden edge
 *   outweighs any set of real ones; n * BIG <= 2^52, so everything fits int64.
 * The optimum is not unique under ties, so the library returns the result of one stated procedure: the textbook O(n^2 m)
 * shortest-augmenting-path Hungarian method on int64.
 *   If R <= C the lines are the rows and the posts the columns, otherwise the roles swap (the same procedure on the
 *   transpose).  n lines, m posts, n <= m.  Start with u[n] = 0, v[m] = 0, p[m] = none.  For line i = 0 .. n-1 in index order:
 *     minv[j] = +inf, way[j] = none, used[j] = false, i0 = i, j0 = none.
 *     Loop (each pass counts one step):
 *       for every unused j: cur = a[i0][j] - u[i0] - v[j]; if cur < minv[j] then minv[j] = cur and way[j] = j0;
 *       j1 = the unused post of smallest minv, lowest j among equals; delta = minv[j1];
 *       u[i] += delta; for every used j: u[p[j]] += delta and v[j] -= delta; for every unused j: minv[j] -= delta;
 *       used[j1] = true, j0 = j1; leave the loop if p[j0] is none, else i0 = p[j0].
 *     Augment: walk way back from j0, moving each p along (p[j0] = p[way[j0]], j0 = way[j0]); the last post gets i.
 * Outputs, in the caller's orientation whichever side was the lines:
 *   col_of int32 [B][R]  the column row r is paired with over a real edge, -1 otherwise;
 *   row_of int32 [B][C]  the inverse;
 *   u int64 [B][R], v int64 [B][C]  the duals of the rows and of the columns;
 *   info int64 [B][4] = {matched, total, steps, status}: total is the sum over real pairs, status SC_ASSIGN_OK or SC_ASSIGN_BAD.
 * Certificate (it holds for the procedure's output and proves optimality without any reference):
 *   u[r] + v[c] <= a[r][c] for all r, c;  the duals of the longer side are <= 0, and 0 on unpaired posts (a post paired over a
 *   forbidden edge reads -1 but may carry a dual: at most min(R, C) - matched of them);
 *   sum u + sum v == total + SC_ASSIGN_BIG * (min(R, C) - matched).
 * Bound on work: line i takes at most i + 1 passes, so steps <= n (n + 1) / 2 = 524 800 at 1024; the kernel's loops are
 *   bounded by it.  The kernels apply the deltas lazily (one running offset, u and v settled once per line); in integers that
 *   equals the eager form above exactly, and every output equals the CPU statements (tests/assign_twin.py in NumPy,
 *   tests/cpp/assign_ref.c in C) bit for bit, steps included.
 *
 * sc_field_cost_matrix: cost[r][f] = g[f][cell[r]], plus col_cost[f] when given (int32 [F] or NULL, 0 ..
 *   SC_FIELD_SEED_COST_MAX: a price per goal); the sum is done in int64 and clamped to INT32_MAX - 1; SC_FIELD_INF stays
 *   SC_FIELD_INF; a cell[r] out of range makes that whole row SC_FIELD_INF.  g int32 [F][H][W] is any field array: plain,
 *   weighted or multi-source.  One thread per (r, f).
 * sc_assign_batch: B problems, one workgroup each (64, 256 or 1024 threads by max(R, C); R > C: a transpose into context
 *   scratch, 4 * B * R * C bytes, comes first).  row_of, u and v may be NULL.  B == 0 is a no-op.
 * sc_fleet_assign_batch: the two calls above with B = 1 and C = F; its parameter list is the matrix call's followed by what
 *   sc_assign_batch takes after cost, B, R, C.  cost may be NULL: the matrix then lives in context scratch (4 * R * F bytes).
 * Device pointers; the calls only enqueue on the context's stream (kernels timed under SC_K_ASTAR): no host synchronisation,
 * no device-to-host copy.  The _host forms take host pointers, check the data before any launch (a g value below 0 or a
 * col_cost outside its range: SC_ERR_INVALID), copy, run, copy back and synchronise.
 * Errors: SC_ERR_INVALID for NULL cost / col_of / info (g, cell in the matrix calls), R or C (F in the combined call) outside
 *   1 .. SC_ASSIGN_MAX_DIM, B < 0, and in the matrix call F < 1, R < 1, R * F > 2^30, W or H outside 1 .. SC_MAX_DIM. */
#define SC_ASSIGN_MAX_DIM 1024
#define SC_ASSIGN_BIG (1ll << 42)
#define SC_ASSIGN_OK 0
#define SC_ASSIGN_BAD 1
int sc_field_cost_matrix(sc_ctx* ctx, const int32_t* g, int F, int W, int H, const int32_t* cell, int R, const int32_t* col_cost,
                         int32_t* cost);
int sc_field_cost_matrix_host(sc_ctx* ctx, const int32_t* g, int F, int W, int H, const int32_t* cell, int R, const int32_t* col_cost,
                              int32_t* cost);
int sc_assign_batch(sc_ctx* ctx, const int32_t* cost, int B, int R, int C, int32_t* col_of, int32_t* row_of, int64_t* u, int64_t* v,
                    int64_t* info);
int sc_assign_batch_host(sc_ctx* ctx, const int32_t* cost, int B, int R, int C, int32_t* col_of, int32_t* row_of, int64_t* u, int64_t* v,
                         int64_t* info);
int sc_fleet_assign_batch(sc_ctx* ctx, const int32_t* g, int F, int W, int H, const int32_t* cell, int R, const int32_t* col_cost,
                          int32_t* cost, int32_t* col_of, int32_t* row_of, int64_t* u, int64_t* v, int64_t* info);
int sc_fleet_assign_batch_host(sc_ctx* ctx, const int32_t* g, int F, int W, int H, const int32_t* cell, int R, const int32_t* col_cost,
                               int32_t* cost, int32_t* col_of, int32_t* row_of, int64_t* u, int64_t* v, int64_t* info);

/* ---- exploration frontiers: known space, clusters, costs, a goal per robot ----------------------------------------
 * Every planner above takes the map as known.  These calls add a planner-visible notion of "known", find the frontier --
 * the known, traversable cells that touch unknown space -- grouped into clusters, and give the robots x clusters cost matrix
 * in the form sc_assign_batch takes, so that one stream carries known -> EDT -> field per robot -> frontiers -> matrix ->
 * matching -> paths with no host hop.  The reference's counterpart is planner::pick_next_goal_point (sea_current.hpp:433-519,
 * unfinished there: no parity claim).  DESIGN.md section 22.  Everything is integer and uniquely defined; tests/frontier_twin.py
 * states it in NumPy, tests/cpp/frontier_ref.c in C, and every output equals them bit for bit.  Cells are c = y*W + x.
 *
 * sc_known_from_discs: known[c] = (base ? base[c] != 0 : 0) | exists disc: (x-cx)^2 + (y-cy)^2 <= r2, in int64, written as 0 / 1.
 *   discs int32 [R][3] = (cx, cy, r2); a disc with r2 < 0 is ignored; R == 0 copies base or clears (discs may then be NULL).
 *   base uint8 [H][W] may be NULL or alias known.  One grid, one kernel, timed as SC_K_MOVES: the sibling of sc_occ_from_rects.
 * sc_d2_known_i32: d2k[c] = known[c] ? d2[c] : 0 over [G][H][W]; d2k may alias d2.  With d2 the EDT of the observed obstacles,
 *   every planner run on d2k (A*, fields, components, space-time plans) moves through known free space only, while clearance is
 *   still measured from real obstacles, not from the edge of the unknown.  One kernel, timed as SC_K_MOVES.
 *
 * sc_frontier_batch: d2 int32 and known uint8 [G][H][W]; thr = max(r2_clear, 1).
 *   Frontier cell: Fr(c) <=> known[c] != 0 and d2[c] >= thr and some orthogonal neighbour n inside the grid has known[n] == 0.
 *     Cells outside the grid are not unknown.
 *   Cluster: an 8-connected set of frontier cells (frontier cells along a slanted boundary touch only diagonally, so the
 *     4-connected labelling of sc_components_batch would shatter them).  Its representative is its smallest cell index.
 *   label int32 [G][H][W], may be NULL: the representative of the cell's cluster, -1 where !Fr(c).
 *   Listed clusters: those of at least min_size cells, in ascending order of representative; L their number.
 *   ncl int32 [G][2] = {L, the number of all clusters}; L is reported in full even when L > Cmax.
 *   For k < min(L, Cmax): rep[g][k] the representative, csize[g][k] the cell count, cbox[g][k] = {x0, y0, x1, y1} inclusive
 *     (int32 [G][Cmax][4], may be NULL), csum[g][k] = {sum x, sum y} (int64 [G][Cmax][2], may be NULL: the caller's centroid).
 *     Rows k >= min(L, Cmax) read -1 / 0 / zeros.  rep and csize are int32 [G][Cmax].
 *   slot int32 [G][H][W], may be NULL: the column k of the cell's cluster, -1 where the cell is no frontier cell or its
 *     cluster is not listed (too small, or beyond Cmax).
 *   1 <= Cmax <= SC_FRONTIER_MAX_CLUSTERS, min_size >= 1.
 *   Only enqueues: at most eight kernels whatever the map (one wavefront per 64 x 64 tile labels it in registers, a lock-free
 *   union across tile edges, a flatten, a two-level count and scan for the ranks), no workgroup waits for another, integer
 *   atomics only, every output independent of execution order.  Timed as SC_K_MOVES.  Scratch: G * W * H * 4 B (8 B when
 *   label is NULL) + G * ceil(W * H / 256) * 4 B; grows only.
 *
 * sc_frontier_cost_matrix: g int32 [F][H][W] is any field array (plain, weighted, multi-source) rooted at the robots and
 *   computed on d2k; field f lives on grid fgrid[f] (int32 [F]; NULL only with G == 1; out of range: the whole row
 *   SC_FIELD_INF / -1).  slot and csize are what sc_frontier_batch wrote with the same G, W, H, Cmax.  For column k:
 *   m = min g[f][c] over the cells of f's grid with slot == k.  No such cell, or m == SC_FIELD_INF: cost[f][k] = SC_FIELD_INF
 *   and cell[f][k] = -1.  Otherwise cell[f][k] = the smallest c attaining m and
 *   cost[f][k] = min(m + gain * (size_cap - min(csize[k], size_cap)), INT32_MAX - 1), in int64.
 *   gain == 0 is the nearest-frontier rule; gain > 0 prefers large clusters and keeps the costs non-negative, as
 *   sc_assign_batch requires.  cost and cell are int32 [F][Cmax]: sc_assign_batch's layout with B = 1, R = F, C = Cmax.
 *   Three launches (key fill, 64-bit atomicMin of g << 32 | c per frontier cell and field, read-out), timed as SC_K_ASTAR.
 *   Scratch: F * Cmax * 8 B.
 *
 * sc_fleet_explore_batch: one grid; sc_frontier_batch -> the matrix (robot r = field r) -> sc_assign_batch -> per robot
 *   goal[r] = cell[r][col_of[r]], or -1 when unmatched; gcost[r] = g[r][goal[r]], or -1.  Matched robots get pairwise
 *   different clusters.  label, slot, ncl, rep, csize, cbox, csum, cost, cell, col_of, row_of (int32 [Cmax]) and info
 *   (int64 [4], sc_assign_batch's) may each be NULL: what the chain needs of them then lives in context scratch.
 *   sc_field_paths_batch(..., qfield = r, target = goal[r], to_root = 0) then yields the paths; a -1 target reads
 *   SC_Q_BAD_ENDPOINT by the existing rule.  Timed as its parts.
 *
 * Device pointers; the calls only enqueue on the context's stream.  The _host forms take host pointers, check the data
 * before any launch (a g value below 0: SC_ERR_INVALID), copy, run, copy back and synchronise.
 * Errors: SC_ERR_INVALID for NULL mandatory pointers (everything not called optional above), W or H outside 1..SC_MAX_DIM,
 *   G <= 0, R < 0, F < 1, min_size < 1, Cmax outside 1..SC_FRONTIER_MAX_CLUSTERS (1..SC_ASSIGN_MAX_DIM, like F, in
 *   sc_fleet_explore_batch), F * Cmax > 2^30, gain < 0, size_cap < 0, gain * size_cap > 2^30, fgrid NULL with G > 1. */
#define SC_FRONTIER_MAX_CLUSTERS 65536
int sc_known_from_discs(sc_ctx* ctx, const uint8_t* base, const int32_t* discs, int R, int W, int H, uint8_t* known);
int sc_known_from_discs_host(sc_ctx* ctx, const uint8_t* base, const int32_t* discs, int R, int W, int H, uint8_t* known);
int sc_d2_known_i32(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int G, int W, int H, int32_t* d2k);
int sc_d2_known_i32_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int G, int W, int H, int32_t* d2k);
int sc_frontier_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int G, int W, int H, int32_t r2_clear, int min_size, int Cmax,
                      int32_t* label, int32_t* slot, int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox, int64_t* csum);
int sc_frontier_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int G, int W, int H, int32_t r2_clear, int min_size,
                           int Cmax, int32_t* label, int32_t* slot, int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox,
                           int64_t* csum);
int sc_frontier_cost_matrix(sc_ctx* ctx, const int32_t* g, int F, const int32_t* fgrid, const int32_t* slot, const int32_t* csize, int G,
                            int W, int H, int Cmax, int32_t gain, int32_t size_cap, int32_t* cost, int32_t* cell);
int sc_frontier_cost_matrix_host(sc_ctx* ctx, const int32_t* g, int F, const int32_t* fgrid, const int32_t* slot, const int32_t* csize,
                                 int G, int W, int H, int Cmax, int32_t gain, int32_t size_cap, int32_t* cost, int32_t* cell);
int sc_fleet_explore_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size, int Cmax,
                           const int32_t* g, int F, int32_t gain, int32_t size_cap, int32_t* label, int32_t* slot, int32_t* ncl,
                           int32_t* rep, int32_t* csize, int32_t* cbox, int64_t* csum, int32_t* cost, int32_t* cell, int32_t* col_of,
                           int32_t* row_of, int64_t* info, int32_t* goal, int32_t* gcost);
int sc_fleet_explore_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size,
                                int Cmax, const int32_t* g, int F, int32_t gain, int32_t size_cap, int32_t* label, int32_t* slot,
                                int32_t* ncl, int32_t* rep, int32_t* csize, int32_t* cbox, int64_t* csum, int32_t* cost, int32_t* cell,
                                int32_t* col_of, int32_t* row_of, int64_t* info, int32_t* goal, int32_t* gcost);

/* ---- line-of-sight sensing: known space that walls block, and what a pose would reveal ---------------------------
 * sc_known_from_discs marks a cell known when it lies in a sensing disc, whatever stands between it and the sensor.  These
 * calls cast one ray per (view, cell of the view's box) instead.  The reference has no counterpart (no parity claim); the
 * definitions are integer and unique; tests/views_twin.py states them in NumPy, tests/cpp/views_ref.c in C, and every output
 * equals both bit for bit.  DESIGN.md section 23.  Cells are c = y*W + x.
 *
 * Inputs.  occ uint8 [H][W]: the map the sensor meets (in a simulation the true map, for a prediction the observed one).
 *   views int32 [R][3] = (cx, cy, r2), the layout of discs.  A view with r2 < 0, or with its centre outside the grid, is
 *   ignored.
 * Clear(a, b): sc_path_waypoints_batch's Visible(a, b) with the cell test occ == 0 in place of T: every cell whose closed unit
 *   square meets the closed segment between the centres of a and b has occ = 0 (the supercover, a and b included; a ray
 *   through a cell corner needs both side cells: A*'s no-corner-cutting rule).  Integer tests in doubled coordinates, exact
 *   for every grid the library accepts.
 * Seen free cell.  vis[c] <=> exists view v: (x-cx)^2 + (y-cy)^2 <= r2 (int64) and Clear(v, c).  vis[c] implies occ[c] = 0;
 *   a view standing on an occupied cell sees nothing.
 * Seen surface.  surf[c] <=> occ[c] != 0 and an orthogonal neighbour n inside the grid has vis[n]: the face of a wall that
 *   bounds the seen free space is observed at any angle (a centre-to-centre ray reaches a wall cell only within 45 degrees of
 *   its normal, and every free cell along a wall seen obliquely would be a spurious frontier cell).  A surface cell may lie
 *   one cell outside the disc.
 *
 * sc_known_from_views: known[c] = (base ? base[c] != 0 : 0) | vis[c] | surf[c], written as 0 / 1; vis and surf come from
 *   this call's views only; nothing depends on the order of the views or of execution.  occ_seen[c] = known[c] ? occ[c] : 0
 *   (may be NULL): the map the EDT of the observed obstacles takes.  base may be NULL or known itself; occ_seen must be
 *   neither occ nor known.  R == 0 copies base or clears (views may then be NULL).  A memset, one ray kernel per 65535 views
 *   and one kernel per cell, timed as SC_K_MOVES.  Scratch: W * H bytes; grows only.
 *   Consequences: with occ == 0 everywhere and all centres in the grid, known equals sc_known_from_discs of the same rows;
 *   vis lies inside the discs and known \ base inside the discs dilated by one orthogonal step; from a frontier cell with
 *   r2 >= 1 a view reveals the unknown orthogonal neighbour (free: Clear at distance 1; occupied: surface).
 * sc_view_gain_batch: gain[i] = #{c : known[c] == 0 and vis_i[c]} (int32 [N]) for view i alone; 0 for an ignored view.
 *   With occ the observed map (unknown cells read 0) it predicts what pose i would reveal; with occ the true map it is
 *   exactly the number of free cells sc_known_from_views(known, occ, view i) newly marks.  N == 0 is a no-op.  A memset and
 *   one kernel per 65535 candidates (one integer atomicAdd per wavefront), timed as SC_K_MOVES.
 *
 * Device pointers; the calls only enqueue on the context's stream.  The _host forms take host pointers, copy, run, copy back
 * and synchronise.  Errors: SC_ERR_INVALID for NULL mandatory pointers, R < 0, N < 0, W or H outside 1..SC_MAX_DIM, occ_seen
 * equal to occ or to known. */
int sc_known_from_views(sc_ctx* ctx, const uint8_t* base, const uint8_t* occ, const int32_t* views, int R, int W, int H, uint8_t* known,
                        uint8_t* occ_seen);
int sc_known_from_views_host(sc_ctx* ctx, const uint8_t* base, const uint8_t* occ, const int32_t* views, int R, int W, int H,
                             uint8_t* known, uint8_t* occ_seen);
int sc_view_gain_batch(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H, int32_t* gain);
int sc_view_gain_batch_host(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H,
                            int32_t* gain);

/* ---- sensors with a field of view: sector views and the gain of every heading --------------------------------------
 * The calls above see a full circle.  These give a view a sector, tell for a candidate pose what every heading would reveal
 * at the cost of one pass of rays, and turn goal cells into view rows on the stream.  The reference has no counterpart (no
 * parity claim); the definitions are integer and unique; tests/sectors_twin.py states them in NumPy, tests/cpp/sectors_ref.c
 * in C, and every output equals both bit for bit.  DESIGN.md section 27.  Cells are c = y*W + x.  cross(p, q) = px*qy - py*qx,
 * dot is the usual; d is a cell's offset from the view's centre.
 *
 * Half-open sector In(d; a, b): the sector counter-clockwise from direction a (inclusive) to direction b (exclusive).  a and b
 *   are int32 pairs whose components lie in -32767 .. 32767.
 *   d = (0, 0): true.  The centre belongs to every sector.
 *   a = b = (0, 0): true.  This is the full circle.
 *   Otherwise let s = cross(a, b):
 *     s > 0: cross(a, d) >= 0 and cross(d, b) > 0.
 *     s < 0 (more than half a turn): not (cross(b, d) >= 0 and cross(d, a) > 0).
 *     s = 0 and dot(a, b) < 0 (exactly half a turn): cross(a, d) > 0 or (cross(a, d) = 0 and dot(a, d) > 0).
 *     s = 0 and dot(a, b) > 0, exactly one of a, b zero, or a component out of range: the view is IGNORED.  It sees nothing
 *       and its gain is 0, like r2 < 0.
 *   With W, H <= SC_MAX_DIM every product is below 2^30, so int32 suffices in the kernel; the twin and the C statement use
 *   int64.
 * Sector view.  sviews int32 [R][7] = (cx, cy, r2, ax, ay, bx, by).  vis[c] and surf[c] are the section above's, with
 *   "and In(c - centre; a, b)" added to the disc test of vis.  The surf rule is unchanged: an occupied cell with a seen
 *   orthogonal neighbour, which may lie just outside the sector as it may lie outside the disc.  A row with a = b = 0 is
 *   exactly the view (cx, cy, r2).
 * Heading table.  dirs int32 [B][2], a HOST pointer in both call forms (a small parameter table, validated before any launch
 *   and handed to the kernel as an argument).  It is valid iff 3 <= B <= SC_VIEW_MAX_BINS; every component lies in
 *   -32767 .. 32767; cross(u_b, u_{(b+1) mod B}) > 0 for every b; and exactly one b has u_b in the upper half-open plane
 *   (y > 0 or (y = 0 and x > 0)) and its successor not in it (one turn, not several).  Bin b is In(d; u_b, u_{b+1}) for d != 0.
 *   The bins of a valid table partition the offsets; the centre is in no bin.
 * Gain per heading.  For view i = (cx, cy, r2):
 *   hist[i][b] = #{c != centre : known[c] = 0 and vis_i[c] and bin(c - centre) = b},
 *   c0[i] = [known[centre] = 0 and vis_i[centre]],
 *   gainh[i][h] = c0[i] + sum over j < span of hist[i][(h + j) mod B], 1 <= span <= B,
 *   best[i] = (max over h of gainh[i][h], the smallest h attaining it).  An ignored view gives zeros and best = (0, 0).
 *   Identities: sum_b hist[i][b] + c0[i] = sc_view_gain_batch's gain[i]; for span < B, gainh[i][h] is the sector gain of
 *   (cx, cy, r2, u_h, u_{(h+span) mod B}); at span = B it is gain[i].
 *
 * sc_known_from_sectors: sc_known_from_views over sector rows; the aliasing and the R == 0 rule are that call's.  A memset,
 *   one ray kernel per 65535 rows and one kernel per cell, timed as SC_K_MOVES.  Scratch: W * H bytes (shared with
 *   sc_known_from_views); grows only.
 * sc_sector_gain_batch: gain[i] = #{c : known[c] == 0 and vis_i[c]} (int32 [N]) for sector row i alone; 0 for an ignored row.
 *   N == 0 is a no-op.
 * sc_view_gain_headings_batch: views int32 [N][3]; best int32 [N][2], mandatory; hist and gainh int32 [N][B], each may be
 *   NULL (hist then lives in context scratch, which only grows: 4 N (B + 1) bytes).  N == 0 is a no-op.  Two memsets, one ray
 *   kernel per 65535 candidates (integer atomicAdds only; nothing depends on the order of execution) and one kernel with a
 *   wavefront per candidate, timed as SC_K_MOVES.
 * sc_views_from_cells: views[i] = (cell[i] % W, cell[i] / W, r2) (cell int32 [N], views int32 [N][3]); a cell outside
 *   0 .. W*H - 1 gives (0, 0, -1), an ignored view: this covers the -1 of sc_fleet_explore_batch's unmatched robot, so its
 *   goal feeds the gain calls with no host hop.  N == 0 is a no-op.
 *
 * Device pointers, except dirs; the calls only enqueue on the context's stream.  The _host forms take host pointers, copy,
 * run, copy back and synchronise.  Errors: SC_ERR_INVALID for NULL mandatory pointers (best included), R < 0, N < 0, W or H
 * outside 1..SC_MAX_DIM, occ_seen equal to occ or to known, a dirs table that is not valid, span outside 1 .. B,
 * N * B > 2^30. */
#define SC_VIEW_MAX_BINS 64
int sc_known_from_sectors(sc_ctx* ctx, const uint8_t* base, const uint8_t* occ, const int32_t* sviews, int R, int W, int H, uint8_t* known,
                          uint8_t* occ_seen);
int sc_known_from_sectors_host(sc_ctx* ctx, const uint8_t* base, const uint8_t* occ, const int32_t* sviews, int R, int W, int H,
                               uint8_t* known, uint8_t* occ_seen);
int sc_sector_gain_batch(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* sviews, int N, int W, int H, int32_t* gain);
int sc_sector_gain_batch_host(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* sviews, int N, int W, int H,
                              int32_t* gain);
int sc_view_gain_headings_batch(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H,
                                const int32_t* dirs, int B, int span, int32_t* hist, int32_t* gainh, int32_t* best);
int sc_view_gain_headings_batch_host(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* views, int N, int W, int H,
                                     const int32_t* dirs, int B, int span, int32_t* hist, int32_t* gainh, int32_t* best);
int sc_views_from_cells(sc_ctx* ctx, const int32_t* cell, int N, int W, int H, int32_t r2, int32_t* views);
int sc_views_from_cells_host(sc_ctx* ctx, const int32_t* cell, int N, int W, int H, int32_t r2, int32_t* views);

/* ---- coordinated exploration goals: greedy picks by what each view reveals -----------------------------------------
 * sc_fleet_explore_batch matches robots to clusters on travel cost and cluster size.  These calls pick (robot, candidate)
 * pairs greedily by utility = weighted gain of the candidate's view minus weighted travel cost, and discount every other
 * candidate by the cells a pick has claimed (coordinated next-best-view selection, Burgard et al. / Simmons et al.), all on
 * the stream.  The reference has no counterpart (no parity claim); the definitions are integer and unique;
 * tests/explore_gain_twin.py states them in NumPy, tests/cpp/explore_gain_ref.c in C, and every output equals both bit for
 * bit.  DESIGN.md section 29.  Cells are c = y*W + x.  vis, surf, Clear, In, heading tables, hist, c0 and gainh are those of
 * the two sections above.
 *
 * sc_explore_gain_batch.
 *   Inputs.  occ uint8 [H][W]: the map the prediction meets (the observed map, unknown cells reading 0).  known uint8 [H][W].
 *     g int32 [R][H][W]: fields rooted at the robots (any field array, as for sc_frontier_cost_matrix).  cand int32 [N]:
 *     candidate cells; a candidate is DEAD when its cell lies outside 0 .. W*H - 1 or stands on occ != 0: its gain is 0 and it
 *     is never picked.  r2 >= 0: the sensing radius squared.  dirs (a HOST pointer, int32 [B][2]) and span: dirs == NULL is the
 *     full circle (B and span ignored); otherwise a valid heading table and 1 <= span < B.  Weights wg, wc in 0 .. 2^20;
 *     min_gain >= 0; rounds in 0 .. SC_ASSIGN_MAX_DIM, the cap on picks.
 *   State.  kw = known (a working copy in context scratch, or known_out when given); all robots free, all candidates untaken.
 *   Gain of candidate n against kw.  Full circle: gain[n] = #{c : kw[c] == 0 and vis_n[c]} for the view (cand x, cand y, r2),
 *     its heading -1.  With a table: (gain[n], heading[n]) = best of the view against kw (the largest gainh[n][h], the smallest
 *     h attaining it).
 *   Round t = 0, 1, ... while t < min(rounds, R, N).  A pair (r, n) is eligible when r is free, n is alive and untaken,
 *     g[r][cand[n]] != SC_FIELD_INF and gain[n] >= min_gain.  No eligible pair: stop.  Otherwise take the eligible pair of
 *     largest score = wg * gain[n] - wc * g[r][cand[n]] (int64); ties go to the smallest r, then the smallest n.  Record
 *     goal[r] = cand[n], cand_of[r] = n, gcost[r] = g[r][cand[n]], ggain[r] = gain[n], head[r] = heading[n], pick[r] = t; mark
 *     r assigned and n taken; kw = sc_known_from_views(base = kw, occ, that one view) -- with a table sc_known_from_sectors
 *     of the row (cx, cy, r2, u_h, u_{(h + span) mod B}) -- so both vis and surf cells become known; recompute every gain.
 *   Outputs (int32).  goal [R], gcost [R], npick [1] (the number of picks): mandatory.  ggain, head, cand_of, pick [R];
 *     gain0, gain_end [N] (the gains before the first round and after the last); known_out uint8 [H][W] (the final kw; 0 / 1
 *     once a pick was made, a copy of known otherwise; must not be occ, may be known): each may be NULL.  Unpicked robots read
 *     -1, their ggain 0.  N == 0 writes those and returns.
 *   How it runs.  The call only enqueues a fixed sequence of min(rounds, R, N) rounds; the host reads nothing in between.
 *     Before the rounds the gains come from sc_view_gain_batch's / sc_view_gain_headings_batch's kernels.  A round is a
 *     two-stage reduction over the R * N pairs on the total order (score, r, n) that stores the chosen row on the device; the
 *     ray kernel of that row (vis_new); a delta pass over (tile of the chosen box, candidate) that walks a ray from the
 *     candidate only to cells with vis_new and kw == 0 inside its disc and subtracts the count from gain[n] (with a table from
 *     hist[n][bin] and c0[n], after which a wavefront per candidate re-derives best); and the combination of vis_new into kw.
 *     When no pair is eligible a done word is set and every kernel of the later rounds leaves on reading it.  No workgroup
 *     waits for another, integer atomics only, no output depends on the order of execution.  Timed as SC_K_MOVES (its parts).
 *   Scratch (grows only): 64 B of state + W*H B for kw when known_out is NULL + 2 W*H B for vis_new (two buffers take turns, so
 *     that no round needs a memset) + 12 N B of views + 4 N (B + 3) B for best, hist and c0 (8 N B full circle) + 4 (R + N) B of
 *     marks + 4 R N B of gathered costs + 4 KiB of partial results.
 *
 * sc_frontier_centres: a candidate that does not depend on the robot.  slot int32 [G][H][W], csize int32 [G][Cmax], csum int64
 *   [G][Cmax][2] as sc_frontier_batch wrote them.  centre[g][k] (int32 [G][Cmax]) = the cell of listed cluster k of grid g that
 *   minimises |csize * x - sumx| + |csize * y - sumy| (int64); ties go to the smallest cell index; rows k >= min(L, Cmax) read
 *   -1.  Two passes (key and cell do not fit one 64-bit word): a 64-bit atomicMin of the key, then an atomicMin of the cell
 *   among those attaining it.  Two memsets and three kernels, timed as SC_K_MOVES.  Scratch: G * Cmax * 8 B.
 *
 * sc_fleet_explore_gain_batch: one grid; sc_frontier_batch -> sc_frontier_centres -> sc_explore_gain_batch with cand = centre,
 *   N = Cmax (rows beyond L are -1, hence dead).  label, slot, ncl, rep, csize, cbox, csum and centre may each be NULL: what
 *   the chain needs of them then lives in context scratch.  goal is what sc_field_paths_batch takes as targets (a -1 target
 *   reads SC_Q_BAD_ENDPOINT by the existing rule).  Timed as its parts.
 *
 * Device pointers, except dirs; the calls only enqueue on the context's stream.  The _host forms take host pointers, check the
 * data before any launch (a g value below 0: SC_ERR_INVALID), copy, run, copy back and synchronise.
 * Errors: SC_ERR_INVALID for NULL mandatory pointers, W or H outside 1..SC_MAX_DIM, R outside 1..SC_ASSIGN_MAX_DIM, N (Cmax)
 *   outside 0..SC_FRONTIER_MAX_CLUSTERS (1.. for Cmax), R * N > 2^26, r2 < 0, wg or wc outside 0..2^20, min_gain < 0, rounds
 *   outside 0..SC_ASSIGN_MAX_DIM, a dirs table that is not valid, span outside 1 .. B - 1, known_out equal to occ, G <= 0,
 *   min_size < 1. */
int sc_explore_gain_batch(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* g, int R, const int32_t* cand, int N, int W,
                          int H, int32_t r2, const int32_t* dirs, int B, int span, int32_t wg, int32_t wc, int32_t min_gain, int rounds,
                          int32_t* goal, int32_t* gcost, int32_t* ggain, int32_t* head, int32_t* cand_of, int32_t* pick, int32_t* npick,
                          int32_t* gain0, int32_t* gain_end, uint8_t* known_out);
int sc_explore_gain_batch_host(sc_ctx* ctx, const uint8_t* occ, const uint8_t* known, const int32_t* g, int R, const int32_t* cand, int N,
                               int W, int H, int32_t r2, const int32_t* dirs, int B, int span, int32_t wg, int32_t wc, int32_t min_gain,
                               int rounds, int32_t* goal, int32_t* gcost, int32_t* ggain, int32_t* head, int32_t* cand_of, int32_t* pick,
                               int32_t* npick, int32_t* gain0, int32_t* gain_end, uint8_t* known_out);
int sc_frontier_centres(sc_ctx* ctx, const int32_t* slot, const int32_t* csize, const int64_t* csum, int G, int W, int H, int Cmax,
                        int32_t* centre);
int sc_frontier_centres_host(sc_ctx* ctx, const int32_t* slot, const int32_t* csize, const int64_t* csum, int G, int W, int H, int Cmax,
                             int32_t* centre);
int sc_fleet_explore_gain_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size, int Cmax,
                                const uint8_t* occ, const int32_t* g, int R, int32_t r2, const int32_t* dirs, int B, int span, int32_t wg,
                                int32_t wc, int32_t min_gain, int rounds, int32_t* label, int32_t* slot, int32_t* ncl, int32_t* rep,
                                int32_t* csize, int32_t* cbox, int64_t* csum, int32_t* centre, int32_t* goal, int32_t* gcost, int32_t* ggain,
                                int32_t* head, int32_t* cand_of, int32_t* pick, int32_t* npick, int32_t* gain0, int32_t* gain_end,
                                uint8_t* known_out);
int sc_fleet_explore_gain_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, int W, int H, int32_t r2_clear, int min_size,
                                     int Cmax, const uint8_t* occ, const int32_t* g, int R, int32_t r2, const int32_t* dirs, int B, int span,
                                     int32_t wg, int32_t wc, int32_t min_gain, int rounds, int32_t* label, int32_t* slot, int32_t* ncl,
                                     int32_t* rep, int32_t* csize, int32_t* cbox, int64_t* csum, int32_t* centre, int32_t* goal,
                                     int32_t* gcost, int32_t* ggain, int32_t* head, int32_t* cand_of, int32_t* pick, int32_t* npick,
                                     int32_t* gain0, int32_t* gain_end, uint8_t* known_out);

/* ---- planning in poses: heading fields with turn costs and oriented footprints --------------------------------------
 * The planners above plan for a disc without a heading: a state is a cell, turning is free, a goal carries no orientation.
 * These calls plan over poses (cell, heading): a per-heading collision mask of a rectangular body, exact cost fields over
 * the 8 W H poses with a price for turning and for reversing, and their read-out.  The reference has no counterpart (no parity
 * claim); the definitions are integer and unique; tests/pose_twin.py states them in NumPy, tests/cpp/pose_ref.c in C, and
 * every output equals both bit for bit.  DESIGN.md section 28.  Cells are c = y*W + x.
 *
 * Headings.  There are SC_POSE_HEADINGS = 8, counter-clockwise in (x, y): hx = {1,1,0,-1,-1,-1,0,1}, hy = {0,1,1,1,0,-1,-1,-1}.
 *   Heading k is A*'s move index {0,4,2,5,1,7,3,6}[k].  w_k is 10 for even k and 14 for odd k.
 *   T(c) <=> d2[c] >= max(r2_clear, 1) as everywhere.
 * Footprint mask (sc_footprint_mask_u8).  hmask is uint8 [batch][H][W].  The body is a rectangle in the robot's frame.  Its
 *   extents are whole cells, 0 <= front, back, left, right <= SC_FOOTPRINT_MAX = 32, with left counter-clockwise of the
 *   heading.  The rectangle is inflated by the disc that r2_clear already stands for.  Let n = hx^2 + hy^2,
 *   u = dx*hx + dy*hy and v = -dx*hy + dy*hx.  Offset (dx, dy) is covered at heading k iff both of these hold:
 *     u >= 0 ? u^2 <= n*front^2 : u^2 <= n*back^2
 *     v >= 0 ? v^2 <= n*left^2 : v^2 <= n*right^2
 *   In words, the cell's centre lies in the closed rectangle, decided exactly for the diagonals.
 *   Bit k of hmask[c] is set iff T(c + o) holds for every covered offset o that lands in the grid.  Offsets outside the
 *   grid are free, as the disc's are today.  Anchor: with all four extents 0, hmask[c] = T(c) ? 0xFF : 0.
 *   Not modelled: cells partly covered whose centre is outside, and the corners' sweep during a 45 degree turn.  The caller
 *   pads the extents.
 * Pose graph.  Pose (c, k) is valid iff T(c) and (hmask == NULL or bit k of hmask[c]).  Edges out of (c, k):
 *   Forward to (c + h_k, k), cost w_k.  It is legal iff A*'s move c -> c + h_k is legal and both poses are valid.  A*'s
 *     rule means in grid, both cells T, and for a diagonal both side cells T.
 *   Reverse to (c - h_k, k), cost w_k + rev_cost, with the same legality.  It exists only when rev_cost >= 0.
 *     rev_cost = -1 means no reversing, and other negative values are SC_ERR_INVALID.
 *   Turn on the spot to (c, k +- 1 mod 8), cost turn_cost >= 0.  It is legal iff both poses are valid.
 *   No arc moves (forward while turning) and no costmap.
 * Field (sc_pose_field_batch).  gp is int32 [F][8][H][W].  With toward = 0, gp[f][k][c] is the exact optimal cost from the
 *   root pose to (c, k).  It is SC_FIELD_INF where (c, k) is invalid or unreachable.  rhead[f] in 0..7 seeds that pose at
 *   0.  rhead[f] = -1 seeds every valid heading of the root cell at 0.  The whole field is SC_FIELD_INF with status
 *   SC_Q_BAD_ENDPOINT in four cases: the root cell is out of range; the root pose is invalid (for -1: no valid heading);
 *   rhead is outside -1..7; fgrid is out of range.
 *   toward = 1 gives the cost from (c, k) to the root pose.  It is needed because reversing makes the graph asymmetric.  By
 *   definition it is the toward = 0 field of root heading rhead + 4 with its layers renamed k -> k + 4 (and the bits of
 *   hmask renamed with them: layer j of the renamed search is valid where bit j + 4 is set).  Transposing the graph swaps
 *   the roles of forward and reverse, which is what negating every heading vector does.  The twin checks this identity
 *   against a Dijkstra on the transposed graph.
 *   Before any launch or allocation, SC_ERR_INVALID unless 0 <= turn_cost <= 255, -1 <= rev_cost <= 255 and, in 64 bits,
 *   max(14 + max(rev_cost, 0), turn_cost) * (8*W*H - 1) <= INT32_MAX - 1.  An optimal path visits every state at most once.
 * Read-out (sc_pose_paths_batch).  turn_cost = 0 is SC_ERR_INVALID here: zero-cost turn cycles have no unique walk.  The
 *   field call accepts 0.  thead[q] in 0..7, or -1 for the cheapest heading at the target, smallest k on a tie (k as the
 *   caller numbers the layers of gp).  The walk goes from the target pose back to a seeded state, on the toward = 0
 *   numbering.  For a toward field, rename as above and rename the written headings back.  From (c, k) with
 *   v = gp[k][c] > 0 or not a seed, take the first candidate whose edge is legal and whose gp + edge cost == v:
 *     1. The forward predecessor (c - h_k, k).
 *     2. The reverse predecessor (c + h_k, k), only if rev_cost >= 0.
 *     3. The turn from k - 1.
 *     4. The turn from k + 1.
 *   Every edge is positive, so g falls strictly and the walk ends.  Legality is read from d2 and hmask, not inferred from g.
 *   One entry per state is written: path int32 [Q][Lmax] cells and head uint8 [Q][Lmax].  to_root = 0 writes root..target
 *   and to_root = 1 writes target..root.  For a toward field, to_root = 1 is the driving order.
 *   cells_only = 1 drops every entry whose cell equals the previous written entry's cell.  The first state of each cell (in
 *   the order written) stays.  path is then an 8-connected cell path that sc_path_waypoints_batch takes.  len counts what is
 *   written.
 *   Statuses, len, cost and truncation past Lmax follow sc_field_paths_batch: SC_Q_OK; SC_Q_BAD_ENDPOINT (qfield, the field's
 *   grid, its root cell or rhead out of range, the root pose or the target pose invalid, thead outside -1..7, thead = -1 on
 *   a target cell that is not T), len 0 and cost -1; SC_Q_NO_PATH (gp at the target pose is SC_FIELD_INF, or no candidate
 *   matches: gp is not the field of these arguments), len 0 and cost -1; SC_Q_TRUNCATED with len = the needed count and the
 *   cost (path and head unspecified).
 * Device pointers; the calls only enqueue on the context's stream, so sc_edt_u8_i32 -> sc_footprint_mask_u8 ->
 * sc_pose_field_batch -> sc_pose_paths_batch -> sc_path_waypoints_batch runs with one synchronise.  hmask of the pose calls is
 * uint8 [G][H][W] or NULL.  rounds: chip-wide relaxation launches before the per-field finisher; the result is identical for
 * every value; rounds < 0 = the library default 4 * (ceil(W/32) + ceil(H/32)) + 16.  Errors: SC_ERR_INVALID for NULL mandatory
 * pointers (hmask, fgrid with G == 1 and fstatus may be NULL), W or H outside 1..SC_MAX_DIM, batch, G, F <= 0, Q < 0
 * (Q == 0 is a no-op), Lmax <= 0, an extent outside 0..SC_FOOTPRINT_MAX, and the cost rules above.  The _host forms take host
 * pointers, check the data (sc_pose_paths_batch_host: every gp value >= 0), copy, run, copy back and synchronise.  Scratch
 * grows only: the mask keeps two summed-area tables of one grid, 4 (W+1) (H+1) + 4 (W+H)^2 bytes; the field about 12 B per
 * (field, 32 x 32 tile).  The field and the read-out are timed as SC_K_ASTAR, the mask as SC_K_MOVES. */
#define SC_POSE_HEADINGS 8
#define SC_FOOTPRINT_MAX 32
int sc_footprint_mask_u8(sc_ctx* ctx, const int32_t* d2, int W, int H, int batch, int32_t r2_clear, int front, int back, int left,
                         int right, uint8_t* hmask);
int sc_footprint_mask_u8_host(sc_ctx* ctx, const int32_t* d2, int W, int H, int batch, int32_t r2_clear, int front, int back, int left,
                              int right, uint8_t* hmask);
int sc_pose_field_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int G, const int32_t* fgrid, int W, int H,
                        int32_t r2_clear, int turn_cost, int rev_cost, int toward, const int32_t* root, const int32_t* rhead, int F,
                        int rounds, int32_t* gp, int32_t* fstatus);
int sc_pose_field_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int G, const int32_t* fgrid, int W, int H,
                             int32_t r2_clear, int turn_cost, int rev_cost, int toward, const int32_t* root, const int32_t* rhead,
                             int F, int rounds, int32_t* gp, int32_t* fstatus);
int sc_pose_paths_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int G, const int32_t* fgrid, int W, int H,
                        int32_t r2_clear, int turn_cost, int rev_cost, int toward, const int32_t* gp, const int32_t* root,
                        const int32_t* rhead, int F, const int32_t* qfield, const int32_t* target, const int32_t* thead, int Q, int Lmax,
                        int to_root, int cells_only, int32_t* path, uint8_t* head, int32_t* len, int32_t* cost, int32_t* status);
int sc_pose_paths_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int G, const int32_t* fgrid, int W, int H,
                             int32_t r2_clear, int turn_cost, int rev_cost, int toward, const int32_t* gp, const int32_t* root,
                             const int32_t* rhead, int F, const int32_t* qfield, const int32_t* target, const int32_t* thead, int Q,
                             int Lmax, int to_root, int cells_only, int32_t* path, uint8_t* head, int32_t* len, int32_t* cost,
                             int32_t* status);

/* ---- occupancy from range scans: beam casts and log-odds maps ------------------------------------------------------
 * The calls above take the map to be sensed and hand back a mask.  These two take measurements: a beam has an origin, an end
 * and either the cell where it stopped or no return.  sc_scan_cast_batch is the simulated range sensor (it casts beams through
 * a true map), sc_logodds_update the standard occupancy-grid update from beams: free along the beam, occupied at its end, as
 * clamped integer log-odds that accumulate over calls and can take a cell back.  The reference has no counterpart (no parity
 * claim); the definitions are integer and unique; tests/scan_twin.py states them in NumPy, tests/cpp/scan_ref.c in C, and
 * every output equals both bit for bit.  DESIGN.md section 24.  Cells are c = y*W + x.
 *
 * Walk(a, b): the supercover of the segment between the centres of cells a and b (every cell whose closed unit square meets
 *   the closed segment; a ray through a cell corner touches both side cells) as a SEQUENCE: column i = 0 .. D of the major
 *   axis (D = max(|dx|, |dy|), m = min(|dx|, |dy|), the x axis is the major one when |dx| >= |dy|), and inside a column the
 *   rows rlo(i) .. rhi(i) counted away from a,
 *     rhi(i) = min(floor(((2i+1) m + D) / 2D), m),   rlo(i) = ceil(((2i-1) m - D) / 2D) for i >= 1, 0 for i = 0.
 *   a = b is the one cell a.  a lies inside the grid; b may lie outside: the sequence ends before its first cell outside the
 *   grid (the segment leaves the grid once; a cell inside the grid that the segment only touches at a corner after that
 *   point is not part of the walk).  At an exact corner crossing the cell on the near column (the larger row of column i)
 *   comes before the cell of the next column.
 * Rays int32 [N][4] = (ax, ay, bx, by), aligned as int32 (no more is needed).  A ray is IGNORED when a lies outside the
 *   grid or |bx - ax| or |by - ay| exceeds SC_SCAN_MAX_REACH (then (2D+1) m + D < 2^30: the walk's products stay in int32).
 *
 * sc_scan_cast_batch: hit int32 [N].  hit[k] = SC_SCAN_IGNORED for an ignored ray or occ[a] != 0 (a sensor standing in an
 *   obstacle sees nothing); else the first cell of Walk(a, b), in sequence order, with occ != 0; else SC_SCAN_NO_RETURN.
 *   Consequence: for b inside the grid, hit = SC_SCAN_NO_RETURN <=> Clear(a, b) of the section above.  N == 0 is a no-op.
 *   One kernel, one lane per ray in ceil(N / 256) workgroups, timed as SC_K_MOVES.
 * sc_logodds_update: L int32 [H][W] (NULL: a fresh map of zeros; may be Lout), hit[k] what the cast wrote -- for recorded data
 *   the cell of the beam's end with b that cell, or SC_SCAN_NO_RETURN with b at maximum range.  A beam is ignored when its
 *   ray is, or hit[k] = SC_SCAN_IGNORED (the device form also ignores a hit below -2 or >= W*H; the _host form returns
 *   SC_ERR_INVALID for one before any launch).  For every other beam the cells of Walk(a, b) before the first occurrence of
 *   cell hit[k] are MISSED (all of them when hit[k] = -1 or the cell is not on the walk), and cell hit[k] >= 0 is HIT.  With M
 *   the cells missed and S the cells hit by some beam of this call,
 *     Lout[c] = clamp(L[c] + (c in S ? l_hit : c in M ? -l_miss : 0), -l_clamp, l_clamp)      (the sum in 64 bits).
 *   One update per cell and call however many beams cross it; a hit wins over a miss within a call (a wall cell that
 *   neighbouring beams graze is not eroded); nothing depends on the order of the beams or of execution.  Several scans that
 *   should each count are several calls.  Optional outputs (either or both NULL), written as 0 / 1:
 *     occ_est[c] = Lout[c] >= t_occ,   known[c] = Lout[c] >= t_occ or Lout[c] <= -t_free:
 *   the (known, occ_seen) pair of the calls above; unknown cells read 0 in occ_est.  N == 0 applies no beam, still clamps and
 *   writes the outputs (a stored map -> masks; rays and hit may then be NULL).
 *   Consequence (soundness): fed the cast's hit of a true map with the same rays, every missed cell has occ = 0 and every hit
 *   cell occ != 0; with l_hit >= t_occ and l_miss >= t_free occ_est never contradicts the true map.
 *   One kernel per beam batch (plain byte stores of 1 into two flag maps) and one kernel per cell, timed as SC_K_MOVES.
 *   Scratch: 2 * W * H bytes; grows only.
 *
 * Device pointers; the calls only enqueue on the context's stream.  The _host forms take host pointers, copy, run, copy back
 * and synchronise.  Errors: SC_ERR_INVALID for NULL mandatory pointers (Lout; occ and hit of the cast; rays and hit when
 * N > 0), N < 0, W or H outside 1..SC_MAX_DIM, l_hit < 0, l_miss < 0, l_clamp outside 0..2^30, t_occ < 1, t_free < 1, occ_est
 * or known equal to each other or to L or Lout. */
#define SC_SCAN_NO_RETURN (-1)  /* hit: the beam met no occupied cell */
#define SC_SCAN_IGNORED (-2)    /* hit: the ray was ignored, or the sensor stands on an occupied cell */
#define SC_SCAN_MAX_REACH 16384 /* |bx - ax|, |by - ay| of a ray that is not ignored */
int sc_scan_cast_batch(sc_ctx* ctx, const uint8_t* occ, const int32_t* rays, int N, int W, int H, int32_t* hit);
int sc_scan_cast_batch_host(sc_ctx* ctx, const uint8_t* occ, const int32_t* rays, int N, int W, int H, int32_t* hit);
int sc_logodds_update(sc_ctx* ctx, const int32_t* L, const int32_t* rays, const int32_t* hit, int N, int W, int H, int32_t l_hit,
                      int32_t l_miss, int32_t l_clamp, int32_t t_occ, int32_t t_free, int32_t* Lout, uint8_t* occ_est, uint8_t* known);
int sc_logodds_update_host(sc_ctx* ctx, const int32_t* L, const int32_t* rays, const int32_t* hit, int N, int W, int H, int32_t l_hit,
                           int32_t l_miss, int32_t l_clamp, int32_t t_occ, int32_t t_free, int32_t* Lout, uint8_t* occ_est,
                           uint8_t* known);

/* ---- scan matching: a scan's pose against the map -----------------------------------------------------------------
 * The calls above take the sensor's cell as given.  sc_scan_match_batch asks the opposite question: given a scan's end points
 * and the map so far, where was the sensor?  It scores every pose of a window around a prior against the likelihood field of
 * the map (the exact EDT of occ_est, capped) and returns the best one, with the number of poses that tie with it.  The
 * reference has no counterpart (no parity claim); the definition is integer and unique; tests/match_twin.py states it in
 * NumPy, tests/cpp/match_ref.c in C, and every output equals both bit for bit.  DESIGN.md section 25.  Cells are c = y*W + x.
 *
 * Inputs.  d2 int32 [H][W] from sc_edt_u8_i32, normally of occ_est (a grid without obstacles reads SC_EDT_INF).
 *   known uint8 [H][W], optional: NULL means that every cell of the grid is known.
 *   pts int32 [S][R][N][2] = (px, py): the scan's end points as cell offsets from the sensor cell, one set per scan s and
 *     candidate rotation r.  The caller rotates the points; the kernels know no angles.  A point is ABSENT when px or py lies
 *     outside -SC_SCAN_MAX_REACH .. SC_SCAN_MAX_REACH; SC_MATCH_ABSENT is the value the helpers write (a no-return beam has
 *     no end point).
 *   centre int32 [S][2] = (cx, cy), the prior sensor cell.  A scan is IGNORED when cx or cy lies outside
 *     -SC_SCAN_MAX_REACH .. SC_MAX_DIM + SC_SCAN_MAX_REACH: every sum of coordinates then stays far inside int32.
 *   wx, wy in 0 .. SC_MATCH_MAX_HALF, d2_cap in 1 .. 32767, unk in 0 .. d2_cap, N in 1 .. SC_MATCH_MAX_POINTS, R in
 *     1 .. SC_MATCH_MAX_ROT.
 * Cost of a cell.  cost(x, y) = unk when (x, y) lies outside the grid or known[c] = 0, else min(d2[c], d2_cap).
 * Score, for dy in [-wy, wy] and dx in [-wx, wx]:
 *     score[s][r][dy][dx] = sum over the present points k of cost(cx + dx + px_k, cy + dy + py_k).
 *   It is at most 32767 * 65536 = 2 147 418 112 < 2^31: an int32.
 * Best pose of scan s: the candidate with the lexicographically smallest (score, dx^2 + dy^2, r, dy, dx).  Ties go to the
 *   smallest displacement, then to the earliest rotation: a caller who has a prior heading puts it first.  Rotations with
 *   different numbers of present points are compared as they are (a rotation that loses points scores less); giving every
 *   rotation the same points is the caller's business.
 * Outputs.  best int32 [S][6] = (r, dx, dy, score, n_points, n_ties): n_points the present points of rotation r, n_ties the
 *   number of candidates of the whole volume whose score equals the best.  An ignored scan reads (SC_MATCH_IGNORED, 0, 0, 0,
 *   0, 0).  score int32 [S][R][2 wy + 1][2 wx + 1], optional (NULL allowed): the whole volume, for callers who want a
 *   covariance; an ignored scan's part is written as zeros.  With score NULL nothing of the volume's size is written.
 * Consequences.  All points absent: score 0 everywhere, best = (0, 0, 0, 0, 0, R (2 wx + 1)(2 wy + 1)).  If the points are
 *   the hits of sc_scan_cast_batch on a true map from cell a, and d2 is that map's, the candidate that puts the sensor at a
 *   scores 0; if it lies in the window and n_ties = 1, best is that candidate.
 *
 * Three kernels, timed as SC_K_MOVES, no atomics and no float operations: a cost pass (one thread per cell: the uint16 cost
 * map with a border of unk), the score kernel (256 candidates per workgroup, its 4 or 16 wavefronts share the points and
 * add their partial sums in LDS; it leaves its smallest key and the candidates at that score) and a pick kernel (one workgroup
 * per scan).  Scratch: 2 (W + 2)(H + 2) + 2 bytes and 16 S R ceil((2 wx + 1)(2 wy + 1) / 256) bytes; grows only.
 *
 * Device pointers; the call only enqueues on the context's stream (... -> sc_logodds_update -> sc_edt_u8_i32 ->
 * sc_scan_match_batch runs on one stream).  The _host form takes host pointers, copies, runs, copies back and synchronises;
 * it returns SC_ERR_INVALID for an ignored centre before any launch (the device form writes the ignored row).  Errors:
 * SC_ERR_INVALID for NULL d2, pts, centre or best, S < 0, R, N, W, H, wx, wy, d2_cap or unk outside their ranges, score equal
 * to best.  S == 0 is a no-op. */
#define SC_MATCH_ABSENT INT32_MIN  /* pts: the value the helpers write for a point that is not there */
#define SC_MATCH_IGNORED (-1)      /* best[s][0] of an ignored scan */
#define SC_MATCH_MAX_HALF 64       /* wx, wy */
#define SC_MATCH_MAX_POINTS 65536  /* N */
#define SC_MATCH_MAX_ROT 256       /* R */
int sc_scan_match_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre, int S, int R,
                        int N, int W, int H, int wx, int wy, int32_t d2_cap, int32_t unk, int32_t* best, int32_t* score);
int sc_scan_match_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre, int S,
                             int R, int N, int W, int H, int wx, int wy, int32_t d2_cap, int32_t unk, int32_t* best, int32_t* score);

/* ---- wide-window scan matching: an exact pruned search over a cost pyramid ----------------------------------------
 * sc_scan_match_batch scores every pose of a window of at most +-64 cells.  A robot that has lost its pose, or that comes
 * back to a mapped place after a long loop, needs windows of hundreds or thousands of cells, where only one pose wins and
 * most of the volume is wasted.  sc_scan_match_wide_batch searches such a window with lower bounds from a min-pooled pyramid
 * of the same cost map and opens only the blocks of poses whose bound does not exceed a score already in hand.  Only blocks
 * with bound > U are dropped, so the result is the same `best` row, ties included, as the dense volume.  Integer and unique;
 * tests/match_wide_twin.py states it in NumPy, tests/cpp/match_wide_ref.c in C, and every output equals both bit for bit.
 * DESIGN.md section 26.
 *
 * Inputs.  d2, known (optional), pts [S][R][N][2], centre [S][2], d2_cap, unk: those of sc_scan_match_batch, with the same
 *   rules for absent points and ignored scans, and cost(x, y) the same function over the whole plane (unk outside the grid
 *   or where known is 0).
 *   wx, wy in 0 .. SC_MATCH_WIDE_MAX_HALF (2048).  top in 0 .. SC_MATCH_WIDE_MAX_TOP (5).  max_nodes in
 *   SC_MATCH_WIDE_MIN_NODES (64) .. SC_MATCH_WIDE_MAX_NODES (2^22), with S max_nodes <= SC_MATCH_WIDE_MAX_TOTAL (2^26).
 *   R (2 wx + 1)(2 wy + 1) <= INT32_MAX, since n_ties is an int32.
 * Pooled cost, bounds and nodes.  P_m(x, y) = min over 0 <= i, j < m of cost(x + i, y + j) for m = 4^j, and P_1 = cost.
 *   A node (r, dx0, dy0) of size m stands for the candidates dx0 <= dx < dx0 + m, dy0 <= dy < dy0 + m of rotation r that lie
 *   in the window.  Its bound is B_m = sum over the present points k of P_m(cx + dx0 + px_k, cy + dy0 + py_k).  It is at
 *   most the score of every candidate the node stands for; it is an int32 by the argument of sc_scan_match_batch, and for
 *   m = 1 it is the score itself.  Its children are the up to 16 nodes of size m/4 at (dx0 + a m/4, dy0 + b m/4),
 *   a, b in 0 .. 3, with dx0' <= wx and dy0' <= wy.
 * Procedure per scan (part of the definition, because its counts are outputs).
 *   1. An ignored scan reads (SC_MATCH_IGNORED, 0, 0, 0, 0, 0) and has zero stats.
 *   2. If no rotation has a present point, the result is best = (0, 0, 0, 0, 0, R (2 wx + 1)(2 wy + 1)) and zero stats: the
 *      closed form of sc_scan_match_batch; no search runs.
 *   3. Start: U = min over r of score(r, 0, 0).  The nodes of size m = 4^top are (r, -wx + i m, -wy + j m) for all r and all
 *      i, j with dx0 <= wx and dy0 <= wy.  If their count exceeds max_nodes, the call returns SC_ERR_INVALID (the host tests
 *      this before anything runs).
 *   4. Level of size m: bound every node, and set n_j to the number of nodes bounded, with m = 4^j.  If m = 1, go to step 5.
 *      Otherwise run one dive per rotation r: among r's nodes take the smallest (B, dy0, dx0); if its B exceeds the U of the
 *      start of this level, r does not dive; else bound its children and take the smallest (B, dy0, dx0) among them, and
 *      repeat down to size 1: the last B is a true score v_r.  n_dive counts every child bounded in dives.  After the dives,
 *      U <- min(U, all v_r).  Survivors are the nodes with B <= U; the next level's nodes are their children.  If the next
 *      level has more than max_nodes nodes, the scan reads (SC_MATCH_OVERFLOW, 0, 0, 0, 0, 0); its n_j are filled down to
 *      the level just bounded, the levels below are 0, and n_dive and U are what they were at that point.
 *   5. Over the leaves, best is the smallest (score, dx^2 + dy^2, r, dy, dx); n_ties is the number of leaves whose score
 *      equals the best score; n_points is as in sc_scan_match_batch.
 * Why the result equals the dense search.  A candidate whose score equals the best has every ancestor at B <= best <= U, so
 *   all tying candidates reach the leaves.  The minimum and the ties do not depend on U, on the dives or on any order of
 *   execution; the counts depend only on the stated procedure.
 * Outputs.  best int32 [S][6], as sc_scan_match_batch.  stats int32 [S][8] = (n_0, .., n_5, n_dive, U), optional (NULL
 *   allowed).  There is no score volume.
 *
 * Kernels, timed as SC_K_MOVES, integer only: the cost pass of sc_scan_match_batch, two pooling passes per level, an init
 * kernel, per level a bound kernel (a wave takes four parents and bounds their 64 children), a dive kernel (one workgroup
 * per scan and rotation) and an expand kernel (wave-aggregated appends), and a pick kernel: 4 + 5 top launches and three
 * memsets.  Scratch, grows only: the pooled maps, 2 (W + m + 1)(H + m + 1) bytes per level m = 4 .. 4^top and one of
 * m = 4^top / 2; 20 S max_nodes + 8 S R + 96 S bytes of lists, bounds, keys and counters.
 *
 * Device pointers; the call only enqueues on the context's stream and never synchronises.  The _host form takes host
 * pointers, copies, runs, copies back and synchronises; it returns SC_ERR_INVALID for an ignored centre before any launch.
 * Errors: SC_ERR_INVALID for NULL d2, pts, centre or best, S < 0, R, N, W, H, wx, wy, d2_cap, unk, top or max_nodes outside
 * their ranges, too many nodes at the top level, stats equal to best.  S == 0 is a no-op. */
#define SC_MATCH_OVERFLOW (-2)              /* best[s][0] of a scan whose next level had more than max_nodes nodes */
#define SC_MATCH_WIDE_MAX_HALF 2048         /* wx, wy */
#define SC_MATCH_WIDE_MAX_TOP 5             /* top: nodes of up to 1024 x 1024 candidates */
#define SC_MATCH_WIDE_MIN_NODES 64          /* max_nodes */
#define SC_MATCH_WIDE_MAX_NODES (1 << 22)   /* max_nodes */
#define SC_MATCH_WIDE_MAX_TOTAL (1 << 26)   /* S * max_nodes */
int sc_scan_match_wide_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre, int S,
                             int R, int N, int W, int H, int wx, int wy, int32_t d2_cap, int32_t unk, int top, int max_nodes,
                             int32_t* best, int32_t* stats);
int sc_scan_match_wide_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* known, const int32_t* pts, const int32_t* centre,
                                  int S, int R, int N, int W, int H, int wx, int wy, int32_t d2_cap, int32_t unk, int top,
                                  int max_nodes, int32_t* best, int32_t* stats);

/* ---- re-planning in space-time around the scheduled fleet -------------------------------------------------------
 * sc_fleet_schedule_batch only delays: a path that finds no free slot comes back SC_SLOT_UNRESOLVED.  These calls plan such a
 * robot again in (cell, time): the paths that did get a slot are rasterised into reservations, and an exact earliest-arrival
 * search on the time-expanded grid goes around them.  The result is knot rows that sc_traj_conflicts_batch takes directly.  The
 * reference has nothing of this kind.
 *
 * Definition (tests/tplan_twin.py states it in NumPy, tests/cpp/tplan_ref.c in C; every output equals them exactly).
 *   Clock and grid.  Layer t is tick t of the knots' clock, tau_t = T0 + t * dt_c; there are L = K + 1 layers.  The caller
 *     chooses dt_c as the time one grid move takes.  A cell's centre is the point sc_cells_to_points_batch writes: (x_min +
 *     (c % W + 0.5) * res_x, y_min + (c / W + 0.5) * res_y) in float32 without contraction, widened to fp64 where needed.
 *     Bitmaps are uint32 [H][Wq], Wq = ceil(W / 32): cell (x, y) is bit x & 31 of word [y][x >> 5]; bits at x >= W are 0.
 *   Reservation.  res uint32 [L][H][Wq].  For path q and interval k with both knots present, cell c is hit iff m2 < R*R of the
 *     path conflicts above with d0 = knot[q][k] - c, d1 = knot[q][k+1] - c, R = radius[q] + pad: the same operations in the same
 *     order, fp64, no fused multiply-adds.  It says "a robot standing at c through interval k would conflict with q".  A hit
 *     sets c's bit in layers k and k+1.  An interval with an absent knot reserves nothing (the conflicts call does not compare
 *     it).  Paths whose tstatus is not SC_TRAJ_OK reserve nothing (tstatus NULL = all OK), nor do paths with select[q] == 0
 *     (select int32 [P], NULL = all).  A path that is OK and whose radius is outside the contract becomes SC_TRAJ_BAD, as in
 *     the conflicts call, and reserves nothing.  The call ORs into res: several calls accumulate, the caller zeroes it first.
 *   Why pad.  pad is the caller's fp64 argument; the library does not derive it.  Let pad >= r_new + hyp / 2 with hyp =
 *     sqrt(res_x^2 + res_y^2), the longest move, and let a robot of radius r_new step between cells that are unreserved at
 *     their layers.  Then it never comes within radius[q] + r_new of q on a compared interval:
 *       on interval t the robot is at a + lam * (b - a), lam in [0, 1], a its cell at layer t and b at layer t+1;
 *       a (unreserved at layer t) and b (at layer t+1) are both at least R from q's motion relative to a standing robot on
 *       interval t; the robot's offset from the nearer of a and b is at most |b - a| / 2 <= hyp / 2,
 *       so it stays at least R - hyp / 2 >= radius[q] + r_new away.
 *   Search, for each of B queries.  start, goal: cells; t_start: the layer at which the robot appears (int32 [B], NULL = 0; it
 *     is absent before); hold: 0 or 1, one value for the call.  free(c) and the move byte of a cell are sc_moves_i32_u8's for
 *     r2_clear (no corner cutting, directions d in its order, delta_d = (dx, dy) = {1,-1,0,0,1,-1,1,-1}, {0,0,1,-1,1,1,-1,-1}).
 *       reach[t_start] = {start};
 *       reach[t+1] = the cells c unreserved at layer t+1 with c in reach[t] (a wait) or c = s + delta_d for some s in reach[t]
 *         with bit d of moves[s] set.
 *     t_hold = with hold, 1 + the last layer at which goal is reserved (0 if never); without hold, 0.
 *     arrive = the smallest t >= max(t_start, t_hold) with goal in reach[t].
 *     status (sc_tplan_status), decided in this order: SC_TP_BAD_ENDPOINT when start or goal is out of range or not free, or
 *     t_start is outside 0 .. L-1; SC_TP_START_BLOCKED when start is reserved at t_start; SC_TP_NO_PATH when there is no
 *     arrival by layer L-1; else SC_TP_OK.  res NULL = nothing is reserved.
 *   Path.  Walk back from (goal, arrive).  The predecessor of cell c at layer t is c itself if c is in reach[t-1] (waits come
 *     first: otherwise they pile up as back-and-forth moves); failing that, c - delta_d for the first d in 0 .. 7 with
 *     c - delta_d in reach[t-1] and bit d of moves[c - delta_d] set.  This is one stated earliest-arrival path; it is NOT the
 *     shortest in metres among them, and nothing is smoothed.
 *   Outputs, each may be NULL except status.  path int32 [B][L]: path[b][i] = the cell at layer t_start + i for i < len[b],
 *     entries past len are not written.  len, arrive, status int32 [B]; len = arrive - t_start + 1; len 0 and arrive -1 when the
 *     status is not OK.  knots_out fp64 [B][L][2]: NaN before t_start, the cell's centre at layers t_start .. arrive, after
 *     arrive the goal's centre with hold and NaN without, all NaN when the status is not OK.  A caller puts knots_out behind the
 *     fleet's rows in one [P+B][K+1][2] buffer and calls sc_traj_conflicts_batch: a failed plan is NaN rows, which reserve
 *     nothing and conflict with nobody.  reach uint32 [B][L][H][Wq] (NULL = context scratch): defined for layers t_start ..
 *     arrive, or .. L-1 when there is no arrival; other layers, and all layers of a query that is BAD_ENDPOINT or
 *     START_BLOCKED, are unspecified.
 *
 * sc_traj_reserve_batch: ORs the reservations of P knot rows into res.
 * sc_tplan_batch: the search.  The frame (x_min .. res_y) is read for knots_out only.
 * sc_fleet_replan_batch: the arguments of both, then r_new fp64 [B] and sequential.  It reserves the selected fleet paths; with
 *   sequential = 0 it plans all B robots against them in one batch (r_new may be NULL); with sequential = 1 it plans robot i
 *   and then reserves knots_out[i] with radius r_new[i] and the same pad, for i = 0, 1, .., so that robot i+1 goes around it:
 *   prioritised planning in the caller's order (needs r_new and knots_out).  L must be K + 1.
 * Device pointers; the calls only enqueue on the context's stream (kernels timed under SC_K_ASTAR): no host synchronisation, no
 * device-to-host copy.  Scratch of the context: W * H bytes of move bytes and eight direction planes uint32 [8][H][Wq]; 24 bytes
 * per query of a group; 4 * L bytes per query when knots_out is asked without path; and, when reach is NULL, B_g * L * H * Wq * 4
 * bytes of layers: the B queries are served in groups of B_g that fit a budget, SC_TPLAN_GB GiB (a decimal number, at most 64, default 8) in the
 * environment when the context is created.  One query whose layers exceed the budget is SC_ERR_INVALID, with the needed size in
 * sc_last_error.  A launch of the search advances SC_TPLAN_LAYERS layers (1 .. 16, default 16, which measured best; read at context creation); no
 * output depends on it.
 * The _host forms take host pointers (res and tstatus are copied back) and return SC_ERR_INVALID before any launch for a radius
 * or r_new outside the contract.
 * Errors: SC_ERR_INVALID for NULL required pointers (knots, radius, res in the reserving calls; d2, start, goal, status), W or H
 * outside 1 .. SC_MAX_DIM, P outside 1 .. 16384, K outside 1 .. 65535, P * (K+1) > 2^26, L outside 1 .. 65536, L != K + 1 in
 * the combined call, pad not finite or negative, B outside 1 .. 65536, and, where the frame is read (the reserving calls, and
 * knots_out), x_min or y_min not finite or res_x, res_y not finite and positive. */
typedef enum {
    SC_TP_OK = 0,
    SC_TP_NO_PATH = 1,
    SC_TP_BAD_ENDPOINT = 2,
    SC_TP_START_BLOCKED = 3
} sc_tplan_status;
int sc_traj_reserve_batch(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius, const int32_t* select,
                          double pad, int W, int H, float x_min, float y_min, float res_x, float res_y, uint32_t* res);
int sc_traj_reserve_batch_host(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius,
                               const int32_t* select, double pad, int W, int H, float x_min, float y_min, float res_x, float res_y,
                               uint32_t* res);
int sc_tplan_batch(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear, const uint32_t* res, int L, const int32_t* start,
                   const int32_t* goal, const int32_t* t_start, int B, int hold, int32_t* path, int32_t* len, int32_t* arrive,
                   int32_t* status, double* knots_out, float x_min, float y_min, float res_x, float res_y, uint32_t* reach);
int sc_tplan_batch_host(sc_ctx* ctx, const int32_t* d2, int W, int H, int32_t r2_clear, const uint32_t* res, int L, const int32_t* start,
                        const int32_t* goal, const int32_t* t_start, int B, int hold, int32_t* path, int32_t* len, int32_t* arrive,
                        int32_t* status, double* knots_out, float x_min, float y_min, float res_x, float res_y, uint32_t* reach);
int sc_fleet_replan_batch(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius, const int32_t* select,
                          double pad, int W, int H, float x_min, float y_min, float res_x, float res_y, uint32_t* res, const int32_t* d2,
                          int32_t r2_clear, int L, const int32_t* start, const int32_t* goal, const int32_t* t_start, int B, int hold,
                          int32_t* path, int32_t* len, int32_t* arrive, int32_t* status, double* knots_out, uint32_t* reach,
                          const double* r_new, int sequential);
int sc_fleet_replan_batch_host(sc_ctx* ctx, const double* knots, int32_t* tstatus, int P, int K, const double* radius,
                               const int32_t* select, double pad, int W, int H, float x_min, float y_min, float res_x, float res_y,
                               uint32_t* res, const int32_t* d2, int32_t r2_clear, int L, const int32_t* start, const int32_t* goal,
                               const int32_t* t_start, int B, int hold, int32_t* path, int32_t* len, int32_t* arrive, int32_t* status,
                               double* knots_out, uint32_t* reach, const double* r_new, int sequential);

/* ---- the reference's own planner, batched -----------------------------------------------
 * planning_space::fast_marching_trees (sea_current.hpp:1339-1407) with near (:1328-1337), cost (:1315-1326) and
 * intersects (:142-178): FMT* from starts[q] to goals[q] (float [Q][2]) over n shared free samples (float [n][2], e.g.
 * from sample_free :1294-1313; the reference draws them inside the call) with connection radius rn (the reference
 * compares distances with rn squared; so does this) around obstacle edges lines (float [E][4]).  path float
 * [Q][Lmax][2] start..goal, len [Q], cost float [Q] (cost-to-come of the goal), status [Q] (SC_Q_OK / SC_Q_NO_PATH /
 * SC_Q_TRUNCATED).  Equal costs are resolved towards the lowest node index (samples in order, then goal, then start);
 * the reference resolves them by unordered_set iteration order. */
#define SC_FMT_MAX_SAMPLES 2046
#define SC_FMT_MAX_EDGES 512
int sc_fmt_star_batch(sc_ctx* ctx, const float* samples, int n, const float* starts, const float* goals, int Q, float rn,
                      const float* lines, int E, int Lmax, float* path, int32_t* len, float* cost, int32_t* status);
int sc_fmt_star_batch_host(sc_ctx* ctx, const float* samples, int n, const float* starts, const float* goals, int Q, float rn,
                           const float* lines, int E, int Lmax, float* path, int32_t* len, float* cost, int32_t* status);

/* ---- multi-GPU: query sharding and the gather of result paths --------------------------------
 * One process (context) per GPU.  Queries shard in contiguous blocks: rank r of `world` owns [q0, q1) as sc_rank_range
 * says, plans them with sc_astar_batch on its own replica of the grid (every rank recomputes the EDT: cheaper than
 * moving 4 B/cell), and sc_allgather_paths leaves EVERY rank with every query's result, in query order.  The reference
 * has no collective of any kind (its only transport is the ZMQ REP loop, examples/zmq_test.cpp:18-22); this is the
 * exchange BASELINE.json names ("RCCL all-gather of result paths over xGMI").
 *
 * Communicator: sc_comm_unique_id on one rank, the 128 bytes handed to all ranks by whatever launched them, then
 * sc_comm_init on each (ncclCommInitRank); or sc_comm_adopt of an ncclComm_t the caller already has.  RCCL is loaded
 * at run time (dlopen), so single-GPU users need no librccl.
 *
 * sc_allgather_paths (device pointers, enqueued on the context's stream, no host synchronisation):
 *   in   path [Q_local][Lmax], len / cost / status [Q_local]   this rank's sc_astar_batch results
 *   out  len_all / cost_all / status_all [Q_total], offsets_all int64 [Q_total + 1] (cells in front of each query;
 *        only paths with status SC_Q_OK count), cells_all [cells_capacity] the paths back to back (may be NULL),
 *        path_all [Q_total][Lmax] the fixed-stride parity layout (may be NULL), *truncated != 0 if some rank's paths
 *        exceeded cap_cells (bit 0: cells beyond it read -1; gather again with a larger cap_cells) or cells_all is too
 *        small (bit 1).
 *   cap_cells: cells a rank's message can carry (the same on all ranks).  One ncclAllGather of
 *        sc_gather_msg_words(Q_total, world, cap_cells) = 2 + 3 ceil(Q_total / world) + cap_cells (rounded up to even)
 *        int32 per rank. */
void sc_rank_range(int Q, int world, int rank, int* q0, int* q1);
int sc_comm_unique_id(void* id128);
int sc_comm_init(sc_ctx* ctx, const void* id128, int nranks, int rank);
int sc_comm_adopt(sc_ctx* ctx, void* nccl_comm, int nranks, int rank);
int sc_comm_destroy(sc_ctx* ctx);
int sc_allgather_paths(sc_ctx* ctx, const int32_t* path, const int32_t* len, const int32_t* cost, const int32_t* status,
                       int Q_local, int Q_total, int Lmax, int cap_cells, int32_t* len_all, int32_t* cost_all, int32_t* status_all,
                       int64_t* offsets_all, int32_t* cells_all, int64_t cells_capacity, int32_t* path_all, int32_t* truncated);
/* bytes every rank received in the last sc_allgather_paths on this context */
int sc_allgather_last_bytes(sc_ctx* ctx, int64_t* bytes);
/* The two halves of sc_allgather_paths on their own, for a caller whose transport is not RCCL (the reference's is ZMQ,
 * examples/zmq_test.cpp:18-22) and for tests that play several ranks on one GPU.  Device pointers, enqueued, no host
 * synchronisation, no communicator needed.
 *   sc_gather_msg_words : int32 words of one rank's message for (Q_total, world, cap_cells); 0 for bad arguments.
 *   sc_gather_pack      : rank `rank` of `world` packs its Q_local results into msg [sc_gather_msg_words] (Q_local must be
 *                         what sc_rank_range gives that rank; 0 is allowed and the input pointers may then be NULL).
 *   sc_gather_unpack    : msgs = the `world` messages back to back in rank order -> the outputs of sc_allgather_paths.
 *   *truncated: bit 0 = some rank's paths exceeded cap_cells (cells beyond it read -1), bit 1 = cells_all is smaller
 *   than offsets_all[Q_total] (cells beyond cells_capacity are not written).  sc_allgather_paths sets the same bits. */
int64_t sc_gather_msg_words(int Q_total, int world, int cap_cells);
int sc_gather_pack(sc_ctx* ctx, const int32_t* path, const int32_t* len, const int32_t* cost, const int32_t* status, int Q_local,
                   int Q_total, int world, int rank, int Lmax, int cap_cells, int32_t* msg);
int sc_gather_unpack(sc_ctx* ctx, const int32_t* msgs, int world, int Q_total, int Lmax, int cap_cells, int32_t* len_all,
                     int32_t* cost_all, int32_t* status_all, int64_t* offsets_all, int32_t* cells_all, int64_t cells_capacity,
                     int32_t* path_all, int32_t* truncated);

#ifdef __cplusplus
}
#endif
#endif
