/* sea_current_hip_car.h -- car-like pose planning: arc moves instead of turns on the spot.
 *
 * Part of the C ABI of libsea_current_hip.so: same library, same sc_ctx, same conventions as sea_current_hip.h, which
 * this header includes.  The six entries stand in a header of their own because the ABI and stream-order suites pin the
 * symbol sets of sea_current_hip.h and sea_current_hip_update.h exactly; the stream contract of these entries has its own
 * test.  SC_ABI_VERSION stays 1 and SC_K_COUNT stays 15.  tests/car_twin.py states the definition in NumPy,
 * tests/cpp/car_ref.c in C, and every output equals both bit for bit.  Cells are c = y*W + x.
 *
 * Definition.
 *
 * Headings, h_k, w_k (10 for even k, 14 for odd k), T(c), pose validity (T(c) and bit k of hmask[c], or T(c) without a
 * mask) and A*'s move legality are those of the pose calls of sea_current_hip.h (section 28).
 *
 * Parameters:
 *   - arc_n in 1 .. SC_ARC_MAX = 4;
 *   - arc_cost in 0 .. 255;
 *   - rev_cost in -1 .. 255, where -1 means no reversing.
 *
 * Arc.  For a pose (c, k) and a sense s = +-1, let k' = (k + s) mod 8.  The walk's cells are:
 *   - p_i = c + i*h_k for i = 0 .. n;
 *   - p_(n+j) = p_n + j*h_k' for j = 0 .. n.
 * A(c, k, s) is legal iff both of these hold:
 *   - each of the 2n steps p_i -> p_(i+1) is a legal A* move (in grid, both cells T, and for a diagonal both side cells T);
 *   - the poses (p_i, k) for i = 0 .. n and (p_(n+j), k') for j = 0 .. n are valid.  The corner p_n must be valid at both
 *     headings.
 * It ends in (p_2n, k').
 * This is "n cells straight, 45 degrees, n cells straight".  Chained arcs leave 2n straight cells between heading changes.
 * That is a turning radius of about 3*arc_n cells, and the stair path's length is within 10 % of the true arc's.
 *
 * Graph.  Edges out of a valid pose (c, k):
 *   1. Forward to (c + h_k, k), cost w_k.
 *   2. Reverse to (c - h_k, k), cost w_k + rev_cost.
 *   3. Forward arc A(c, k, +1), cost 24*arc_n + arc_cost.
 *   4. Forward arc A(c, k, -1), cost 24*arc_n + arc_cost.
 *   5. Reverse arc undoing an arc of sense +1, cost 24*arc_n + arc_cost + 2*arc_n*rev_cost.
 *   6. Reverse arc undoing an arc of sense -1, cost 24*arc_n + arc_cost + 2*arc_n*rev_cost.
 *   - Edges 1 and 2 have section 28's legality.
 *   - Edges 2, 5 and 6 exist only if rev_cost >= 0.
 *   - For every legal A(c', j, s) that ends in (c, k), edges 5 and 6 go from (c, k) to (c', j).
 * There is no turn on the spot.  Every edge cost is positive.
 *
 * Arc mask (sc_arc_mask_u16).  amask is uint16 [batch][H][W].  Bit 2k + (s < 0) of amask[c] is set iff A(c, k, s) is legal.
 *   Cells with !T(c) read 0.
 *
 * Field (sc_car_field_batch).  gp is int32 [F][8][H][W].
 *   - With toward = 0, gp[f][k][c] is the exact cost from the root pose to (c, k).
 *   - With toward = 1, it is the exact cost from (c, k) to the root pose.  That is stated directly as a Dijkstra over
 *     in-edges; the implementation may rename layers as section 28 does.
 *   - rhead, bad roots, fgrid, SC_FIELD_INF and fstatus are as in sc_pose_field_batch.
 *   - Before any launch or allocation the call returns SC_ERR_INVALID in two cases: the parameters are out of range, or, in
 *     64 bits, (24*arc_n + arc_cost + 2*arc_n*max(rev_cost, 0)) * (8*W*H - 1) > INT32_MAX - 1.
 *
 * Read-out (sc_car_paths_batch).  From a state x with value v > 0, take the first edge, in the order 1 .. 6 above, that is
 *   legal and whose far end y has gp[y] + cost == v.
 *   - toward = 0 takes in-edges y -> x.
 *   - toward = 1 takes out-edges x -> y.
 *   - For kinds 5 and 6 the sense is that of the forward arc being undone.
 *   - Legality of straight moves is read from d2 and hmask.  Legality of arcs is read from amask, with every index
 *     bounds-checked.
 *   Entries are one per cell, in the caller's choice of order (to_root as in section 28):
 *   - An arc contributes its 2n - 1 intermediate cells between its end poses.
 *   - Each intermediate cell carries the heading of the leg by which it is reached in driving order.  Driving order is
 *     root -> target for toward = 0 and target -> root for toward = 1.
 *   - path is therefore always 8-connected and goes straight into sc_path_waypoints_batch.  No cells_only is needed.
 *   - thead = -1, statuses, len, cost and truncation are as in sc_pose_paths_batch.
 *
 * The calls.
 * sc_arc_mask_u16: d2 int32 [batch][H][W], hmask uint8 [batch][H][W] or NULL, amask uint16 [batch][H][W] out.
 * sc_car_field_batch: d2, hmask (or NULL), G, fgrid, W, H, r2_clear, toward, root, rhead, F, gp and fstatus (may be NULL) as
 *   sc_pose_field_batch takes them; amask uint16 [G][H][W] is mandatory.  rounds: chip-wide relaxation launches before the
 *   per-field finisher; the result is identical for every value >= 0; < 0 picks the library default
 *   4 * (ceil(W/32) + ceil(H/32)) + 16; values above 65536 count as 65536.
 * sc_car_paths_batch: the same leading arguments, then gp, root, rhead and F as the field call took and returned them, and
 *   qfield, target, thead, Q, Lmax, to_root, path int32 [Q][Lmax], head uint8 [Q][Lmax], len, cost, status int32 [Q] as
 *   sc_pose_paths_batch takes them.  Q == 0 is a no-op.
 * If amask is not the mask of these arguments the values are unspecified, but every access stays in bounds and the calls
 * end.  Device pointers; the calls only enqueue on the context's stream: no host synchronisation, no device-to-host copy, no
 * workgroup waits for another; sc_edt_u8_i32 -> sc_footprint_mask_u8 -> sc_arc_mask_u16 -> sc_car_field_batch ->
 * sc_car_paths_batch -> sc_path_waypoints_batch runs with one synchronise.  Errors: SC_ERR_INVALID for NULL mandatory
 * pointers (hmask, fgrid with G == 1 and fstatus may be NULL), W or H outside 1..SC_MAX_DIM, batch, G, F <= 0, Q < 0,
 * Lmax <= 0 and the parameter rules above.  The _host forms take host pointers, check the data (sc_car_paths_batch_host:
 * every gp value >= 0), copy through the shared staging buffer, run, copy back and synchronise.  Scratch grows only: the
 * field keeps about 12 B per (field, 32 x 32 tile); the mask and the read-out keep none.  The field and the read-out are timed
 * as SC_K_ASTAR, the mask as SC_K_MOVES. */
#ifndef SEA_CURRENT_HIP_CAR_H
#define SEA_CURRENT_HIP_CAR_H
#include "sea_current_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SC_ARC_MAX 4

int sc_arc_mask_u16(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int W, int H, int batch, int32_t r2_clear, int arc_n,
                    uint16_t* amask);
int sc_arc_mask_u16_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, int W, int H, int batch, int32_t r2_clear, int arc_n,
                         uint16_t* amask);
int sc_car_field_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, const uint16_t* amask, int G, const int32_t* fgrid, int W,
                       int H, int32_t r2_clear, int arc_n, int arc_cost, int rev_cost, int toward, const int32_t* root,
                       const int32_t* rhead, int F, int rounds, int32_t* gp, int32_t* fstatus);
int sc_car_field_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, const uint16_t* amask, int G, const int32_t* fgrid,
                            int W, int H, int32_t r2_clear, int arc_n, int arc_cost, int rev_cost, int toward, const int32_t* root,
                            const int32_t* rhead, int F, int rounds, int32_t* gp, int32_t* fstatus);
int sc_car_paths_batch(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, const uint16_t* amask, int G, const int32_t* fgrid, int W,
                       int H, int32_t r2_clear, int arc_n, int arc_cost, int rev_cost, int toward, const int32_t* gp,
                       const int32_t* root, const int32_t* rhead, int F, const int32_t* qfield, const int32_t* target,
                       const int32_t* thead, int Q, int Lmax, int to_root, int32_t* path, uint8_t* head, int32_t* len, int32_t* cost,
                       int32_t* status);
int sc_car_paths_batch_host(sc_ctx* ctx, const int32_t* d2, const uint8_t* hmask, const uint16_t* amask, int G, const int32_t* fgrid,
                            int W, int H, int32_t r2_clear, int arc_n, int arc_cost, int rev_cost, int toward, const int32_t* gp,
                            const int32_t* root, const int32_t* rhead, int F, const int32_t* qfield, const int32_t* target,
                            const int32_t* thead, int Q, int Lmax, int to_root, int32_t* path, uint8_t* head, int32_t* len,
                            int32_t* cost, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif
