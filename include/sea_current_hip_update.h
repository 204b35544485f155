/* sea_current_hip_update.h -- repair of cost fields after a map change.
 *
 * Part of the C ABI of libsea_current_hip.so: same library, same sc_ctx, same conventions as sea_current_hip.h, which
 * this header includes.  The four entries stand in a header of their own because the stream-order suite pins the
 * device entries of sea_current_hip.h to the chains it declares; the stream contract of these entries has its own
 * test.  SC_ABI_VERSION stays 1 and SC_K_COUNT stays 15 (timed as SC_K_ASTAR).
 *
 * Definition.  Graph, T(c), move legality and costs are those of the cost fields (sc_cost_field_batch); weighted, those
 * of the weighted fields: w(n -> c) = w_d + min(pen[c], pen_cap).  Primes mark the new map: T' from d2_new, w' from
 * pen_new.  Let g be the exact field of the old map for root r.
 *
 *   Unsupported set U.  U is the least set with the following property.  A cell c with g[c] finite is in U if either
 *   condition holds:
 *     - !T'(c).
 *     - c is not the root, and every neighbour n satisfying all three points below is in U:
 *         - the move n -> c is legal under T';
 *         - g[n] is finite;
 *         - g[n] + w'(n -> c) == g[c].
 *   The root is supported by itself iff T'(r).  U is well defined because g rises strictly along such edges.
 *
 *   Setting the cells of U to SC_FIELD_INF leaves only values that are costs of legal paths in the new map (induction
 *   over g).  Relaxation from there reaches the unique fixed point of the fields.  Cells that became free and penalties
 *   that fell need no raise: relaxation lowers them.
 *
 *   Result.  g and fstatus become what sc_cost_field_batch (or the weighted form) returns for the new map.  This
 *   includes a root that became blocked (all SC_FIELD_INF, SC_Q_BAD_ENDPOINT), a root that became free (the field
 *   appears) and an out-of-range fgrid[f] (exactly what the fresh call leaves in g and fstatus).  If g on entry is not
 *   the old map's field, the values returned are unspecified; every access still stays in bounds and the call ends.
 *
 *   stats[f][0]: the number of cells of the field's grid with T != T'; weighted: also the cells with T && T' whose
 *   capped penalties differ (0 for an out-of-range fgrid[f]).  stats[f][1]: |U|.  Both are independent of execution
 *   order.  stats int32 [F][2] may be NULL.
 *
 * sc_cost_field_update_batch: d2_old, d2_new int32 [G][H][W]; fgrid, W, H, r2_clear, root, F as sc_cost_field_batch took
 *   them for g; g int32 [F][H][W] in and out.  Argument and overflow rules are those of sc_cost_field_batch.
 *   d2_old == d2_new (and equal pen pointers) is allowed and changes nothing.  rounds: the chip-wide launches of the
 *   raise phase and of the relaxation before their per-field finishers complete what is left; the result is identical
 *   for every value >= 0; < 0 picks the defaults (raise: tile columns + tile rows + 8, relaxation: that of
 *   sc_cost_field_batch); values above 65536 count as 65536.  Device pointers; the call only enqueues on the context's stream: no host synchronisation, no
 *   device-to-host copy, no workgroup waits for another.  The raise phase is complete before the relaxation reads g.
 *   Scratch: that of sc_cost_field_batch, a second block of traversability masks of the same size, and about 28 B more per
 *   (field, 64 x 64 tile); grows only.
 * sc_cost_field_weighted_update_batch: the same for fields of sc_cost_field_weighted_batch; pen_old, pen_new uint8
 *   [G][H][W], pen_cap the one g was computed with.
 * The _host forms take host pointers, refuse a negative g value (SC_ERR_INVALID) before any launch, copy, run, copy g,
 *   fstatus and stats back and synchronise. */
#ifndef SEA_CURRENT_HIP_UPDATE_H
#define SEA_CURRENT_HIP_UPDATE_H
#include "sea_current_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int sc_cost_field_update_batch(sc_ctx* ctx, const int32_t* d2_old, const int32_t* d2_new, int G, const int32_t* fgrid, int W, int H,
                               int32_t r2_clear, const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus, int32_t* stats);
int sc_cost_field_update_batch_host(sc_ctx* ctx, const int32_t* d2_old, const int32_t* d2_new, int G, const int32_t* fgrid, int W, int H,
                                    int32_t r2_clear, const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus,
                                    int32_t* stats);
int sc_cost_field_weighted_update_batch(sc_ctx* ctx, const int32_t* d2_old, const uint8_t* pen_old, const int32_t* d2_new,
                                        const uint8_t* pen_new, int pen_cap, int G, const int32_t* fgrid, int W, int H, int32_t r2_clear,
                                        const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus, int32_t* stats);
int sc_cost_field_weighted_update_batch_host(sc_ctx* ctx, const int32_t* d2_old, const uint8_t* pen_old, const int32_t* d2_new,
                                             const uint8_t* pen_new, int pen_cap, int G, const int32_t* fgrid, int W, int H,
                                             int32_t r2_clear, const int32_t* root, int F, int rounds, int32_t* g, int32_t* fstatus,
                                             int32_t* stats);

#ifdef __cplusplus
}
#endif
#endif
