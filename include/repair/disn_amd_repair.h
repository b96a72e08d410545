/*
 * disn_amd_repair.h -- repair of device meshes to a manifold: weld, drop, stitch and split.  The ninth header of
 * libdisn_amd.so, in a directory of its own as include/dc/ and include/check/.  Conventions, error codes and
 * DISN_ABI_VERSION are those of disn_amd.h, which this header includes and leaves as it is; the entries below are
 * additions to the same library.  The stage acts on what disn_mesh_check_batch reports.
 *
 * B meshes back to back as disn_mc_emit_batch, disn_dc_emit_batch and the mesh stages leave them: verts [sum nv][3],
 * faces [sum nf][3] int32 with indices LOCAL to their mesh, v_off_host / f_off_host [B+1] int64 ascending from 0.
 * Limits: those of disn_mesh_clean_* (sum nf <= INT32_MAX/3, sum nv <= INT32_MAX); disn_mesh_repair_workspace_bytes is
 * 0 beyond them.  ONE count call, ONE read-back of the [B][DISN_REPAIR_FIELDS] sizes, ONE emit call, as
 * disn_mesh_clean_*; every launch on the caller's stream, no host synchronisation inside.
 *
 * THE RULE is postprocess.repair_arrays (disn_amd/postprocess.py), restated operation by operation.  Every output is a
 * function of integers and of the SIGNS of float64 expressions on the float32 coordinates: + - x only, each rounded
 * once, in the order written, no fused multiply-add (mesh_repair.hip is compiled without contraction).
 *   status    0 ok; 2 a face index outside [0, nv_b); 4 a coordinate that is not finite; 3 a table is full (sized for
 *             at most half of its slots: not reached).  Of several, the largest.  A mesh with a status comes back
 *             UNCHANGED: NV_OUT = nv_b, NF_OUT = nf_b, vmap and kept the identity, every other field 0.  An empty mesh
 *             has status 0 and zeros.
 *   weld      (flag DISN_REPAIR_WELD) vertices whose three float32 coordinates are equal after adding 0.0f (-0 equals
 *             +0) merge into the smallest index of their group; WELDED_VERTICES: the vertices merged away.  Without
 *             the flag every vertex stands for itself.  Everything below works on the welded indices.
 *   drop      a face with a repeated index (REPEATED_FACES).  Of several faces with the same unordered triple, all of
 *             one cyclic orientation, all but the smallest face index (DUPLICATE_FACES).  A triple held in BOTH
 *             orientations is a pillow: all its faces go (PILLOW_FACES).  Zero-area faces on three distinct positions
 *             stay.  The survivors keep their order and orientation.
 *   edges     of the survivors; face (a, b, c) gives the corner pairs (a, b), (b, c), (c, a).  An undirected edge held
 *             by exactly two corner pairs is regular and its two faces are PARTNERS there; one held by three or more is
 *             singular (SINGULAR_EDGES).
 *   stitch    (flag DISN_REPAIR_STITCH) on a singular edge of k faces, k even and k <= DISN_REPAIR_MAX_FAN.  lo < hi its
 *             ends, e = p_hi - p_lo, d_m = p_opp(m) - p_lo, r = the d of the edge's smallest face index.
 *               cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)
 *               dot(a, b)   = (a0 b0 + a1 b1) + a2 b2
 *               det(a, b, c) = (a0 (b1 c2 - b2 c1) - a1 (b0 c2 - b2 c0)) + a2 (b0 c1 - b1 c0)
 *             For every other face s_m = det(e, r, d_m), c_m = dot(cross(e, r), cross(e, d_m)); half 0 when s_m > 0 or
 *             (s_m == 0 and c_m > 0); half 1 when s_m < 0 or (s_m == 0 and c_m < 0); both zero: the edge fails.  Face m
 *             is BEFORE n when half_m < half_n, or the halves are equal and det(e, d_m, d_n) > 0; the reference is
 *             before everyone; rank_m = the number of faces before m.  The ranks must be a permutation of 0 .. k-1 (a
 *             tie or an inconsistency of rounding fails the edge; no sort is involved), and the direction of the
 *             corner pair (lo -> hi or not) must alternate around the cycle of ranks.  Then each face that runs
 *             hi -> lo, at rank q, is the partner of the face at rank (q + 1) mod k (STITCHED_EDGES).  An edge the rule
 *             does not apply to, or fails on, is CUT: no face has a partner there.
 *   split     the corners (f, i), (g, i) of partners f, g at an edge {i, j} are related, and so are their corners at j;
 *             the classes are the transitive closure.  A stitched edge two of whose pairs have the same (class at lo,
 *             class at hi) is pinched (PINCHED_EDGES; counted in STITCHED_EDGES too).  The classes are computed AGAIN
 *             with every pinched edge cut; that result is final.
 *   numbering first the referenced welded vertices in ascending order, each for the class of its smallest corner
 *             (corner 3 f + k of input face f), then one new vertex per further class in the order of the classes'
 *             smallest corners (ADDED_VERTICES).  Unreferenced and welded-away vertices disappear (DROPPED_VERTICES).
 *             NV_OUT = nv_b - DROPPED_VERTICES + ADDED_VERTICES <= 3 NF_OUT.  vmap_out[new] = the input vertex (local)
 *             whose position is copied; kept_out[new face] = the input face (local).
 * The result is manifold: every face has at most one partner per edge, so the corners of a vertex form paths and cycles
 * and a class touches a cut edge with at most its two path ends; the second pass only refines the classes, so distinct
 * pairs of an unpinched stitched edge keep distinct signatures.  Every output edge has at most two faces, every output
 * vertex one fan.  Not in scope: self-intersections, the other pairing at a pinched edge; orientation and the holes a cut
 * edge opens are disn_mesh_close_*'s (include/close/disn_amd_close.h).
 *
 *   disn_mesh_repair_count_batch  counts [B][DISN_REPAIR_FIELDS] int64: device.  Leaves in ws what the emit reads.
 *   disn_mesh_repair_emit_batch   the same inputs and ws, untouched in between; counts_host: the counts read back.
 *       verts_out [sum NV_OUT][3], faces_out [sum NF_OUT][3], vmap_out [sum NV_OUT], kept_out [sum NF_OUT]: device, the
 *       meshes back to back in input order; nothing is written beyond those sums.
 *   DISN_E_ARG for a missing pointer, B < 1, offsets that do not ascend from 0, unknown flag bits or counts_host beyond
 *   what the inputs allow; DISN_E_SHAPE beyond the limits; DISN_E_WS for a workspace below
 *   disn_mesh_repair_workspace_bytes: all on the host, before anything is enqueued or written.
 * No kernel waits for another workgroup.  Every probe loop is bounded by its table's size; a row of the rank rule has
 * at most DISN_REPAIR_MAX_FAN entries; every walk of the union-find goes strictly downwards.  The atomics are 32- and
 * 64-bit integer ones: no floating-point atomic.  The host arrays must stay valid until the stream has passed the call.
 */
#ifndef DISN_AMD_REPAIR_H
#define DISN_AMD_REPAIR_H

#include "../disn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DISN_REPAIR_NV_OUT 0
#define DISN_REPAIR_NF_OUT 1
#define DISN_REPAIR_STATUS 2
#define DISN_REPAIR_WELDED_VERTICES 3
#define DISN_REPAIR_REPEATED_FACES 4
#define DISN_REPAIR_DUPLICATE_FACES 5
#define DISN_REPAIR_PILLOW_FACES 6
#define DISN_REPAIR_SINGULAR_EDGES 7
#define DISN_REPAIR_STITCHED_EDGES 8
#define DISN_REPAIR_PINCHED_EDGES 9
#define DISN_REPAIR_ADDED_VERTICES 10
#define DISN_REPAIR_DROPPED_VERTICES 11
#define DISN_REPAIR_FIELDS 12

#define DISN_REPAIR_WELD 1            /* flags */
#define DISN_REPAIR_STITCH 2
#define DISN_REPAIR_MAX_FAN 16

size_t disn_mesh_repair_workspace_bytes(int B, int64_t nv_total, int64_t nf_total);
int disn_mesh_repair_count_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                 const int64_t* f_off_host, int B, int flags, int64_t* counts, void* ws,
                                 size_t ws_bytes, void* stream);
int disn_mesh_repair_emit_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                const int64_t* f_off_host, int B, int flags, const int64_t* counts_host,
                                float* verts_out, int32_t* faces_out, int32_t* vmap_out, int32_t* kept_out, void* ws,
                                size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DISN_AMD_REPAIR_H */
