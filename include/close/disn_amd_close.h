/*
 * disn_amd_close.h -- closing of manifold device meshes: consistent orientation and hole filling.  The tenth header of
 * libdisn_amd.so, in a directory of its own as include/repair/.  Conventions, error codes and DISN_ABI_VERSION are those
 * of disn_amd.h, which this header includes and leaves as it is; the entries below are additions to the same library.
 * The stage stands behind disn_mesh_repair_*, whose output never has status 16, and makes true what
 * disn_mesh_check_batch reports as `closed` and `oriented`.
 *
 * B meshes back to back as the meshers and the mesh stages leave them: verts [sum nv][3], faces [sum nf][3] int32 with
 * indices LOCAL to their mesh, v_off_host / f_off_host [B+1] int64 ascending from 0.  Limits: those of
 * disn_mesh_clean_* (sum nf <= INT32_MAX/3, sum nv <= INT32_MAX); disn_mesh_close_workspace_bytes is 0 beyond them.
 * ONE count call, ONE read-back of the [B][DISN_CLOSE_FIELDS] sizes, ONE emit call; every launch on the caller's
 * stream, no host synchronisation inside.
 *
 * THE RULE is postprocess.close_arrays (disn_amd/postprocess.py), restated operation by operation: the same integers
 * and the same position bits.
 *   status    0 ok; 2 a face index outside [0, nv_b); 4 a coordinate that is not finite; 16 (not manifold) a face with
 *             a repeated index, an undirected edge held by three or more corner pairs, or a vertex on more than two
 *             boundary edges: tests on integers alone, made where every index is valid; 3 a table is full (sized for at
 *             most half of its slots: not reached).  Of several, the largest.  A mesh with a status comes back
 *             UNCHANGED: NV_OUT = nv_b, NF_OUT = nf_b, vmap and kept the identity, every other field 0.  An empty mesh
 *             has status 0 and zeros.
 *   edges     as disn_mesh_repair_*: face (a, b, c) gives the corner pairs (a, b), (b, c), (c, a), corner 3 f + k is
 *             pair k of face f.  An undirected edge held by two pairs makes its faces PARTNERS; held by one, it is
 *             boundary.
 *   orient    (flag DISN_CLOSE_ORIENT; without it COMPONENTS, UNORIENTABLE_COMPONENTS and FLIPPED_FACES are 0)  The
 *             components are the classes of faces under "partners" (COMPONENTS); a component's root is its smallest
 *             face.  Two partners are related by 1 when their pairs at the shared edge run the same way, else by 0.  A
 *             component is orientable when every face can be given a parity, the root 0, such that every relation
 *             holds; the parity is then unique.  A non-orientable component (UNORIENTABLE_COMPONENTS) keeps its faces
 *             as they are; it is still filled.  Of an orientable one, n0 and n1 count the faces of parity 0 and 1 and
 *             K = 1 if n1 > n0 else 0: the majority stays, a tie keeps the root.  Every face of parity != K is written
 *             as (a, c, b) (FLIPPED_FACES).  A consistent component is never touched without DISN_CLOSE_OUTWARD.
 *   fill      (flag DISN_CLOSE_FILL; without it LOOPS, FILLED_LOOPS and FILL_FACES are 0)  Boundary vertices joined by
 *             a boundary pair belong to one loop; its id is its smallest vertex, its length L its number of boundary
 *             pairs (LOOPS).  A loop with L <= max_hole (at most DISN_CLOSE_MAX_HOLE) is filled (FILLED_LOOPS): one new
 *             vertex c and, for every boundary pair (a -> b) of the loop, one face (c, b, a) -- (c, a, b) when the
 *             pair's face is flipped (FILL_FACES).  A fan from a centre never names an edge the mesh already has.
 *             The centre: E = the frexp exponent of the mesh's largest |coordinate| (0 when that is 0);
 *             q(x) = rint((double)x 2^(40-E)) as int64 of every coordinate of the tail a of every boundary pair of the
 *             loop, in the input's orientation; S = their sum; centre = (float)((double)S / (double)L * 2^(E-40)).
 *   outward   (flag DISN_CLOSE_OUTWARD, needs DISN_CLOSE_ORIENT; wrong for cavities)  on the orientable components with
 *             no unfilled boundary pair: t_f = ((x0 c0 + y0 c1) + z0 c2) / 6, c = p1 x p2, as disn_mesh_check_batch
 *             writes its volume terms, of an input face as it came and of a fill face as (c, b, a);
 *             tq_f = rint(t_f 2^(30-3E)) as int64; V = the sum of tq_f over the component's faces, fill faces
 *             included, + for parity K, - otherwise, a fill face having the parity of its pair's face.  V < 0: K
 *             becomes 1 - K.
 *   numbering verts_out = the nv_b input vertices in place (unreferenced ones stay), then one centre per filled loop in
 *             ascending loop id; faces_out = the nf_b input faces in order, then the fill faces in ascending corner of
 *             their pairs.  vmap_out[i] = i for an input vertex, the loop id for a centre; kept_out[f] = f for an
 *             input face, the pair's face for a fill face.  NV_OUT = nv_b + FILLED_LOOPS, NF_OUT = nf_b + FILL_FACES.
 * Guarantee, for status 0 with both flags and no loop over max_hole: disn_mesh_check_batch of the output reports no
 * boundary edge, no non-manifold edge, the non-manifold vertices of the input, and no misoriented edge when
 * UNORIENTABLE_COMPONENTS is 0.  Limits: a fan over a non-planar loop may intersect itself or the mesh; caps are flat;
 * non-orientable components stay as they are; a centre inherits the further per-vertex rows of its loop's id.
 *
 *   disn_mesh_close_count_batch  counts [B][DISN_CLOSE_FIELDS] int64: device.  Leaves in ws what the emit reads.
 *   disn_mesh_close_emit_batch   the same inputs, flags, max_hole and ws, untouched in between; counts_host: the counts
 *       read back.  verts_out [sum NV_OUT][3], faces_out [sum NF_OUT][3], vmap_out [sum NV_OUT], kept_out [sum NF_OUT]:
 *       device, the meshes back to back in input order; nothing is written beyond those sums.
 *   DISN_E_ARG for a missing pointer, B < 1, offsets that do not ascend from 0, unknown flag bits, OUTWARD without
 *   ORIENT, max_hole outside [0, DISN_CLOSE_MAX_HOLE] or counts_host beyond what the inputs allow; DISN_E_SHAPE beyond
 *   the limits; DISN_E_WS for a workspace below disn_mesh_close_workspace_bytes: all on the host, before anything is
 *   enqueued or written.
 * No kernel waits for another workgroup.  The probe loop of the edge table is bounded by the table's size; every walk
 * of the two union-finds goes strictly downwards.  The atomics are 32- and 64-bit integer ones: no floating-point
 * atomic, so no sum depends on its order.  The host arrays must stay valid until the stream has passed the call.
 */
#ifndef DISN_AMD_CLOSE_H
#define DISN_AMD_CLOSE_H

#include "../disn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DISN_CLOSE_NV_OUT 0
#define DISN_CLOSE_NF_OUT 1
#define DISN_CLOSE_STATUS 2
#define DISN_CLOSE_COMPONENTS 3
#define DISN_CLOSE_UNORIENTABLE_COMPONENTS 4
#define DISN_CLOSE_FLIPPED_FACES 5
#define DISN_CLOSE_LOOPS 6
#define DISN_CLOSE_FILLED_LOOPS 7
#define DISN_CLOSE_FILL_FACES 8
#define DISN_CLOSE_FIELDS 9

#define DISN_CLOSE_ORIENT 1            /* flags */
#define DISN_CLOSE_FILL 2
#define DISN_CLOSE_OUTWARD 4
#define DISN_CLOSE_MAX_HOLE 4194304    /* 2^22: with |q| <= 2^40 a loop's sum stays within int64 */
#define DISN_CLOSE_STATUS_NOT_MANIFOLD 16

size_t disn_mesh_close_workspace_bytes(int B, int64_t nv_total, int64_t nf_total);
int disn_mesh_close_count_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                const int64_t* f_off_host, int B, int flags, int64_t max_hole, int64_t* counts,
                                void* ws, size_t ws_bytes, void* stream);
int disn_mesh_close_emit_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                               const int64_t* f_off_host, int B, int flags, int64_t max_hole,
                               const int64_t* counts_host, float* verts_out, int32_t* faces_out, int32_t* vmap_out,
                               int32_t* kept_out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DISN_AMD_CLOSE_H */
