/*
 * disn_amd_smooth.h -- Taubin lambda|mu smoothing of device meshes: the fifth header of libdisn_amd.so.  Conventions,
 * error codes and DISN_ABI_VERSION are those of disn_amd.h, which this header includes and leaves as it is; the entries
 * below are additions to the same library.
 *
 * B meshes back to back as disn_mc_emit_batch, disn_mesh_clean_emit_batch and disn_mesh_simplify_emit_batch leave them:
 * verts [sum nv][3], faces [sum nf][3] int32 with indices LOCAL to their mesh, v_off_host / f_off_host [B+1] int64
 * ascending from 0; limits as disn_mesh_clean_*: sum nf <= INT32_MAX/3, sum nv <= INT32_MAX
 * (disn_mesh_smooth_workspace_bytes is 0 beyond them).  The faces never change: only out_verts [sum nv][3] is written.
 *
 * THE RULE is postprocess.smooth_arrays (disn_amd/postprocess.py), restated operation by operation.  It is integer sums
 * and float64 + - x / only (mesh_smooth.hip is compiled without contraction): no output bit rests on the order of a sum.
 *   edges     every face gives its three corner pairs (a, b), (b, c), (c, a); a pair of equal indices is ignored, so a
 *             degenerate face is legal; an undirected edge {i, j} counts once however many faces hold it.  N(i) = the
 *             distinct neighbours of i, deg(i) = |N(i)|
 *   boundary  an edge held by exactly ONE corner pair of the whole mesh is a boundary edge, its two ends are boundary
 *             vertices (a duplicated face makes its edges non-boundary)
 *   movable   deg(i) > 0 and, with pin_boundary != 0, no boundary vertex.  Any other vertex keeps its input bits, -0.0
 *             and denormals included
 *   step      t = 0 .. 2 iters - 1, factor s = lam for even t and mu for odd t; Jacobi: every vertex from the positions
 *             of the step before.  q(x) = (int64) rint((double) x 2^32); S_i = the int64 sum of q(v_j) over j in N(i);
 *             m_i = ((double) S_i 2^-32) / (double) deg(i); v'_i = (float) ((double) v_i + s (m_i - (double) v_i)),
 *             per coordinate, in float64 exactly as written, no fused multiply-add
 *   cap       max_move_host[b] = r >= 0: after every step each coordinate of v'_i is clamped in float64 to
 *             [(double) v0_i - r, (double) v0_i + r] before the cast, v0 the INPUT position: a box, no square root.
 *             r < 0, or max_move_host == NULL: no cap
 *   range     status 7 (DISN_SMOOTH_RANGE) for a mesh with a finite coordinate beyond +-1024 at input or after any step,
 *             or with a vertex of more than 2^20 distinct neighbours: within the bounds |S_i| < 2^20 2^10 2^32 = 2^62
 *
 *   disn_mesh_smooth_batch  1 <= iters <= DISN_SMOOTH_MAX_ITERS, 0 < lam <= 1, -1.5 <= mu < 0, every max_move_host[b]
 *       negative or finite (DISN_E_ARG otherwise, and for a missing pointer or offsets that do not ascend from 0);
 *       DISN_E_SHAPE beyond the limits; DISN_E_WS for a workspace below disn_mesh_smooth_workspace_bytes (nothing is
 *       written).  out_verts [sum nv][3] float32, status [B] int32 (device).
 *   status: 0 ok; 2 a face index outside [0, nv_b) (the first kernel compares every index with its mesh's size, every
 *       later one skips that mesh: nothing is addressed through an unchecked index); 3 the edge table is full (it is
 *       sized for at most half of its slots: not reached); 4 a vertex coordinate that is not finite; 7 the range, as
 *       above; of several, the largest.  A mesh with a status gets its INPUT vertices in out_verts and leaves its
 *       neighbours as they are; an empty mesh has status 0 and nothing is written for it.
 * No kernel waits for another workgroup; every probe loop is bounded by its table's size; the loop over the steps holds
 * no atomic (the build's are 32- and 64-bit integer ones); there is no floating-point atomic; no host synchronisation
 * and no read-back.  The host arrays must stay valid until the stream has passed the call.
 */
#ifndef DISN_AMD_SMOOTH_H
#define DISN_AMD_SMOOTH_H

#include "disn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DISN_SMOOTH_MAX_ITERS 64
#define DISN_SMOOTH_RANGE 7

size_t disn_mesh_smooth_workspace_bytes(int B, int64_t nv_total, int64_t nf_total);
int disn_mesh_smooth_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                           const int64_t* f_off_host, int B, int iters, double lam, double mu, int pin_boundary,
                           const double* max_move_host, float* out_verts, int32_t* status, void* ws, size_t ws_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DISN_AMD_SMOOTH_H */
