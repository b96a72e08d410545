/*
 * disn_amd_simplify.h -- mesh simplification by quadric vertex clustering on the device: the second header of
 * libdisn_amd.so.  Conventions, error codes and DISN_ABI_VERSION are those of disn_amd.h, which this header includes
 * and leaves as it is; the entries below are additions to the same library.
 *
 * B meshes back to back as disn_mc_emit_batch and disn_mesh_clean_emit_batch leave them: verts [sum nv][3], faces
 * [sum nf][3] int32 with indices LOCAL to their mesh, v_off_host / f_off_host [B+1] int64 ascending from 0; limits as
 * disn_mesh_clean_*: sum nf <= INT32_MAX/3, sum nv <= INT32_MAX (disn_mesh_simplify_workspace_bytes is 0 beyond them).
 *
 * THE RULE is postprocess.simplify_arrays (disn_amd/postprocess.py), restated operation by operation; mesh b has the
 * lattice lattice_host[b] = {origin x, y, z, h} (doubles) of cells_host[b] cells per axis, 1 <= cells <= 1024, h > 0:
 *   cell      per axis floorf((v - (float)origin) * (float)(1 / h)), clamped to [0, cells-1]; the vertices of one cell
 *             are a cluster; clusters are numbered by their smallest member vertex
 *   faces     a face whose three clusters are not distinct is dropped; with dedup != 0 only the smallest face index
 *             survives among the faces of one unordered cluster triple; survivors keep their order and orientation
 *   sums      per cluster, as int64 multiples of 2^-32 (rint of reals of magnitude <= 1; integer atomic adds, so the
 *             sums do not depend on the order): the ten entries of w [n;d][n;d]^T of every face that touches it, the
 *             three sums of its members' positions in the cell, the member count
 *   position  x = the minimiser of the regularised quadric by the adjugate in float64, clipped to the cell;
 *             v' = (float)(centre + h x)
 *
 *   disn_mesh_simplify_count_batch  counts [B][4] int64 (device) = {output vertices, output faces, faces dropped as
 *       duplicates, status} per mesh.  status: 0 ok; 2 a face index outside [0, nv_b) (the first kernel compares every
 *       index with its mesh's size, every later one skips that mesh: nothing is addressed through an unchecked
 *       index); 3 internal table full; 4 a vertex coordinate that is not finite; 5 CAPACITY OF THE KEY LAYOUT: with
 *       dedup the key of a face is its three cluster numbers, counted through the batch, 21 bits each -- a mesh
 *       whose faces reach cluster number 2^21 = 2 097 152 of the batch gets status 5 (split the batch, or dedup = 0).
 *       A mesh with a status has sizes 0 and leaves its neighbours as they are alone.  An empty mesh: all 0.
 *   disn_mesh_simplify_emit_batch   after the caller read `counts` back (sizes_host; same ws, untouched in between --
 *       it holds the lattices -- and the same meshes): out_verts [sum nv'][3], out_faces [sum nf'][3] (local again), first
 *       [sum nv'] = the smallest member (local) of every output vertex, vmap [sum nv] = the output vertex (local) of
 *       every input vertex (-1 throughout a mesh with a status).
 * No kernel waits for another workgroup; every probe loop is bounded by its table's size; there is no floating-point
 * atomic; no host synchronisation.  The host arrays must stay valid until the stream has passed the call.
 */
#ifndef DISN_AMD_SIMPLIFY_H
#define DISN_AMD_SIMPLIFY_H

#include "disn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DISN_SIMPLIFY_MAX_CELLS 1024

size_t disn_mesh_simplify_workspace_bytes(int B, int64_t nv_total, int64_t nf_total);
int disn_mesh_simplify_count_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                   const int64_t* f_off_host, const double* lattice_host, const int32_t* cells_host,
                                   int B, int dedup, int64_t* counts, void* ws, size_t ws_bytes, void* stream);
int disn_mesh_simplify_emit_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                  const int64_t* f_off_host, int B, const int64_t* sizes_host, float* out_verts,
                                  int32_t* out_faces, int32_t* vmap, int32_t* first, void* ws, size_t ws_bytes,
                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DISN_AMD_SIMPLIFY_H */
