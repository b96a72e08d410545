/*
 * disn_amd_check.h -- topology, orientation and self-intersection checks of device meshes: the eighth header of
 * libdisn_amd.so, one directory below the first five, as include/dc/.  Conventions, error codes and DISN_ABI_VERSION are
 * those of disn_amd.h, which this header includes and leaves as it is; the entries below are additions to the same
 * library.  The stage measures; it changes and repairs nothing.
 *
 * B meshes back to back as disn_mc_emit_batch, disn_dc_emit_batch and the mesh stages leave them: verts [sum nv][3],
 * faces [sum nf][3] int32 with indices LOCAL to their mesh, v_off_host / f_off_host [B+1] int64 ascending from 0.
 * Limits: those of disn_mesh_clean_* (sum nf <= INT32_MAX/3, sum nv <= INT32_MAX) and sum nf <= DISN_CHECK_MAX_FACES
 * (a slot of the cell table is a uint32); disn_mesh_check_workspace_bytes is 0 beyond them.
 *
 * THE RULE is postprocess.check_arrays (disn_amd/postprocess.py), restated operation by operation.  The counts are
 * integers; the geometry is float64 + - x and sqrt on the float32 coordinates, each rounded once, in the order written,
 * no fused multiply-add (mesh_check.hip is compiled without contraction).
 *   part      a face with a repeated index counts in INDEX_DEGENERATE_FACES and takes no further part.  Every other
 *             face gives the corner pairs (a, b), (b, c), (c, a)
 *   topology  UNREFERENCED_VERTICES: named by no face that takes part.  EDGES: the distinct undirected {i, j};
 *             BOUNDARY_EDGES: held by exactly one corner pair; NONMANIFOLD_EDGES: by three or more; MISORIENTED_EDGES:
 *             by exactly two, both from the smaller index or both from the larger (orientation is not judged on a
 *             non-manifold edge).  NONMANIFOLD_VERTICES: two corners (f, i), (g, i) of vertex i are related when f and
 *             g share an undirected edge {i, j}, however many faces hold it; a fan is a class of the transitive closure;
 *             the field counts the vertices with two or more fans (a bow-tie counts; a vertex on a four-face edge all
 *             of whose corners are related does not: the edge is counted already).  EULER = referenced vertices -
 *             EDGES + faces that take part
 *   geometry  u = p1 - p0, w = p2 - p0, cross = (u1 w2 - u2 w1, u2 w0 - u0 w2, u0 w1 - u1 w0).  ZERO_AREA_FACES:
 *             faces that take part with cross == (0, 0, 0), either sign.  sums[b][0] = area = the sum of
 *             0.5 sqrt((c0 c0 + c1 c1) + c2 c2); sums[b][1] = volume = the sum of ((x0 d0 + y0 d1) + z0 d2) / 6,
 *             d = p1 x p2 written as cross is.  The ORDER of the two sums is the implementation's and fixed: slab s of
 *             DISN_CHECK_SLABS holds the faces [s n / SLABS, (s+1) n / SLABS) of its mesh (n = nf_b), thread t of 256
 *             adds the slab's faces t, t + 256, .. in ascending order, the 256 partial sums meet in a binary tree
 *             (stride 128, 64, .. 1), and the slabs are added in ascending order.  A function of nf_b alone: the same
 *             bits from run to run and in any batch.  No floating-point atomic.
 *   pairs     among the faces that take part.  CANDIDATE_PAIRS: pairs f < g whose float32 bounding boxes overlap,
 *             closed (lo_f <= hi_g and lo_g <= hi_f on every axis): exact, whatever the broad phase.
 *             orient(a, b, c, d) = (u0 (v1 w2 - v2 w1) - u1 (v0 w2 - v2 w0)) + u2 (v0 w1 - v1 w0), u = b - a, v = c - a,
 *             w = d - a.  An edge (p, q) PIERCES a triangle (a, b, c) when orient(a,b,c,p) orient(a,b,c,q) < 0 (the
 *             float64 product) and orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) are all > 0 or all < 0.  A pair
 *             INTERSECTS when one of the edges (p0,p1), (p1,p2), (p2,p0) of either face pierces the other.  Every zero
 *             is a no: touching at a vertex or along an edge and coplanar overlaps do not count; two faces that share
 *             an edge have an end of every edge on the other's plane.  INTERSECTING_PAIRS; INTERSECTING_FACES: faces
 *             in at least one such pair
 *   cap       max_pairs_host[b] candidate pairs (the Python default: DISN_CHECK_PAIRS_PER_FACE nf_b + 4096).  A mesh
 *             with CANDIDATE_PAIRS above it gets status 8 (DISN_CHECK_PAIRS) and INTERSECTING_* = -1; nothing of its
 *             narrow phase runs.  The device ALSO gives status 8, before it counts the candidates, when its work
 *             estimate -- the sum over the grid cells of n (n - 1) / 2, n the faces listed in the cell, plus (large
 *             faces) x nf_b -- exceeds DISN_CHECK_WORK_FACTOR max_pairs_host[b] + 4096; CANDIDATE_PAIRS is then -1 too
 *   status    0 ok; 2 a face index outside [0, nv_b): only NV and NF are valid; 3 the edge table is full (sized for at
 *             most half of its slots: not reached), as 2; 4 a coordinate that is not finite: the topological fields are
 *             valid, the geometric ones not; 8 as above.  Of several, the largest.  An invalid count is -1, an invalid
 *             sum 0.  An empty mesh has status 0 and zeros.
 *   face_flags [sum nf] uint8, NULL ok: 1 in an intersecting pair, 2 zero area or a repeated index, 4 on a boundary
 *             edge, 8 on a non-manifold edge, 16 on a misoriented edge; a bit whose field is invalid stays 0.
 *
 *   disn_mesh_check_batch  counts [B][DISN_CHECK_FIELDS] int64, sums [B][2] float64, status [B] int32: device.
 *       DISN_E_ARG for a missing pointer, offsets that do not ascend from 0 or a negative cap; DISN_E_SHAPE beyond the
 *       limits; DISN_E_WS for a workspace below disn_mesh_check_workspace_bytes: all on the host, before anything is
 *       enqueued or written.  max_pairs_total of the workspace query is reserved (the workspace holds no pair list) and
 *       must be >= 0.
 * Not covered: connected components (disn_mesh_components_device reports them), duplicate faces (they show as
 * non-manifold edges), coplanar overlaps, any repair.
 * No kernel waits for another workgroup; every probe loop is bounded by its table's size, every walk of the union-find
 * goes strictly downwards; the atomics are 32- and 64-bit integer ones; no host synchronisation and no read-back.  The
 * host arrays must stay valid until the stream has passed the call.
 */
#ifndef DISN_AMD_CHECK_H
#define DISN_AMD_CHECK_H

#include "../disn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DISN_CHECK_NV 0
#define DISN_CHECK_NF 1
#define DISN_CHECK_UNREFERENCED_VERTICES 2
#define DISN_CHECK_INDEX_DEGENERATE_FACES 3
#define DISN_CHECK_EDGES 4
#define DISN_CHECK_BOUNDARY_EDGES 5
#define DISN_CHECK_NONMANIFOLD_EDGES 6
#define DISN_CHECK_MISORIENTED_EDGES 7
#define DISN_CHECK_NONMANIFOLD_VERTICES 8
#define DISN_CHECK_EULER 9
#define DISN_CHECK_ZERO_AREA_FACES 10
#define DISN_CHECK_CANDIDATE_PAIRS 11
#define DISN_CHECK_INTERSECTING_PAIRS 12
#define DISN_CHECK_INTERSECTING_FACES 13
#define DISN_CHECK_FIELDS 14

#define DISN_CHECK_PAIRS 8            /* the status of a mesh over its cap */
#define DISN_CHECK_PAIRS_PER_FACE 256
#define DISN_CHECK_WORK_FACTOR 8
#define DISN_CHECK_SLABS 32
#define DISN_CHECK_MAX_FACES (1 << 27)

#define DISN_CHECK_FLAG_INTERSECTS 1
#define DISN_CHECK_FLAG_DEGENERATE 2
#define DISN_CHECK_FLAG_BOUNDARY 4
#define DISN_CHECK_FLAG_NONMANIFOLD 8
#define DISN_CHECK_FLAG_MISORIENTED 16

size_t disn_mesh_check_workspace_bytes(int B, int64_t nv_total, int64_t nf_total, int64_t max_pairs_total);
int disn_mesh_check_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                          const int64_t* f_off_host, int B, const int64_t* max_pairs_host, int64_t* counts,
                          double* sums, uint8_t* face_flags, int32_t* status, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DISN_AMD_CHECK_H */
