/*
 * disn_amd_dc.h -- dual contouring of B signed-distance grids from Hermite data: a second mesher beside
 * disn_mc_*_batch, in the same library.  Conventions, error codes and DISN_ABI_VERSION are those of disn_amd.h, which
 * this header includes and leaves as it is; the entries below are additions.  The header lives one directory below the
 * five headers of include/ (include/dc/), whose number and contents stay what they are.
 *
 * B grids [B][(R+1)^3] float32 of one R in .dist order (x fastest), boxes sdf_params_host [B][6] float64 on the HOST
 * = {x0, y0, z0, x1, y1, z1}, as disn_mc_emit_batch takes them; the same limits: R in 1 .. 1290 and
 * 3 B (R+1)^3 < 2^32 (disn_dc_workspace_bytes is 0 beyond them, the entries return DISN_E_SHAPE).  Outputs of the
 * grids lie back to back in grid order; face indices are LOCAL to their grid.
 *
 * THE RULE is isosurface.dual_contour_arrays (disn_amd/isosurface.py), restated operation by operation
 * (dual_contour.hip is compiled without contraction); n = R + 1, p = (iz n + iy) n + ix, inside = vol < iso, the axis
 * values ax_k[i] are the float32 values disn_mc_emit uses for the box.
 *   points    one Hermite point per cut grid edge, ranked in the flat order 3 p + axis: c0 + t (c1 - c0) on the cut axis,
 *             t = (iso - v0) / (v1 - v0), float32 -- bit for bit and in order the vertices of disn_mc_emit.  ne = their
 *             number
 *   cells     a cell of the R^3 cells is ACTIVE when any of its 12 edges is cut; its vertex id is its rank among the
 *             active cells in flat (iz, iy, ix) order.  nv = their number
 *   quadric   float64, world units, relative to the cell's low corner: d_i = (double) point_i - (double) corner.  The
 *             cell's cut edges in the order of the marching-cubes cube-edge ids 0 .. 11 (mc_tables.h, kMcEdge); a row
 *             with normal g (float32, ANY length): s = (gx gx + gy gy) + gz gz; if s is finite and > 0:
 *             A += g g^T / s, b -= g (g . d) / s (each entry (gi gj) / s, (gi ((gx dx + gy dy) + gz dz)) / s; no
 *             square root); otherwise the row adds nothing to A and b.  EVERY cut edge counts in the mean m of the d_i
 *   position  lam = (tr(A) reg) / 3 + 2^-40; x solves (A + lam I) x = lam m - b by the adjugate in the operation order
 *             of postprocess._simplify_solve; det <= 0 or x not finite: x = m.  x is clipped per axis to
 *             [0, (double) ax[i+1] - (double) ax[i]]; v = (float) ((double) corner + x)
 *   faces     the cut edges in rank order; an edge of axis a has a quad when its two other indices are in 1 .. R-1.
 *             (u, v) = the two axes after a in cyclic order (x: y z, y: z x, z: x y); the cells at (u, v) offsets
 *             (-1,-1), (0,-1), (0,0), (-1,0) are q0 .. q3.  Split along q0-q2 unless |q1-q3|^2 < |q0-q2|^2 (float64
 *             squared distances of the float32 positions, (dx^2 + dy^2) + dz^2), then along q1-q3; equality keeps
 *             q0-q2.  Low end of the edge inside: (q0,q1,q2), (q0,q2,q3), or (q0,q1,q3), (q1,q2,q3); otherwise each
 *             triangle has its last two indices swapped: the geometric normal points along +grad, the winding of
 *             disn_mc_emit.  nf = 2 x (cut edges with a quad).  Edges on the grid's boundary leave the surface open
 *   grid normals  (disn_dc_grid_normals_batch, for callers without a network) at the point of an edge of axis a between
 *             grid points p0, p1, float64 from the float32 values: g_a = (v1 - v0) / (c1 - c0);
 *             g_k = (1 - t) D_k(p0) + t D_k(p1) for k != a, t the float32 t above,
 *             D_k(p) = (vol[p + e_k] - vol[p - e_k]) / (ax_k[i+1] - ax_k[i-1]), indices clamped to the grid; cast to
 *             float32, NOT normalised
 * KNOWN LIMITS.  In a cell that the surface crosses in more than one sheet, ONE vertex serves every sheet: the mesh can
 * be non-manifold there.  Triangles may be degenerate in position (two cells' vertices can coincide on a shared face);
 * they are never degenerate in index.  reg = 2^-10 is what mesh simplification uses; whether it is the best value on a
 * trained network's normals has NOT been measured.
 *
 *   disn_dc_workspace_bytes    the workspace every entry below takes
 *   disn_dc_count_batch        counts [B][3] int64 (device) = {ne, nv, nf}; fills ws for the other three entries, which
 *                              must be given the SAME sdf, B, R, iso and ws, unchanged in between
 *   disn_dc_points_batch       points [sum ne][3] float32
 *   disn_dc_grid_normals_batch normals [sum ne][3] float32
 *   disn_dc_emit_batch         points, normals [sum ne][3] (device, read) -> verts [sum nv][3] float32, faces [sum nf][3]
 *                              int32; 0 < reg <= 1
 * DISN_E_ARG for a NULL pointer, a non-positive B or R, a reg outside (0, 1] or not a number; DISN_E_SHAPE beyond the
 * limits; DISN_E_WS for a workspace below disn_dc_workspace_bytes.  Every refusal is made on the host before anything is
 * enqueued.  One thread per cell sums its own at most 12 rows in float64 registers: there are no atomics of any kind,
 * no kernel waits for another workgroup, and no entry synchronises with the host or reads back.
 */
#ifndef DISN_AMD_DC_H
#define DISN_AMD_DC_H

#include "../disn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t disn_dc_workspace_bytes(int B, int R);
int disn_dc_count_batch(const float* sdf, int B, int R, float iso, uint64_t* counts, void* ws, size_t ws_bytes,
                        void* stream);
int disn_dc_points_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, float* points,
                         void* ws, size_t ws_bytes, void* stream);
int disn_dc_grid_normals_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso,
                               float* normals, void* ws, size_t ws_bytes, void* stream);
int disn_dc_emit_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, const float* points,
                       const float* normals, double reg, float* verts, int32_t* faces, void* ws, size_t ws_bytes,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DISN_AMD_DC_H */
