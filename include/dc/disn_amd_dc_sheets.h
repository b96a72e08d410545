/*
 * disn_amd_dc_sheets.h -- per-sheet dual contouring of B signed-distance grids from Hermite data: a third mesher beside
 * disn_mc_*_batch and disn_dc_*_batch, in the same library.  Conventions, error codes and DISN_ABI_VERSION are those of
 * disn_amd.h; disn_amd_dc.h, which this header includes, states the grids, the boxes, the Hermite points, the grid
 * normals, the quadric, the position and the faces, and stays as it is.  The entries below are additions.
 *
 * disn_dc_*_batch puts ONE vertex into a cell, which serves every sheet of the surface that crosses the cell: thin
 * plates and parts closer than a cell are welded, and edges carry more than two faces.  Here a cell gets one vertex per
 * SHEET.  THE RULE is isosurface.dual_contour_sheets_arrays (disn_amd/isosurface.py), restated operation by operation
 * (dual_contour_sheets.hip is compiled without contraction):
 *   case      of a cell: bit i set when corner i is inside (vol < iso); corners 0 .. 7 at (0,0,0) (1,0,0) (1,1,0) (0,1,0)
 *             (0,0,1) (1,0,1) (1,1,1) (0,1,1), the numbering of the marching-cubes table (tools/gen_mc_tables.py)
 *   loops     the cut edges of a case are paired face by face (an ambiguous face by the table's one rule) and close into
 *             loops, one per sheet; every cut edge lies on exactly one.  A case has 0 .. 4 loops of 3 .. 7 edges,
 *             numbered by their smallest cube-edge id (csrc/mc_loops.h: kMcNloop, kMcLoop; tools/gen_mc_loops.py)
 *   vertices  the cells in flat (iz, iy, ix) order, the loops of a cell in loop-id order:
 *             id = (exclusive scan of kMcNloop[case] over the cells)[cell] + loop.  nv = the sum of the loop counts
 *   quadric   disn_amd_dc.h's, restricted to the loop's edges: visited in cube-edge-id order, the same float64
 *             arithmetic, the same rule for rows whose s is not finite and positive, the mean m over the LOOP's edges
 *             only, the same lam, solve, fallback to m and clip to the cell.  A loop in a one-loop cell has the vertex
 *             of disn_dc_emit_batch bit for bit; a batch whose active cells all have one loop gives its meshes bit for bit
 *   faces     the quads, their order, the split, the tie rule and the winding of disn_amd_dc.h; ne and nf are its ne and
 *             nf.  The index of cell q_k is base[cell] + kMcLoop[case(cell)][e], e the cube edge under which that cell
 *             sees the grid edge: for an edge of axis a and cell offset (du, dv), the cube edge of axis a whose low
 *             corner lies at (-du, -dv) on the (u, v) axes (csrc/mc_loops.h: kMcQuadEdge)
 * The limits of disn_amd_dc.h, and 4 B R^3 < 2^32: the loop ranks go through the same 32-bit scan.
 * (disn_dcs_workspace_bytes is 0 beyond them, the entries return DISN_E_SHAPE.)
 * KNOWN LIMIT that remains.  When two cells share an ambiguous face (four cut edges) and in BOTH cells both of that
 * face's segments lie on one loop, the two dual edges across the face join the same two vertices: that edge carries four
 * faces (three where a quad is missing at the grid's boundary).  It shows on plates close to one cell thick and on
 * noise; curing it means re-pairing such faces per grid, which is not built.  Triangles may be degenerate in position,
 * never in index.  reg: as disn_amd_dc.h.
 *
 *   disn_dcs_workspace_bytes    the workspace every entry below takes
 *   disn_dcs_count_batch        counts [B][3] int64 (device) = {ne, nv, nf}; fills ws for the other three entries, which
 *                               must be given the SAME sdf, B, R, iso and ws, unchanged in between
 *   disn_dcs_points_batch       points [sum ne][3] float32: those of disn_dc_points_batch
 *   disn_dcs_grid_normals_batch normals [sum ne][3] float32: those of disn_dc_grid_normals_batch
 *   disn_dcs_emit_batch         points, normals [sum ne][3] (device, read) -> verts [sum nv][3] float32, faces
 *                               [sum nf][3] int32, LOCAL to their grid; 0 < reg <= 1
 * The workspaces of the two families are not interchangeable.  DISN_E_ARG for a NULL pointer, a non-positive B or R, a
 * reg outside (0, 1] or not a number; DISN_E_SHAPE beyond the limits; DISN_E_WS for a workspace below
 * disn_dcs_workspace_bytes.  Every refusal is made on the host before anything is enqueued.  One thread per cell sums
 * the at most 7 rows of each of its loops in float64 registers: there are no atomics of any kind, no kernel waits for
 * another workgroup, and no entry synchronises with the host or reads back.
 */
#ifndef DISN_AMD_DC_SHEETS_H
#define DISN_AMD_DC_SHEETS_H

#include "disn_amd_dc.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t disn_dcs_workspace_bytes(int B, int R);
int disn_dcs_count_batch(const float* sdf, int B, int R, float iso, uint64_t* counts, void* ws, size_t ws_bytes,
                         void* stream);
int disn_dcs_points_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, float* points,
                          void* ws, size_t ws_bytes, void* stream);
int disn_dcs_grid_normals_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso,
                                float* normals, void* ws, size_t ws_bytes, void* stream);
int disn_dcs_emit_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, const float* points,
                        const float* normals, double reg, float* verts, int32_t* faces, void* ws, size_t ws_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DISN_AMD_DC_SHEETS_H */
