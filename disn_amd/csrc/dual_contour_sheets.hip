// Per-sheet dual contouring (include/dc/disn_amd_dc_sheets.h): a third mesher beside marching_cubes.hip and
// dual_contour.hip.  One vertex per (cell, loop): the cut edges of a cell's marching-cubes case lie on closed loops, one
// per sheet of the surface in the cell (mc_loops.h, derived by tools/gen_mc_loops.py), and each loop gets the vertex
// that the quadric of ITS crossings places.  THE RULE is isosurface.dual_contour_sheets_arrays, restated operation by
// operation (THIS FILE IS COMPILED WITH -ffp-contract=off); the header states it in full.
//
// Points, grid normals, the quadric with its solve and the split of a quad are dual_contour.hip's, shared through
// dual_contour_common.hpp; so is the workspace, whose cell "flag" here is the cell's loop count 0 .. 4 and whose cell
// scan therefore gives the first vertex id of every cell.  Passes: flags -> three exclusive scans -> sizes; points;
// grid normals; vertices (one thread per cell with a loop: the case from the 8 corners, then per loop its at most 7 rows
// summed in float64 registers in cube-edge order: no atomics); faces (one thread per edge with a quad: the case of each
// of the four cells, its loop of the edge).  The loop table is constant data of the library.
#include "dual_contour_common.hpp"

#include "../../include/dc/disn_amd_dc_sheets.h"

#include "mc_loops.h"       // kMcNloop, kMcLoop, kMcQuadEdge (DISN_MC_QUAL is __constant__ const here)

namespace disn {

// pass 1: the cell's flag is the number of its loops
__global__ __launch_bounds__(256) void dcs_flags_batch_kernel(const float* __restrict__ vol, int n, unsigned np,
                                                              unsigned total, float iso,
                                                              unsigned* __restrict__ eflag,
                                                              unsigned* __restrict__ qflag,
                                                              unsigned* __restrict__ cflag) {
  const unsigned R = (unsigned)n - 1, nc = R * R * R;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    const unsigned b = (unsigned)q / np, p = (unsigned)q - b * np;
    const int ix = (int)(p % n), iy = (int)((p / n) % n), iz = (int)(p / ((size_t)n * n));
    const int c = dc_flags_point(vol + (size_t)b * np, n, iso, p, ix, iy, iz, eflag + (size_t)3 * b * np,
                                 qflag + (size_t)3 * b * np);
    if (c >= 0) cflag[(size_t)b * nc + ((size_t)iz * R + iy) * R + ix] = (unsigned)kMcNloop[c];
  }
}

// pass 3: the vertices of a cell, one per loop in loop-id order, at the GLOBAL ranks cidx[cell] + loop.  An edge has a
// loop id exactly when it is cut, so the rank of every edge that is read is that of a point
__global__ __launch_bounds__(256) void dcs_verts_batch_kernel(const float* __restrict__ vol, DcBoxes boxes, int n,
                                                              unsigned np, unsigned b0, unsigned nb, float iso,
                                                              double reg, const unsigned* __restrict__ eidx,
                                                              const unsigned* __restrict__ cflag,
                                                              const unsigned* __restrict__ cidx,
                                                              const float* __restrict__ points,
                                                              const float* __restrict__ normals,
                                                              float* __restrict__ verts) {
  const unsigned R = (unsigned)n - 1, nc = R * R * R;
  const size_t first = (size_t)b0 * nc, total = (size_t)nb * nc;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    const int nl = (int)cflag[first + q];
    if (!nl) continue;
    const unsigned lb = (unsigned)q / nc, c = (unsigned)q - lb * nc;
    const int ix = (int)(c % R), iy = (int)((c / R) % R), iz = (int)(c / (R * R));
    const DcCell cell = dc_cell(dc_spec(boxes, lb, n), ix, iy, iz);
    const int cs = dc_cell_case(vol + (size_t)(b0 + lb) * np, n, iso, ix, iy, iz);
    const unsigned* ei = eidx + (size_t)3 * (b0 + lb) * np;
    float* o = verts + (size_t)cidx[first + q] * 3;
    for (int l = 0; l < nl; ++l) {
      DcQuadric Q;
      for (int e = 0; e < 12; ++e) {
        if ((int)kMcLoop[cs][e] != l) continue;
        Q.add(cell, points, normals, ei[dc_cube_edge_slot(n, ix, iy, iz, e)]);
      }
      Q.solve(cell, reg, o + 3 * l);
    }
  }
}

// pass 4: as dual_contour.hip's, the vertex of cell q_k being the one of the loop on which q_k has the edge
__global__ __launch_bounds__(256) void dcs_faces_batch_kernel(const float* __restrict__ vol, int n, unsigned np,
                                                              size_t total, float iso,
                                                              const unsigned* __restrict__ qflag,
                                                              const unsigned* __restrict__ qidx,
                                                              const unsigned* __restrict__ cidx,
                                                              const float* __restrict__ verts,
                                                              int* __restrict__ faces) {
  const unsigned R = (unsigned)n - 1, nc = R * R * R, ne = 3 * np;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    if (!qflag[q]) continue;
    const unsigned b = (unsigned)(q / ne), e = (unsigned)(q - (size_t)b * ne);
    const unsigned p = e / 3;
    const int a = (int)(e - 3 * p);
    const int ix = (int)(p % n), iy = (int)((p / n) % n), iz = (int)(p / ((unsigned)n * n));
    const unsigned* ci = cidx + (size_t)b * nc;
    const float* v = vol + (size_t)b * np;
    unsigned id[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int cx, cy, cz;
      dc_quad_cell(a, k, ix, iy, iz, &cx, &cy, &cz);
      const int cs = dc_cell_case(v, n, iso, cx, cy, cz);
      id[k] = ci[((size_t)cz * R + cy) * R + cx] + (unsigned)kMcLoop[cs][kMcQuadEdge[a][k]];   // the edge is cut: >= 0
    }
    dc_quad_faces(id, (int)ci[0], v[p] < iso, verts, faces + (size_t)qidx[q] * 6);
  }
}

// dual_contour.hip's limits, and the loop ranks (at most 4 per cell) through the same 32-bit scan
static bool dcs_batch_ok(int B, int R) {
  if (!dc_batch_ok(B, R)) return false;
  const unsigned long long r = (unsigned long long)R;
  return 4ull * (unsigned long long)B * r * r * r < (1ull << 32);
}

}  // namespace disn

// ---- the C entries of include/dc/disn_amd_dc_sheets.h: argument and workspace checks, then the launches ----
using namespace disn;

extern "C" {

size_t disn_dcs_workspace_bytes(int B, int R) { return dcs_batch_ok(B, R) ? dc_ws_bytes(B, R) : 0; }

int disn_dcs_count_batch(const float* sdf, int B, int R, float iso, uint64_t* counts, void* ws, size_t ws_bytes,
                         void* stream) {
  if (!sdf || !counts || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!dcs_batch_ok(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < dc_ws_bytes(B, R)) return DISN_E_WS;
  const DcWs w = dc_layout(ws, B, R);
  const int n = R + 1;
  const size_t np = (size_t)n * n * n;
  hipLaunchKernelGGL(dcs_flags_batch_kernel, dim3(dc_blocks_for(B * np)), dim3(256), 0, (hipStream_t)stream, sdf, n,
                     (unsigned)np, (unsigned)(B * np), iso, w.eflag, w.qflag, w.cflag);
  DISN_TRY(hipGetLastError());
  DISN_TRY(dc_scan_counts(w, B, R, reinterpret_cast<unsigned long long*>(counts), (hipStream_t)stream));
  return 0;
}

int disn_dcs_points_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, float* points,
                          void* ws, size_t ws_bytes, void* stream) {
  if (!sdf || !sdf_params_host || !points || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!dcs_batch_ok(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < dc_ws_bytes(B, R)) return DISN_E_WS;
  DISN_TRY(dc_hermite_launch(false, sdf, sdf_params_host, B, R, iso, points, dc_layout(ws, B, R), (hipStream_t)stream));
  return 0;
}

int disn_dcs_grid_normals_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso,
                                float* normals, void* ws, size_t ws_bytes, void* stream) {
  if (!sdf || !sdf_params_host || !normals || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!dcs_batch_ok(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < dc_ws_bytes(B, R)) return DISN_E_WS;
  DISN_TRY(dc_hermite_launch(true, sdf, sdf_params_host, B, R, iso, normals, dc_layout(ws, B, R), (hipStream_t)stream));
  return 0;
}

int disn_dcs_emit_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, const float* points,
                        const float* normals, double reg, float* verts, int32_t* faces, void* ws, size_t ws_bytes,
                        void* stream) {
  if (!sdf || !sdf_params_host || !points || !normals || !verts || !faces || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!(reg > 0.0 && reg <= 1.0)) return DISN_E_ARG;   // a NaN fails both comparisons
  if (!dcs_batch_ok(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < dc_ws_bytes(B, R)) return DISN_E_WS;
  const DcWs w = dc_layout(ws, B, R);
  const int n = R + 1;
  const size_t np = (size_t)n * n * n, nc = (size_t)R * R * R;
  for (int b0 = 0; b0 < B; b0 += kMcBatchBoxes) {
    const int nb = B - b0 < kMcBatchBoxes ? B - b0 : kMcBatchBoxes;
    hipLaunchKernelGGL(dcs_verts_batch_kernel, dim3(dc_blocks_for(nc * nb)), dim3(256), 0, (hipStream_t)stream, sdf,
                       dc_boxes(sdf_params_host, b0, nb, R), n, (unsigned)np, (unsigned)b0, (unsigned)nb, iso, reg,
                       w.eidx, w.cflag, w.cidx, points, normals, verts);
    DISN_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(dcs_faces_batch_kernel, dim3(dc_blocks_for(B * 3 * np)), dim3(256), 0, (hipStream_t)stream, sdf, n,
                     (unsigned)np, (size_t)B * 3 * np, iso, w.qflag, w.qidx, w.cidx, verts, faces);
  DISN_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
