// Dual contouring of the predicted field from Hermite data (include/dc/disn_amd_dc.h): a second mesher beside
// marching_cubes.hip.  One vertex per cell that the surface crosses, placed by a quadric error function built from the
// crossing points of the cell's cut edges and the field's normals at them; one quad (two triangles) per cut grid edge
// that has four cells around it.  THE RULE is isosurface.dual_contour_arrays, restated operation by operation (THIS
// FILE IS COMPILED WITH -ffp-contract=off); the header states it in full.
//
// The Hermite points are the vertices of disn_mc_emit, bit for bit and in order: grid_coord and the edge body restate
// marching_cubes.hip's (which stay file-static there, untouched), and tests compare the two on the device.  The device
// bodies that dual_contour_sheets.hip needs as well (points, grid normals, the quadric and its solve, the quad's split,
// the workspace) live in dual_contour_common.hpp; this file keeps what is its own: the cell flag and the two passes.
// Passes: flags (cut edges, edges with a quad, active cells) -> three exclusive scans (exclusive_scan of
// marching_cubes.hip) -> sizes; points; grid normals; vertices (one thread per ACTIVE cell, its at most 12 rows summed
// in float64 registers in cube-edge order: no atomics); faces (one thread per edge with a quad).  All are HBM-bound
// streaming passes; B grids share one scan and one read-back of the sizes, as in disn_mc_*_batch.
#include "dual_contour_common.hpp"

#include "../../include/dc/disn_amd_dc.h"

namespace disn {

// pass 1: a cell is active exactly when its eight corners are not all on one side
__global__ __launch_bounds__(256) void dc_flags_batch_kernel(const float* __restrict__ vol, int n, unsigned np,
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
    if (c >= 0) cflag[(size_t)b * nc + ((size_t)iz * R + iy) * R + ix] = (c != 0 && c != 255) ? 1u : 0u;
  }
}

// ---------------------------------------------------------------------------
// pass 3: one vertex per active cell.  The thread of a cell sums the rows of its own cut edges in cube-edge order
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dc_verts_batch_kernel(DcBoxes boxes, int n, unsigned np, unsigned b0,
                                                             unsigned nb, double reg,
                                                             const unsigned* __restrict__ eflag,
                                                             const unsigned* __restrict__ eidx,
                                                             const unsigned* __restrict__ cflag,
                                                             const unsigned* __restrict__ cidx,
                                                             const float* __restrict__ points,
                                                             const float* __restrict__ normals,
                                                             float* __restrict__ verts) {
  const unsigned R = (unsigned)n - 1, nc = R * R * R;
  const size_t first = (size_t)b0 * nc, total = (size_t)nb * nc;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    if (!cflag[first + q]) continue;
    const unsigned lb = (unsigned)q / nc, c = (unsigned)q - lb * nc;
    const int ix = (int)(c % R), iy = (int)((c / R) % R), iz = (int)(c / (R * R));
    const DcCell cell = dc_cell(dc_spec(boxes, lb, n), ix, iy, iz);
    const unsigned* ef = eflag + (size_t)3 * (b0 + lb) * np;
    const unsigned* ei = eidx + (size_t)3 * (b0 + lb) * np;
    DcQuadric Q;
    for (int e = 0; e < 12; ++e) {
      const size_t slot = dc_cube_edge_slot(n, ix, iy, iz, e);
      if (!ef[slot]) continue;
      Q.add(cell, points, normals, ei[slot]);      // the point's GLOBAL rank: points / normals are the batch's arrays
    }
    Q.solve(cell, reg, verts + (size_t)cidx[first + q] * 3);   // the vertex goes to its GLOBAL rank
  }
}

// ---------------------------------------------------------------------------
// pass 4: two triangles per cut edge with a quad.  The triangles go to their GLOBAL rank; their vertex ids are LOCAL to
// the grid (the grid's first vertex rank taken off).  Reads the positions pass 3 wrote (same stream, the launch before)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dc_faces_batch_kernel(const float* __restrict__ vol, int n, unsigned np,
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
    unsigned id[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int cx, cy, cz;
      dc_quad_cell(a, k, ix, iy, iz, &cx, &cy, &cz);
      id[k] = ci[((size_t)cz * R + cy) * R + cx];
    }
    dc_quad_faces(id, (int)ci[0], vol[(size_t)b * np + p] < iso, verts, faces + (size_t)qidx[q] * 6);
  }
}

static hipError_t dc_count_launch(const float* vol, int B, int R, float iso, unsigned long long* counts, void* ws,
                                  hipStream_t st) {
  const DcWs w = dc_layout(ws, B, R);
  const int n = R + 1;
  const size_t np = (size_t)n * n * n;
  hipLaunchKernelGGL(dc_flags_batch_kernel, dim3(dc_blocks_for(B * np)), dim3(256), 0, st, vol, n, (unsigned)np,
                     (unsigned)(B * np), iso, w.eflag, w.qflag, w.cflag);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : dc_scan_counts(w, B, R, counts, st);
}

}  // namespace disn

// ---- the C entries of include/dc/disn_amd_dc.h: argument and workspace checks, then the launches ----
using namespace disn;

extern "C" {

size_t disn_dc_workspace_bytes(int B, int R) { return dc_batch_ok(B, R) ? dc_ws_bytes(B, R) : 0; }

int disn_dc_count_batch(const float* sdf, int B, int R, float iso, uint64_t* counts, void* ws, size_t ws_bytes,
                        void* stream) {
  if (!sdf || !counts || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!dc_batch_ok(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < dc_ws_bytes(B, R)) return DISN_E_WS;
  DISN_TRY(dc_count_launch(sdf, B, R, iso, reinterpret_cast<unsigned long long*>(counts), ws, (hipStream_t)stream));
  return 0;
}

int disn_dc_points_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, float* points,
                         void* ws, size_t ws_bytes, void* stream) {
  if (!sdf || !sdf_params_host || !points || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!dc_batch_ok(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < dc_ws_bytes(B, R)) return DISN_E_WS;
  DISN_TRY(dc_hermite_launch(false, sdf, sdf_params_host, B, R, iso, points, dc_layout(ws, B, R), (hipStream_t)stream));
  return 0;
}

int disn_dc_grid_normals_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso,
                               float* normals, void* ws, size_t ws_bytes, void* stream) {
  if (!sdf || !sdf_params_host || !normals || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!dc_batch_ok(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < dc_ws_bytes(B, R)) return DISN_E_WS;
  DISN_TRY(dc_hermite_launch(true, sdf, sdf_params_host, B, R, iso, normals, dc_layout(ws, B, R), (hipStream_t)stream));
  return 0;
}

int disn_dc_emit_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, const float* points,
                       const float* normals, double reg, float* verts, int32_t* faces, void* ws, size_t ws_bytes,
                       void* stream) {
  if (!sdf || !sdf_params_host || !points || !normals || !verts || !faces || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!(reg > 0.0 && reg <= 1.0)) return DISN_E_ARG;   // a NaN fails both comparisons
  if (!dc_batch_ok(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < dc_ws_bytes(B, R)) return DISN_E_WS;
  const DcWs w = dc_layout(ws, B, R);
  const int n = R + 1;
  const size_t np = (size_t)n * n * n, nc = (size_t)R * R * R;
  for (int b0 = 0; b0 < B; b0 += kMcBatchBoxes) {
    const int nb = B - b0 < kMcBatchBoxes ? B - b0 : kMcBatchBoxes;
    hipLaunchKernelGGL(dc_verts_batch_kernel, dim3(dc_blocks_for(nc * nb)), dim3(256), 0, (hipStream_t)stream,
                       dc_boxes(sdf_params_host, b0, nb, R), n, (unsigned)np, (unsigned)b0, (unsigned)nb, reg, w.eflag,
                       w.eidx, w.cflag, w.cidx, points, normals, verts);
    DISN_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(dc_faces_batch_kernel, dim3(dc_blocks_for(B * 3 * np)), dim3(256), 0, (hipStream_t)stream, sdf, n,
                     (unsigned)np, (size_t)B * 3 * np, iso, w.qflag, w.qidx, w.cidx, verts, faces);
  DISN_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
