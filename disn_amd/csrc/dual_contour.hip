// Dual contouring of the predicted field from Hermite data (include/dc/disn_amd_dc.h, include/dc/disn_amd_dc_sheets.h):
// the second and third mesher beside marching_cubes.hip.  One quad (two triangles) per cut grid edge that has four
// cells around it; the vertices of a cell are placed by a quadric error function built from the crossing points of
// cut edges and the field's normals at them.  Two RULES say which vertices a cell has:
//   per cell  (disn_dc_*):  one vertex per cell that the surface crosses, from all of its cut edges.  THE RULE is
//             isosurface.dual_contour_arrays
//   per sheet (disn_dcs_*): one vertex per (cell, loop): the cut edges of a cell's marching-cubes case lie on closed
//             loops, one per sheet of the surface in the cell (mc_loops.h, derived by tools/gen_mc_loops.py), and each
//             loop gets the vertex that the quadric of ITS crossings places.  THE RULE is
//             isosurface.dual_contour_sheets_arrays
// both restated operation by operation (THIS FILE IS COMPILED WITH -ffp-contract=off); the headers state them in full.
//
// The Hermite points are the vertices of disn_mc_emit_batch: the same kernel of grid_mesh.hpp, which also holds the
// axis values, the case, the flags of a grid point and the cut edge.  Passes: flags (cut edges, edges with a quad, what
// a cell adds to the vertex count) -> three exclusive scans (exclusive_scan of marching_cubes.hip) -> sizes; points;
// grid normals; vertices (one thread per cell with a vertex, the rows of each vertex summed in float64 registers in
// cube-edge order, the vertices of a cell in loop-id order: no atomics); faces (one thread per edge with a quad).  All
// are HBM-bound streaming passes; B grids share one scan and one read-back of the sizes, as in disn_mc_*_batch.  The
// three kernels and the entries are templates over the rule; the loop table is constant data of the library.
#include "grid_mesh.hpp"

#include "../../include/dc/disn_amd_dc_sheets.h"      // includes disn_amd_dc.h

#include "mc_loops.h"       // kMcNloop, kMcLoop, kMcQuadEdge (DISN_MC_QUAL is __constant__ const here)

namespace disn {
namespace {

// ---------------------------------------------------------------------------
// the two rules.  count: what a cell of that case adds to the vertex count (kMax at most); member: whether cube edge e
// (edge slot `slot` of the grid's flags ef) belongs to vertex l of the cell; offset: which of its vertices cell q_k
// gives to the quad of an edge of axis a (that edge is cut).  cell_case is the case as far as the rule reads it after
// pass 1: the per-cell rule takes membership from the cut flags and computes none
// ---------------------------------------------------------------------------
struct DcPerCell {
  static constexpr int kMax = 1;
  static __device__ __forceinline__ unsigned count(int cs) { return (cs != 0 && cs != 255) ? 1u : 0u; }
  static __device__ __forceinline__ int cell_case(const float* __restrict__, int, float, size_t) { return 0; }
  static __device__ __forceinline__ bool member(int, const unsigned* __restrict__ ef, size_t slot, int, int) {
    return ef[slot] != 0;
  }
  static __device__ __forceinline__ unsigned offset(int, int, int) { return 0u; }
};

struct DcPerSheet {
  static constexpr int kMax = 4;
  static __device__ __forceinline__ unsigned count(int cs) { return (unsigned)kMcNloop[cs]; }
  static __device__ __forceinline__ int cell_case(const float* __restrict__ vol, int n, float iso, size_t p) {
    return grid_cell_case(vol, n, iso, p);
  }
  // an edge has a loop id exactly when it is cut, so the rank of every edge that is read is that of a point
  static __device__ __forceinline__ bool member(int cs, const unsigned* __restrict__, size_t, int e, int l) {
    return (int)kMcLoop[cs][e] == l;
  }
  static __device__ __forceinline__ unsigned offset(int cs, int a, int k) {
    return (unsigned)kMcLoop[cs][kMcQuadEdge[a][k]];
  }
};

// ---------------------------------------------------------------------------
// pass 1: per grid point its three cut-edge flags and quad flags; for the low corner of a cell, the cell's count
// ---------------------------------------------------------------------------
template <class Rule>
__global__ __launch_bounds__(256) void dc_flags_batch_kernel(const float* __restrict__ vol, int n, unsigned np,
                                                             unsigned total, float iso,
                                                             unsigned* __restrict__ eflag,
                                                             unsigned* __restrict__ qflag,
                                                             unsigned* __restrict__ cflag) {
  const unsigned R = (unsigned)n - 1, nc = R * R * R;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    const unsigned b = (unsigned)q / np, p = (unsigned)q - b * np;
    const int ix = (int)(p % n), iy = (int)((p / n) % n), iz = (int)(p / ((size_t)n * n));
    bool cut[3];
    const int c = grid_flags_point(vol + (size_t)b * np, n, iso, p, ix, iy, iz, eflag + (size_t)3 * b * np, cut);
    // a cut edge has a quad when all four cells around it exist: its two other indices in 1 .. R-1
    const int hi = n - 2;
    const bool mx = ix >= 1 && ix <= hi, my = iy >= 1 && iy <= hi, mz = iz >= 1 && iz <= hi;
    unsigned* qf = qflag + (size_t)3 * b * np + (size_t)3 * p;
    qf[0] = (cut[0] && my && mz) ? 1u : 0u;
    qf[1] = (cut[1] && mz && mx) ? 1u : 0u;
    qf[2] = (cut[2] && mx && my) ? 1u : 0u;
    if (c >= 0) cflag[(size_t)b * nc + ((size_t)iz * R + iy) * R + ix] = Rule::count(c);
  }
}

// counts[b] = {points, vertices, triangles} of grid b: the difference of consecutive bases, the grand totals closing
// the last; two triangles per quad
__global__ void dc_batch_counts_kernel(const unsigned* __restrict__ eidx, const unsigned* __restrict__ cidx,
                                       const unsigned* __restrict__ qidx, size_t ne, size_t nc, int B,
                                       const unsigned long long* __restrict__ totals,
                                       unsigned long long* __restrict__ counts) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const bool last = b + 1 >= B;
  const unsigned long long e0 = eidx[(size_t)b * ne], c0 = cidx[(size_t)b * nc], q0 = qidx[(size_t)b * ne];
  const unsigned long long e1 = last ? totals[0] : eidx[(size_t)(b + 1) * ne];
  const unsigned long long c1 = last ? totals[1] : cidx[(size_t)(b + 1) * nc];
  const unsigned long long q1 = last ? totals[2] : qidx[(size_t)(b + 1) * ne];
  counts[3 * b + 0] = e1 - e0;
  counts[3 * b + 1] = c1 - c0;
  counts[3 * b + 2] = 2ull * (q1 - q0);
}

// ---------------------------------------------------------------------------
// grid normals: the field's finite-difference gradient at the Hermite points, float64 from the float32 values
// ---------------------------------------------------------------------------
// D_k at grid point pt whose index on axis k is i: central difference, the indices clamped to the grid
__device__ __forceinline__ double dc_central(const float* __restrict__ vol, const GridSpec& g, size_t pt, int k, int i) {
  const int n = g.res;
  const size_t step = k == 0 ? 1 : (k == 1 ? (size_t)n : (size_t)n * n);
  const int ip = i + 1 < n ? i + 1 : n - 1, im = i > 0 ? i - 1 : 0;
  const double num = (double)vol[pt + (size_t)(ip - i) * step] - (double)vol[pt - (size_t)(i - im) * step];
  const double den = (double)grid_coord(g, k, ip) - (double)grid_coord(g, k, im);
  return num / den;
}

__global__ __launch_bounds__(256) void dc_grid_normals_batch_kernel(const float* __restrict__ vol, GridBoxes boxes,
                                                                    int n, unsigned ne, unsigned b0, unsigned nb,
                                                                    float iso, const unsigned* __restrict__ eflag,
                                                                    const unsigned* __restrict__ eidx,
                                                                    float* __restrict__ normals) {
  const size_t first = (size_t)b0 * ne, total = (size_t)nb * ne;
  const unsigned np = ne / 3;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    if (!eflag[first + q]) continue;
    const unsigned lb = (unsigned)q / ne, e = (unsigned)q - lb * ne;
    const GridSpec g = grid_box_spec(boxes, lb, n);
    const float* v = vol + (size_t)(b0 + lb) * np;
    const GridEdge E = grid_edge(v, g, iso, e);
    const double t = (double)E.t;
    float* o = normals + (size_t)eidx[first + q] * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double gk;
      if (k == E.a) {
        gk = ((double)E.v1 - (double)E.v0) / ((double)E.c1 - (double)E.c0);
      } else {
        const double d0 = dc_central(v, g, E.p, k, E.idx[k]);
        const double d1 = dc_central(v, g, E.p + E.step, k, E.idx[k]);
        gk = (1.0 - t) * d0 + t * d1;
      }
      o[k] = (float)gk;
    }
  }
}

// ---------------------------------------------------------------------------
// pass 3: the quadric of a set of rows, summed by ONE thread in float64 registers in the order the rows are added, and
// the regularised 3x3 solve by the adjugate (postprocess._simplify_solve's order)
// ---------------------------------------------------------------------------
struct DcCell {       // a cell's low corner and its extent, float64 of the float32 axis values
  double corner[3], hi[3];
};

__device__ __forceinline__ DcCell dc_cell(const GridSpec& g, int ix, int iy, int iz) {
  const int ci[3] = {ix, iy, iz};
  DcCell c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c.corner[k] = (double)grid_coord(g, k, ci[k]);
    c.hi[k] = (double)grid_coord(g, k, ci[k] + 1) - c.corner[k];
  }
  return c;
}

struct DcQuadric {
  double axx = 0.0, axy = 0.0, axz = 0.0, ayy = 0.0, ayz = 0.0, azz = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
  double sx = 0.0, sy = 0.0, sz = 0.0, cnt = 0.0;

  // the row of the point of GLOBAL rank `rank`: every row counts in the mean, a row whose s is not finite and positive
  // adds nothing else
  __device__ __forceinline__ void add(const DcCell& c, const float* __restrict__ points,
                                      const float* __restrict__ normals, size_t rank) {
    const size_t r = rank * 3;
    const double dx = (double)points[r + 0] - c.corner[0];
    const double dy = (double)points[r + 1] - c.corner[1];
    const double dz = (double)points[r + 2] - c.corner[2];
    sx = sx + dx; sy = sy + dy; sz = sz + dz;
    cnt = cnt + 1.0;
    const double gx = (double)normals[r + 0], gy = (double)normals[r + 1], gz = (double)normals[r + 2];
    const double s = (gx * gx + gy * gy) + gz * gz;
    if (!(s > 0.0) || !isfinite(s)) return;
    const double gd = (gx * dx + gy * dy) + gz * dz;
    axx = axx + (gx * gx) / s; axy = axy + (gx * gy) / s; axz = axz + (gx * gz) / s;
    ayy = ayy + (gy * gy) / s; ayz = ayz + (gy * gz) / s; azz = azz + (gz * gz) / s;
    bx = bx - (gx * gd) / s; by = by - (gy * gd) / s; bz = bz - (gz * gd) / s;
  }

  // the vertex: solved, fallen back to the mean, clipped to the cell, cast
  __device__ __forceinline__ void solve(const DcCell& c, double reg, float* __restrict__ o) const {
    const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
    const double lam = (((axx + ayy) + azz) * reg) / 3.0 + 9.094947017729282e-13;   // reg tr(A) / 3 + 2^-40
    const double m00 = axx + lam, m11 = ayy + lam, m22 = azz + lam;
    const double m01 = axy, m02 = axz, m12 = ayz;
    const double r0 = lam * mx - bx, r1 = lam * my - by, r2 = lam * mz - bz;
    const double c00 = m11 * m22 - m12 * m12;
    const double c01 = m02 * m12 - m01 * m22;
    const double c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02;
    const double c12 = m01 * m02 - m00 * m12;
    const double c22 = m00 * m11 - m01 * m01;
    const double det = (m00 * c00 + m01 * c01) + m02 * c02;
    double x0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
    double x1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
    double x2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
    if (!(det > 0.0) || !isfinite(x0) || !isfinite(x1) || !isfinite(x2)) {
      x0 = mx; x1 = my; x2 = mz;
    }
    x0 = x0 < 0.0 ? 0.0 : (x0 > c.hi[0] ? c.hi[0] : x0);
    x1 = x1 < 0.0 ? 0.0 : (x1 > c.hi[1] ? c.hi[1] : x1);
    x2 = x2 < 0.0 ? 0.0 : (x2 > c.hi[2] ? c.hi[2] : x2);
    o[0] = (float)(c.corner[0] + x0);
    o[1] = (float)(c.corner[1] + x1);
    o[2] = (float)(c.corner[2] + x2);
  }
};

// the vertices of a cell, one per loop in loop-id order, at the GLOBAL ranks cidx[cell] + loop; the thread of a cell
// sums the rows of each in cube-edge order
template <class Rule>
__global__ __launch_bounds__(256) void dc_verts_batch_kernel(const float* __restrict__ vol, GridBoxes boxes, int n,
                                                             unsigned np, unsigned b0, unsigned nb, float iso,
                                                             double reg, const unsigned* __restrict__ eflag,
                                                             const unsigned* __restrict__ eidx,
                                                             const unsigned* __restrict__ cflag,
                                                             const unsigned* __restrict__ cidx,
                                                             const float* __restrict__ points,
                                                             const float* __restrict__ normals,
                                                             float* __restrict__ verts) {
  const unsigned R = (unsigned)n - 1, nc = R * R * R;
  const size_t first = (size_t)b0 * nc, total = (size_t)nb * nc;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    const unsigned cf = cflag[first + q];
    if (!cf) continue;
    const int nl = Rule::kMax == 1 ? 1 : (int)cf;
    const unsigned lb = (unsigned)q / nc, c = (unsigned)q - lb * nc;
    const int ix = (int)(c % R), iy = (int)((c / R) % R), iz = (int)(c / (R * R));
    const DcCell cell = dc_cell(grid_box_spec(boxes, lb, n), ix, iy, iz);
    const int cs = Rule::cell_case(vol + (size_t)(b0 + lb) * np, n, iso, ((size_t)iz * n + iy) * n + ix);
    const unsigned* ef = eflag + (size_t)3 * (b0 + lb) * np;
    const unsigned* ei = eidx + (size_t)3 * (b0 + lb) * np;
    float* o = verts + (size_t)cidx[first + q] * 3;
    for (int l = 0; l < nl; ++l) {
      DcQuadric Q;
      for (int e = 0; e < 12; ++e) {
        const size_t slot = grid_cube_edge_slot(n, ix, iy, iz, e);
        if (!Rule::member(cs, ef, slot, e, l)) continue;
        Q.add(cell, points, normals, ei[slot]);      // the point's GLOBAL rank: points / normals are the batch's arrays
      }
      Q.solve(cell, reg, o + 3 * l);
    }
  }
}

// ---------------------------------------------------------------------------
// pass 4: the quad of a cut edge.  (u, v): the two axes after a in cyclic order; cell q_k lies at (u, v) offsets
// (-1,-1), (0,-1), (0,0), (-1,0); the quad flag says that both indices are in 1 .. R-1
// ---------------------------------------------------------------------------
__device__ __forceinline__ void dc_quad_cell(int a, int k, int ix, int iy, int iz, int* cx, int* cy, int* cz) {
  const int du[4] = {-1, 0, 0, -1}, dv[4] = {-1, -1, 0, 0};
  *cx = ix + (a == 1 ? dv[k] : (a == 2 ? du[k] : 0));   // x is u of a = 2, v of a = 1
  *cy = iy + (a == 2 ? dv[k] : (a == 0 ? du[k] : 0));   // y is u of a = 0, v of a = 2
  *cz = iz + (a == 0 ? dv[k] : (a == 1 ? du[k] : 0));   // z is u of a = 1, v of a = 0
}

// two triangles from the GLOBAL vertex ranks id[0..4) of q0 .. q3: the shorter diagonal of the positions pass 3 wrote
// (equality keeps q0-q2), the winding by the side of the edge's low end, the ids made LOCAL to the grid (minus base)
__device__ __forceinline__ void dc_quad_faces(const unsigned id[4], int base, bool inside,
                                              const float* __restrict__ verts, int* __restrict__ o) {
  double px[4], py[4], pz[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float* vp = verts + (size_t)id[k] * 3;
    px[k] = (double)vp[0]; py[k] = (double)vp[1]; pz[k] = (double)vp[2];
  }
  const double ax = px[0] - px[2], ay = py[0] - py[2], az = pz[0] - pz[2];
  const double bx = px[1] - px[3], by = py[1] - py[3], bz = pz[1] - pz[3];
  const double d02 = (ax * ax + ay * ay) + az * az;
  const double d13 = (bx * bx + by * by) + bz * bz;
  const bool other = d13 < d02;
  const int q0 = (int)id[0] - base, q1 = (int)id[1] - base, q2 = (int)id[2] - base, q3 = (int)id[3] - base;
  int t[6];
  if (!other) { t[0] = q0; t[1] = q1; t[2] = q2; t[3] = q0; t[4] = q2; t[5] = q3; }
  else        { t[0] = q0; t[1] = q1; t[2] = q3; t[3] = q1; t[4] = q2; t[5] = q3; }
  o[0] = t[0]; o[1] = inside ? t[1] : t[2]; o[2] = inside ? t[2] : t[1];
  o[3] = t[3]; o[4] = inside ? t[4] : t[5]; o[5] = inside ? t[5] : t[4];
}

// The triangles go to their GLOBAL rank; their vertex ids are LOCAL to the grid (the grid's first vertex rank taken
// off).  Reads the positions pass 3 wrote (same stream, the launch before)
template <class Rule>
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
    const float* v = vol + (size_t)b * np;
    unsigned id[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int cx, cy, cz;
      dc_quad_cell(a, k, ix, iy, iz, &cx, &cy, &cz);
      const int cs = Rule::cell_case(v, n, iso, ((size_t)cz * n + cy) * n + cx);
      id[k] = ci[((size_t)cz * R + cy) * R + cx] + Rule::offset(cs, a, k);
    }
    dc_quad_faces(id, (int)ci[0], v[p] < iso, verts, faces + (size_t)qidx[q] * 6);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// cflag: what a cell adds to the vertex count (per cell: 0 / 1, per sheet: its loops)
struct DcWs {
  unsigned *eflag, *eidx, *qflag, *qidx, *cflag, *cidx, *bsum;
  unsigned long long* totals;  // {points, vertices, quads} of the whole batch
  size_t total;
};

DcWs dc_layout(void* ws, int B, int R) {
  const size_t n = (size_t)R + 1, ne = (size_t)B * 3 * n * n * n, nc = (size_t)B * R * R * R;
  WsCursor c(ws);
  DcWs w;
  w.eflag = c.take<unsigned>(ne);
  w.eidx = c.take<unsigned>(ne);
  w.qflag = c.take<unsigned>(ne);
  w.qidx = c.take<unsigned>(ne);
  w.cflag = c.take<unsigned>(nc);
  w.cidx = c.take<unsigned>(nc);
  w.bsum = c.take<unsigned>(scan_bsum_items(ne));
  w.totals = c.take<unsigned long long>(3);
  w.total = c.next();
  return w;
}

size_t dc_ws_bytes(int B, int R) { return dc_layout(nullptr, B, R).total; }

// the three scans behind a flags pass, and the per-grid sizes
hipError_t dc_scan_counts(const DcWs& w, int B, int R, unsigned long long* counts, hipStream_t st) {
  const size_t n = (size_t)R + 1, np = n * n * n, nc = (size_t)R * R * R;
  hipError_t e;
  if ((e = exclusive_scan(w.eflag, w.eidx, B * 3 * np, w.bsum, w.totals, st)) != hipSuccess) return e;
  if ((e = exclusive_scan(w.cflag, w.cidx, B * nc, w.bsum, w.totals + 1, st)) != hipSuccess) return e;
  if ((e = exclusive_scan(w.qflag, w.qidx, B * 3 * np, w.bsum, w.totals + 2, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(dc_batch_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, st, w.eidx, w.cidx, w.qidx, 3 * np,
                     nc, B, w.totals, counts);
  return hipGetLastError();
}

// the points, or (normals = true) the grid normals, of all B grids: the boxes travel as kernel arguments,
// kMcBatchBoxes per launch
hipError_t dc_hermite_launch(bool normals, const float* sdf, const double* sdf_params_host, int B, int R, float iso,
                             float* out, const DcWs& w, hipStream_t st) {
  const int n = R + 1;
  const size_t np = (size_t)n * n * n;
  const auto kernel = normals ? dc_grid_normals_batch_kernel : grid_points_batch_kernel;
  for (int b0 = 0; b0 < B; b0 += kMcBatchBoxes) {
    const int nb = B - b0 < kMcBatchBoxes ? B - b0 : kMcBatchBoxes;
    hipLaunchKernelGGL(kernel, dim3(blocks_for(3 * np * nb)), dim3(256), 0, st, sdf,
                       grid_boxes(sdf_params_host, b0, nb, R), n, (unsigned)(3 * np), (unsigned)b0, (unsigned)nb, iso,
                       w.eflag, w.eidx, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- the bodies of the C entries, once for both rules: argument and workspace checks, then the launches ----
// marching cubes' limits, and the vertex ranks (at most Rule::kMax per cell) through the same 32-bit scan
template <class Rule>
bool dc_batch_ok(int B, int R) {
  if (!grid_batch_ok(B, R)) return false;
  const unsigned long long r = (unsigned long long)R;
  return (unsigned long long)Rule::kMax * (unsigned long long)B * r * r * r < (1ull << 32);
}

template <class Rule>
size_t dc_workspace_bytes(int B, int R) { return dc_batch_ok<Rule>(B, R) ? dc_ws_bytes(B, R) : 0; }

template <class Rule>
int dc_count_batch(const float* sdf, int B, int R, float iso, uint64_t* counts, void* ws, size_t ws_bytes,
                   void* stream) {
  if (!sdf || !counts || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!dc_batch_ok<Rule>(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < dc_ws_bytes(B, R)) return DISN_E_WS;
  const DcWs w = dc_layout(ws, B, R);
  const int n = R + 1;
  const size_t np = (size_t)n * n * n;
  hipLaunchKernelGGL(dc_flags_batch_kernel<Rule>, dim3(blocks_for(B * np)), dim3(256), 0, (hipStream_t)stream, sdf, n,
                     (unsigned)np, (unsigned)(B * np), iso, w.eflag, w.qflag, w.cflag);
  DISN_TRY(hipGetLastError());
  DISN_TRY(dc_scan_counts(w, B, R, reinterpret_cast<unsigned long long*>(counts), (hipStream_t)stream));
  return 0;
}

template <class Rule>
int dc_hermite_batch(bool normals, const float* sdf, const double* sdf_params_host, int B, int R, float iso, float* out,
                     void* ws, size_t ws_bytes, void* stream) {
  if (!sdf || !sdf_params_host || !out || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!dc_batch_ok<Rule>(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < dc_ws_bytes(B, R)) return DISN_E_WS;
  DISN_TRY(dc_hermite_launch(normals, sdf, sdf_params_host, B, R, iso, out, dc_layout(ws, B, R), (hipStream_t)stream));
  return 0;
}

template <class Rule>
int dc_emit_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, const float* points,
                  const float* normals, double reg, float* verts, int32_t* faces, void* ws, size_t ws_bytes,
                  void* stream) {
  if (!sdf || !sdf_params_host || !points || !normals || !verts || !faces || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!(reg > 0.0 && reg <= 1.0)) return DISN_E_ARG;   // a NaN fails both comparisons
  if (!dc_batch_ok<Rule>(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < dc_ws_bytes(B, R)) return DISN_E_WS;
  const DcWs w = dc_layout(ws, B, R);
  const int n = R + 1;
  const size_t np = (size_t)n * n * n, nc = (size_t)R * R * R;
  for (int b0 = 0; b0 < B; b0 += kMcBatchBoxes) {
    const int nb = B - b0 < kMcBatchBoxes ? B - b0 : kMcBatchBoxes;
    hipLaunchKernelGGL(dc_verts_batch_kernel<Rule>, dim3(blocks_for(nc * nb)), dim3(256), 0, (hipStream_t)stream, sdf,
                       grid_boxes(sdf_params_host, b0, nb, R), n, (unsigned)np, (unsigned)b0, (unsigned)nb, iso, reg,
                       w.eflag, w.eidx, w.cflag, w.cidx, points, normals, verts);
    DISN_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(dc_faces_batch_kernel<Rule>, dim3(blocks_for(B * 3 * np)), dim3(256), 0, (hipStream_t)stream, sdf,
                     n, (unsigned)np, (size_t)B * 3 * np, iso, w.qflag, w.qidx, w.cidx, verts, faces);
  DISN_TRY(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace disn

// ---- the C entries of include/dc/disn_amd_dc.h (per cell) and include/dc/disn_amd_dc_sheets.h (per sheet) ----
using namespace disn;

extern "C" {

size_t disn_dc_workspace_bytes(int B, int R) { return dc_workspace_bytes<DcPerCell>(B, R); }
size_t disn_dcs_workspace_bytes(int B, int R) { return dc_workspace_bytes<DcPerSheet>(B, R); }

int disn_dc_count_batch(const float* sdf, int B, int R, float iso, uint64_t* counts, void* ws, size_t ws_bytes,
                        void* stream) {
  return dc_count_batch<DcPerCell>(sdf, B, R, iso, counts, ws, ws_bytes, stream);
}
int disn_dcs_count_batch(const float* sdf, int B, int R, float iso, uint64_t* counts, void* ws, size_t ws_bytes,
                         void* stream) {
  return dc_count_batch<DcPerSheet>(sdf, B, R, iso, counts, ws, ws_bytes, stream);
}

int disn_dc_points_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, float* points,
                         void* ws, size_t ws_bytes, void* stream) {
  return dc_hermite_batch<DcPerCell>(false, sdf, sdf_params_host, B, R, iso, points, ws, ws_bytes, stream);
}
int disn_dcs_points_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, float* points,
                          void* ws, size_t ws_bytes, void* stream) {
  return dc_hermite_batch<DcPerSheet>(false, sdf, sdf_params_host, B, R, iso, points, ws, ws_bytes, stream);
}

int disn_dc_grid_normals_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso,
                               float* normals, void* ws, size_t ws_bytes, void* stream) {
  return dc_hermite_batch<DcPerCell>(true, sdf, sdf_params_host, B, R, iso, normals, ws, ws_bytes, stream);
}
int disn_dcs_grid_normals_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso,
                                float* normals, void* ws, size_t ws_bytes, void* stream) {
  return dc_hermite_batch<DcPerSheet>(true, sdf, sdf_params_host, B, R, iso, normals, ws, ws_bytes, stream);
}

int disn_dc_emit_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, const float* points,
                       const float* normals, double reg, float* verts, int32_t* faces, void* ws, size_t ws_bytes,
                       void* stream) {
  return dc_emit_batch<DcPerCell>(sdf, sdf_params_host, B, R, iso, points, normals, reg, verts, faces, ws, ws_bytes,
                                  stream);
}
int disn_dcs_emit_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, const float* points,
                        const float* normals, double reg, float* verts, int32_t* faces, void* ws, size_t ws_bytes,
                        void* stream) {
  return dc_emit_batch<DcPerSheet>(sdf, sdf_params_host, B, R, iso, points, normals, reg, verts, faces, ws, ws_bytes,
                                   stream);
}

}  // extern "C"
