// What the two dual-contouring meshers share (dual_contour.hip: one vertex per cell; dual_contour_sheets.hip: one per
// sheet of a cell): the grid's axis values, the Hermite point and the grid normal of a cut edge with their kernels, the
// flags of a grid point, the quadric of a set of rows with its solve, the cells and the split of a quad, the workspace
// and the launches of the shared passes.  Everything has internal linkage, as in mesh_batch.hpp: each of the two
// translation units keeps its own copy and no kernel is launched across them.  BOTH FILES ARE COMPILED WITH
// -ffp-contract=off; every body below restates isosurface.dual_contour_arrays operation by operation.
#pragma once

#include "kernels.hpp"

#define DISN_MC_QUAL __constant__ const
#include "mc_tables.h"      // kMcEdge: the cube-edge ids of tools/gen_mc_tables.edge_geometry (the row order of a cell)

namespace disn {
namespace {

// the float32 axis value of marching_cubes.hip (numpy.linspace in float64, the last point the box's own end)
__device__ __forceinline__ float dc_grid_coord(const GridSpec& g, int a, int i) {
  double v = (double)i * g.step[a];
  v = v + g.start[a];
  if (i == g.res - 1 && g.res > 1) v = g.stop[a];
  return (float)v;
}

struct DcBox { double start[3], step[3], stop[3]; };
struct DcBoxes { DcBox b[kMcBatchBoxes]; };   // 32 * 72 B of kernel arguments, as the marching-cubes vertex launch

__device__ __forceinline__ GridSpec dc_spec(const DcBoxes& boxes, unsigned lb, int n) {
  GridSpec g;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g.start[a] = boxes.b[lb].start[a];
    g.step[a] = boxes.b[lb].step[a];
    g.stop[a] = boxes.b[lb].stop[a];
  }
  g.res = n;
  return g;
}

// ---------------------------------------------------------------------------
// pass 1: per grid point its three cut-edge flags and quad flags; for a grid point that is the low corner of a cell,
// the cell's marching-cubes case (bit i = corner i of tools/gen_mc_tables inside)
// ---------------------------------------------------------------------------
// vol, eflag and qflag are the grid's OWN blocks, so no neighbour (+1, +n, +n^2) leaves the grid.  -> the case of the
// cell at p, or -1 when p is the low corner of no cell
__device__ __forceinline__ int dc_flags_point(const float* __restrict__ vol, int n, float iso, size_t p, int ix,
                                              int iy, int iz, unsigned* __restrict__ eflag,
                                              unsigned* __restrict__ qflag) {
  const int R = n - 1;
  const bool in0 = vol[p] < iso;
  const bool hx = ix < R, hy = iy < R, hz = iz < R;
  const bool inx = hx ? vol[p + 1] < iso : in0;
  const bool iny = hy ? vol[p + n] < iso : in0;
  const bool inz = hz ? vol[p + (size_t)n * n] < iso : in0;
  const bool ex = hx && inx != in0, ey = hy && iny != in0, ez = hz && inz != in0;
  // an edge has a quad when all four cells around it exist: its two other indices in 1 .. R-1
  const bool mx = ix >= 1 && ix <= R - 1, my = iy >= 1 && iy <= R - 1, mz = iz >= 1 && iz <= R - 1;
  eflag[3 * p + 0] = ex ? 1u : 0u;
  eflag[3 * p + 1] = ey ? 1u : 0u;
  eflag[3 * p + 2] = ez ? 1u : 0u;
  qflag[3 * p + 0] = (ex && my && mz) ? 1u : 0u;
  qflag[3 * p + 1] = (ey && mz && mx) ? 1u : 0u;
  qflag[3 * p + 2] = (ez && mx && my) ? 1u : 0u;
  if (!(hx && hy && hz)) return -1;
  const size_t nn = (size_t)n * n;
  int c = in0 ? 1 : 0;
  c |= inx ? 2 : 0;
  c |= (vol[p + 1 + n] < iso) ? 4 : 0;
  c |= iny ? 8 : 0;
  c |= inz ? 16 : 0;
  c |= (vol[p + nn + 1] < iso) ? 32 : 0;
  c |= (vol[p + nn + 1 + n] < iso) ? 64 : 0;
  c |= (vol[p + nn + n] < iso) ? 128 : 0;
  return c;
}

// the case of cell (ix, iy, iz) of a grid, all three in 0 .. R-1
__device__ __forceinline__ int dc_cell_case(const float* __restrict__ vol, int n, float iso, int ix, int iy, int iz) {
  const size_t nn = (size_t)n * n, p = ((size_t)iz * n + iy) * n + ix;
  int c = (vol[p] < iso) ? 1 : 0;
  c |= (vol[p + 1] < iso) ? 2 : 0;
  c |= (vol[p + 1 + n] < iso) ? 4 : 0;
  c |= (vol[p + n] < iso) ? 8 : 0;
  c |= (vol[p + nn] < iso) ? 16 : 0;
  c |= (vol[p + nn + 1] < iso) ? 32 : 0;
  c |= (vol[p + nn + 1 + n] < iso) ? 64 : 0;
  c |= (vol[p + nn + n] < iso) ? 128 : 0;
  return c;
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
// pass 2: the Hermite point of a cut edge (marching_cubes.hip's vertex, operation by operation)
// ---------------------------------------------------------------------------
struct DcEdge {
  size_t p, step;
  int a, idx[3];
  float v0, v1, t, c0, c1;
};

__device__ __forceinline__ DcEdge dc_edge(const float* __restrict__ vol, const GridSpec& g, float iso, size_t e) {
  const int n = g.res;
  DcEdge E;
  E.p = e / 3;
  E.a = (int)(e - 3 * E.p);
  E.idx[0] = (int)(E.p % n);
  E.idx[1] = (int)((E.p / n) % n);
  E.idx[2] = (int)(E.p / ((size_t)n * n));
  E.step = E.a == 0 ? 1 : (E.a == 1 ? (size_t)n : (size_t)n * n);
  E.v0 = vol[E.p];
  E.v1 = vol[E.p + E.step];
  E.t = (iso - E.v0) / (E.v1 - E.v0);
  const int ia = E.a == 0 ? E.idx[0] : (E.a == 1 ? E.idx[1] : E.idx[2]);
  E.c0 = dc_grid_coord(g, E.a, ia);
  E.c1 = dc_grid_coord(g, E.a, ia + 1);
  return E;
}

__global__ __launch_bounds__(256) void dc_points_batch_kernel(const float* __restrict__ vol, DcBoxes boxes, int n,
                                                              unsigned ne, unsigned b0, unsigned nb, float iso,
                                                              const unsigned* __restrict__ eflag,
                                                              const unsigned* __restrict__ eidx,
                                                              float* __restrict__ points) {
  const size_t first = (size_t)b0 * ne, total = (size_t)nb * ne;
  const unsigned np = ne / 3;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    if (!eflag[first + q]) continue;
    const unsigned lb = (unsigned)q / ne, e = (unsigned)q - lb * ne;
    const GridSpec g = dc_spec(boxes, lb, n);
    const DcEdge E = dc_edge(vol + (size_t)(b0 + lb) * np, g, iso, e);
    float pos[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) pos[k] = dc_grid_coord(g, k, E.idx[k]);
    const float d = E.t * (E.c1 - E.c0);
    const float cut = E.c0 + d;
    float* o = points + (size_t)eidx[first + q] * 3;
    o[0] = E.a == 0 ? cut : pos[0];
    o[1] = E.a == 1 ? cut : pos[1];
    o[2] = E.a == 2 ? cut : pos[2];
  }
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
  const double den = (double)dc_grid_coord(g, k, ip) - (double)dc_grid_coord(g, k, im);
  return num / den;
}

__global__ __launch_bounds__(256) void dc_grid_normals_batch_kernel(const float* __restrict__ vol, DcBoxes boxes,
                                                                    int n, unsigned ne, unsigned b0, unsigned nb,
                                                                    float iso, const unsigned* __restrict__ eflag,
                                                                    const unsigned* __restrict__ eidx,
                                                                    float* __restrict__ normals) {
  const size_t first = (size_t)b0 * ne, total = (size_t)nb * ne;
  const unsigned np = ne / 3;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    if (!eflag[first + q]) continue;
    const unsigned lb = (unsigned)q / ne, e = (unsigned)q - lb * ne;
    const GridSpec g = dc_spec(boxes, lb, n);
    const float* v = vol + (size_t)(b0 + lb) * np;
    const DcEdge E = dc_edge(v, g, iso, e);
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
    c.corner[k] = (double)dc_grid_coord(g, k, ci[k]);
    c.hi[k] = (double)dc_grid_coord(g, k, ci[k] + 1) - c.corner[k];
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

// the rank slot (3 p + axis) of cube edge e of cell (ix, iy, iz)
__device__ __forceinline__ size_t dc_cube_edge_slot(int n, int ix, int iy, int iz, int e) {
  const size_t gp = ((size_t)(iz + kMcEdge[e][2]) * n + (iy + kMcEdge[e][1])) * n + (ix + kMcEdge[e][0]);
  return 3 * gp + kMcEdge[e][3];
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

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// cflag: what a cell contributes to the vertex count (dual_contour.hip: 0 / 1, dual_contour_sheets.hip: its loops)
struct DcWs {
  unsigned *eflag, *eidx, *qflag, *qidx, *cflag, *cidx, *bsum;
  unsigned long long* totals;  // {points, vertices, quads} of the whole batch
  size_t total;
};

inline DcWs dc_layout(void* ws, int B, int R) {
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

inline size_t dc_ws_bytes(int B, int R) { return dc_layout(nullptr, B, R).total; }

inline int dc_blocks_for(size_t total) {
  size_t b = (total + 255) / 256;
  if (b > 16384) b = 16384;
  return (int)(b < 1 ? 1 : b);
}

// a batch is supported when its 3*B*(R+1)^3 edge slots fit the 32-bit scan (disn_mc_*_batch's limits)
inline bool dc_batch_ok(int B, int R) {
  if (B < 1 || R < 1 || R > 1290) return false;
  const unsigned long long n = (unsigned long long)R + 1;
  return 3ull * (unsigned long long)B * n * n * n < (1ull << 32);
}

inline DcBoxes dc_boxes(const double* sdf_params_host, int b0, int nb, int R) {
  DcBoxes boxes = {};
  for (int i = 0; i < nb; ++i) {
    GridSpec g;
    grid_spec(sdf_params_host + 6 * (size_t)(b0 + i), R, &g);
    for (int a = 0; a < 3; ++a) {
      boxes.b[i].start[a] = g.start[a];
      boxes.b[i].step[a] = g.step[a];
      boxes.b[i].stop[a] = g.stop[a];
    }
  }
  return boxes;
}

// the three scans behind a flags pass, and the per-grid sizes
inline hipError_t dc_scan_counts(const DcWs& w, int B, int R, unsigned long long* counts, hipStream_t st) {
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
inline hipError_t dc_hermite_launch(bool normals, const float* sdf, const double* sdf_params_host, int B, int R,
                                    float iso, float* out, const DcWs& w, hipStream_t st) {
  const int n = R + 1;
  const size_t np = (size_t)n * n * n;
  for (int b0 = 0; b0 < B; b0 += kMcBatchBoxes) {
    const int nb = B - b0 < kMcBatchBoxes ? B - b0 : kMcBatchBoxes;
    if (normals)
      hipLaunchKernelGGL(dc_grid_normals_batch_kernel, dim3(dc_blocks_for(3 * np * nb)), dim3(256), 0, st, sdf,
                         dc_boxes(sdf_params_host, b0, nb, R), n, (unsigned)(3 * np), (unsigned)b0, (unsigned)nb, iso,
                         w.eflag, w.eidx, out);
    else
      hipLaunchKernelGGL(dc_points_batch_kernel, dim3(dc_blocks_for(3 * np * nb)), dim3(256), 0, st, sdf,
                         dc_boxes(sdf_params_host, b0, nb, R), n, (unsigned)(3 * np), (unsigned)b0, (unsigned)nb, iso,
                         w.eflag, w.eidx, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

#define DISN_TRY(expr)                    \
  do {                                    \
    hipError_t _e = (expr);               \
    if (_e != hipSuccess) return (int)_e; \
  } while (0)

}  // namespace
}  // namespace disn
