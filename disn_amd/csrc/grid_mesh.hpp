// The per-grid bodies that the three meshers of a predicted field share (marching_cubes.hip; dual_contour.hip with its
// two vertex rules): the grid's axis values, the boxes of a batch as kernel arguments, the case of a cell, the flags of
// a grid point, the cut edge with its point and the batched kernel that writes the points, the slot of a cube edge and
// the limits of a batch.  Everything has internal linkage, as in mesh_batch.hpp: each of the two translation units
// keeps its own copy and no kernel is launched across them.  BOTH ARE COMPILED WITH -ffp-contract=off: order and
// arithmetic are those of oracle/mc_oracle.py and isosurface.hermite_points_arrays, compared bit for bit.
//   edge slot  = 3*p + axis, p = (iz*n + iy)*n + ix; a cut edge's rank in that order is its vertex / point id
//   case       = bit i set when corner i of tools/gen_mc_tables is inside (vol < iso)
#pragma once

#include "kernels.hpp"

#define DISN_MC_QUAL __constant__ const
#include "mc_tables.h"      // kMcEdge: the cube-edge ids of tools/gen_mc_tables.edge_geometry (the row order of a cell)

#define DISN_TRY(expr)                    \
  do {                                    \
    hipError_t _e = (expr);               \
    if (_e != hipSuccess) return (int)_e; \
  } while (0)

namespace disn {
namespace {

// the float32 axis value: numpy.linspace in float64, the last point the box's own end
__device__ __forceinline__ float grid_coord(const GridSpec& g, int a, int i) {
  double v = (double)i * g.step[a];
  v = v + g.start[a];
  if (i == g.res - 1 && g.res > 1) v = g.stop[a];
  return (float)v;
}

// the boxes of up to kMcBatchBoxes grids of one resolution travel as kernel arguments
struct GridBox { double start[3], step[3], stop[3]; };
struct GridBoxes { GridBox b[kMcBatchBoxes]; };   // 32 * 72 B

__device__ __forceinline__ GridSpec grid_box_spec(const GridBoxes& boxes, unsigned lb, int n) {
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

// grids b0 .. b0+nb-1 of sdf_params_host [B,6], nb <= kMcBatchBoxes
inline GridBoxes grid_boxes(const double* sdf_params_host, int b0, int nb, int R) {
  GridBoxes boxes = {};
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

// whether the corner at offset (dx, dy, dz) of the cell whose low corner is grid point p is inside
struct GridCorner {
  const float* __restrict__ vol;
  int n;
  float iso;
  size_t p;
  __device__ __forceinline__ bool operator()(int dx, int dy, int dz) const {
    return vol[p + dx + (size_t)dy * n + (size_t)dz * n * n] < iso;
  }
};

// the case of a cell from its eight corners, inside(dx, dy, dz) answering for each
template <class Inside>
__device__ __forceinline__ int grid_case_of(const Inside& inside) {
  int c = inside(0, 0, 0) ? 1 : 0;
  c |= inside(1, 0, 0) ? 2 : 0;
  c |= inside(1, 1, 0) ? 4 : 0;
  c |= inside(0, 1, 0) ? 8 : 0;
  c |= inside(0, 0, 1) ? 16 : 0;
  c |= inside(1, 0, 1) ? 32 : 0;
  c |= inside(1, 1, 1) ? 64 : 0;
  c |= inside(0, 1, 1) ? 128 : 0;
  return c;
}

// the case of the cell whose low corner is grid point p (all three of its indices below R)
__device__ __forceinline__ int grid_cell_case(const float* __restrict__ vol, int n, float iso, size_t p) {
  return grid_case_of(GridCorner{vol, n, iso, p});
}

// pass 1 of every mesher, one grid point p = (ix, iy, iz) of an n^3 grid: writes its three cut-edge flags -> the case
// of the cell at p, or -1 when p is the low corner of no cell; cut (optional): the three flags it wrote.  vol and eflag
// are the grid's OWN blocks, so no neighbour (+1, +n, +n^2) leaves the grid
__device__ __forceinline__ int grid_flags_point(const float* __restrict__ vol, int n, float iso, size_t p, int ix,
                                                int iy, int iz, unsigned* __restrict__ eflag, bool* cut = nullptr) {
  const int R = n - 1;
  const GridCorner corner{vol, n, iso, p};
  const bool in0 = corner(0, 0, 0);
  const bool hx = ix < R, hy = iy < R, hz = iz < R;
  const bool inx = hx ? corner(1, 0, 0) : in0;
  const bool iny = hy ? corner(0, 1, 0) : in0;
  const bool inz = hz ? corner(0, 0, 1) : in0;
  const bool ex = hx && inx != in0, ey = hy && iny != in0, ez = hz && inz != in0;
  eflag[3 * p + 0] = ex ? 1u : 0u;
  eflag[3 * p + 1] = ey ? 1u : 0u;
  eflag[3 * p + 2] = ez ? 1u : 0u;
  if (cut) { cut[0] = ex; cut[1] = ey; cut[2] = ez; }
  if (!(hx && hy && hz)) return -1;
  // the four corners read above are not read again
  return grid_case_of([&](int dx, int dy, int dz) {
    return dx + dy + dz > 1 ? corner(dx, dy, dz) : (dx ? inx : (dy ? iny : (dz ? inz : in0)));
  });
}

// a cut edge.  e: edge slot of this grid; t = (iso - v0)/(v1 - v0) in float32, c0 / c1 the axis values of its ends
struct GridEdge {
  size_t p, step;
  int a, idx[3];
  float v0, v1, t, c0, c1;
};

__device__ __forceinline__ GridEdge grid_edge(const float* __restrict__ vol, const GridSpec& g, float iso, size_t e) {
  const int n = g.res;
  GridEdge E;
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
  E.c0 = grid_coord(g, E.a, ia);
  E.c1 = grid_coord(g, E.a, ia + 1);
  return E;
}

// pass 2: its point, c0 + t*(c1 - c0) on the cut axis: marching cubes' vertex, dual contouring's Hermite point
__device__ __forceinline__ void grid_edge_point(const GridSpec& g, const GridEdge& E, float* __restrict__ o) {
  float pos[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) pos[k] = grid_coord(g, k, E.idx[k]);
  const float d = E.t * (E.c1 - E.c0);
  const float cut = E.c0 + d;
  o[0] = E.a == 0 ? cut : pos[0];
  o[1] = E.a == 1 ? cut : pos[1];
  o[2] = E.a == 2 ? cut : pos[2];
}

// B grids of one resolution share one scan over their concatenated flags (grid b's lie at b*ne), so a cut edge's scan
// value is its GLOBAL rank and a grid's first one is its base.  Every grid is addressed through its own block of vol.
// All flat counts are below 2^32 (grid_batch_ok), so the split of a flat index into (grid, element) is 32-bit.
// Grids b0 .. b0+nb-1 (boxes.b[0..nb)), ne = 3*n^3: the point of every cut edge goes to its GLOBAL rank
__global__ __launch_bounds__(256) void grid_points_batch_kernel(const float* __restrict__ vol, GridBoxes boxes, int n,
                                                                unsigned ne, unsigned b0, unsigned nb, float iso,
                                                                const unsigned* __restrict__ eflag,
                                                                const unsigned* __restrict__ eidx,
                                                                float* __restrict__ points) {
  const size_t first = (size_t)b0 * ne, total = (size_t)nb * ne;
  const unsigned np = ne / 3;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    if (!eflag[first + q]) continue;
    const unsigned lb = (unsigned)q / ne, e = (unsigned)q - lb * ne;
    const GridSpec g = grid_box_spec(boxes, lb, n);
    grid_edge_point(g, grid_edge(vol + (size_t)(b0 + lb) * np, g, iso, e), points + (size_t)eidx[first + q] * 3);
  }
}

// the edge slot of cube edge e of cell (ix, iy, iz)
__device__ __forceinline__ size_t grid_cube_edge_slot(int n, int ix, int iy, int iz, int e) {
  const size_t gp = ((size_t)(iz + kMcEdge[e][2]) * n + (iy + kMcEdge[e][1])) * n + (ix + kMcEdge[e][0]);
  return 3 * gp + kMcEdge[e][3];
}

inline int blocks_for(size_t total) {
  size_t b = (total + 255) / 256;
  if (b > 16384) b = 16384;
  return (int)(b < 1 ? 1 : b);
}

// a batch is supported when its 3*B*(R+1)^3 edge slots fit the 32-bit scan
inline bool grid_batch_ok(int B, int R) {
  if (B < 1 || R < 1 || R > 1290) return false;
  const unsigned long long n = (unsigned long long)R + 1;
  return 3ull * (unsigned long long)B * n * n * n < (1ull << 32);
}

}  // namespace
}  // namespace disn
