// Narrow-band grid evaluation: the selection, the point list and the fill around a dense grid tensor of
// which only the coarse lattice (every index a multiple of the stride s) and the points near the surface are evaluated
// by the network.  All of it works on the stored values v = pred_sdf / sdf_weight; "inside" is v < iso, the convention
// of marching_cubes.hip's mc_flags_point, so a coarse cell holds a crossing of its own corners iff lo < iso && hi >= iso.
//
//   cell rule   lo / hi of a coarse cell's 8 lattice corners, t = margin * (hi - lo), active iff lo - t < iso && hi + t >= iso
//   dilation    one round of the 26-neighbourhood, clipped at the box
//   point flags a fine point is a band point iff it is no lattice point and lies in the CLOSED box of an active cell
//   compaction  exclusive scan of the flags (marching_cubes.hip's), the flagged flat indices in ascending order
//   coordinates / scatter of a list of flat indices (or of a run of the lattice): the query in front and behind the MLP
//   fill        every point that is neither gets the trilinear interpolant of its cell's corners, clamped to [lo, hi]
//
// THIS FILE IS COMPILED WITH -ffp-contract=off: tests/grid_band_reference.py restates the arithmetic in float32 and the
// results are compared bit for bit.  Streaming kernels, no LDS beyond the scan's; a grid has (R+1)^3 < 2^31 points
// (R <= 1289, band_shape_ok), so every flat index fits 32 bits and an int32 list.
#include "kernels.hpp"

namespace disn {

namespace {

inline int band_blocks(size_t total) {
  size_t b = (total + 255) / 256;
  if (b > 16384) b = 16384;
  return (int)(b < 1 ? 1 : b);
}

// the 8 lattice corners of coarse cell (cx, cy, cz), index dz*4 + dy*2 + dx; every address is a lattice point of the
// n^3 grid: (c + 1) * s <= C * s = n - 1 on every axis
__device__ __forceinline__ void band_corners(const float* grid, unsigned n, unsigned s, unsigned cx, unsigned cy,
                                             unsigned cz, float v[8]) {
  const size_t p = ((size_t)(cz * s) * n + cy * s) * n + cx * s;
  const size_t dx = s, dy = (size_t)s * n, dz = (size_t)s * n * n;
  v[0] = grid[p];           v[1] = grid[p + dx];
  v[2] = grid[p + dy];      v[3] = grid[p + dy + dx];
  v[4] = grid[p + dz];      v[5] = grid[p + dz + dx];
  v[6] = grid[p + dz + dy]; v[7] = grid[p + dz + dy + dx];
}

__device__ __forceinline__ void band_minmax(const float v[8], float& lo, float& hi) {
  lo = v[0];
  hi = v[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    lo = fminf(lo, v[k]);
    hi = fmaxf(hi, v[k]);
  }
}

// the cells whose closed box holds index i of one axis: i / s, and the one below it when i is a multiple of s; clipped
// to 0 .. C - 1 (i = R gives C - 1 alone)
__device__ __forceinline__ void band_axis_cells(unsigned i, unsigned s, unsigned C, unsigned& c0, unsigned& c1) {
  c1 = i / s;
  c0 = (i % s == 0 && c1 > 0) ? c1 - 1 : c1;
  if (c1 > C - 1) c1 = C - 1;
}

__device__ __forceinline__ bool band_in_active_box(const unsigned* __restrict__ mask, unsigned s, unsigned C, unsigned ix,
                                                   unsigned iy, unsigned iz) {
  unsigned x0, x1, y0, y1, z0, z1;
  band_axis_cells(ix, s, C, x0, x1);
  band_axis_cells(iy, s, C, y0, y1);
  band_axis_cells(iz, s, C, z0, z1);
  for (unsigned z = z0; z <= z1; ++z)
    for (unsigned y = y0; y <= y1; ++y)
      for (unsigned x = x0; x <= x1; ++x)
        if (mask[((size_t)z * C + y) * C + x]) return true;
  return false;
}

__device__ __forceinline__ bool band_on_lattice(unsigned s, unsigned ix, unsigned iy, unsigned iz) {
  return ix % s == 0 && iy % s == 0 && iz % s == 0;
}

__device__ __forceinline__ float band_lerp(float a, float b, float t) {
  const float u = 1.0f - t;
  const float p = u * a;
  const float q = t * b;
  return p + q;
}

// grid_points_kernel's expression (numpy.linspace in float64, cast to float32)
__device__ __forceinline__ float band_coord(const GridSpec& g, int a, int i) {
  double v = (double)i * g.step[a];
  v = v + g.start[a];
  if (i == g.res - 1 && g.res > 1) v = g.stop[a];
  return (float)v;
}

// entry i of a point list: idx[i], or (idx == nullptr) point i of the lattice of stride s in flat (lz, ly, lx) order
// over (C + 1)^3, as its index in the n^3 grid
__device__ __forceinline__ unsigned band_listed(const int* __restrict__ idx, unsigned s, unsigned C1, unsigned n,
                                                size_t i) {
  if (idx) return (unsigned)idx[i];
  const unsigned l = (unsigned)i;
  const unsigned lx = l % C1, ly = (l / C1) % C1, lz = l / (C1 * C1);
  return ((lz * s) * n + ly * s) * n + lx * s;
}

__global__ __launch_bounds__(256) void band_cell_rule_kernel(const float* __restrict__ grid, unsigned n, unsigned s,
                                                             unsigned C, float iso, float margin,
                                                             unsigned* __restrict__ mask) {
  const size_t nc = (size_t)C * C * C;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nc; q += (size_t)gridDim.x * blockDim.x) {
    const unsigned c = (unsigned)q;
    float v[8], lo, hi;
    band_corners(grid, n, s, c % C, (c / C) % C, c / (C * C), v);
    band_minmax(v, lo, hi);
    const float d = hi - lo;
    const float t = margin * d;
    const float a = lo - t;
    const float b = hi + t;
    mask[q] = (a < iso && b >= iso) ? 1u : 0u;
  }
}

__global__ __launch_bounds__(256) void band_dilate_kernel(const unsigned* __restrict__ in, unsigned C,
                                                          unsigned* __restrict__ out) {
  const size_t nc = (size_t)C * C * C;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nc; q += (size_t)gridDim.x * blockDim.x) {
    const unsigned c = (unsigned)q;
    const unsigned cx = c % C, cy = (c / C) % C, cz = c / (C * C);
    const unsigned x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < C ? cx + 1 : C - 1;
    const unsigned y0 = cy > 0 ? cy - 1 : 0, y1 = cy + 1 < C ? cy + 1 : C - 1;
    const unsigned z0 = cz > 0 ? cz - 1 : 0, z1 = cz + 1 < C ? cz + 1 : C - 1;
    unsigned any = 0;
    for (unsigned z = z0; z <= z1; ++z)
      for (unsigned y = y0; y <= y1; ++y)
        for (unsigned x = x0; x <= x1; ++x) any |= in[((size_t)z * C + y) * C + x];
    out[q] = any ? 1u : 0u;
  }
}

__global__ __launch_bounds__(256) void band_point_flags_kernel(const unsigned* __restrict__ mask, unsigned n, unsigned s,
                                                               unsigned C, unsigned* __restrict__ flag) {
  const size_t np = (size_t)n * n * n;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < np; q += (size_t)gridDim.x * blockDim.x) {
    const unsigned p = (unsigned)q;
    const unsigned ix = p % n, iy = (p / n) % n, iz = p / (n * n);
    flag[q] = (!band_on_lattice(s, ix, iy, iz) && band_in_active_box(mask, s, C, ix, iy, iz)) ? 1u : 0u;
  }
}

// the flagged indices in ascending order; an entry beyond the list's capacity is dropped (the count tells)
__global__ __launch_bounds__(256) void band_compact_kernel(const unsigned* __restrict__ flag,
                                                           const unsigned* __restrict__ off, size_t np, size_t cap,
                                                           int* __restrict__ idx) {
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < np; q += (size_t)gridDim.x * blockDim.x)
    if (flag[q] && off[q] < cap) idx[off[q]] = (int)q;
}

__global__ __launch_bounds__(256) void band_coords_kernel(GridSpec g, const int* __restrict__ idx, unsigned s,
                                                          unsigned C1, size_t first, size_t count,
                                                          float* __restrict__ pts) {
  const unsigned n = (unsigned)g.res;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned p = band_listed(idx, s, C1, n, first + i);
    pts[i * 3 + 0] = band_coord(g, 0, (int)(p % n));
    pts[i * 3 + 1] = band_coord(g, 1, (int)((p / n) % n));
    pts[i * 3 + 2] = band_coord(g, 2, (int)(p / (n * n)));
  }
}

// grid[point i of the list] = vals[i]; an index outside the grid (a caller's list) is skipped
__global__ __launch_bounds__(256) void band_scatter_kernel(const float* __restrict__ vals, const int* __restrict__ idx,
                                                           unsigned s, unsigned C1, unsigned n, size_t first,
                                                           size_t count, float* __restrict__ grid) {
  const size_t np = (size_t)n * n * n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned p = band_listed(idx, s, C1, n, first + i);
    if (p < np) grid[p] = vals[i];
  }
}

// reads lattice points only and writes none of them: in place on the one tensor
__global__ __launch_bounds__(256) void band_fill_kernel(float* grid, unsigned n, unsigned s, unsigned C,
                                                        const unsigned* __restrict__ mask) {
  const size_t np = (size_t)n * n * n;
  const float fs = (float)s;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < np; q += (size_t)gridDim.x * blockDim.x) {
    const unsigned p = (unsigned)q;
    const unsigned ix = p % n, iy = (p / n) % n, iz = p / (n * n);
    if (band_on_lattice(s, ix, iy, iz) || band_in_active_box(mask, s, C, ix, iy, iz)) continue;
    const unsigned cx = ix / s < C - 1 ? ix / s : C - 1;
    const unsigned cy = iy / s < C - 1 ? iy / s : C - 1;
    const unsigned cz = iz / s < C - 1 ? iz / s : C - 1;
    const float tx = (float)(ix - cx * s) / fs, ty = (float)(iy - cy * s) / fs, tz = (float)(iz - cz * s) / fs;
    float v[8], lo, hi;
    band_corners(grid, n, s, cx, cy, cz, v);
    band_minmax(v, lo, hi);
    const float x00 = band_lerp(v[0], v[1], tx), x01 = band_lerp(v[2], v[3], tx);
    const float x10 = band_lerp(v[4], v[5], tx), x11 = band_lerp(v[6], v[7], tx);
    const float y0 = band_lerp(x00, x01, ty), y1 = band_lerp(x10, x11, ty);
    const float r = band_lerp(y0, y1, tz);
    grid[q] = fminf(fmaxf(r, lo), hi);
  }
}

struct BandWs {
  unsigned *flag, *off, *bsum, *mtmp, *coff;
  size_t total;
};

BandWs band_layout(void* ws, int R, int s) {
  const size_t n = (size_t)R + 1, np = n * n * n, C = (size_t)(R / s), nc = C * C * C;
  WsCursor c(ws);
  BandWs w;
  w.flag = c.take<unsigned>(np);
  w.off = c.take<unsigned>(np);
  w.bsum = c.take<unsigned>(scan_bsum_items(np));
  w.mtmp = c.take<unsigned>(nc);
  w.coff = c.take<unsigned>(nc);
  w.total = c.next();
  return w;
}

}  // namespace

static size_t band_select_ws_bytes(int R, int s) { return band_layout(nullptr, R, s).total; }

// band_shape_ok(R, s) is the caller's to check.  cell_mask [(R/s)^3] 0 / 1; idx: the band points' flat indices in
// ascending order (entries beyond idx_capacity are dropped); counts (device) = {band points, active cells}
static hipError_t band_select_launch(const float* grid, int R, int s, float iso, float margin, int dilate,
                                     int* cell_mask, int* idx, size_t idx_capacity, unsigned long long* counts,
                                     void* ws, hipStream_t st) {
  const BandWs w = band_layout(ws, R, s);
  const unsigned n = (unsigned)R + 1, C = (unsigned)(R / s);
  const size_t np = (size_t)n * n * n, nc = (size_t)C * C * C;
  // the rounds ping-pong between the caller's mask and the workspace's; the last one lands in the caller's
  unsigned* user = reinterpret_cast<unsigned*>(cell_mask);
  unsigned* cur = (dilate & 1) ? w.mtmp : user;
  unsigned* nxt = (dilate & 1) ? user : w.mtmp;
  hipLaunchKernelGGL(band_cell_rule_kernel, dim3(band_blocks(nc)), dim3(256), 0, st, grid, n, (unsigned)s, C, iso,
                     margin, cur);
  for (int r = 0; r < dilate; ++r) {
    hipLaunchKernelGGL(band_dilate_kernel, dim3(band_blocks(nc)), dim3(256), 0, st, cur, C, nxt);
    unsigned* t = cur;
    cur = nxt;
    nxt = t;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = exclusive_scan(user, w.coff, nc, w.bsum, counts + 1, st)) != hipSuccess) return e;   // active cells
  hipLaunchKernelGGL(band_point_flags_kernel, dim3(band_blocks(np)), dim3(256), 0, st, user, n, (unsigned)s, C, w.flag);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = exclusive_scan(w.flag, w.off, np, w.bsum, counts, st)) != hipSuccess) return e;      // band points
  hipLaunchKernelGGL(band_compact_kernel, dim3(band_blocks(np)), dim3(256), 0, st, w.flag, w.off, np, idx_capacity,
                     idx);
  return hipGetLastError();
}

hipError_t band_coords_launch(const GridSpec& g, const int* idx, int s, size_t first, size_t count, float* pts,
                              hipStream_t st) {
  const unsigned C1 = s > 0 ? (unsigned)((g.res - 1) / s + 1) : 1u;
  hipLaunchKernelGGL(band_coords_kernel, dim3(band_blocks(count)), dim3(256), 0, st, g, idx, (unsigned)s, C1, first,
                     count, pts);
  return hipGetLastError();
}

hipError_t band_scatter_launch(const float* vals, const int* idx, int R, int s, size_t first, size_t count, float* grid,
                               hipStream_t st) {
  const unsigned C1 = s > 0 ? (unsigned)(R / s + 1) : 1u;
  hipLaunchKernelGGL(band_scatter_kernel, dim3(band_blocks(count)), dim3(256), 0, st, vals, idx, (unsigned)s, C1,
                     (unsigned)R + 1, first, count, grid);
  return hipGetLastError();
}

static hipError_t band_fill_launch(float* grid, int R, int s, const int* cell_mask, hipStream_t st) {
  const unsigned n = (unsigned)R + 1;
  hipLaunchKernelGGL(band_fill_kernel, dim3(band_blocks((size_t)n * n * n)), dim3(256), 0, st, grid, n, (unsigned)s,
                     (unsigned)(R / s), reinterpret_cast<const unsigned*>(cell_mask));
  return hipGetLastError();
}

}  // namespace disn

// ---- the C entries of include/disn_amd.h: argument and workspace checks, then the launchers above ----
using namespace disn;

#define DISN_TRY(expr)                    \
  do {                                    \
    hipError_t _e = (expr);               \
    if (_e != hipSuccess) return (int)_e; \
  } while (0)

extern "C" {

size_t disn_grid_band_select_workspace_bytes(int R, int stride) {
  return band_shape_ok(R, stride) ? band_select_ws_bytes(R, stride) : 0;
}

int disn_grid_band_select(const float* grid, int R, int stride, float iso, float margin, int dilate,
                          int32_t* cell_mask, int32_t* idx, int64_t idx_capacity, uint64_t* counts, void* ws,
                          size_t ws_bytes, void* stream) {
  if (!grid || !cell_mask || !idx || !counts || !ws || !band_shape_ok(R, stride) || dilate < 0 || idx_capacity < 0 ||
      !(margin >= 0.0f))
    return DISN_E_ARG;
  if (ws_bytes < band_select_ws_bytes(R, stride)) return DISN_E_WS;
  DISN_TRY(band_select_launch(grid, R, stride, iso, margin, dilate, cell_mask, idx, (size_t)idx_capacity,
                              reinterpret_cast<unsigned long long*>(counts), ws, (hipStream_t)stream));
  return 0;
}

int disn_grid_band_fill(float* grid, int R, int stride, const int32_t* cell_mask, void* stream) {
  if (!grid || !cell_mask || !band_shape_ok(R, stride)) return DISN_E_ARG;
  DISN_TRY(band_fill_launch(grid, R, stride, cell_mask, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
