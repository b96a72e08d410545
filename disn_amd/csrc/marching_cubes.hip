// Iso-surface extraction on the device: replaces the reference's
//   to_binary -> .dist file -> os.system("./isosurface/computeMarchingCubes f.dist f.obj -i iso")
// round trip (test/create_sdf.py:292-323) for the grid that is already resident in HBM.
//
// Indexed marching cubes: one vertex per cut grid edge (shared by the up to four cells around
// it), one index triple per triangle; case table derived in tools/gen_mc_tables.py (face-
// consistent, crack-free).  Order and arithmetic are those of oracle/mc_oracle.py, so the
// result is compared bit for bit (THIS FILE IS COMPILED WITH -ffp-contract=off):
//   vertex id  = rank of the cut edge in the flat order 3*p + axis, p = (iz*n + iy)*n + ix
//   position   = c0 + t*(c1 - c0) on the cut axis, t = (iso - v0)/(v1 - v0), float32
//   faces      = cells in flat order (iz,iy,ix) over R^3, triangles in table order
// All kernels are HBM-bound streaming passes over the (R+1)^3 grid; the scans are three-pass
// (block scan, scan of block sums, add).  The per-element bodies are shared by the single-grid kernels and
// the batched ones (B grids, one scan, one read-back of the sizes: a group of views of the test set); those that dual
// contouring needs as well (axis value, case, flags, cut edge and its point, the batched vertex kernel) are
// grid_mesh.hpp's.  This file keeps the scan, the triangle table walk, the workspaces and its entries.
#include "grid_mesh.hpp"

namespace disn {

// ---------------------------------------------------------------------------
// exclusive scan of uint32, 4096 items per block
// ---------------------------------------------------------------------------
constexpr int kScanItems = 16;
constexpr int kScanBlock = 256 * kScanItems;

__global__ __launch_bounds__(256) void scan_block_kernel(const unsigned* __restrict__ in,
                                                         unsigned* __restrict__ out, size_t n,
                                                         unsigned* __restrict__ bsum) {
  __shared__ unsigned wsum[4];
  const size_t base = (size_t)blockIdx.x * kScanBlock + (size_t)threadIdx.x * kScanItems;
  unsigned v[kScanItems];
  unsigned tsum = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    v[i] = (base + i < n) ? in[base + i] : 0u;
    tsum += v[i];
  }
  // inclusive scan of the 64 thread sums of a wave, then of the 4 wave sums
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = tsum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned u = __shfl_up(inc, off);
    if (lane >= off) inc += u;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  unsigned woff = 0;
  for (int w = 0; w < wave; ++w) woff += wsum[w];
  unsigned run = woff + inc - tsum;  // exclusive prefix of this thread
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    if (base + i < n) out[base + i] = run;
    run += v[i];
  }
  if (threadIdx.x == 255) bsum[blockIdx.x] = woff + inc;
}

// one block: exclusive scan of the block sums in place, grand total -> *total
__global__ __launch_bounds__(1024) void scan_sums_kernel(unsigned* __restrict__ bsum, int nb,
                                                         unsigned long long* __restrict__ total) {
  __shared__ unsigned long long carry;
  __shared__ unsigned wsum[16];
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + threadIdx.x;
    const unsigned v = i < nb ? bsum[i] : 0u;
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned u = __shfl_up(inc, off);
      if (lane >= off) inc += u;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    const unsigned long long c = carry;
    if (i < nb) bsum[i] = (unsigned)(c + woff + inc - v);
    __syncthreads();
    if (threadIdx.x == 1023) carry = c + woff + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void scan_add_kernel(unsigned* __restrict__ out, size_t n,
                                                       const unsigned* __restrict__ bsum) {
  const size_t base = (size_t)blockIdx.x * kScanBlock + (size_t)threadIdx.x * kScanItems;
  const unsigned add = bsum[blockIdx.x];
#pragma unroll
  for (int i = 0; i < kScanItems; ++i)
    if (base + i < n) out[base + i] += add;
}

static_assert(kScanBlock == kScanBlockItems, "kernels.hpp sizes the callers' block sums");
hipError_t exclusive_scan(const unsigned* in, unsigned* out, size_t n, unsigned* bsum,
                          unsigned long long* total, hipStream_t st) {
  const int nb = (int)((n + kScanBlock - 1) / kScanBlock);
  hipLaunchKernelGGL(scan_block_kernel, dim3(nb), dim3(256), 0, st, in, out, n, bsum);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, st, bsum, nb, total);
  hipLaunchKernelGGL(scan_add_kernel, dim3(nb), dim3(256), 0, st, out, n, bsum);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// pass 1: cut-edge flags (3 per grid point) and triangle counts (1 per cell)
// ---------------------------------------------------------------------------
// one grid point p of an n^3 grid: its three edge flags and (where it is the low corner of a cell) the cell's count;
// vol, eflag and ccount are the grid's OWN blocks
__device__ __forceinline__ void mc_flags_point(const float* __restrict__ vol, int n, float iso, size_t p,
                                               unsigned* __restrict__ eflag, unsigned* __restrict__ ccount) {
  const int R = n - 1;
  const int ix = (int)(p % n), iy = (int)((p / n) % n), iz = (int)(p / ((size_t)n * n));
  const int c = grid_flags_point(vol, n, iso, p, ix, iy, iz, eflag);
  if (c >= 0) ccount[((size_t)iz * R + iy) * R + ix] = kMcNtri[c];
}

__global__ __launch_bounds__(256) void mc_flags_kernel(const float* __restrict__ vol, int n,
                                                       float iso, unsigned* __restrict__ eflag,
                                                       unsigned* __restrict__ ccount) {
  const size_t total = (size_t)n * n * n;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (size_t)gridDim.x * blockDim.x)
    mc_flags_point(vol, n, iso, p, eflag, ccount);
}

// pass 2: one vertex per cut edge, at its rank
__global__ __launch_bounds__(256) void mc_verts_kernel(const float* __restrict__ vol, GridSpec g,
                                                       float iso, const unsigned* __restrict__ eflag,
                                                       const unsigned* __restrict__ eidx,
                                                       float* __restrict__ verts) {
  const int n = g.res;
  const size_t total = (size_t)3 * n * n * n;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (size_t)gridDim.x * blockDim.x) {
    if (!eflag[e]) continue;
    grid_edge_point(g, grid_edge(vol, g, iso, e), verts + (size_t)eidx[e] * 3);
  }
}

// pass 3: index triples.  c: cell of this grid, coff/eidx: the grid's own blocks of the two scans; vbase is taken off
// every vertex id (0 for a grid scanned alone, the grid's first vertex rank in a batch scan)
__device__ __forceinline__ void mc_cell_faces(const float* __restrict__ vol, int n, float iso, size_t c,
                                              const unsigned* __restrict__ coff,
                                              const unsigned* __restrict__ eidx, unsigned vbase,
                                              int* __restrict__ faces) {
  const int R = n - 1;
  const int ix = (int)(c % R), iy = (int)((c / R) % R), iz = (int)(c / ((size_t)R * R));
  const int mask = grid_cell_case(vol, n, iso, ((size_t)iz * n + iy) * n + ix);
  const int nt = kMcNtri[mask];
  if (!nt) return;
  int* o = faces + (size_t)coff[c] * 3;
  for (int k = 0; k < 3 * nt; ++k) {
    const int e = kMcTri[mask][k];
    o[k] = (int)(eidx[grid_cube_edge_slot(n, ix, iy, iz, e)] - vbase);
  }
}

__global__ __launch_bounds__(256) void mc_faces_kernel(const float* __restrict__ vol, int n,
                                                       float iso, const unsigned* __restrict__ coff,
                                                       const unsigned* __restrict__ eidx,
                                                       int* __restrict__ faces) {
  const int R = n - 1;
  const size_t cells = (size_t)R * R * R;
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells;
       c += (size_t)gridDim.x * blockDim.x)
    mc_cell_faces(vol, n, iso, c, coff, eidx, 0u, faces);
}

// ---------------------------------------------------------------------------
// B grids of one resolution in one set of passes: the flags and counts of grid b lie at b*3*n^3 and b*R^3 of the
// concatenated arrays, ONE scan runs over each, and a grid's first scan value is its vertex / triangle base.  Every
// grid is addressed through its own block of vol (the element bodies above see one grid and nothing else), so the
// order and the arithmetic per grid are those of the single-grid kernels.  All flat counts are below 2^32 (the API
// refuses larger batches), so the split of a flat index into (grid, element) is 32-bit.  The vertices of a batch are
// written by grid_mesh.hpp's grid_points_batch_kernel.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mc_flags_batch_kernel(const float* __restrict__ vol, int n, unsigned np,
                                                             unsigned total, float iso,
                                                             unsigned* __restrict__ eflag,
                                                             unsigned* __restrict__ ccount) {
  const unsigned R = (unsigned)n - 1, nc = R * R * R;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    const unsigned b = (unsigned)q / np, p = (unsigned)q - b * np;
    mc_flags_point(vol + (size_t)b * np, n, iso, p, eflag + (size_t)3 * b * np, ccount + (size_t)b * nc);
  }
}

// counts[b] = {vertices, triangles} of grid b: the difference of consecutive bases, the grand totals closing the last
__global__ void mc_batch_counts_kernel(const unsigned* __restrict__ eidx, const unsigned* __restrict__ coff,
                                       size_t ne, size_t nc, int B,
                                       const unsigned long long* __restrict__ totals,
                                       unsigned long long* __restrict__ counts) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const unsigned long long v0 = eidx[(size_t)b * ne], f0 = coff[(size_t)b * nc];
  const unsigned long long v1 = b + 1 < B ? eidx[(size_t)(b + 1) * ne] : totals[0];
  const unsigned long long f1 = b + 1 < B ? coff[(size_t)(b + 1) * nc] : totals[1];
  counts[2 * b + 0] = v1 - v0;
  counts[2 * b + 1] = f1 - f0;
}

// the triangle goes to its GLOBAL rank; its vertex ids are LOCAL to the grid (the grid's vertex base taken off)
__global__ __launch_bounds__(256) void mc_faces_batch_kernel(const float* __restrict__ vol, int n, unsigned np,
                                                             unsigned total, float iso,
                                                             const unsigned* __restrict__ coff,
                                                             const unsigned* __restrict__ eidx,
                                                             int* __restrict__ faces) {
  const unsigned R = (unsigned)n - 1, nc = R * R * R;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    const unsigned b = (unsigned)q / nc, c = (unsigned)q - b * nc;
    const unsigned* ei = eidx + (size_t)3 * b * np;
    // (coff is indexed at the flat cell, so its values are global ranks; faces is the whole batch's array)
    mc_cell_faces(vol + (size_t)b * np, n, iso, c, coff + (size_t)b * nc, ei, ei[0], faces);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct McWs {
  unsigned *eflag, *eidx, *ccount, *coff, *bsum;
  size_t total;
};

static McWs mc_layout(void* ws, int R) {
  const size_t n = (size_t)R + 1, ne = 3 * n * n * n, nc = (size_t)R * R * R;
  WsCursor c(ws);
  McWs w;
  w.eflag = c.take<unsigned>(ne);
  w.eidx = c.take<unsigned>(ne);
  w.ccount = c.take<unsigned>(nc);
  w.coff = c.take<unsigned>(nc);
  w.bsum = c.take<unsigned>(scan_bsum_items(ne));
  w.total = c.next();
  return w;
}

static size_t mc_ws_bytes(int R) { return mc_layout(nullptr, R).total; }

struct McBatchWs {
  unsigned *eflag, *eidx, *ccount, *coff, *bsum;
  unsigned long long* totals;  // {vertices, triangles} of the whole batch
  size_t total;
};

static McBatchWs mc_batch_layout(void* ws, int B, int R) {
  const size_t n = (size_t)R + 1, ne = (size_t)B * 3 * n * n * n, nc = (size_t)B * R * R * R;
  WsCursor c(ws);
  McBatchWs w;
  w.eflag = c.take<unsigned>(ne);
  w.eidx = c.take<unsigned>(ne);
  w.ccount = c.take<unsigned>(nc);
  w.coff = c.take<unsigned>(nc);
  w.bsum = c.take<unsigned>(scan_bsum_items(ne));
  w.totals = c.take<unsigned long long>(2);
  w.total = c.next();
  return w;
}

static size_t mc_batch_ws_bytes(int B, int R) { return mc_batch_layout(nullptr, B, R).total; }

// counts[0] = vertices, counts[1] = triangles (device memory); fills ws for mc_emit_launch
static hipError_t mc_count_launch(const float* vol, int R, float iso, unsigned long long* counts, void* ws,
                                  hipStream_t st) {
  const McWs w = mc_layout(ws, R);
  const int n = R + 1;
  const size_t np = (size_t)n * n * n, nc = (size_t)R * R * R;
  hipLaunchKernelGGL(mc_flags_kernel, dim3(blocks_for(np)), dim3(256), 0, st, vol, n, iso, w.eflag,
                     w.ccount);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = exclusive_scan(w.eflag, w.eidx, 3 * np, w.bsum, counts, st)) != hipSuccess) return e;
  return exclusive_scan(w.ccount, w.coff, nc, w.bsum, counts + 1, st);
}

static hipError_t mc_emit_launch(const float* vol, const GridSpec& g, float iso, float* verts, int* faces,
                                 void* ws, hipStream_t st) {
  const int R = g.res - 1;
  const McWs w = mc_layout(ws, R);
  const size_t np = (size_t)g.res * g.res * g.res, nc = (size_t)R * R * R;
  hipLaunchKernelGGL(mc_verts_kernel, dim3(blocks_for(3 * np)), dim3(256), 0, st, vol, g, iso,
                     w.eflag, w.eidx, verts);
  hipLaunchKernelGGL(mc_faces_kernel, dim3(blocks_for(nc)), dim3(256), 0, st, vol, g.res, iso, w.coff,
                     w.eidx, faces);
  return hipGetLastError();
}

// B grids [B,(R+1)^3] in one set of passes: counts [B,2] per grid; verts / faces of all grids back to back in grid
// order, face indices local to their grid.  B*3*(R+1)^3 < 2^32 is the caller's to check (grid_batch_ok)
static hipError_t mc_count_batch_launch(const float* vol, int B, int R, float iso, unsigned long long* counts,
                                        void* ws, hipStream_t st) {
  const McBatchWs w = mc_batch_layout(ws, B, R);
  const int n = R + 1;
  const size_t np = (size_t)n * n * n, nc = (size_t)R * R * R;
  hipLaunchKernelGGL(mc_flags_batch_kernel, dim3(blocks_for(B * np)), dim3(256), 0, st, vol, n, (unsigned)np,
                     (unsigned)(B * np), iso, w.eflag, w.ccount);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = exclusive_scan(w.eflag, w.eidx, B * 3 * np, w.bsum, w.totals, st)) != hipSuccess) return e;
  if ((e = exclusive_scan(w.ccount, w.coff, B * nc, w.bsum, w.totals + 1, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(mc_batch_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, st, w.eidx, w.coff, 3 * np, nc, B,
                     w.totals, counts);
  return hipGetLastError();
}

// vertices of all B grids, their boxes kMcBatchBoxes per launch / triangles of all B grids
static hipError_t mc_verts_batch_launch(const float* vol, const double* sdf_params_host, int B, int R, float iso,
                                        float* verts, void* ws, hipStream_t st) {
  const McBatchWs w = mc_batch_layout(ws, B, R);
  const int n = R + 1;
  const size_t np = (size_t)n * n * n;
  for (int b0 = 0; b0 < B; b0 += kMcBatchBoxes) {
    const int nb = B - b0 < kMcBatchBoxes ? B - b0 : kMcBatchBoxes;
    hipLaunchKernelGGL(grid_points_batch_kernel, dim3(blocks_for(3 * np * nb)), dim3(256), 0, st, vol,
                       grid_boxes(sdf_params_host, b0, nb, R), n, (unsigned)(3 * np), (unsigned)b0, (unsigned)nb, iso,
                       w.eflag, w.eidx, verts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

static hipError_t mc_faces_batch_launch(const float* vol, int B, int R, float iso, int* faces, void* ws,
                                        hipStream_t st) {
  const McBatchWs w = mc_batch_layout(ws, B, R);
  const int n = R + 1;
  const size_t np = (size_t)n * n * n, nc = (size_t)R * R * R;
  hipLaunchKernelGGL(mc_faces_batch_kernel, dim3(blocks_for(B * nc)), dim3(256), 0, st, vol, n, (unsigned)np,
                     (unsigned)(B * nc), iso, w.coff, w.eidx, faces);
  return hipGetLastError();
}

}  // namespace disn

// ---- the C entries of include/disn_amd.h: argument and workspace checks, then the launchers above ----
using namespace disn;

extern "C" {

size_t disn_mc_workspace_bytes(int R) { return (R < 1 || R > 1290) ? 0 : mc_ws_bytes(R); }

int disn_mc_count(const float* sdf, int R, float iso, uint64_t* counts, void* ws, size_t ws_bytes,
                  void* stream) {
  if (!sdf || !counts || !ws || R < 1) return DISN_E_ARG;
  if (R > 1290) return DISN_E_SHAPE;  // 3*(R+1)^3 edge slots must fit the 32-bit scan
  if (ws_bytes < mc_ws_bytes(R)) return DISN_E_WS;
  DISN_TRY(mc_count_launch(sdf, R, iso, reinterpret_cast<unsigned long long*>(counts), ws,
                           (hipStream_t)stream));
  return 0;
}

int disn_mc_emit(const float* sdf, const double* sdf_params_host, int R, float iso, float* verts,
                 int32_t* faces, void* ws, size_t ws_bytes, void* stream) {
  GridSpec g;
  if (!sdf || !verts || !faces || !ws || !grid_spec(sdf_params_host, R, &g)) return DISN_E_ARG;
  if (R > 1290) return DISN_E_SHAPE;
  if (ws_bytes < mc_ws_bytes(R)) return DISN_E_WS;
  DISN_TRY(mc_emit_launch(sdf, g, iso, verts, faces, ws, (hipStream_t)stream));
  return 0;
}

size_t disn_mc_batch_workspace_bytes(int B, int R) { return grid_batch_ok(B, R) ? mc_batch_ws_bytes(B, R) : 0; }

int disn_mc_count_batch(const float* sdf, int B, int R, float iso, uint64_t* counts, void* ws, size_t ws_bytes,
                        void* stream) {
  if (!sdf || !counts || !ws || B < 1 || R < 1) return DISN_E_ARG;
  if (!grid_batch_ok(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < mc_batch_ws_bytes(B, R)) return DISN_E_WS;
  DISN_TRY(mc_count_batch_launch(sdf, B, R, iso, reinterpret_cast<unsigned long long*>(counts), ws,
                                 (hipStream_t)stream));
  return 0;
}

int disn_mc_emit_batch(const float* sdf, const double* sdf_params_host, int B, int R, float iso, float* verts,
                       int32_t* faces, void* ws, size_t ws_bytes, void* stream) {
  if (!sdf || !verts || !faces || !ws || !sdf_params_host || B < 1 || R < 1) return DISN_E_ARG;
  if (!grid_batch_ok(B, R)) return DISN_E_SHAPE;
  if (ws_bytes < mc_batch_ws_bytes(B, R)) return DISN_E_WS;
  DISN_TRY(mc_verts_batch_launch(sdf, sdf_params_host, B, R, iso, verts, ws, (hipStream_t)stream));
  DISN_TRY(mc_faces_batch_launch(sdf, B, R, iso, faces, ws, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
