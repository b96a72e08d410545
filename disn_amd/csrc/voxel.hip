// Voxel IoU of triangle meshes (test/test_iou.py of the reference, whose voxel grids come from PyMesh): surface
// voxelisation, cavity fill, the reference's corner -> index map and the intersection / union counts, on gfx950.
// THIS FILE IS COMPILED WITH -ffp-contract=off: the overlap test below is restated operation for operation in
// tests/voxel_reference.py and every output (a bit set or an integer) is compared bit for bit.  DESIGN §4r.
//
// Bit grids.  An n^3 grid is n*n rows of wpr = ceil(n/32) words: cell (x, y, z) is bit (x & 31) of word
// (z*n + y)*wpr + (x >> 5); the padding bits of a row's last word are always 0.  The KEY grid holds voxel keys
// kmin .. kmin+n-1 per axis (x = kx - kmin), the INDEX grid is the reference's dim^3 array.
//
// Surface voxels.  h = 2.0f / dim, hh = h * 0.5f; voxel k is the closed box of centre c = float(k) * h and half side
// hh.  Triangle (p0, p1, p2) overlaps it when none of 13 axes separates (Akenine-Moller), with
//   v_i = p_i - c;  e0 = p1 - p0, e1 = p2 - p1, e2 = p0 - p2 (from the untranslated vertices);
//   sep(a, b, c, r) = min(a, b, c) > r || max(a, b, c) < -r          (touching is overlap)
//   box axes     sep(v0.x, v1.x, v2.x, hh), then y, z
//   per edge e   X x e: q_i = e.z*v_i.y - e.y*v_i.z, r = (|e.z| + |e.y|) * hh
//                Y x e: q_i = e.x*v_i.z - e.z*v_i.x, r = (|e.x| + |e.z|) * hh
//                Z x e: q_i = e.y*v_i.x - e.x*v_i.y, r = (|e.y| + |e.x|) * hh      (all three vertices projected)
//   plane        n = (e0.y*e1.z - e0.z*e1.y, e0.z*e1.x - e0.x*e1.z, e0.x*e1.y - e0.y*e1.x),
//                s = (n.x*v0.x + n.y*v0.y) + n.z*v0.z, r = ((|n.x| + |n.y|) + |n.z|) * hh, separated when s > r || s < -r
// A zero edge or a zero normal gives q = r = 0 on its axes, which never separates: degenerate triangles fall
// through to the axes that remain meaningful.
// Candidate keys per axis: lo = floor((min/h - 0.5) + 0.99), hi = ceil((max/h + 0.5) - 0.99): the exact range
// widened by at most one key (0.01 of a cell is four orders above the rounding of these expressions), so the
// set of occupied keys is that of testing every key.  Keys kmin-1 and kmin+n are sentinels: a candidate range
// that passes them, or an overlap on one, raises flag bit 0 (the mesh leaves the key range); nothing is clamped.
//
// Load balance.  voxel_tri_kernel: a wave takes 64 triangles, one per lane, to set them up; those with at most
// kSmall candidate cells are packed: the wave's lanes stride over the concatenated cells of all of them (prefix sum
// over the lanes, a six-step search per slot).  The others go to a queue.  voxel_big_kernel: a fixed grid walks the
// queue; the kChunk-cell chunks of all queued triangles are dealt round robin to the blocks, a cell per thread.  A 12-triangle box spanning the grid and a 50 k-triangle marching-cubes mesh both fill the device.
// Bits are set with atomicOr and counts added with integer atomicAdd: the result does not depend on the order.
#include "../../include/disn_amd.h"
#include "kernels.hpp"

namespace disn {

namespace {

constexpr int kSmall = 64;       // most candidate cells of a packed triangle
constexpr int kChunk = 256;      // cells of one block step in voxel_big_kernel: one per thread
constexpr int kBigBlocks = 512;
constexpr int kFillBatch = 8;    // sweeps between two reads of the "changed" flag
constexpr int kFillMaxIter = 4096;

struct VoxGrid {
  float h, hh;
  int kmin, n, wpr;
};

struct Tri {
  float p[9];
  int lo[3], ex, ey, ez;
};

__device__ __forceinline__ bool sep3(float a, float b, float c, float r) {
  return fminf(fminf(a, b), c) > r || fmaxf(fmaxf(a, b), c) < -r;
}

__device__ __forceinline__ bool edge_sep(float ex, float ey, float ez, const float* v, float hh) {
  float r = (fabsf(ez) + fabsf(ey)) * hh;
  if (sep3(ez * v[1] - ey * v[2], ez * v[4] - ey * v[5], ez * v[7] - ey * v[8], r)) return true;
  r = (fabsf(ex) + fabsf(ez)) * hh;
  if (sep3(ex * v[2] - ez * v[0], ex * v[5] - ez * v[3], ex * v[8] - ez * v[6], r)) return true;
  r = (fabsf(ey) + fabsf(ex)) * hh;
  return sep3(ey * v[0] - ex * v[1], ey * v[3] - ex * v[4], ey * v[6] - ex * v[7], r);
}

__device__ __forceinline__ bool tri_box_overlap(const float* p, float cx, float cy, float cz, float hh) {
  float v[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    v[3 * i] = p[3 * i] - cx;
    v[3 * i + 1] = p[3 * i + 1] - cy;
    v[3 * i + 2] = p[3 * i + 2] - cz;
  }
  if (sep3(v[0], v[3], v[6], hh) || sep3(v[1], v[4], v[7], hh) || sep3(v[2], v[5], v[8], hh)) return false;
  const float e0x = p[3] - p[0], e0y = p[4] - p[1], e0z = p[5] - p[2];
  const float e1x = p[6] - p[3], e1y = p[7] - p[4], e1z = p[8] - p[5];
  const float e2x = p[0] - p[6], e2y = p[1] - p[7], e2z = p[2] - p[8];
  if (edge_sep(e0x, e0y, e0z, v, hh) || edge_sep(e1x, e1y, e1z, v, hh) || edge_sep(e2x, e2y, e2z, v, hh))
    return false;
  const float nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
  const float s = (nx * v[0] + ny * v[1]) + nz * v[2];
  const float r = ((fabsf(nx) + fabsf(ny)) + fabsf(nz)) * hh;
  return !(s > r || s < -r);
}

// -> 0 ok, 1 the triangle leaves the key range (or is not finite), 2 a face index is out of range
__device__ __forceinline__ int tri_setup(const float* verts, int64_t nv, const int* faces, int64_t t, const VoxGrid& g,
                                         Tri& T) {
  const int i0 = faces[3 * t], i1 = faces[3 * t + 1], i2 = faces[3 * t + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return 2;
  const int idx[3] = {i0, i1, i2};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    T.p[3 * i] = verts[3 * (int64_t)idx[i]];
    T.p[3 * i + 1] = verts[3 * (int64_t)idx[i] + 1];
    T.p[3 * i + 2] = verts[3 * (int64_t)idx[i] + 2];
  }
  float fin = 0.0f;   // fminf / fmaxf skip a NaN: catch it (and infinities) here
#pragma unroll
  for (int i = 0; i < 9; ++i) fin += T.p[i] * 0.0f;
  if (!(fin == 0.0f)) return 1;
  const float klo = (float)(g.kmin - 1), khi = (float)(g.kmin + g.n);
  int hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float mn = fminf(fminf(T.p[a], T.p[3 + a]), T.p[6 + a]);
    const float mx = fmaxf(fmaxf(T.p[a], T.p[3 + a]), T.p[6 + a]);
    const float lo_f = floorf((mn / g.h - 0.5f) + 0.99f);
    const float hi_f = ceilf((mx / g.h + 0.5f) - 0.99f);
    if (!(lo_f >= klo && hi_f <= khi)) return 1;
    T.lo[a] = (int)lo_f;
    hi[a] = (int)hi_f;
  }
  T.ex = hi[0] - T.lo[0] + 1;
  T.ey = hi[1] - T.lo[1] + 1;
  T.ez = hi[2] - T.lo[2] + 1;
  return 0;
}

__device__ __forceinline__ void test_and_set(const float* p, int kx, int ky, int kz, const VoxGrid& g,
                                             unsigned* bits, int* flags) {
  if (!tri_box_overlap(p, (float)kx * g.h, (float)ky * g.h, (float)kz * g.h, g.hh)) return;
  const int x = kx - g.kmin, y = ky - g.kmin, z = kz - g.kmin;
  if ((unsigned)x >= (unsigned)g.n || (unsigned)y >= (unsigned)g.n || (unsigned)z >= (unsigned)g.n) {
    atomicOr(flags, 1);   // a sentinel key
    return;
  }
  atomicOr(&bits[((size_t)z * g.n + y) * g.wpr + (x >> 5)], 1u << (x & 31));
}

__global__ __launch_bounds__(256) void voxel_tri_kernel(const float* verts, int64_t nv, const int* faces, int64_t nf,
                                                        VoxGrid g, unsigned* bits, int* flags, int2* queue,
                                                        int* qcount) {
  __shared__ float s_p[4][64][9];
  __shared__ int s_lo[4][64][3];
  __shared__ int s_ext[4][64];
  __shared__ int s_pre[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int n = 0;
  if (t < nf) {
    Tri T;
    const int rc = tri_setup(verts, nv, faces, t, g, T);
    if (rc) {
      atomicOr(flags, rc);
    } else {
      const int cells = T.ex * T.ey * T.ez;   // <= (n + 2)^3, n <= 1024
      if (cells <= kSmall) {
        n = cells;
#pragma unroll
        for (int i = 0; i < 9; ++i) s_p[w][lane][i] = T.p[i];
        s_lo[w][lane][0] = T.lo[0];
        s_lo[w][lane][1] = T.lo[1];
        s_lo[w][lane][2] = T.lo[2];
        s_ext[w][lane] = T.ex | (T.ey << 8);
      } else {
        queue[atomicAdd(qcount, 1)] = make_int2((int)t, cells);
      }
    }
  }
  int inc = n;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  s_pre[w][lane] = inc;
  __syncthreads();
  const int total = s_pre[w][63];
  for (int s = lane; s < total; s += 64) {
    int j = 0;   // the first triangle whose inclusive prefix exceeds s
#pragma unroll
    for (int step = 32; step; step >>= 1)
      if (s_pre[w][j + step - 1] <= s) j += step;
    const int local = s - (j ? s_pre[w][j - 1] : 0);
    const int ex = s_ext[w][j] & 0xff, ey = s_ext[w][j] >> 8;
    const int ix = local % ex, iy = (local / ex) % ey, iz = local / (ex * ey);
    float p[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) p[i] = s_p[w][j][i];
    test_and_set(p, s_lo[w][j][0] + ix, s_lo[w][j][1] + iy, s_lo[w][j][2] + iz, g, bits, flags);
  }
}

__global__ __launch_bounds__(256) void voxel_big_kernel(const float* verts, int64_t nv, const int* faces, VoxGrid g,
                                                        unsigned* bits, int* flags, const int2* queue,
                                                        const int* qcount) {
  __shared__ int2 s_q[256];   // the queue, a tile at a time: one load per thread instead of a serial walk of global memory
  const int nq = *qcount, G = gridDim.x, b = blockIdx.x;
  int off = 0;   // chunks dealt so far, modulo G
  for (int base = 0; base < nq; base += 256) {
    __syncthreads();
    if (base + (int)threadIdx.x < nq) s_q[threadIdx.x] = queue[base + threadIdx.x];
    __syncthreads();
    const int m = nq - base < 256 ? nq - base : 256;
    for (int j = 0; j < m; ++j) {
      const int2 e = s_q[j];
      const int chunks = (e.y + kChunk - 1) / kChunk;
      const int c0 = (b - off + G) % G;
      if (c0 < chunks) {
        Tri T;
        if (tri_setup(verts, nv, faces, e.x, g, T) == 0) {   // (it was 0 when the triangle was queued)
          const int exy = T.ex * T.ey;
          for (int c = c0; c < chunks; c += G) {
            // consecutive cells run along x, so the lanes that hit one word are neighbours: OR their bits down the
            // run (word indices never decrease along a chunk) and let the run's first lane issue one atomic
            const int s = c * kChunk + threadIdx.x;
            const int lane = threadIdx.x & 63;
            unsigned word = 0xffffffffu - lane, mask = 0;   // (no cell: a word index of its own)
            if (s < e.y) {
              const int iz = s / exy, r = s - iz * exy, iy = r / T.ex, ix = r - iy * T.ex;
              const int kx = T.lo[0] + ix, ky = T.lo[1] + iy, kz = T.lo[2] + iz;
              const int x = kx - g.kmin, y = ky - g.kmin, z = kz - g.kmin;
              const bool inside = (unsigned)x < (unsigned)g.n && (unsigned)y < (unsigned)g.n && (unsigned)z < (unsigned)g.n;
              if (inside) word = ((unsigned)z * g.n + y) * g.wpr + (x >> 5);   // < 2^25
              if (tri_box_overlap(T.p, (float)kx * g.h, (float)ky * g.h, (float)kz * g.h, g.hh)) {
                if (inside) mask = 1u << (x & 31);
                else atomicOr(flags, 1);   // a sentinel key
              }
            }
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
              const unsigned ow = __shfl_down(word, d, 64), om = __shfl_down(mask, d, 64);
              if (lane + d < 64 && ow == word) mask |= om;
            }
            const unsigned pw = __shfl_up(word, 1, 64);
            if (mask && (lane == 0 || pw != word)) atomicOr(&bits[word], mask);
          }
        }
      }
      off = (off + chunks) % G;
    }
  }
}

__device__ __forceinline__ unsigned row_mask(int xw, int n, int wpr) {
  return (xw == wpr - 1 && (n & 31)) ? ((1u << (n & 31)) - 1u) : 0xffffffffu;
}

// outside seeds: the unoccupied cells of the grid's six faces (the grid padded by one empty layer joins them)
__global__ __launch_bounds__(256) void fill_init_kernel(const unsigned* S, int n, int wpr, unsigned* O) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * n * wpr) return;
  const int xw = (int)(i % wpr), y = (int)((i / wpr) % n), z = (int)(i / ((int64_t)wpr * n));
  unsigned m = 0;
  if (y == 0 || y == n - 1 || z == 0 || z == n - 1) m = row_mask(xw, n, wpr);
  if (xw == 0) m |= 1u;
  if (xw == wpr - 1) m |= 1u << ((n - 1) & 31);
  O[i] = m & ~S[i];
}

// one sweep: a word takes what its six neighbours hold, then spreads it along x through its free cells.  The
// update is monotone and in place, so any interleaving reaches the same fixed point; `changed` tells the host
// whether a sweep still moved.
__global__ __launch_bounds__(256) void fill_sweep_kernel(const unsigned* S, int n, int wpr, unsigned* O, int* changed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * n * wpr) return;
  const int xw = (int)(i % wpr), y = (int)((i / wpr) % n), z = (int)(i / ((int64_t)wpr * n));
  const int64_t sy = wpr, sz = (int64_t)wpr * n;
  const unsigned o = O[i];
  const unsigned free_ = row_mask(xw, n, wpr) & ~S[i];
  unsigned m = o;
  if (y > 0) m |= O[i - sy];
  if (y < n - 1) m |= O[i + sy];
  if (z > 0) m |= O[i - sz];
  if (z < n - 1) m |= O[i + sz];
  if (xw > 0) m |= O[i - 1] >> 31;
  if (xw < wpr - 1) m |= O[i + 1] << 31;
  m &= free_;
  for (int k = 0; k < 32; ++k) {
    const unsigned t = m | (((m << 1) | (m >> 1)) & free_);
    if (t == m) break;
    m = t;
  }
  if (m != o) {
    O[i] = m;
    *changed = 1;
  }
}

__global__ __launch_bounds__(256) void fill_finish_kernel(const unsigned* O, int n, int wpr, unsigned* solid) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * n * wpr) return;
  solid[i] = row_mask((int)(i % wpr), n, wpr) & ~O[i];
}

// every occupied key sets the index cells of its eight corners: lut[c] is the index of corner number c
// (corner c of an axis is the low face of key kmin + c; key x has corners x and x + 1)
__global__ __launch_bounds__(256) void index_scatter_kernel(const unsigned* keys, int n, int wpr, const int* lut, int dim,
                                                            int wpr_i, unsigned* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * n * wpr) return;
  unsigned word = keys[i];
  if (!word) return;
  const int xw = (int)(i % wpr), y = (int)((i / wpr) % n), z = (int)(i / ((int64_t)wpr * n));
  const int jy[2] = {lut[y], lut[y + 1]}, jz[2] = {lut[z], lut[z + 1]};
  while (word) {
    const int x = xw * 32 + __builtin_ctz(word);
    word &= word - 1;
    if (x >= n) break;
    const int jx[2] = {lut[x], lut[x + 1]};
    for (int c = 0; c < 8; ++c) {
      const int ix = jx[c & 1], iy = jy[(c >> 1) & 1], iz = jz[c >> 2];
      if ((unsigned)ix < (unsigned)dim && (unsigned)iy < (unsigned)dim && (unsigned)iz < (unsigned)dim)
        atomicOr(&out[((size_t)iz * dim + iy) * wpr_i + (ix >> 5)], 1u << (ix & 31));
    }
  }
}

__global__ __launch_bounds__(256) void iou_count_kernel(const unsigned* gt, const unsigned* preds, int64_t words,
                                                        unsigned long long* inter, unsigned long long* uni) {
  __shared__ unsigned s_n[2][4];
  const int v = blockIdx.y;
  const unsigned* p = preds + (size_t)v * words;
  unsigned ni = 0, nu = 0;   // a block's share is < 2^32 bits (words <= 2^25)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
    const unsigned a = gt[i], b = p[i];
    ni += __popc(a & b);
    nu += __popc(a | b);
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    ni += __shfl_down(ni, d, 64);
    nu += __shfl_down(nu, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_n[0][threadIdx.x >> 6] = ni;
    s_n[1][threadIdx.x >> 6] = nu;
  }
  __syncthreads();
  if (threadIdx.x == 0) {   // one pair of atomics per block: few adds meet on an address
    const unsigned long long ti = (unsigned long long)s_n[0][0] + s_n[0][1] + s_n[0][2] + s_n[0][3];
    const unsigned long long tu = (unsigned long long)s_n[1][0] + s_n[1][1] + s_n[1][2] + s_n[1][3];
    if (ti) atomicAdd(&inter[v], ti);
    if (tu) atomicAdd(&uni[v], tu);
  }
}

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

static size_t voxel_grid_words(int n) { return (size_t)n * n * ((n + 31) / 32); }

static size_t voxel_surface_ws_bytes(int64_t nf) { return 256 + al256(sizeof(int2) * (size_t)(nf > 0 ? nf : 0)); }

static size_t voxel_fill_ws_bytes(int n) { return 256 + al256(4 * voxel_grid_words(n)); }

static hipError_t voxel_surface_launch(const float* verts, int64_t nv, const int* faces, int64_t nf, int dim, int kmin,
                                       int nkeys, unsigned* bits, int* flags, void* ws, hipStream_t st) {
  hipError_t e;
  if ((e = hipMemsetAsync(bits, 0, 4 * voxel_grid_words(nkeys), st)) != hipSuccess) return e;
  if (nf == 0) return hipSuccess;
  int* qcount = static_cast<int*>(ws);
  int2* queue = reinterpret_cast<int2*>(static_cast<char*>(ws) + 256);
  if ((e = hipMemsetAsync(qcount, 0, sizeof(int), st)) != hipSuccess) return e;
  const float h = 2.0f / (float)dim;
  const VoxGrid g{h, h * 0.5f, kmin, nkeys, (nkeys + 31) / 32};
  voxel_tri_kernel<<<blocks256(nf), 256, 0, st>>>(verts, nv, faces, nf, g, bits, flags, queue, qcount);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  voxel_big_kernel<<<kBigBlocks, 256, 0, st>>>(verts, nv, faces, g, bits, flags, queue, qcount);
  return hipGetLastError();
}

// 0, a hipError_t, or DISN_E_CONVERGE; synchronises `st` once per batch of sweeps
static int voxel_fill_launch(const unsigned* surf, int n, unsigned* solid, void* ws, hipStream_t st) {
  const int wpr = (n + 31) / 32;
  const unsigned nb = blocks256((int64_t)voxel_grid_words(n));
  int* changed = static_cast<int*>(ws);
  unsigned* O = reinterpret_cast<unsigned*>(static_cast<char*>(ws) + 256);
  hipError_t e;
  fill_init_kernel<<<nb, 256, 0, st>>>(surf, n, wpr, O);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  bool converged = false;
  for (int it = 0; it < kFillMaxIter && !converged; it += kFillBatch) {
    if ((e = hipMemsetAsync(changed, 0, sizeof(int), st)) != hipSuccess) return (int)e;
    for (int k = 0; k < kFillBatch; ++k) fill_sweep_kernel<<<nb, 256, 0, st>>>(surf, n, wpr, O, changed);
    int c = 1;
    if ((e = hipMemcpyAsync(&c, changed, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e;
    converged = c == 0;
  }
  if (!converged) return DISN_E_CONVERGE;
  fill_finish_kernel<<<nb, 256, 0, st>>>(O, n, wpr, solid);
  return (int)hipGetLastError();
}

static hipError_t voxel_index_grid_launch(const unsigned* keys, int nkeys, const int* lut, int dim, unsigned* out,
                                          hipStream_t st) {
  hipError_t e;
  if ((e = hipMemsetAsync(out, 0, 4 * voxel_grid_words(dim), st)) != hipSuccess) return e;
  index_scatter_kernel<<<blocks256((int64_t)voxel_grid_words(nkeys)), 256, 0, st>>>(
      keys, nkeys, (nkeys + 31) / 32, lut, dim, (dim + 31) / 32, out);
  return hipGetLastError();
}

static hipError_t voxel_iou_launch(const unsigned* gt, const unsigned* preds, int nviews, int64_t words,
                                   int64_t* inter, int64_t* uni, hipStream_t st) {
  hipError_t e;
  if ((e = hipMemsetAsync(inter, 0, sizeof(int64_t) * nviews, st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(uni, 0, sizeof(int64_t) * nviews, st)) != hipSuccess) return e;
  const int64_t per = (words + 2047) / 2048;   // at least 8 words per thread
  const unsigned bx = (unsigned)(per < 8 ? (per > 0 ? per : 1) : 8);
  iou_count_kernel<<<dim3(bx, (unsigned)nviews), 256, 0, st>>>(gt, preds, words,
                                                               reinterpret_cast<unsigned long long*>(inter),
                                                               reinterpret_cast<unsigned long long*>(uni));
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

static int voxel_axis(int n) { return n < 1 ? DISN_E_ARG : (n > 1024 ? DISN_E_SHAPE : 0); }

size_t disn_voxel_grid_words(int n) { return voxel_axis(n) ? 0 : voxel_grid_words(n); }

size_t disn_voxel_surface_workspace_bytes(int64_t nf) {
  return (nf < 0 || nf > INT32_MAX) ? 0 : voxel_surface_ws_bytes(nf);
}

int disn_voxel_surface(const float* verts, int64_t nv, const int32_t* faces, int64_t nf, int dim, int kmin, int nkeys,
                       uint32_t* bits, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
  if (!bits || !flags || !ws || nv < 0 || nf < 0 || dim < 1) return DISN_E_ARG;
  if (nf > 0 && (!verts || !faces)) return DISN_E_ARG;
  if (int rc = voxel_axis(nkeys)) return rc;
  if (dim > 1024 || kmin < -4096 || kmin > 4096 || nf > INT32_MAX || nv > INT32_MAX) return DISN_E_SHAPE;   // int32 faces
  if (ws_bytes < voxel_surface_ws_bytes(nf)) return DISN_E_WS;
  DISN_TRY(voxel_surface_launch(verts, nv, faces, nf, dim, kmin, nkeys, bits, flags, ws, (hipStream_t)stream));
  return 0;
}

size_t disn_voxel_fill_workspace_bytes(int n) { return voxel_axis(n) ? 0 : voxel_fill_ws_bytes(n); }

int disn_voxel_fill(const uint32_t* surface, int n, uint32_t* solid, void* ws, size_t ws_bytes, void* stream) {
  if (!surface || !solid || !ws) return DISN_E_ARG;
  if (int rc = voxel_axis(n)) return rc;
  if (ws_bytes < voxel_fill_ws_bytes(n)) return DISN_E_WS;
  return voxel_fill_launch(surface, n, solid, ws, (hipStream_t)stream);
}

int disn_voxel_index_grid(const uint32_t* keys, int nkeys, const int32_t* lut, int dim, uint32_t* index_bits,
                          void* stream) {
  if (!keys || !lut || !index_bits) return DISN_E_ARG;
  if (int rc = voxel_axis(nkeys)) return rc;
  if (int rc = voxel_axis(dim)) return rc;
  DISN_TRY(voxel_index_grid_launch(keys, nkeys, lut, dim, index_bits, (hipStream_t)stream));
  return 0;
}

int disn_voxel_iou(const uint32_t* gt, const uint32_t* preds, int nviews, int64_t words, int64_t* inter,
                   int64_t* uni, void* stream) {
  if (!gt || !preds || !inter || !uni || nviews < 1 || words < 1) return DISN_E_ARG;
  if (nviews > 65535 || words > ((int64_t)1 << 25)) return DISN_E_SHAPE;
  DISN_TRY(voxel_iou_launch(gt, preds, nviews, words, inter, uni, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
