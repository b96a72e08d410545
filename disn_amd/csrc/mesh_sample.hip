// Area-weighted surface samples of device meshes (include/disn_amd_sample.h; the rule is disn_amd/metrics.py
// sample_surface_arrays, restated here operation by operation): B meshes back to back, n samples each.
//
//   validate indices and coordinates -> one thread per face: s = |e1 x e2|^2 in float64, the mesh's maximum as an
//   unsigned atomic max of the double's bits (non-negative doubles order as their bits do, so no bit depends on the
//   order) -> status 6 for a mesh without area -> one thread per face: the integer weight q -> the inclusive scan of q
//   over ALL faces of the call in uint64, three passes (blocks, block sums, add) -> one thread per sample: the two
//   random words, a binary search in the mesh's slice of the scan, the point and the normal.
//
// NO KERNEL WAITS FOR ANOTHER WORKGROUP (the scan is three launches, no look-back).  EVERY LOOP IS BOUNDED: by the grid
// stride, by the number of block sums, by 32 steps of the binary search.  NO FLOATING-POINT ATOMIC.  No host read-back.
// Compiled with -ffp-contract=off: the float64 and float32 arithmetic rounds as numpy's does.
// (mesh_of, mix64, the two validators and the host-side helpers are those of mesh_batch.hpp.)
#include "mesh_batch.hpp"

#include "../../include/disn_amd_sample.h"

namespace disn {
namespace {

enum { ST_NO_AREA = DISN_SAMPLE_NO_AREA };     // this stage's own status: no faces, or no face with an area
constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;
constexpr int kScanItems = 16;
constexpr int kScanBlock = kThreads * kScanItems;
static_assert(kScanBlock == kScanBlockItems, "scan_bsum_items sizes the block sums");

// N = e1 x e2 of global face f of mesh b in float64 and s = (N.x^2 + N.y^2) + N.z^2; the mesh's indices are checked
__device__ __forceinline__ double face_normal(const float* __restrict__ verts, const int* __restrict__ faces,
                                              long long v0, long long f, double N[3]) {
  const float* a = verts + 3 * (v0 + faces[3 * f]);
  const float* b = verts + 3 * (v0 + faces[3 * f + 1]);
  const float* c = verts + 3 * (v0 + faces[3 * f + 2]);
  const double e1x = (double)b[0] - (double)a[0], e1y = (double)b[1] - (double)a[1], e1z = (double)b[2] - (double)a[2];
  const double e2x = (double)c[0] - (double)a[0], e2y = (double)c[1] - (double)a[1], e2z = (double)c[2] - (double)a[2];
  N[0] = e1y * e2z - e1z * e2y;
  N[1] = e1z * e2x - e1x * e2z;
  N[2] = e1x * e2y - e1y * e2x;
  return (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2];
}

// the exact integer square root of x <= 2^62: a float64 estimate, corrected by +-1 with integer multiplies
__device__ __forceinline__ unsigned long long isqrt64(unsigned long long x) {
  unsigned long long r = (unsigned long long)sqrt((double)x);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (r * r > x) --r;
    if ((r + 1) * (r + 1) <= x) ++r;
  }
  return r;
}

__global__ __launch_bounds__(kThreads) void face_max_kernel(const float* __restrict__ verts,
                                                            const int* __restrict__ faces,
                                                            const long long* __restrict__ voff,
                                                            const long long* __restrict__ foff, int B, long long nf,
                                                            const int* __restrict__ status,
                                                            unsigned long long* smax) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b]) continue;
    double N[3];
    const unsigned long long bits = (unsigned long long)__double_as_longlong(face_normal(verts, faces, voff[b], f, N));
    if (bits > smax[b]) atomicMax(&smax[b], bits);           // the plain read only spares atomics: it can but lag
  }
}

__global__ __launch_bounds__(kThreads) void area_status_kernel(const long long* __restrict__ foff, int B,
                                                               const unsigned long long* __restrict__ smax,
                                                               int* status) {
  GRID_STRIDE(b, B) {
    if (status[b] == 0 && (foff[b + 1] == foff[b] || smax[b] == 0ull)) status[b] = ST_NO_AREA;
  }
}

__global__ __launch_bounds__(kThreads) void weight_kernel(const float* __restrict__ verts,
                                                          const int* __restrict__ faces,
                                                          const long long* __restrict__ voff,
                                                          const long long* __restrict__ foff, int B, long long nf,
                                                          const int* __restrict__ status,
                                                          const unsigned long long* __restrict__ smax,
                                                          unsigned long long* __restrict__ cum) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    unsigned long long q = 0;
    if (!status[b]) {
      double N[3];
      const double s = face_normal(verts, faces, voff[b], f, N);
      const double r = s / __longlong_as_double((long long)smax[b]);
      q = isqrt64((unsigned long long)floor(r * 4611686018427387904.0));
    }
    cum[f] = q;
  }
}

// inclusive scan of uint64 in place, kScanBlock items per block; the block's sum -> bsum[block]
__global__ __launch_bounds__(kThreads) void scan_block_kernel(unsigned long long* __restrict__ data, long long n,
                                                              unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long wsum[kThreads / 64];
  const long long base = (long long)blockIdx.x * kScanBlock + (long long)threadIdx.x * kScanItems;
  unsigned long long v[kScanItems], tsum = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    v[i] = (base + i < n) ? data[base + i] : 0ull;
    tsum += v[i];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long inc = tsum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long u = __shfl_up(inc, off, 64);
    if (lane >= off) inc += u;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  unsigned long long woff = 0;
  for (int w = 0; w < wave; ++w) woff += wsum[w];
  unsigned long long run = woff + inc - tsum;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    run += v[i];
    if (base + i < n) data[base + i] = run;
  }
  if (threadIdx.x == kThreads - 1) bsum[blockIdx.x] = woff + inc;
}

// one block: exclusive scan of the nb block sums in place
__global__ __launch_bounds__(1024) void scan_sums_kernel(unsigned long long* __restrict__ bsum, int nb) {
  __shared__ unsigned long long carry;
  __shared__ unsigned long long wsum[16];
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + threadIdx.x;
    const unsigned long long v = i < nb ? bsum[i] : 0ull;
    unsigned long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long u = __shfl_up(inc, off, 64);
      if (lane >= off) inc += u;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    const unsigned long long c = carry;
    if (i < nb) bsum[i] = c + woff + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = c + woff + inc;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void scan_add_kernel(unsigned long long* __restrict__ data, long long n,
                                                            const unsigned long long* __restrict__ bsum) {
  const long long base = (long long)blockIdx.x * kScanBlock + (long long)threadIdx.x * kScanItems;
  const unsigned long long add = bsum[blockIdx.x];
#pragma unroll
  for (int i = 0; i < kScanItems; ++i)
    if (base + i < n) data[base + i] += add;
}

// sample i of mesh b: item = b n + i
__global__ __launch_bounds__(kThreads) void sample_kernel(const float* __restrict__ verts,
                                                          const int* __restrict__ faces,
                                                          const long long* __restrict__ voff,
                                                          const long long* __restrict__ foff, int n, long long items,
                                                          const int* __restrict__ status,
                                                          const unsigned long long* __restrict__ seeds,
                                                          const unsigned long long* __restrict__ cum,
                                                          float* __restrict__ points, float* __restrict__ normals,
                                                          int* __restrict__ face_idx) {
  GRID_STRIDE(item, items) {
    const int b = (int)(item / n);
    const unsigned long long i = (unsigned long long)(item - (long long)b * n);
    float p[3] = {0.0f, 0.0f, 0.0f}, nr[3] = {0.0f, 0.0f, 0.0f};
    int local = 0;
    if (!status[b]) {                                          // so the mesh has a face with q > 0: total > 0
      const unsigned long long seed = seeds[b];
      const unsigned long long r0 = mix64(seed + kGolden * (2 * i + 1)), r1 = mix64(seed + kGolden * (2 * i + 2));
      const long long f0 = foff[b], f1 = foff[b + 1];
      const unsigned long long below = f0 > 0 ? cum[f0 - 1] : 0ull;
      const unsigned long long target = __umul64hi(r0, cum[f1 - 1] - below);     // < total
      long long lo = f0, hi = f1 - 1;                          // the first face with cum - below > target
      for (int step = 0; step < 32 && lo < hi; ++step) {       // f1 - f0 < 2^31
        const long long mid = lo + ((hi - lo) >> 1);
        if (cum[mid] - below > target) hi = mid;
        else lo = mid + 1;
      }
      local = (int)(lo - f0);
      const long long v0 = voff[b];
      const float* A = verts + 3 * (v0 + faces[3 * lo]);
      const float* Bc = verts + 3 * (v0 + faces[3 * lo + 1]);
      const float* Cc = verts + 3 * (v0 + faces[3 * lo + 2]);
      const float u1 = (float)(unsigned)(r1 >> 40) * 5.9604644775390625e-8f;
      const float u2 = (float)(unsigned)((r1 >> 16) & 0xFFFFFFull) * 5.9604644775390625e-8f;
      const float t = sqrtf(u1);
      const float wa = 1.0f - t, wb = t * (1.0f - u2), wc = t * u2;
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = (wa * A[k] + wb * Bc[k]) + wc * Cc[k];
      if (normals) {
        double N[3];
        const double len = sqrt(face_normal(verts, faces, v0, lo, N));
#pragma unroll
        for (int k = 0; k < 3; ++k) nr[k] = (float)(N[k] / len);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      points[3 * item + k] = p[k];
      if (normals) normals[3 * item + k] = nr[k];
    }
    if (face_idx) face_idx[item] = local;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
struct SampleWs {
  long long *voff, *foff;                          // [B+1] each
  unsigned long long* seeds;                       // [B]
  unsigned long long* smax;                        // [B]   zeroed
  unsigned long long* cum;                         // [nf]
  unsigned long long* bsum;                        // [scan_bsum_items(nf)]
  size_t total;
};

SampleWs sample_layout(void* ws, int B, long long nf) {
  WsCursor c(ws);
  const size_t b1 = (size_t)B + 1, f = (size_t)(nf > 0 ? nf : 1);
  SampleWs w;
  w.voff = c.take<long long>(b1); w.foff = c.take<long long>(b1);
  w.seeds = c.take<unsigned long long>(b1);
  w.smax = c.take<unsigned long long>(b1);
  w.cum = c.take<unsigned long long>(f);
  w.bsum = c.take<unsigned long long>(scan_bsum_items(f));
  w.total = c.next();
  return w;
}

bool batch_ok(int B, int64_t nv, int64_t nf, int n) {
  return mesh_limits_ok(B, nv, nf) && n >= 1 && n <= DISN_SAMPLE_MAX_N;
}

}  // namespace
}  // namespace disn

using namespace disn;

extern "C" size_t disn_mesh_sample_workspace_bytes(int B, int64_t nv_total, int64_t nf_total, int n) {
  return batch_ok(B, nv_total, nf_total, n) ? sample_layout(nullptr, B, nf_total).total : 0;
}

extern "C" int disn_mesh_sample_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                      const int64_t* f_off_host, int B, const uint64_t* seeds_host, int n,
                                      float* points, float* normals, int32_t* face_idx, int32_t* status, void* ws,
                                      size_t ws_bytes, void* stream) {
  if (!offsets_ok(v_off_host, f_off_host, B) || !seeds_host || !points || !status || !ws) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if ((nv > 0 && !verts) || (nf > 0 && !faces)) return DISN_E_ARG;
  if (!batch_ok(B, nv, nf, n)) return DISN_E_SHAPE;
  if (ws_bytes < sample_layout(nullptr, B, nf).total) return DISN_E_WS;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "seeds travel as uint64");
  hipStream_t st = (hipStream_t)stream;
  const SampleWs w = sample_layout(ws, B, nf);
  MESH_TRY(upload_offsets(w.voff, w.foff, v_off_host, f_off_host, B, st));
  MESH_TRY(hipMemcpyAsync(w.seeds, seeds_host, (size_t)B * 8, hipMemcpyHostToDevice, st));
  MESH_TRY(hipMemsetAsync(w.smax, 0, (size_t)B * 8, st));
  MESH_TRY(hipMemsetAsync(status, 0, (size_t)B * 4, st));
  if (nf > 0) MESH_LAUNCH(validate_faces_kernel, nf, faces, w.voff, w.foff, B, nf, status);
  if (nv > 0) MESH_LAUNCH(validate_verts_kernel, nv, verts, w.voff, B, nv, status);
  if (nf > 0) MESH_LAUNCH(face_max_kernel, nf, verts, faces, w.voff, w.foff, B, nf, status, w.smax);
  MESH_LAUNCH(area_status_kernel, B, w.foff, B, w.smax, status);
  if (nf > 0) {
    MESH_LAUNCH(weight_kernel, nf, verts, faces, w.voff, w.foff, B, nf, status, w.smax, w.cum);
    const int nb = (int)((nf + kScanBlock - 1) / kScanBlock);
    hipLaunchKernelGGL(scan_block_kernel, dim3(nb), dim3(kThreads), 0, st, w.cum, (long long)nf, w.bsum);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, st, w.bsum, nb);
    hipLaunchKernelGGL(scan_add_kernel, dim3(nb), dim3(kThreads), 0, st, w.cum, (long long)nf, w.bsum);
    MESH_TRY(hipGetLastError());
  }
  const long long items = (long long)B * n;
  MESH_LAUNCH(sample_kernel, items, verts, faces, w.voff, w.foff, n, items, status, w.seeds, w.cum, points, normals,
              face_idx);
  return 0;
}
